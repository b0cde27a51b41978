"""Generate tests/golden/detect.npz from the REFERENCE keypoint detector and keypoint selection.

Run from the repo root:  python tests/golden/make_detect_golden.py
Needs the reference tree (HN_REFERENCE, as make_golden.py; read-only, never copied).  The definitions are
AST-extracted at run time and executed on the CPU with ``torch`` in scope (model/det.py imports torchvision and
utils/image_utils.py imports skimage; neither is needed):
  RFDet (model/det.py); InvertedResidual, channel_shuffle (model/operations.py); L2Norm (utils/math_utils.py);
  filtbordmask, filter_border, nms, topk_map, get_gauss_filter_weight, soft_nms_3d, soft_max_and_argmax_1d,
  clip_patch (utils/image_utils.py); Network.inference (model/network.py), called with a stand-in ``self`` whose
  descriptor returns zeros (only its keypoint outputs are kept).
Only data is written: the weights blob, the images, the reference's fp32 score / ori, an fp64 evaluation of each
(the same module in .double(), stored as fp32 differences as clip_patch.npz does), process's three fp32 outputs,
the inference-style kpts / scale / ori / score, the stable-keypoint flags and JSON metadata.

Inputs: seeded weights with the BatchNorm running statistics and affine parameters and the InstanceNorm affine
parameters randomised away from their defaults; 3 uniform-noise images of 61 x 83 (odd, no multiple of any tile,
larger than one tile plus halos).

Conditions asserted here, each recorded in the metadata:
  0 < E_score = max |fp32 - fp64| < 1e-4;
  orientation pixels whose fp64 pre-division pair norm is below 0.05 are excluded from value comparison (the
  division amplifies the error there without bound) and their share is <= 1 %; E_ori is the maximum over the rest;
  every image has at least K strictly positive NMS survivors, and at both top-K steps the reference's K-th and
  (K+1)-th values differ by more than 1e-5 relative, so that no cut falls inside a group of equal values;
  "stable" keypoints are those the reference selection returns on the fp32 score, on the fp64 score (rounded to
  fp32, the dtype the reference's blur weights have) and on four seeded perturbations of the fp32 score by uniform
  noise of amplitude 4 E_score; their share is >= 90 %.
"""
from __future__ import annotations

import ast
import json
import os
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference tree: HN_REFERENCE, or a "reference" directory beside the repository
REF = os.environ.get("HN_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
BASE = os.path.join(REF, "FDLNet-master", "latency", "NASNet")

SEED = 2037
B, H, W = 3, 61, 83
K = 48
DET_ARGS = dict(score_com_strength=100.0, scale_com_strength=100.0, nms_thresh=0.0, nms_ksize=5, topk=K,
                gauss_ksize=15, gauss_sigma=0.5)  # config.py's values but for topk
NORM_FLOOR = 0.05
WANTED = {
    "model/det.py": ("RFDet",),
    "model/operations.py": ("InvertedResidual", "channel_shuffle"),
    "utils/math_utils.py": ("L2Norm",),
    "utils/image_utils.py": ("filtbordmask", "filter_border", "nms", "topk_map", "get_gauss_filter_weight",
                             "soft_nms_3d", "soft_max_and_argmax_1d", "clip_patch"),
}


def reference_namespace():
    ns = {"torch": torch, "nn": nn, "F": F}
    for rel, names in WANTED.items():
        tree = ast.parse(open(os.path.join(BASE, rel)).read())
        keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
        assert len(keep) == len(names), (rel, [n.name for n in keep])
        exec(ast.unparse(ast.Module(body=keep, type_ignores=[])), ns)
    tree = ast.parse(open(os.path.join(BASE, "model/network.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Network"]
    fn = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "inference"]
    assert len(cls) == 1 and len(fn) == 1
    exec(ast.unparse(ast.Module(body=fn, type_ignores=[])), ns)
    return ns


def seeded_detector(ns):
    torch.manual_seed(SEED)
    det = ns["RFDet"](**DET_ARGS)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for m in det.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
            elif isinstance(m, nn.InstanceNorm2d):
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
    return det.eval()


def kth_gap(maps, k):
    """min over images of (v_k - v_{k+1}) / v_k of the descending order of [B,H,W,1] maps."""
    s = maps.reshape(maps.shape[0], -1).sort(dim=-1, descending=True)[0].double()
    return float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min())


def main():
    ns = reference_namespace()
    det = seeded_detector(ns)
    sd = det.state_dict()
    blob = np.concatenate([v.detach().float().reshape(-1).numpy() for k, v in sd.items()
                           if not k.endswith("num_batches_tracked")]).astype(np.float32)
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    images = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(SEED + 2))
    im_info = torch.ones(B, 2)
    net = types.SimpleNamespace(det=det, TOPK=K, PSIZE=32, des=lambda p: p.new_zeros(p.shape[0], 128))

    def select(score):  # the reference's inference from a given raw score map on
        def fake_det(_):
            return score, scale32, ori32
        fake_det.process = det.process
        fake = types.SimpleNamespace(det=fake_det, TOPK=K, PSIZE=32, des=net.des)
        return ns["inference"](fake, images, im_info, images)

    with torch.no_grad():
        score32, scale32, ori32 = det(images)
        assert float((scale32 - 32.0).abs().max()) == 0.0
        im_scale, kpts, _, kscale, kori, kscore = ns["inference"](net, images, im_info, images)
        proc, topk_mask, topk_value = det.process(score32)
        det64 = seeded_detector(ns).double()
        score64, _, ori64 = det64(images.double())
        pre = det64.insnorm_ori(det64.conv_ori(det64.features(images.double())))
        pair_norm = pre.norm(p=2, dim=1)
    assert tuple(kpts.shape) == (B * K, 4) and kpts.dtype == torch.int64
    e_score = float((score32.double() - score64).abs().max())
    assert 0.0 < e_score < 1e-4, e_score
    ori_excluded = pair_norm < NORM_FLOOR
    excluded_share = float(ori_excluded.double().mean())
    assert excluded_share <= 0.01, excluded_share
    d_ori = (ori32.double() - ori64).abs().amax(dim=-1)
    e_ori, e_ori_all = float(d_ori[~ori_excluded].max()), float(d_ori.max())
    assert 0.0 < e_ori < 1e-3, e_ori
    survivors = [int((topk_value[b] > 0).sum()) for b in range(B)]
    assert min(survivors) >= K, survivors
    gap1, gap2 = kth_gap(topk_value, K), kth_gap(proc, K)
    assert gap1 > 1e-5 and gap2 > 1e-5, (gap1, gap2)

    def rows(t):
        return {tuple(r) for r in t[:, :3].tolist()}

    with torch.no_grad():
        sets = [rows(kpts), rows(select(score64.float())[1])]
        same_first_stage = bool(torch.equal(det.process(score64.float())[1], topk_mask))
        g = torch.Generator().manual_seed(SEED + 3)
        for _ in range(4):
            noise = (2.0 * torch.rand(score32.shape, generator=g) - 1.0) * (4.0 * e_score)
            sets.append(rows(select(score32 + noise)[1]))
    common = set.intersection(*sets)
    stable = np.array([tuple(r) in common for r in kpts[:, :3].tolist()])
    stable_share = float(stable.mean())
    assert stable_share >= 0.9, stable_share

    d_score = (score64 - score32.double()).float()
    d_ori32 = (ori64 - ori32.double()).float()
    assert float((score32.double() + d_score.double() - score64).abs().max()) < 1e-12
    meta = {"source": "FDLNet-master/latency/NASNet model/det.py, model/network.py:148-183, utils/image_utils.py; "
                      "fp32 on the CPU",
            "seed": SEED, "B": B, "H": H, "W": W, "K": K, "det_args": DET_ARGS, "border": 8, "scale": 32.0,
            "state_dict_keys": keys, "E_score": e_score, "E_ori": e_ori, "E_ori_all_pixels": e_ori_all,
            "ori_norm_floor": NORM_FLOOR, "ori_excluded_share": excluded_share, "nms_survivors": survivors,
            "kth_gap_first": gap1, "kth_gap_second": gap2, "first_stage_same_in_fp64": same_first_stage,
            "perturbation": 4.0 * e_score, "stable_share": stable_share}
    out = {"blob": blob, "images": images.numpy(), "score32": score32.squeeze(-1).numpy(), "ori32": ori32.numpy(),
           "score64_minus_score32": d_score.squeeze(-1).numpy(), "ori64_minus_ori32": d_ori32.numpy(),
           "ori_excluded": ori_excluded.numpy(), "proc_score": proc.squeeze(-1).numpy(),
           "proc_mask": topk_mask.squeeze(-1).numpy(), "proc_value": topk_value.squeeze(-1).numpy(),
           "kpts": kpts.numpy(), "kscale": kscale.numpy(), "kori": kori.numpy(), "kscore": kscore.numpy(),
           "stable": stable, "meta": json.dumps(meta)}
    path = os.path.join(HERE, "detect.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps({k: v for k, v in meta.items() if k != "state_dict_keys"}, indent=1))


if __name__ == "__main__":
    main()
