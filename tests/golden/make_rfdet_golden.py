"""Generate tests/golden/rfdet.npz from the REFERENCE RF-Net detector (RFDetSO) and its keypoint selection.

Run from the repo root:  python tests/golden/make_rfdet_golden.py
Needs the reference tree (HN_REFERENCE, as make_detect_golden.py; read-only, never copied).  The definitions are
AST-extracted at run time from FDLNet-master/latency/rfnet and executed on the CPU with ``torch`` in scope:
  RFDetModule (model/rf_det_module.py); RFDetSO (model/rf_det_so.py); L2Norm (utils/math_utils.py);
  filtbordmask, filter_border, nms, topk_map, get_gauss_filter_weight, soft_nms_3d, soft_max_and_argmax_1d,
  clip_patch (utils/image_utils.py); RFNetSO.inference (model/rf_net_so.py), called with a stand-in ``self`` whose
  descriptor returns zeros (only its keypoints are kept; scale and orientation are gathered at them as
  ``inference`` gathers them for clip_patch); HardNetNeiMask of model/rf_des.py for its state_dict key list only.
Only data is written: the weights blob and key list, the images, the reference's fp32 score / scale / ori, an fp64
evaluation of each (the same module in .double() with scale_list cast; stored as fp32 differences), the
orientation exclusion mask, process's three fp32 outputs, the inference-style kpts / scale / ori / score, the
stable-keypoint flags and JSON metadata.

Inputs: weights by tests/rfdet_ref.py's ``randomise_`` (weights_init, InstanceNorm affine parameters and conv_o*
heads moved off their defaults); 3 uniform-noise images of 61 x 83.

Conditions asserted here, each recorded in the metadata:
  0 < E_score = max |fp32 - fp64| < 1e-4;  0 < E_scale < 1e-2;
  orientation pixels where any of the ten per-level pre-division norms, or the final one, is below 0.05 in fp64 are
  excluded from value comparison, their share is <= 1 %, and E_ori is the maximum over the rest;
  every image has at least K strictly positive NMS survivors, and at both top-K steps the reference's K-th and
  (K+1)-th values differ by more than 1e-5 relative;
  the selected keypoints' scales take at least 5 distinct values;
  "stable" keypoints (make_detect_golden.py's definition: returned on the fp32 score, on the fp64 score rounded to
  fp32 and on four seeded perturbations of amplitude 4 E_score) are >= 90 %.
"""
from __future__ import annotations

import ast
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: rfdet_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: hardnetnas_amd (the seeded initialiser)
import rfdet_ref as R  # noqa: E402

REF = os.environ.get("HN_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
BASE = os.path.join(REF, "FDLNet-master", "latency", "rfnet")

SEED = int(os.environ.get("HN_RFDET_SEED", "2041"))
B, H, W = 3, 61, 83
K = R.K
WANTED = {
    "model/rf_det_module.py": ("RFDetModule",),
    "model/rf_det_so.py": ("RFDetSO",),
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
    tree = ast.parse(open(os.path.join(BASE, "model/rf_net_so.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "RFNetSO"]
    fn = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "inference"]
    assert len(cls) == 1 and len(fn) == 1
    exec(ast.unparse(ast.Module(body=fn, type_ignores=[])), ns)
    # inference masked_selects with topk_map's uint8 mask, which current torch rejects: inside inference (and the
    # process it calls) the mask is the same one as bool
    plain_topk, plain_inference = ns["topk_map"], ns["inference"]

    def inference(*a, **k):
        ns["topk_map"] = lambda *x, **y: plain_topk(*x, **y).bool()
        try:
            return plain_inference(*a, **k)
        finally:
            ns["topk_map"] = plain_topk
    ns["inference"] = inference
    des_ns = {"torch": torch, "nn": nn}
    tree = ast.parse(open(os.path.join(BASE, "model/rf_des.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HardNetNeiMask"]
    assert len(keep) == 1
    exec(ast.unparse(ast.Module(body=keep, type_ignores=[])), des_ns)
    ns["RFDesReference"] = des_ns["HardNetNeiMask"]
    return ns


def kth_gap(maps, k):
    """min over images of (v_k - v_{k+1}) / v_k of the descending order of [B,H,W,1] maps."""
    s = maps.reshape(maps.shape[0], -1).sort(dim=-1, descending=True)[0].double()
    return float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min())


def main():
    ns = reference_namespace()
    torch.manual_seed(SEED)  # the constructor draws the conv biases, which weights_init leaves as they are
    det = R.randomise_(ns["RFDetSO"](**R.DET_ARGS), SEED)
    sd = det.state_dict()
    keys = list(sd)
    blob = np.concatenate([v.detach().float().reshape(-1).numpy() for v in sd.values()]).astype(np.float32)
    assert blob.size == 21890 and len(keys) == 100
    images = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(SEED + 2))
    im_info = torch.ones(B, 2)
    zeros_des = lambda p: p.new_zeros(p.shape[0], 128)  # noqa: E731
    net = types.SimpleNamespace(det=det, TOPK=K, PSIZE=32, des=zeros_des)

    def gather(m, kpts):  # the rows of a [B,H,W,...] map at the keypoints: inference's masked_select, in its order
        return m[kpts[:, 0], kpts[:, 1], kpts[:, 2]]

    with torch.no_grad():
        score32, scale32, ori32 = det(images)

        def select(score):  # the reference's inference from a given raw score map on
            def fake_det(_):
                return score, scale32, ori32
            fake_det.process = det.process
            fake = types.SimpleNamespace(det=fake_det, TOPK=K, PSIZE=32, des=zeros_des)
            return ns["inference"](fake, images, im_info, images)

        im_scale, kpts, _ = ns["inference"](net, images, im_info, images)
        assert torch.equal(im_scale, scale32)
        kscale = gather(scale32.squeeze(-1), kpts)
        kori = gather(ori32.squeeze(-2), kpts)
        kscore = gather(score32.squeeze(-1), kpts)
        proc, topk_mask, topk_value = det.process(score32)

        # the fp64 evaluation, with every norm L2Norm divides by recorded: ten per-level ones, then the final one
        det64 = copy.deepcopy(det).double()
        det64.scale_list = det64.scale_list.double()
        norms, plain = [], ns["L2Norm"]

        def recording(input, dim=-1):
            norms.append(torch.norm(input, p=2, dim=dim))
            return plain(input, dim=dim)
        ns["L2Norm"] = recording
        try:
            score64, scale64, ori64 = det64(images.double())
        finally:
            ns["L2Norm"] = plain
        assert len(norms) == 11 and all(tuple(n.reshape(B, H, W).shape) == (B, H, W) for n in norms)
        min_norm = torch.stack([n.reshape(B, H, W) for n in norms]).min(dim=0)[0]
    assert tuple(score32.shape) == (B, H, W, 1) and tuple(scale32.shape) == (B, H, W, 1)
    assert tuple(ori32.shape) == (B, H, W, 1, 2)
    assert tuple(kpts.shape) == (B * K, 4) and kpts.dtype == torch.int64
    e_score = float((score32.double() - score64).abs().max())
    assert 0.0 < e_score < 1e-4, e_score
    e_scale = float((scale32.double() - scale64).abs().max())
    assert 0.0 < e_scale < 1e-2, e_scale
    ori_excluded = min_norm < R.NORM_FLOOR
    excluded_share = float(ori_excluded.double().mean())
    assert excluded_share <= 0.01, excluded_share
    d_ori = (ori32.double() - ori64).abs().amax(dim=-1).squeeze(-1)
    e_ori, e_ori_all = float(d_ori[~ori_excluded].max()), float(d_ori.max())
    assert 0.0 < e_ori < 1e-3, e_ori
    survivors = [int((topk_value[b] > 0).sum()) for b in range(B)]
    assert min(survivors) >= K, survivors
    gap1, gap2 = kth_gap(topk_value, K), kth_gap(proc, K)
    assert gap1 > 1e-5 and gap2 > 1e-5, (gap1, gap2)
    distinct_scales = int(torch.unique(kscale).numel())
    assert distinct_scales >= 5, distinct_scales

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
    d_scale = (scale64 - scale32.double()).float()
    d_ori32 = (ori64 - ori32.double()).float()
    assert float((score32.double() + d_score.double() - score64).abs().max()) < 1e-12
    assert float((scale32.double() + d_scale.double() - scale64).abs().max()) < 1e-11
    meta = {"source": "FDLNet-master/latency/rfnet model/rf_det_so.py, model/rf_det_module.py, "
                      "model/rf_net_so.py:160-180, utils/image_utils.py; fp32 on the CPU",
            "seed": SEED, "B": B, "H": H, "W": W, "K": K, "det_args": R.DET_ARGS, "border": 8,
            "state_dict_keys": keys, "rfdes_state_dict_keys": list(ns["RFDesReference"](1.0, 1.0).state_dict()),
            "E_score": e_score, "E_scale": e_scale, "E_ori": e_ori, "E_ori_all_pixels": e_ori_all,
            "scale_min": float(scale32.min()), "scale_max": float(scale32.max()), "scale_std": float(scale32.std()),
            "score_max": float(score32.max()),
            "ori_norm_floor": R.NORM_FLOOR, "ori_excluded_share": excluded_share, "nms_survivors": survivors,
            "kth_gap_first": gap1, "kth_gap_second": gap2, "first_stage_same_in_fp64": same_first_stage,
            "distinct_keypoint_scales": distinct_scales, "perturbation": 4.0 * e_score, "stable_share": stable_share}
    out = {"blob": blob, "images": images.numpy(), "score32": score32.squeeze(-1).numpy(),
           "scale32": scale32.squeeze(-1).numpy(), "ori32": ori32.squeeze(-2).numpy(),
           "score64_minus_score32": d_score.squeeze(-1).numpy(), "scale64_minus_scale32": d_scale.squeeze(-1).numpy(),
           "ori64_minus_ori32": d_ori32.squeeze(-2).numpy(), "ori_excluded": ori_excluded.numpy(),
           "proc_score": proc.squeeze(-1).numpy(), "proc_mask": topk_mask.squeeze(-1).numpy(),
           "proc_value": topk_value.squeeze(-1).numpy(), "kpts": kpts.numpy(), "kscale": kscale.numpy(),
           "kori": kori.numpy(), "kscore": kscore.numpy(), "stable": stable, "meta": json.dumps(meta)}
    path = os.path.join(HERE, "rfdet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps({k: v for k, v in meta.items() if "state_dict_keys" not in k}, indent=1))


if __name__ == "__main__":
    main()
