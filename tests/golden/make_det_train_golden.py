"""Generate tests/golden/det_train.npz: one training step of the REFERENCE keypoint detector in train().

Run from the repo root:  python tests/golden/make_det_train_golden.py
Needs the reference tree (HN_REFERENCE, as make_detect_golden.py; read-only, never copied).  ``RFDet`` and what it
calls are AST-extracted at run time exactly as make_detect_golden.py does and executed on the CPU.

The step: the detector seeded as in make_detect_golden.py (BatchNorm and InstanceNorm affines and the running
statistics randomised away from their defaults), put in train(); 2 uniform-noise images of 61 x 83; seeded N(0,1)
upstream gradients Gs [2,61,83] and Go [2,61,83,2];

    score, _, ori = det(images);  ((score[..., 0] * Gs).sum() + (ori * Go).sum()).backward()

run in fp32 and, from the same start, in fp64 (``.double()``).  Only data is written: the 40 start tensors (one blob
in state_dict order), the images, Gs, Go, and the step's results -- score, ori, every parameter gradient (one blob
in parameter order) and every running statistic after the step -- in fp32, with the fp64 values stored as fp32
differences from them (as detect.npz does), plus JSON metadata.

Conditions asserted here, each recorded in the metadata:
  0 < E_score = max |fp32 - fp64| < 1e-4;
  orientation pixels whose fp64 pre-division pair norm is below 0.05 are excluded by value, their share is <= 1 %
  and E_ori, the maximum over the rest, is < 1e-3;
  the reference's own fp32 gradients are within 1e-3 L2-relative of fp64, all tensors together;
  the cancellation set -- every tensor with ||g64_t|| < 1e-3 G, G the L2 norm of all fp64 gradients: the biases
  that the next normalisation removes (exactly zero gradient) and insnorm.bias (almost invariant under the soft
  NMS) -- holds conv.bias, conv_ori.bias, both blocks' banch2.4.bias and insnorm.bias, and the reference's fp32
  values there are within 1e-5 G of fp64 (L2 norm of each tensor's difference).
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_detect_golden as MD  # noqa: E402  (reference_namespace, seeded_detector, DET_ARGS)

SEED = 2053
B, H, W = 2, 61, 83
NORM_FLOOR = 0.05
CANCEL_REL = 1e-3
MUST_CANCEL = ("conv.bias", "conv_ori.bias", "features.1.banch2.4.bias", "features.2.banch2.4.bias", "insnorm.bias")


def seeded(ns, dtype):
    MD.SEED = SEED  # seeded_detector reads the module's seed
    det = MD.seeded_detector(ns).train()
    return det.double() if dtype == torch.float64 else det


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def step(det, images, gs, go):
    score, scale, ori = det(images)
    assert float((scale.detach() - 32.0).abs().max()) < 1e-6  # 32 / (1 + 1e-8): exactly 32 in fp32 only
    ((score[..., 0] * gs).sum() + (ori * go).sum()).backward()
    sd = det.state_dict()
    stats = [v for k, v in sd.items() if k.endswith("running_mean") or k.endswith("running_var")]
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    return score.detach()[..., 0], ori.detach(), [p.grad for _, p in det.named_parameters()], stats


def main():
    ns = MD.reference_namespace()
    det32, det64 = seeded(ns, torch.float32), seeded(ns, torch.float64)
    sd = det32.state_dict()
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    assert len(keys) == 40
    blob = flat([sd[k] for k in keys]).numpy().astype(np.float32)
    param_names = [k for k, _ in det32.named_parameters()]
    stat_names = [k for k in keys if k.endswith("running_mean") or k.endswith("running_var")]
    images = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(SEED + 2))
    g = torch.Generator().manual_seed(SEED + 3)
    gs, go = torch.randn(B, H, W, generator=g), torch.randn(B, H, W, 2, generator=g)

    probe = copy.deepcopy(det64)  # the pre-division pair norm (a forward of its own: it moves running statistics)
    with torch.no_grad():
        pair_norm = probe.insnorm_ori(probe.conv_ori(probe.features(images.double()))).norm(p=2, dim=1)
    s32, o32, g32, r32 = step(det32, images, gs, go)
    s64, o64, g64, r64 = step(det64, images.double(), gs.double(), go.double())

    e_score = float((s32.double() - s64).abs().max())
    assert 0.0 < e_score < 1e-4, e_score
    excluded = pair_norm < NORM_FLOOR
    share = float(excluded.double().mean())
    assert share <= 0.01, share
    d_ori = (o32.double() - o64).abs().amax(dim=-1)
    e_ori = float(d_ori[~excluded].max())
    assert 0.0 < e_ori < 1e-3, e_ori

    G = float(flat(g64).norm())
    err_t = [float((a.double() - b).norm()) for a, b in zip(g32, g64)]
    norm_t = [float(b.norm()) for b in g64]
    grad_rel = float(np.sqrt(sum(e * e for e in err_t))) / G
    assert grad_rel < 1e-3, grad_rel
    cancel = [k for k, n in zip(param_names, norm_t) if n < CANCEL_REL * G]
    assert set(MUST_CANCEL) <= set(cancel), cancel
    cancel_err = max(e for k, e in zip(param_names, err_t) if k in cancel) / G
    assert cancel_err <= 1e-5, cancel_err
    worst_outside = max(e / n for k, e, n in zip(param_names, err_t, norm_t) if k not in cancel)
    stats_rel = max(float(((a.double() - b).abs() / b.abs().clamp_min(1e-30)).max()) for a, b in zip(r32, r64))

    def diff(a64, a32):
        d = (a64 - a32.double()).float()
        assert float((a32.double() + d.double() - a64).abs().max()) <= 1e-7 * float(a64.abs().max()) + 1e-30
        return d

    meta = {"source": "FDLNet-master/latency/NASNet model/det.py in train(), one backward; fp32 and fp64 on the CPU",
            "seed": SEED, "B": B, "H": H, "W": W, "det_args": MD.DET_ARGS, "state_dict_keys": keys,
            "param_names": param_names, "param_numel": [int(p.numel()) for p in g32], "stat_names": stat_names,
            "stat_numel": [int(v.numel()) for v in r32], "E_score": e_score, "E_ori": e_ori,
            "ori_norm_floor": NORM_FLOOR, "ori_excluded_share": share, "grad_norm_G": G,
            "grad_rel_fp32_vs_fp64": grad_rel, "cancel_rel": CANCEL_REL, "cancellation_set": cancel,
            "cancellation_err_over_G": cancel_err, "worst_rel_outside_cancellation": worst_outside,
            "running_stats_rel_fp32_vs_fp64": stats_rel,
            "bn_eps": 1e-5, "in_eps": 1e-5, "momentum": 0.1}
    out = {"blob": blob, "images": images.numpy(), "Gs": gs.numpy(), "Go": go.numpy(),
           "score32": s32.numpy(), "ori32": o32.numpy(),
           "score64_minus_score32": diff(s64, s32).numpy(), "ori64_minus_ori32": diff(o64, o32).numpy(),
           "ori_excluded": excluded.numpy(),
           "grad32": flat(g32).numpy(), "grad64_minus_grad32": diff(flat(g64), flat(g32)).numpy(),
           "stats32": flat(r32).numpy(), "stats64_minus_stats32": diff(flat(r64), flat(r32)).numpy(),
           "meta": json.dumps(meta)}
    path = os.path.join(HERE, "det_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps({k: v for k, v in meta.items() if k not in ("state_dict_keys", "param_names", "param_numel",
                                                                  "stat_names", "stat_numel")}, indent=1))


if __name__ == "__main__":
    main()
