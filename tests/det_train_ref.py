"""Shared by the detector training-step tests: the fixture (tests/golden/det_train.npz, written by
tests/golden/make_det_train_golden.py from the reference), the step itself, and the bars every comparison uses.

The step is ``score, _, ori = det(images); ((score[..., 0] * Gs).sum() + (ori * Go).sum()).backward()`` with the
module in train().  A result is a dict: score [B,H,W], ori [B,H,W,2], grads {name: tensor}, stats {name: tensor}
(the running statistics after the step), nbt (the num_batches_tracked values) and node (the score's grad_fn name).

The bars (``check_step``), against an fp64 evaluation with E the fp32 torch layers' own error on the same case:
  score within 4 E_score, ori within 4 E_ori where the fp64 pre-division pair norm is >= 0.05 (the share of the
  excluded pixels at most 1 %); running statistics within 1e-5 of fp64, relative to the tensor's largest magnitude
  (per element a running mean that happens to sit near zero has no relative precision to speak of);
  all gradients together within 5e-3 L2-relative; every tensor outside the cancellation set (||g64_t|| < 1e-3 G, G
  the L2 norm of all fp64 gradients) within max(2e-2 ||g64_t||, 3 E_t), E_t = ||g32_t - g64_t||; every tensor
  inside it within 1e-4 G (L2 norm of the difference, which bounds every element).
"""
from functools import lru_cache

import numpy as np
import torch

from detect_ref import random_detector, state_dict_from_blob
from fixtures import load
from hardnetnas_amd.detector import RFDet

NORM_FLOOR = 0.05
CANCEL_REL = 1e-3


def _split(flat, names, numels):
    out, i = {}, 0
    for k, n in zip(names, numels):
        out[k] = flat[i:i + n]
        i += n
    assert i == flat.numel()
    return out


@lru_cache(maxsize=None)
def golden():
    """(tensors, meta, ref64, ref32): the fixture and the reference's step in fp64 / fp32 as result dicts."""
    fx = load("det_train")
    meta = fx["meta"]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in fx.items() if k != "meta"}

    def result(kind):
        def get(name):
            a = t[name + "32"].double()
            return a + t[f"{name}64_minus_{name}32"].double() if kind == 64 else a
        return {"score": get("score"), "ori": get("ori"),
                "grads": _split(get("grad"), meta["param_names"], meta["param_numel"]),
                "stats": _split(get("stats"), meta["stat_names"], meta["stat_numel"])}
    return t, meta, result(64), result(32)


def golden_detector():
    """A fresh RFDet in train() with the fixture's start state."""
    t, meta, _, _ = golden()
    det = RFDet(**meta["det_args"])
    det.load_state_dict(state_dict_from_blob(det, t["blob"]), strict=True)
    return det.train()


def contiguous_instance_norm_grads(det):
    """Make the gradient that reaches each InstanceNorm's output contiguous before torch's backward reads it.

    With one image, the gradient arriving through ``permute(0, 2, 3, 1)`` is a [1,C,H,W] view with channels-last
    strides, and torch's instance_norm backward on the CPU then returns a wrong input gradient for C = 2:
    ``torch.autograd.gradcheck`` of ``(instance_norm(x, w, b).permute(0, 2, 3, 1) * g).sum()`` in fp64 fails for
    x [1,2,5,5] and passes for [2,2,5,5], and a two-image batch of the same image twice gives twice the gradients of
    neither torch's one-image run.  The hook changes no value anywhere else; every torch reference step of these
    tests runs with it, so that one-image cases are compared against the mathematics and not against that fault.
    Returns the handles."""
    def hook(_module, _inputs, out):
        if out.requires_grad:
            out.register_hook(lambda g: g.contiguous())
    return [m.register_forward_hook(hook) for m in (det.insnorm, det.insnorm_ori)]


def run_step(det, images, gs, go, forward=None, use_score=True, use_ori=True):
    """One step on ``det`` (whatever its device / dtype); ``forward`` replaces ``det.__call__`` (e.g. forward_torch).
    The torch layers run with ``contiguous_instance_norm_grads``."""
    det.zero_grad(set_to_none=True)
    handles = contiguous_instance_norm_grads(det)
    score, _, ori = (forward or det)(images)
    for h in handles:
        h.remove()
    node = type(score.grad_fn).__name__
    loss = 0.0
    if use_score:
        loss = loss + (score[..., 0] * gs).sum()
    if use_ori:
        loss = loss + (ori * go).sum()
    loss.backward()
    sd = det.state_dict()
    return {"score": score.detach()[..., 0].double().cpu(), "ori": ori.detach().double().cpu(),
            "grads": {k: p.grad.detach().double().cpu().reshape(-1) for k, p in det.named_parameters()
                      if p.grad is not None},
            "stats": {k: v.detach().double().cpu().reshape(-1) for k, v in sd.items()
                      if k.endswith("running_mean") or k.endswith("running_var")},
            "nbt": [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")], "node": node}


def pair_norm64(det, images):
    """The orientation head's fp64 pre-division pair norm [B,H,W] in train() (on a copy: it moves running statistics)."""
    import copy
    d = copy.deepcopy(det).double().cpu().train()
    with torch.no_grad():
        return d.insnorm_ori(d.conv_ori(d.features(images.double().cpu()))).norm(p=2, dim=1)


@lru_cache(maxsize=None)
def torch_case(seed, b, h, w, const=False, use_score=True, use_ori=True):
    """A seeded case on the CPU: (state_dict, images, gs, go, ref64, ref32, excluded) with the module's own
    ``forward_torch`` in train() as the reference, in fp64 and (for E) in fp32.  Computed once, never changed."""
    det = random_detector(seed).train()
    sd = {k: v.clone() for k, v in det.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 7)
    images = torch.full((b, 1, h, w), 0.5) if const else torch.rand(b, 1, h, w, generator=g)
    gs, go = torch.randn(b, h, w, generator=g), torch.randn(b, h, w, 2, generator=g)
    excluded = pair_norm64(det, images) < NORM_FLOOR
    d64 = random_detector(seed).train().double()
    ref64 = run_step(d64, images.double(), gs.double(), go.double(), d64.forward_torch, use_score, use_ori)
    d32 = random_detector(seed).train()
    ref32 = run_step(d32, images, gs, go, d32.forward_torch, use_score, use_ori)
    return sd, images, gs, go, ref64, ref32, excluded


def check_step(res, ref64, ref32, excluded, label, e_score=None, e_ori=None, tiny=False, frozen=()):
    """Assert the module docstring's bars on ``res`` and print every measured value.  ``e_score`` / ``e_ori`` default
    to ref32's own errors.  ``tiny``: skip the per-tensor relative rule where E_t is 0 (a handful of pixels)."""
    out = {}
    share = float(excluded.double().mean())
    if e_score is None:
        e_score = float((ref32["score"] - ref64["score"]).abs().max())
    if e_ori is None:
        d = (ref32["ori"] - ref64["ori"]).abs().amax(dim=-1)
        e_ori = float(d[~excluded].max()) if (~excluded).any() else 0.0
    out["score_err"] = float((res["score"] - ref64["score"]).abs().max())
    d = (res["ori"] - ref64["ori"]).abs().amax(dim=-1)
    out["ori_err"] = float(d[~excluded].max()) if (~excluded).any() else 0.0
    out["stats_rel"] = max(float((res["stats"][k] - v).abs().max() / v.abs().max()) for k, v in ref64["stats"].items())
    names = [k for k in ref64["grads"] if k not in frozen]
    G = float(np.sqrt(sum(float(ref64["grads"][k].norm()) ** 2 for k in names)))
    err = {k: float((res["grads"][k] - ref64["grads"][k]).norm()) for k in names}
    out["grad_rel"] = float(np.sqrt(sum(e * e for e in err.values()))) / G
    cancel = [k for k in names if float(ref64["grads"][k].norm()) < CANCEL_REL * G]
    worst, where, worst_c, where_c = 0.0, "", 0.0, ""
    for k in names:
        n64 = float(ref64["grads"][k].norm())
        e_t = float((ref32["grads"][k] - ref64["grads"][k]).norm())
        if k in cancel:
            if err[k] / G > worst_c:
                worst_c, where_c = err[k] / G, k
            continue
        if tiny and e_t == 0.0:
            continue
        r = err[k] / max(2e-2 * n64, 3.0 * e_t)
        if r > worst:
            worst, where = r, k
    out.update(E_score=e_score, E_ori=e_ori, excluded_share=share, G=G, worst_tensor_over_bar=worst,
               worst_tensor=where, worst_cancel_over_G=worst_c, worst_cancel=where_c, cancel=len(cancel))
    print(label, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in out.items()})
    assert share <= 0.01, (label, share)
    assert out["score_err"] <= 4.0 * e_score, (label, out["score_err"], e_score)
    assert out["ori_err"] <= 4.0 * e_ori, (label, out["ori_err"], e_ori)
    assert out["stats_rel"] <= 1e-5, (label, out["stats_rel"])
    assert out["grad_rel"] <= 5e-3, (label, out["grad_rel"])
    assert worst <= 1.0, (label, where, worst)
    assert worst_c <= 1e-4, (label, where_c, worst_c)
    return out
