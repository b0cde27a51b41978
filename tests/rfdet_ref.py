"""Helpers of the RF-Net detector tests (tests/test_rfdet.py, tests/test_gpu_rfdet.py) and of the fixture generator
tests/golden/make_rfdet_golden.py: the detector's configuration, the seeded weight distributions, the fixture loader
and the orientation exclusion rule."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
RF_LEVELS = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21)
SCALE_LIST = [3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0, 17.0, 19.0, 21.0]  # rfnet/config.py:62
K = 16
# rfnet/config.py's values but for topk
DET_ARGS = dict(score_com_strength=100.0, scale_com_strength=100.0, nms_thresh=0.0, nms_ksize=5, topk=K,
                gauss_ksize=15, gauss_sigma=0.5, ksize=3, padding=1, dilation=1, scale_list=SCALE_LIST)
NORM_FLOOR = 0.05
MARGIN = 4.0  # the project's margin for another fp32 evaluation order


from hardnetnas_amd.detector import randomise_rfdet_ as randomise_  # noqa: E402  (shared with tools/bench_rfdet.py)


def random_rfdet(seed, **over):
    """A seeded RFDetSO of this package.  The constructor runs under ``torch.manual_seed(seed)`` too: the conv
    biases keep their constructor values (weights_init's xavier_uniform_ does not apply to a 1-D tensor)."""
    from hardnetnas_amd.detector import RFDetSO
    torch.manual_seed(seed)
    return randomise_(RFDetSO(**{**DET_ARGS, **over}), seed)


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "rfdet.npz"))
    fx = {k: z[k] for k in z.files if k != "meta"}
    fx["meta"] = json.loads(str(z["meta"]))
    return fx


def fixture_detector(fx, dtype=torch.float32):
    """This package's RFDetSO with the fixture's weights (strict load, the reference's key order)."""
    from hardnetnas_amd.detector import RFDetSO
    det = RFDetSO(**fx["meta"]["det_args"])
    ref = det.state_dict()
    keys = fx["meta"]["state_dict_keys"]
    sd, o = {}, 0
    for k in keys:
        n = ref[k].numel()
        sd[k] = torch.from_numpy(fx["blob"][o:o + n].copy()).view(ref[k].shape)
        o += n
    assert o == fx["blob"].size
    det.load_state_dict(sd, strict=True)
    det = det.eval()
    if dtype == torch.float64:
        det = det.double()
        det.scale_list = det.scale_list.double()
    return det


def ori_min_norm(det, x):
    """[B,H,W]: the smallest of the ten per-level pre-division orientation norms and the final one, in the dtype of
    ``x``, from ``det``'s torch layers.  Where it is small the division amplifies any error without bound."""
    from hardnetnas_amd import detector as D
    feat, scores, orints, mn = x, [], [], None
    for k, rf in enumerate(RF_LEVELS, start=1):
        h = F.leaky_relu(getattr(det, f"insnorm{k}")(getattr(det, f"conv{k}")(feat)))
        scores.append(getattr(det, f"insnorm_s{rf}")(getattr(det, f"conv_s{rf}")(h)).permute(0, 2, 3, 1))
        o = getattr(det, f"conv_o{rf}")(h)
        nrm = o.norm(p=2, dim=1)
        mn = nrm if mn is None else torch.minimum(mn, nrm)
        orints.append((o / nrm.unsqueeze(1)).permute(0, 2, 3, 1).unsqueeze(-2))
        feat = h if k == 1 else h + feat
    p = D.soft_nms_3d(torch.cat(scores, -1), D.SOFT_NMS_KSIZE, D.RF_SOFT_NMS_STRENGTH)
    e1 = torch.exp(det.score_com_strength * (p - p.max(dim=-1, keepdim=True)[0]))
    s1 = e1 / (e1.sum(dim=-1, keepdim=True) + 1e-8)
    final = (torch.cat(orints, -2) * s1.unsqueeze(-1)).sum(dim=-2).norm(p=2, dim=-1)
    return torch.minimum(mn, final)


def reference_errors(det32, images):
    """The fp32 torch module's own error against its fp64 form on ``images`` (CPU fp32 [B,1,H,W]):
    ``(score64 [B,H,W], scale64, ori64 [B,H,W,2], excluded [B,H,W] bool, E_score, E_scale, E_ori)``."""
    import copy
    det64 = copy.deepcopy(det32).double()
    det64.scale_list = det64.scale_list.double()
    with torch.no_grad():
        s32, c32, o32 = det32(images)
        s64, c64, o64 = det64(images.double())
        excluded = ori_min_norm(det64, images.double()) < NORM_FLOOR
    s64, c64, o64 = s64.squeeze(-1), c64.squeeze(-1), o64.squeeze(-2)
    e_score = float((s32.squeeze(-1).double() - s64).abs().max())
    e_scale = float((c32.squeeze(-1).double() - c64).abs().max())
    d = (o32.squeeze(-2).double() - o64).abs().amax(dim=-1)
    e_ori = float(d[~excluded].max()) if (~excluded).any() else 0.0
    return s64, c64, o64, excluded, e_score, e_scale, e_ori
