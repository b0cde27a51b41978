"""Shared by tests/test_detect.py and tests/test_gpu_detect.py: the detector fixture (tests/golden/detect.npz,
written by tests/golden/make_detect_golden.py from the reference) and the torch module loaded with its weights."""
from functools import lru_cache

import numpy as np
import torch

from fixtures import load
from hardnetnas_amd.detector import RFDet


@lru_cache(maxsize=None)
def golden():
    """(tensors, meta): score64 / ori64 restored from the stored fp32 differences."""
    fx = load("detect")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in fx.items() if k != "meta"}
    t["score64"] = t["score32"].double() + t["score64_minus_score32"].double()
    t["ori64"] = t["ori32"].double() + t["ori64_minus_ori32"].double()
    return t, fx["meta"]


def state_dict_from_blob(det, blob):
    """The blob's floats as a state_dict of ``det`` (state_dict order, num_batches_tracked kept as they are)."""
    sd, i = {}, 0
    for k, v in det.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
            continue
        n = v.numel()
        sd[k] = blob[i:i + n].view(v.shape).clone()
        i += n
    assert i == blob.numel()
    return sd


def golden_detector():
    t, meta = golden()
    det = RFDet(**meta["det_args"])
    det.load_state_dict(state_dict_from_blob(det, t["blob"]), strict=True)
    return det.eval()


def random_detector(seed, topk=64, **kw):
    """Seeded weights with every normalisation layer randomised away from its defaults."""
    args = dict(score_com_strength=100.0, scale_com_strength=100.0, nms_thresh=0.0, nms_ksize=5, topk=topk,
                gauss_ksize=15, gauss_sigma=0.5)
    args.update(kw)
    torch.manual_seed(seed)
    det = RFDet(**args)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in det.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d)):
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
    return det.eval()


def ori_pair_norm(det, images):
    """The orientation head's pre-division pair norm [B,H,W] (torch layers, dtype of ``images``)."""
    with torch.no_grad():
        return det.insnorm_ori(det.conv_ori(det.features(images))).norm(p=2, dim=1)
