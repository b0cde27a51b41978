"""The homography ground-truth stage: each new call (hn_warp_score, hn_gt_scale_orin, hn_mask_keypoints,
hn_project_keypoints) and the whole no-grad ``Network.forward`` + ``criterion`` against this package's torch
formulation of the same steps on the same device, timed with hipEvents after warm-up, median of --reps, at the
reference's training shape (batch 1, 240 x 320, TOPK 512; config.py) and at 8 images of 480 x 640.  Images are uniform
noise, the weights seeded, the homographies drawn as the test fixture's.  Run it on an otherwise idle GPU.  Prints
one JSON line and writes it to --out.

The torch side is ``network``'s own torch paths with every native dispatch switched off for the measurement (the
``_hip32`` / ``_native_ok`` predicates patched to False, ``forward_torch`` for the detector, the descriptor's layers,
``loss_neimask(fused=False)``): what a port of the reference's train.py validation step would run.  "launches" is
the number of GPU kernels of one native ``forward`` as the torch profiler counts them (null if it cannot)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gt_helpers as G  # noqa: E402
from hardnetnas_amd import _native, losses, patches  # noqa: E402
from hardnetnas_amd import detector as D  # noqa: E402
from hardnetnas_amd import network as NW  # noqa: E402
from hardnetnas_amd.model import HardNetNeiMask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1x240x320,8x480x640", help="images x height x width")
ap.add_argument("--topk", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


class TorchDet:
    """The detector's torch layers and torch selection behind the detector's interface."""

    def __init__(self, det):
        self.det, self.TOPK, self.loss = det, det.TOPK, det.loss

    def __call__(self, x):
        return self.det.forward_torch(x)

    def process(self, s):
        _, _, _, _, q, mask, v = D.select_keypoints_torch(s.squeeze(-1), *self.det._select_args())
        return q.unsqueeze(-1), mask.unsqueeze(-1), v.unsqueeze(-1)


class TorchDes:
    def __init__(self, des):
        self.des = des

    def __call__(self, x):
        y = self.des.features(self.des.input_norm(x))
        y = y.view(y.size(0), -1)
        return y / torch.norm(y, p=2, dim=-1, keepdim=True)

    def loss(self, a, p, akp, pkp):
        return losses.loss_neimask(a, p, akp, pkp, margin=self.des.MARGIN, C=self.des.C, fused=False)


class torch_paths:
    """Every native dispatch of network.py and patches.py off inside the block."""

    def __enter__(self):
        self.saved = (NW._hip32, patches._native_ok)
        NW._hip32 = lambda *a: False
        patches._native_ok = lambda *a: False

    def __exit__(self, *a):
        NW._hip32, patches._native_ok = self.saved


def kernel_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None
                and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:
        return None


torch.manual_seed(1)
det = D.RFDet(100.0, 100.0, 0.0, 5, args.topk, 15, 0.5).eval().to(dev)
des = HardNetNeiMask(variant="NASNet").eval().to(dev)
net = NW.Network(det, des, 1000.0, 1.0, 32, args.topk).eval()
tnet = NW.Network(TorchDet(det), TorchDes(des), 1000.0, 1.0, 32, args.topk)
out = {"config": "homography ground-truth stage: native calls and Network.forward + criterion vs the torch "
                 "formulation on the same GPU", "topk": args.topk, "reps": args.reps, "sizes": {}}
with torch.no_grad():
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        K = args.topk
        gen = torch.Generator(device=dev).manual_seed(B * H)
        im1 = torch.rand(B, 1, H, W, device=dev, generator=gen)
        im2 = torch.rand(B, 1, H, W, device=dev, generator=gen)
        info = torch.ones(B, 2, device=dev)
        h12_np, h21_np = G.homographies(H, W, G.drawn_motions(B, 77))
        h12, h21 = torch.from_numpy(h12_np).float().to(dev), torch.from_numpy(h21_np).float().to(dev)
        batch = (im1, info, h12, im2, info, h21, im1, im2)
        score, ori = det.forward_maps(im2)
        score4, scale4 = score.unsqueeze(-1), torch.full((B, H, W, 1), 32.0, device=dev)
        mask = _native.select_keypoints(_native.warp_score(score, h12)[0], *det._select_args(), dense=True)["topk_mask"]
        kpts = _native.mask_keypoints(mask, K, ori_map=ori)[0]
        r = {}
        r["warp_score_ms"] = timed(lambda: _native.warp_score(score, h12, border=8))
        r["gt_scale_orin_ms"] = timed(lambda: _native.gt_scale_orin(None, ori, h12, h21, scale_value=32.0))
        r["mask_keypoints_ms"] = timed(lambda: _native.mask_keypoints(mask, K, ori_map=ori))
        r["project_keypoints_ms"] = timed(lambda: _native.project_keypoints(kpts, h12, (B, H, W), ori_map=ori))
        assert net._native_ok(batch)
        r["forward_ms"] = timed(lambda: net(batch))
        r["forward_criterion_ms"] = timed(lambda: net.criterion(net(batch)))
        r["forward_launches"] = kernel_launches(lambda: net(batch))
        with torch_paths():
            r["torch_warp_score_ms"] = timed(lambda: (NW.warp(NW.filter_border(score4), h12),
                                                      NW.warp(torch.ones_like(score4), h12)))
            r["torch_gt_scale_orin_ms"] = timed(lambda: NW.gt_scale_orin(scale4, ori, h12, h21))
            r["torch_mask_keypoints_ms"] = timed(lambda: NW._mask_keypoints(mask.unsqueeze(-1), scale4, ori, None))
            r["torch_project_keypoints_ms"] = timed(lambda: NW.ptCltoCr(kpts, h12, scale4, ori))
            r["torch_forward_ms"] = timed(lambda: tnet(batch))
            r["torch_forward_criterion_ms"] = timed(lambda: tnet.criterion(tnet(batch)))
            r["torch_forward_launches"] = kernel_launches(lambda: tnet(batch))
            t_end = tnet(batch)
        n_end = net(batch)
        r = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        for k in ("warp_score", "gt_scale_orin", "mask_keypoints", "project_keypoints", "forward", "forward_criterion"):
            r["speedup_" + k] = round(r["torch_" + k + "_ms"] / r[k + "_ms"], 1)
        r["max_abs_visible_diff_vs_torch"] = float((n_end["im1_visible"] - t_end["im1_visible"]).abs().max())
        r["limc_rows_shared_with_torch"] = len({tuple(x) for x in n_end["im1_limc"].tolist()}
                                               & {tuple(x) for x in t_end["im1_limc"].tolist()})
        r["limc_rows"] = int(n_end["im1_limc"].shape[0])
        out["sizes"][size] = r
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
