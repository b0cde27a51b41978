"""Forward + backward of the keypoint detector in train(): the native path (hn_det_train_forward / _backward through
DetTrainFunction) against the module's torch layers (RFDet.forward_torch) on the same GPU, and the whole training
step (Network.forward + criterion + det_loss.backward()) both ways.  Timed with hipEvents after warm-up, median of
--reps samples of --inner back-to-back calls.  Run it on an otherwise idle GPU.  Writes --out (default
profiles/det_train_bench.json) and prints it as one JSON line.

"detector": det(images) -> ((score * Gs).sum() + (ori * Go).sum()).backward() at every --shapes entry (BxHxW):
  native_ms / torch_ms      one step each way, autograd's bookkeeping included
  native_launches / torch_launches   GPU kernels of one step as torch.profiler counts them (null if it cannot)
  abi_launches              kernels the two C ABI calls launch themselves (19 forward + 30 backward)
"step": Network.forward + criterion + det_loss.backward() at the first shape with K = --topk keypoints, HardNetNeiMask
NASNet as the descriptor, a mild homography between two noise images:
  native_ms / torch_ms      with RFDet.forward as it dispatches / replaced by forward_torch."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd import network as NW  # noqa: E402
from hardnetnas_amd.detector import RFDet  # noqa: E402
from hardnetnas_amd.model import HardNetNeiMask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1x240x320,8x480x640")
ap.add_argument("--topk", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_train_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
ABI_LAUNCHES = {"forward": 19, "backward": 30}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.inner)
    return statistics.median(ms)


def launches(fn):
    """GPU kernels of one call, as torch.profiler sees them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # the profiler is a convenience here: the times do not depend on it
        print("launch count unavailable:", repr(e), file=sys.stderr)
        return None


def detector(topk):
    torch.manual_seed(0)
    det = RFDet(score_com_strength=100.0, scale_com_strength=100.0, nms_thresh=0.0, nms_ksize=5, topk=topk,
                gauss_ksize=15, gauss_sigma=0.5)
    det.apply(RFDet.weights_init)
    return det.to(dev).train()


out = {"config": "RFDet in train(): forward + backward, native (hn_det_train_*) vs torch layers on the same GPU",
       "reps": args.reps, "calls_per_sample": args.inner, "abi_launches": ABI_LAUNCHES, "detector": {}, "step": {}}
shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
for B, H, W in shapes:
    g = torch.Generator(device=dev).manual_seed(H + B)
    images = torch.rand(B, 1, H, W, device=dev, generator=g)
    gs, go = torch.randn(B, H, W, device=dev, generator=g), torch.randn(B, H, W, 2, device=dev, generator=g)
    det = detector(args.topk)

    def step(forward):
        det.zero_grad(set_to_none=True)
        score, _, ori = forward(images)
        ((score[..., 0] * gs).sum() + (ori * go).sum()).backward()
        return score

    assert "DetTrainFunction" in type(step(det).grad_fn).__name__
    native, torch_ms = timed(lambda: step(det)), timed(lambda: step(det.forward_torch))
    out["detector"][f"{B}x{H}x{W}"] = {
        "native_ms": round(native, 4), "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / native, 2),
        "native_launches": launches(lambda: step(det)), "torch_launches": launches(lambda: step(det.forward_torch))}

if not args.no_step:
    B, H, W = shapes[0]
    g = torch.Generator(device=dev).manual_seed(7)
    im1, im2 = torch.rand(B, 1, H, W, device=dev, generator=g), torch.rand(B, 1, H, W, device=dev, generator=g)
    h12 = torch.tensor([[1.0, 0.01, 2.0], [-0.01, 1.0, -1.5], [1e-5, 0.0, 1.0]], dtype=torch.float64)
    h21 = torch.linalg.inv(h12)
    info = torch.ones(B, 2, device=dev)
    batch = (im1, info, h12.float().to(dev).repeat(B, 1, 1), im2, info, h21.float().to(dev).repeat(B, 1, 1), im1, im2)
    torch.manual_seed(1)
    net = NW.Network(detector(args.topk), HardNetNeiMask(variant="NASNet"), 3.0, 1.0, 32, args.topk).to(dev).train()

    def train_step():
        net.zero_grad(set_to_none=True)
        _, det_loss, _ = net.criterion(net(batch))
        det_loss.backward()

    native = timed(train_step)
    net.det.forward = net.det.forward_torch
    torch_ms = timed(train_step)
    out["step"] = {"shape": [B, H, W], "topk": args.topk, "native_ms": round(native, 4), "torch_ms": round(torch_ms, 4),
                   "speedup": round(torch_ms / native, 3)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
