"""Forward + backward of the keypoint patch extraction under autograd, and of des(clip_patch(...)) in train(): the
native path (hn_clip_patch + hn_clip_patch_backward; hn_nas_train_* / hn_hardnet_train_* with the input gradient)
against this package's torch formulation and torch layers on the same GPU.  Timed with hipEvents after warm-up, median
of --reps samples of --inner back-to-back calls.  Run it on an otherwise idle GPU.  Writes --out (default profiles/clip_grad_bench.json) and prints it as one
JSON line.

"clip": patches.clip_patch(...).backward(dout) with scale and orientation requiring grad, at --keypoints on every
--images size (B = 2 images, keypoints anywhere in them, scale uniform in [4, 64] raw pixels, random orientations):
  native_ms      ClipPatchFunction (two kernels plus autograd's bookkeeping)
  kernels_ms     the two kernels alone, into preallocated buffers
  torch_ms       patches._clip_patch_torch under autograd
"descriptor": des(clip_patch(...)).backward(v) in train() at --des-keypoints on the first image size, for
HardNetNeiMask NASNet / NASNet_0.1 and the stock HardNet:
  native_ms      both native functions
  torch_ms       the torch formulation of clip_patch and the module's torch layers (native_train = False)
  clip_share     kernels_ms of that size over native_ms: the two clip kernels' share of the native step
  des_only_ms    the native descriptor step on detached patches that require grad (forward + backward with the
                 input gradient), and des_no_dx_ms the same without the input gradient: their difference prices
                 the input-gradient kernel."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd import _native  # noqa: E402
from hardnetnas_amd import patches as PT  # noqa: E402
from hardnetnas_amd.model import HardNet, HardNetNeiMask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--keypoints", default="512,1024,4096")
ap.add_argument("--images", default="240x320,480x640")
ap.add_argument("--des-keypoints", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=10, help="calls per timed sample")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_grad_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
B = 2


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):  # a step is tens of microseconds to a few milliseconds: time several back to back
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.inner)
    return statistics.median(ms)


def inputs(n, H, W):
    g = torch.Generator(device=dev).manual_seed(n + H)
    images = torch.rand(B, 1, H, W, device=dev, generator=g)
    kpts = torch.zeros(n, 4, dtype=torch.int64, device=dev)
    kpts[:, 0] = torch.arange(n, device=dev) // ((n + B - 1) // B)
    kpts[:, 1] = torch.randint(0, H, (n,), device=dev, generator=g)
    kpts[:, 2] = torch.randint(0, W, (n,), device=dev, generator=g)
    scale = 4.0 + 60.0 * torch.rand(n, device=dev, generator=g)
    ang = 6.283185307179586 * torch.rand(n, device=dev, generator=g)
    ori = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).contiguous()
    ratio = torch.ones(B, device=dev)
    return images, kpts, scale, ori, ratio, torch.stack([ratio, ratio], dim=1)


def clip_step(clip, kpts, scale, ori, im_info, images, dout):
    sc, orr = scale.detach().requires_grad_(True), ori.detach().requires_grad_(True)
    clip(kpts, sc, orr, im_info, images, 32).backward(dout)
    return sc.grad, orr.grad


def kernels_ms(images, kpts, scale, ori, ratio, dout):
    n = kpts.shape[0]
    patches = torch.empty(n, 1, 32, 32, device=dev)
    ds, do = torch.empty(n, device=dev), torch.empty(n, 2, device=dev)

    def run():
        _native.clip_patch(images, kpts, scale, ori, ratio, out=patches)
        _native.clip_patch_backward(dout, images, kpts, scale, ori, ratio, out_scale=ds, out_ori=do)
    return timed(run)


out = {"config": "clip_patch forward + backward under autograd, native vs torch formulation; "
                 "des(clip_patch) train step, native vs torch layers",
       "images_per_call": B, "reps": args.reps, "calls_per_sample": args.inner, "clip": {}, "descriptor": {}}
sizes = [tuple(int(v) for v in s.split("x")) for s in args.images.split(",")]
for H, W in sizes:
    for n in (int(v) for v in args.keypoints.split(",")):
        images, kpts, scale, ori, ratio, im_info = inputs(n, H, W)
        dout = torch.randn(n, 1, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        native = timed(lambda: clip_step(PT.clip_patch, kpts, scale, ori, im_info, images, dout))
        torch_ms = timed(lambda: clip_step(PT._clip_patch_torch, kpts, scale, ori, im_info, images, dout))
        kern = kernels_ms(images, kpts, scale, ori, ratio, dout)
        gn = clip_step(PT.clip_patch, kpts, scale, ori, im_info, images, dout)
        gt = clip_step(PT._clip_patch_torch, kpts, scale, ori, im_info, images, dout)
        out["clip"][f"{H}x{W}/{n}"] = {
            "keypoints": n, "native_ms": round(native, 4), "kernels_ms": round(kern, 4), "torch_ms": round(torch_ms, 4),
            "speedup": round(torch_ms / native, 1),
            "max_abs_diff_vs_torch": {"d_scale": float((gn[0] - gt[0]).abs().max()),
                                      "d_ori": float((gn[1] - gt[1]).abs().max())},
            "max_abs_grad": {"d_scale": float(gt[0].abs().max()), "d_ori": float(gt[1].abs().max())}}

H, W = sizes[0]
n = args.des_keypoints
images, kpts, scale, ori, ratio, im_info = inputs(n, H, W)
dout = torch.randn(n, 1, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
v = torch.randn(n, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
kern = kernels_ms(images, kpts, scale, ori, ratio, dout)
models = {"fdl_NASNet": lambda: HardNetNeiMask(variant="NASNet"),
          "fdl_NASNet_01": lambda: HardNetNeiMask(variant="NASNet_0.1"), "hardnet": HardNet}
for name, make in models.items():
    torch.manual_seed(0)
    des = make().to(dev).train()

    def step(clip):
        des.zero_grad(set_to_none=True)
        sc, orr = scale.detach().requires_grad_(True), ori.detach().requires_grad_(True)
        des(clip(kpts, sc, orr, im_info, images, 32)).backward(v)

    def des_step(need_dx, x=_native.clip_patch(images, kpts, scale, ori, ratio)):
        des.zero_grad(set_to_none=True)
        des(x.detach().requires_grad_(need_dx)).backward(v)

    des.native_train = True
    native = timed(lambda: step(PT.clip_patch))
    des_dx = timed(lambda: des_step(True))
    des_no = timed(lambda: des_step(False))
    des.native_train = False
    torch_ms = timed(lambda: step(PT._clip_patch_torch))
    out["descriptor"][name] = {"keypoints": n, "image": [H, W], "native_ms": round(native, 4),
                               "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / native, 2),
                               "clip_kernels_ms": round(kern, 4), "clip_share": round(kern / native, 4),
                               "des_only_ms": round(des_dx, 4), "des_no_dx_ms": round(des_no, 4)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
