"""Keypoint patch extraction: the kernel (_native.clip_patch) against the torch formulation of
hardnetnas_amd/patches.py on the same device, and NativeModel.forward_keypoints against clip_patch + forward for
FDLNet's HardNetNeiMask("NASNet") and the stock HardNet, timed with hipEvents after warm-up, median of --reps, at
FDLNet's own size (2 images of 720 x 960, 512 keypoints each) and at 65,536 keypoints on 8 such images.  Scales
are uniform in [4, 64] raw pixels with random orientations.  Run it on an otherwise idle GPU.  Prints one JSON line.

"hbm_fraction" prices the kernel by the bytes it must write (4 KiB per patch; its gathered reads are served by
the caches) against --hbm-gbs, the HBM rate the project uses as achievable.  "clip_share" is the
"clip" stage's share of forward_keypoints from hn_stage_times."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd import _native  # noqa: E402
from hardnetnas_amd.model import HardNet, HardNetNeiMask  # noqa: E402
from hardnetnas_amd.patches import _clip_patch_torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2x512,8x8192", help="images x keypoints per image")
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=960)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--hbm-gbs", type=float, default=6300.0)
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


def footprint_bytes(kpts, scale, ori, H, W):
    """Mean bytes of distinct 128-byte image lines a patch's 4,096 neighbour reads touch (ratio 1)."""
    g = torch.linspace(-1, 1, 32, device=kpts.device)
    s = (scale / 2.0).view(-1, 1, 1)
    c, sn = ori[:, 0].view(-1, 1, 1), ori[:, 1].view(-1, 1, 1)
    x = s * c * g.view(1, 1, 32) - s * sn * g.view(1, 32, 1) + kpts[:, 2].float().view(-1, 1, 1)
    y = s * sn * g.view(1, 1, 32) + s * c * g.view(1, 32, 1) + kpts[:, 1].float().view(-1, 1, 1)
    x0, y0 = x.floor().long(), y.floor().long()
    lines = torch.stack([(yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)) // 32
                         for yy in (y0, y0 + 1) for xx in (x0, x0 + 1)], dim=1).flatten(1).sort(dim=1).values
    distinct = 1 + (lines[:, 1:] != lines[:, :-1]).sum(dim=1)
    return float(distinct.float().mean()) * 128.0


models = {"fdl_NASNet": HardNetNeiMask("NASNet").eval(), "hardnet": HardNet().eval()}
native = {k: _native.NativeModel.from_module(m, dev) for k, m in models.items()}
out = {"config": "clip_patch kernel vs torch formulation; forward_keypoints vs clip_patch + forward",
       "image": [args.height, args.width], "reps": args.reps, "hbm_gbs": args.hbm_gbs, "sizes": {}}
for size in args.sizes.split(","):
    B, per = (int(v) for v in size.split("x"))
    n = B * per
    g = torch.Generator(device=dev).manual_seed(n)
    images = torch.rand(B, 1, args.height, args.width, device=dev, generator=g)
    kpts = torch.zeros(n, 4, dtype=torch.int64, device=dev)
    kpts[:, 0] = torch.arange(n, device=dev) // per
    kpts[:, 1] = torch.randint(0, args.height, (n,), device=dev, generator=g)
    kpts[:, 2] = torch.randint(0, args.width, (n,), device=dev, generator=g)
    scale = 4.0 + 60.0 * torch.rand(n, device=dev, generator=g)
    ang = 6.283185307179586 * torch.rand(n, device=dev, generator=g)
    ori = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).contiguous()
    ratio = torch.ones(B, device=dev)
    im_info = torch.stack([ratio, ratio], dim=1)
    patches = torch.empty(n, 1, 32, 32, device=dev)
    kern = timed(lambda: _native.clip_patch(images, kpts, scale, ori, ratio, out=patches))
    with torch.no_grad():
        torch_ms = timed(lambda: _clip_patch_torch(kpts, scale, ori, im_info, images, 32))
        diff = float((_clip_patch_torch(kpts, scale, ori, im_info, images, 32) - patches).abs().max())
    gbs = n * 4096 / (kern * 1e-3) / 1e9
    gathered = footprint_bytes(kpts[:1024], scale[:1024], ori[:1024], args.height, args.width)
    row = {"keypoints": n, "clip_patch_ms": round(kern, 4), "torch_ms": round(torch_ms, 4),
           "speedup": round(torch_ms / kern, 1), "output_gbs": round(gbs, 1),
           "hbm_fraction": round(gbs / args.hbm_gbs, 4),
           "gathered_bytes_per_patch": round(gathered), "gathered_gbs": round(gbs * gathered / 4096, 1),
           "max_abs_diff_vs_torch": diff, "forward": {}}
    for name, nm in native.items():
        desc = torch.empty(n, 128, device=dev)
        ws = torch.empty(nm.workspace_bytes_kp(n), dtype=torch.uint8, device=dev)
        fused = timed(lambda: nm.forward_keypoints(images, kpts, scale, ori, ratio, out=desc, workspace=ws))
        apart = timed(lambda: nm.forward(_native.clip_patch(images, kpts, scale, ori, ratio, out=patches), out=desc,
                                         workspace=ws))
        nm.set_profiling(True)
        nm.forward_keypoints(images, kpts, scale, ori, ratio, out=desc, workspace=ws)
        torch.cuda.synchronize()
        st = nm.stage_times()
        nm.set_profiling(False)
        total = sum(v[0] for v in st.values())
        row["forward"][name] = {"forward_keypoints_ms": round(fused, 4), "clip_then_forward_ms": round(apart, 4),
                                "clip_stage_ms": round(st["clip"][0], 4),
                                "clip_share": round(st["clip"][0] / total, 4)}
        del ws
    out["sizes"][size] = row
print(json.dumps(out))
