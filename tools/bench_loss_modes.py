"""loss_HardNet's batch reductions, forward plus backward with anchor_swap on: the HIP kernels ('average':
hn_loss_dense.hip, 'random' and -- for context -- 'min': hn_loss.hip) against this package's torch formulation of
the same loss (fused=False: the B x B matrix and autograd) on the same GPU, timed with hipEvents after warm-up,
median of --reps with the two forms alternating, at B = 512, 1,024 and 4,096.  'random' draws its permutation from
the CPU generator inside the timed region on both arms, as a training step does.  For 'average' the file also
states the FLOP of the MFMA products the kernels actually run (forward: the tile and its transpose; backward, in
each of its two passes: both again and the weight product; 2 * 64 * 64 * 128 FLOP per 64 x 64 tile each), the
share of the f32 peak (157.3 TF) that the whole forward + backward step reaches on them, and the peak device
memory each arm allocates above the inputs.  Run it on an otherwise idle GPU.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd.losses import loss_HardNet  # noqa: E402

F32_PEAK = 157.3e12
# kernel launches (and one memset node in the gather backward) of a native forward + backward, from the launch
# functions of hn_loss_dense.hip / hn_loss.hip with anchor_swap on
LAUNCHES = {"average": 3 + 2, "random": 3 + 6, "min": 4 + 6}

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512,1024,4096")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_loss_modes.py needs a GPU"
dev = torch.device("cuda:0")


def inputs(n):
    g = torch.Generator().manual_seed(n)
    unit = torch.nn.functional.normalize
    a = unit(torch.randn(n, 128, generator=g), dim=1)
    p = unit(a + 0.08 * torch.randn(n, 128, generator=g), dim=1)
    return a.to(dev).requires_grad_(True), p.to(dev).requires_grad_(True)


def step(a, p, reduce, fused):
    a.grad = p.grad = None
    loss = loss_HardNet(a, p, anchor_swap=True, batch_reduce=reduce, loss_type="triplet_margin", fused=fused)
    loss.backward()
    return loss


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


out = {"config": "loss_HardNet forward + backward, anchor_swap on, triplet_margin: HIP kernels vs the torch "
                 "formulation (fused=False) on the same GPU; hipEvents, median of reps, the two forms alternating",
       "reps": args.reps, "launches_native": LAUNCHES, "f32_peak_tflops": F32_PEAK / 1e12, "sizes": {}}
for n in (int(v) for v in args.sizes.split(",")):
    a, p = inputs(n)
    row = {}
    for reduce in ("average", "random", "min"):
        forms = {"native": lambda: step(a, p, reduce, True), "torch": lambda: step(a, p, reduce, False)}
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                ms[k].append(one(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {}
        for k, fn in forms.items():
            torch.manual_seed(1)
            loss = fn()
            res[k] = (loss.item(), torch.cat([a.grad, p.grad]).clone())
        r = {"native_ms": round(med["native"], 4), "torch_ms": round(med["torch"], 4),
             "native_ms_min_max": [round(min(ms["native"]), 4), round(max(ms["native"]), 4)],
             "torch_ms_min_max": [round(min(ms["torch"]), 4), round(max(ms["torch"]), 4)],
             "speedup": round(med["torch"] / med["native"], 2),
             "loss_abs_diff": abs(res["native"][0] - res["torch"][0]),
             "grad_l2_rel_diff": float((res["native"][1] - res["torch"][1]).norm() / res["torch"][1].norm())}
        if reduce == "average":
            tiles = -(-n // 64)
            flop = 8 * tiles * tiles * 2 * 64 * 64 * 128  # 2 products forward, 2 x 3 backward
            r["product_flop"] = flop
            r["f32_peak_share"] = round(flop / (med["native"] * 1e-3) / F32_PEAK, 4)
            r["native_peak_bytes"] = peak_bytes(forms["native"])
            r["torch_peak_bytes"] = peak_bytes(forms["torch"])
        row[reduce] = r
    out["sizes"][str(n)] = row
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
