"""FDLNet's neighbour-mask descriptor loss, forward plus backward: the fused kernels (losses.loss_neimask ->
_native.NeiMaskLossFunction, hn_neimask.hip) against the torch formulation of the same loss (fused=False: the
reference's three N x N matrices and autograd) on the same GPU, timed with hipEvents after warm-up, median of
--reps with the two forms alternating, at the reference's size (N = B * TOPK = 512) and at 4,096.  Inputs: the
clustered keypoints of tests/golden/make_neimask_golden.py scaled up (clusters of 5 within +-2 pixels, similar
descriptors, positives moved by up to +-3 pixels, 480 x 640 frame).  Run it on an otherwise idle GPU.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd.losses import loss_neimask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512,4096")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_neimask.py needs a GPU"
dev = torch.device("cuda:0")


def inputs(n):
    g = torch.Generator().manual_seed(n)
    unit = torch.nn.functional.normalize
    k, which = (n + 4) // 5, torch.arange(n) // 5
    cd = unit(torch.randn(k, 128, generator=g), dim=1)
    ck = torch.stack([torch.randint(8, 472, (k,), generator=g), torch.randint(8, 632, (k,), generator=g)], 1)
    a = unit(cd[which] + 0.5 * unit(torch.randn(n, 128, generator=g), dim=1), dim=1)
    p = unit(a + 0.3 * unit(torch.randn(n, 128, generator=g), dim=1), dim=1)
    akp, pkp = torch.zeros(n, 4, dtype=torch.int64), torch.zeros(n, 4, dtype=torch.int64)
    akp[:, 1:3] = ck[which] + torch.randint(-2, 3, (n, 2), generator=g)
    pkp[:, 1:3] = akp[:, 1:3] + torch.randint(-3, 4, (n, 2), generator=g)
    perm = torch.randperm(n, generator=g)
    return tuple(t[perm].contiguous().to(dev) for t in (a, p, akp, pkp))


def step(a, p, akp, pkp, fused):
    a.grad = p.grad = None
    loss = loss_neimask(a, p, akp, pkp, margin=1.0, C=5.0, fused=fused)
    loss.backward()
    return loss


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


out = {"config": "loss_neimask forward + backward, fused kernels vs the torch formulation (fused=False) on the "
                 "same GPU; hipEvents, median of reps, the two forms alternating", "reps": args.reps, "sizes": {}}
for n in (int(v) for v in args.sizes.split(",")):
    a, p, akp, pkp = inputs(n)
    a.requires_grad_(True)
    p.requires_grad_(True)
    forms = {"fused": lambda: step(a, p, akp, pkp, True), "torch": lambda: step(a, p, akp, pkp, False)}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, fn in forms.items():
            ms[k].append(one(fn))
    res = {}
    for k, fn in forms.items():
        loss = fn()
        res[k] = (loss.item(), torch.cat([a.grad, p.grad]).clone())
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["sizes"][str(n)] = {
        "fused_ms": round(med["fused"], 4), "torch_ms": round(med["torch"], 4),
        "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
        "torch_ms_min_max": [round(min(ms["torch"]), 4), round(max(ms["torch"]), 4)],
        "speedup": round(med["torch"] / med["fused"], 2),
        "loss": res["fused"][0], "loss_abs_diff": abs(res["fused"][0] - res["torch"][0]),
        "grad_l2_rel_diff": float((res["fused"][1] - res["torch"][1]).norm() / res["torch"][1].norm())}
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
