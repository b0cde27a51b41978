"""Nearest / second-nearest descriptor matching: the fused matcher (_native.match_nn2) against the torch
formulation of FDLNet's evaluation (matching.distance_matrix_vector + sort, eval_utils.py:168-171), timed with
hipEvents after warm-up, median of --reps, at FDLNet's eval size (512 x 512) and at 16,384 x 16,384.
Run it on an otherwise idle GPU.  Prints one JSON line.

"bf16x3_peak_fraction" prices the matcher's whole call (split, selection, rescoring) as its selection GEMM
(algorithmic flop = 2 * N * M * 128) against the bf16x3 peak, --peak-tflops / 3 (three bf16 MFMA products per
multiply-add), as bench.py prices the forward kernels."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd._native import match_nn2, match_workspace_bytes  # noqa: E402
from hardnetnas_amd.matching import distance_matrix_vector  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512x512,16384x16384")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense bf16 MFMA peak of the device")
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


out = {"config": "match_nn2 vs distance_matrix_vector + sort", "reps": args.reps, "sizes": {}}
for size in args.sizes.split(","):
    n, m = (int(v) for v in size.split("x"))
    g = torch.Generator(device=dev).manual_seed(n + m)
    q = torch.nn.functional.normalize(torch.randn(n, 128, device=dev, generator=g), dim=1)
    db = torch.nn.functional.normalize(torch.randn(m, 128, device=dev, generator=g), dim=1)
    ws = torch.empty(match_workspace_bytes(n, m), dtype=torch.uint8, device=dev)
    fused = timed(lambda: match_nn2(q, db, "unit", workspace=ws))
    torch_ms = timed(lambda: distance_matrix_vector(q, db).sort(dim=-1))
    dist, idx = match_nn2(q, db, "unit", workspace=ws)
    srt, ind = distance_matrix_vector(q, db).sort(dim=-1)
    tflops = 2.0 * n * m * 128 / (fused * 1e-3) / 1e12
    out["sizes"][size] = {"match_nn2_ms": round(fused, 4), "torch_ms": round(torch_ms, 4),
                          "speedup": round(torch_ms / fused, 2),
                          "tflops": round(tflops, 2),
                          "bf16x3_peak_fraction": round(tflops / (args.peak_tflops / 3), 4),
                          "nearest_index_agreement": round((idx[:, 0].long() == ind[:, 0]).float().mean().item(), 6),
                          "max_abs_dist_diff": float((dist - srt[:, :2]).abs().max())}
print(json.dumps(out))
