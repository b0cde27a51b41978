"""Train-mode fixture for the row-segment buckets of the HIP train kernels, from the REFERENCE code
(survey container only, CPU).

Run from the repo root:  python tests/golden/make_train_bucket_golden.py
Writes tests/golden/train_buckets.npz (data only; the reference is executed, never copied).

The train kernels (hn_train.hip: fwd3 / fwd3s / fwd2 / dgrad2 / wgrad2 / wgrad3) pick 4, 2 or 1 row
segments per patch from batch x waves-per-patch at the thresholds 1,024 and 2,048; the other train
fixtures stop at 256 patches.  Here, for each batch size in BATCHES (one per bucket pattern, two of
them odd; tests/test_gpu_dispatch.py::test_train_gradients_in_every_row_segment_bucket has the table):

  * input   synth.synth_patches(B, seed) (seed and SHA-256 in meta);
  * model   ``torch.manual_seed(0); HardNet()`` -- the reference's class and weights_init, obtained as
            make_train_golden.py obtains them (AST-extracted, executed) -- in train(), dropout p = 0,
            BatchNorm momentum at its default;
  * step    one forward and the backward of the smooth objective of
            tests/test_gpu_train.py::test_smooth_loss_gradients_vs_fp64, ``(y * c).sum()``, with
            c = synth.normal(c_seed, B * 128) (regenerable anywhere; SHA-256 in meta).

Stored per B (keys ``b<B>/...``): N_ROWS strided output rows (first and last included) of the fp64 and
the fp32 run; the seven running means / variances after the step (fp32 run); the fp64 run's seven
weight gradients and its input gradient as fixtures.summary(cap=CAP); and ``fp32_err``, the fp32 run's
own L2-relative error against fp64 per gradient (order: GRAD_NAMES) -- the measure of what ReLU-kink
flips cost any fp32 implementation at this batch, which sets the bar of the GPU test.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_train_golden as T          # noqa: E402  (puts the repo root and tests/ on sys.path)
from hardnetnas_amd import synth       # noqa: E402
import fixtures as F                   # noqa: E402

BATCHES = (640, 1031, 2051)
X_SEED = {640: 61, 1031: 62, 2051: 63}
C_SEED = {640: 71, 1031: 72, 2051: 73}
N_ROWS = 64
CAP = 4096
GX_SEED = 100  # projection seed of the input gradient (weight gradient i uses i, as train_hardnet.npz)
GRAD_NAMES = [f"g{i}" for i in T.CONV_IDX] + ["gx"]


def _step(ns, x, c, dtype):
    torch.manual_seed(0)
    model = ns["HardNet"]().to(dtype).train()
    model.features[18].p = 0.0
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = model(xt)
    (y * torch.from_numpy(c).to(dtype)).sum().backward()
    r = {"y": y.detach().numpy(), "gx": xt.grad.numpy()}
    for i in T.BN_IDX:
        r[f"rm{i}"] = model.features[i].running_mean.numpy()
        r[f"rv{i}"] = model.features[i].running_var.numpy()
    for i in T.CONV_IDX:
        r[f"g{i}"] = model.features[i].weight.grad.numpy()
    return r


def main():
    ns = T._ref_ns()
    out = {}
    meta = {"batches": list(BATCHES), "n_rows": N_ROWS, "cap": CAP, "gx_seed": GX_SEED, "grad_names": GRAD_NAMES,
            "dropout_p": 0.0, "momentum": 0.1, "init": "torch.manual_seed(0); HardNet()",
            "objective": "(y * c).sum(), c = synth.normal(c_seed, B * 128) as float32 [B,128]",
            "source": "hardnet/HardNet.py:275-324 + Utils.py:15-22 (AST-extracted, executed with torch %s CPU)"
                      % torch.__version__}
    for b in BATCHES:
        x = synth.synth_patches(b, X_SEED[b])
        c = synth.normal(C_SEED[b], b * 128).astype(np.float32).reshape(b, 128)
        r32, r64 = _step(ns, x, c, torch.float32), _step(ns, x, c, torch.float64)
        rows = np.linspace(0, b - 1, N_ROWS).round().astype(np.int64)
        pre = f"b{b}/"
        out[pre + "rows"] = rows
        out[pre + "y_64"] = r64["y"][rows]
        out[pre + "y_32"] = r32["y"][rows].astype(np.float32)
        for i in T.BN_IDX:
            out[f"{pre}rm{i}_32"] = r32[f"rm{i}"].astype(np.float32)
            out[f"{pre}rv{i}_32"] = r32[f"rv{i}"].astype(np.float32)
        errs = []
        for k in GRAD_NAMES:
            g64 = r64[k]
            seed = GX_SEED if k == "gx" else int(k[1:])
            for kk, v in F.summary(g64, seed, CAP).items():
                out[f"{pre}{k}_{kk}"] = v
            errs.append(float(np.linalg.norm(r32[k].astype(np.float64) - g64) / np.linalg.norm(g64)))
        out[pre + "fp32_err"] = np.array(errs)
        meta[f"b{b}"] = {"x_seed": X_SEED[b], "x_sha256": synth.sha256_f32(x), "c_seed": C_SEED[b],
                         "c_sha256": synth.sha256_f32(c), "fp32_grad_l2rel_vs_fp64": dict(zip(GRAD_NAMES, errs))}
        print(b, "max|y32 - y64|", float(np.abs(r32["y"] - r64["y"]).max()), "fp32 grad errs",
              ["%.2e" % e for e in errs])
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "train_buckets.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("train_buckets.npz:", size, "bytes")
    assert size <= 1_000_000, size


if __name__ == "__main__":
    if not os.path.isdir(T.G.REF):
        sys.exit(f"{T.G.REF} not found: fixtures can only be regenerated in the survey container")
    torch.set_num_threads(8)
    main()
