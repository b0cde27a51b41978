"""End-time spread of the persistent HardNet forward kernels at one full launch (65,536 patches by default):
k_c12s, conv3, conv4 and conv5 from the stamped builds of the experiments library (HN_C12_ABL=64; HN_VARIANT
digits r r r: lane 0 of wave 0 stamps each workgroup's start and end in the 100 MHz clock, past the workspace).
Prints, per kernel, min / median / max of the workgroups' end times after the launch's first start, and the idle
share (max - mean) / max: the CU time the launch leaves unused while it waits for its slowest workgroup.
HN_STATIC_TILES=1 in the environment gives the static tile assignment (the "before" of the claimed tiles).
usage (MI355X): HN_LIB=abl/libhardnet_mi355x.so python tools/tail_timeline.py [patches] [out.json]"""
import json
import os
import sys

os.environ.setdefault("HN_C12_ABL", "64")
os.environ.setdefault("HN_C12_CFG", "15")
os.environ.setdefault("HN_VARIANT", "605rrr")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from hardnetnas_amd._native import NativeModel  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
dev = torch.device("cuda:0")
nm = NativeModel.from_module(bench.build_model("hardnet"), dev)
x = bench.synth_input_on_device(P, dev, 5)
nwg = torch.cuda.get_device_properties(dev).multi_processor_count
C12 = nwg * 8 * 1024  # k_c12s's stamps: 1 KiB per wave
base = nm.workspace_bytes(P)
assert base == P * 40960 * 4, "the stamp addresses assume one full chunk's workspace layout"
ws = torch.zeros(base + C12 + 64 * 1024, dtype=torch.uint8, device=dev)
out = torch.empty((P, 128), device=dev)
for _ in range(3):
    nm.forward(x, out=out, workspace=ws)
torch.cuda.synchronize()

res = {"patches": P, "workgroups": nwg, "static_tiles": os.environ.get("HN_STATIC_TILES", "0")}


def report(name, start, end):
    """start / end: per-workgroup stamps in microseconds"""
    ok = (start > 0) & (end > 0)
    start, end = start[ok], end[ok]
    t0 = start.min()
    e = end - t0
    idle = (e.max() - e.mean()) / e.max()
    res[name] = {"workgroups": int(ok.sum()), "start_max_us": float((start - t0).max()), "end_min_us": float(e.min()),
                 "end_median_us": float(np.median(e)), "end_max_us": float(e.max()), "idle_share": float(idle)}
    print(f"{name:6s} {ok.sum():4d} workgroups, last start {(start - t0).max():7.1f} us; end min {e.min():8.1f}  "
          f"median {np.median(e):8.1f}  max {e.max():8.1f} us; idle share {100 * idle:5.2f} %")


raw = ws[base: base + C12].view(torch.int64).cpu().numpy().reshape(nwg, 8, 128)
rt = raw[:, :, 120:122].astype(np.float64) / 100.0  # 100 MHz -> microseconds
st = np.where(rt[..., 0] > 0, rt[..., 0], np.inf).min(axis=1)
report("k_c12s", np.where(np.isfinite(st), st, 0.0), rt[..., 1].max(axis=1))
tail = ws[base + C12: base + C12 + 64 * 1024].view(torch.int64).cpu().numpy().astype(np.float64) / 100.0
for i, name in enumerate(("conv3", "conv4", "conv5")):
    s = tail[1024 * i: 1024 * i + 2 * nwg].reshape(nwg, 2)
    report(name, s[:, 0], s[:, 1])
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(res, f, indent=1)
