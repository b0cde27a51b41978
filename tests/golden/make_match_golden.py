"""Generate tests/golden/fdl_match.npz from the REFERENCE matching code.

Run from the repo root:  python tests/golden/make_match_golden.py
Needs the reference tree (HN_REFERENCE, as make_golden.py; read-only, never copied): ``distance_matrix_vector`` /
``pairwise_distances``
(FDLNet-master/latency/NASNet/utils/math_utils.py:8-40) and the match-score functions of
utils/eval_utils.py:112-148, 168-197 are AST-extracted and executed on seeded inputs; only data
(inputs, the reference's intermediate and final results, JSON metadata) is written.

Inputs: 300 query and 257 database unit descriptors, 128 of the database rows noisy copies of queries
(normalize(q + 0.3 randn)) at permuted positions; integer keypoint rows (b, y, x, 0), the copies' keypoints
a few pixels from their query's warped keypoint; a ``visible`` mask with some false entries;
DES_THRSH = 1.0, COO_THRSH = 5.0.  A second database ("close/", copies at noise 0.05) is recorded
beside it, on which the thresholded and the ratio score predict matches.

The generator asserts that the reference alone is unambiguous on these inputs, so that an implementation
with another rounding must reproduce its indices and counts exactly: every row's fp64 gap between the best
and the second-best clamp argument >= 1e-4, every nn_value >= 1e-3 from DES_THRSH, every distance ratio
>= 1e-3 from 0.7, every coordinate distance >= 1e-3 from COO_THRSH.
"""
from __future__ import annotations

import ast
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HN_REFERENCE", "/root/reference")
UTILS = os.path.join(REF, "FDLNet-master", "latency", "NASNet", "utils")

SEED = 2024
N_QUERY, N_DB, N_COPY = 300, 257, 128
NOISE = 0.3
NOISE_CLOSE = 0.05
DES_THRSH, COO_THRSH, RATIO = 1.0, 5.0, 0.7
IMAGE_HW = 480


def _extract(path, names):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in keep} == set(names), (path, names)
    return ast.unparse(ast.Module(body=keep, type_ignores=[]))


def reference_functions():
    ns = {"torch": torch, "np": np}
    exec(_extract(os.path.join(UTILS, "math_utils.py"), ["distance_matrix_vector", "pairwise_distances"]), ns)
    exec(_extract(os.path.join(UTILS, "eval_utils.py"),
                  ["nearest_neighbor_match_score", "nearest_neighbor_threshold_match_score",
                   "nearest_neighbor_distance_ratio_match", "nearest_neighbor_distance_ratio_match_score"]), ns)
    return ns


def inputs(noise):
    g = torch.Generator().manual_seed(SEED)
    unit = torch.nn.functional.normalize
    des1 = unit(torch.randn(N_QUERY, 128, generator=g), dim=1)
    des2 = unit(torch.randn(N_DB, 128, generator=g), dim=1)
    src = torch.randperm(N_QUERY, generator=g)[:N_COPY]   # the copied queries ...
    dst = torch.randperm(N_DB, generator=g)[:N_COPY]      # ... and where their copies go
    des2[dst] = unit(des1[src] + noise * torch.randn(N_COPY, 128, generator=g), dim=1)
    kp1w = torch.zeros(N_QUERY, 4, dtype=torch.int64)
    kp1w[:, 1:3] = torch.randint(8, IMAGE_HW - 8, (N_QUERY, 2), generator=g)
    kp2 = torch.zeros(N_DB, 4, dtype=torch.int64)
    kp2[:, 1:3] = torch.randint(8, IMAGE_HW - 8, (N_DB, 2), generator=g)
    # a copy's keypoint: its query's warped keypoint moved by up to 6 pixels each way, so that some land
    # inside COO_THRSH and some outside; offsets at exactly COO_THRSH (3-4-5, 5-0) are drawn again
    off = torch.randint(-6, 7, (N_COPY, 2), generator=g)
    while True:
        bad = ((off.double() ** 2).sum(1).sqrt() - COO_THRSH).abs() < 1e-3
        if not bad.any():
            break
        off[bad] = torch.randint(-6, 7, (int(bad.sum()), 2), generator=g)
    kp2[dst, 1:3] = kp1w[src, 1:3] + off
    visible = torch.rand(N_QUERY, generator=g) > 0.15
    return des1, des2, kp1w, kp2, visible


def record(R, noise):
    """The reference's results on the inputs of one noise level, as (arrays, metadata)."""
    des1, des2, kp1w, kp2, visible = inputs(noise)
    dm = R["distance_matrix_vector"](des1, des2)
    nn_value, nn_idx = dm.min(dim=-1)
    ordered, indices = dm.sort(dim=-1)
    Da, Db, Ia = ordered[:, 0], ordered[:, 1], indices[:, 0]
    predict_label, _ = R["nearest_neighbor_distance_ratio_match"](des1, des2, kp2, RATIO)
    counts = (R["nearest_neighbor_match_score"](des1, des2, kp1w, kp2, visible, COO_THRSH)
              + R["nearest_neighbor_threshold_match_score"](des1, des2, kp1w, kp2, visible, DES_THRSH, COO_THRSH)
              + R["nearest_neighbor_distance_ratio_match_score"](des1, des2, kp1w, kp2, visible, COO_THRSH))

    # the reference alone is unambiguous here
    x32 = 2 - 2 * torch.mm(des1, des2.t())
    x64 = 2 - 2 * torch.mm(des1.double(), des2.double().t())
    e_ref = float((x32.double() - x64).abs().max())
    s64, i64 = x64.sort(dim=-1)
    gap = float((s64[:, 1] - s64[:, 0]).min())
    assert gap >= 1e-4, gap
    assert torch.equal(i64[:, 0], nn_idx) and torch.equal(i64[:, 0], Ia)
    thr_margin = float((nn_value.double() - DES_THRSH).abs().min())
    assert thr_margin >= 1e-3, thr_margin
    ratio_margin = float(((Da.double() / Db.double()) - RATIO).abs().min())
    assert ratio_margin >= 1e-3, ratio_margin
    coo = R["pairwise_distances"](kp1w[:, 1:3].float(), kp2[nn_idx][:, 1:3].float()).diag()
    coo_margin = float((coo.double() - COO_THRSH).abs().min())
    assert coo_margin >= 1e-3, coo_margin
    assert 0 < counts[0] < counts[1]

    meta = {"noise": noise,
            "counts": {"TPNN": counts[0], "PNN": counts[1], "TPNNT": counts[2], "PNNT": counts[3],
                       "TPNNDR": counts[4], "PNNDR": counts[5]},
            "E_ref": e_ref,
            "margins": {"clamp_argument_gap_fp64": gap, "DES_THRSH": thr_margin, "ratio": ratio_margin,
                        "COO_THRSH": coo_margin}}
    out = {"des1": des1.numpy(), "des2": des2.numpy(), "kp1w": kp1w.numpy(), "kp2": kp2.numpy(),
           "visible": visible.numpy(), "nn_value": nn_value.numpy(), "nn_idx": nn_idx.numpy(),
           "Da": Da.numpy(), "Db": Db.numpy(), "Ia": Ia.numpy(), "predict_label": predict_label.numpy()}
    return out, meta


def main():
    R = reference_functions()
    out, meta = record(R, NOISE)
    # a second database whose copies are close (noise 0.05): at NOISE every nearest distance lies above
    # DES_THRSH and every ratio above 0.7, so the thresholded and ratio scores predict nothing there;
    # here they do.  Same queries, keypoints and mask; only des2 and the results are stored again.
    close, close_meta = record(R, NOISE_CLOSE)
    assert all(np.array_equal(close[k], out[k]) for k in ("des1", "kp1w", "kp2", "visible"))
    assert 0 < close_meta["counts"]["TPNNT"] < close_meta["counts"]["PNNT"]
    assert 0 < close_meta["counts"]["TPNNDR"] < close_meta["counts"]["PNNDR"]
    out.update({"close/" + k: v for k, v in close.items() if k not in ("des1", "kp1w", "kp2", "visible")})
    meta.update({"source": "FDLNet-master/latency/NASNet/utils/eval_utils.py:112-148,168-197 over "
                           "math_utils.py:8-40, fp32 on the CPU",
                 "seed": SEED, "n_query": N_QUERY, "n_db": N_DB, "n_copy": N_COPY,
                 "DES_THRSH": DES_THRSH, "COO_THRSH": COO_THRSH, "ratio_threshold": RATIO, "close": close_meta})
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "fdl_match.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
