"""Generate tests/golden/neimask_loss.npz from the REFERENCE neighbour-mask loss.

Run from the repo root:  python tests/golden/make_neimask_golden.py
Needs the reference tree (HN_REFERENCE, as make_golden.py; read-only, never copied): ``HardNetNeiMask.loss``
(FDLNet-master/latency/NASNet/model/des.py:57-96) and ``distance_matrix_vector`` / ``pairwise_distances``
(utils/math_utils.py:8-40) are AST-extracted and executed on seeded inputs in fp32 and fp64 on the CPU; only
data (inputs, the reference's loss, gradients and intermediate results, JSON metadata) is written.

Inputs (N = 200: three 64-row tiles and a remainder of 8), made so that the masks decide the result:
40 spatial clusters of 5 anchor keypoints within +-2 pixels of a centre in a 240 x 320 frame, the descriptors of
a cluster similar (normalize(centre + 0.5 unit noise)); positives normalize(a + 0.3 unit noise) with the
anchor's keypoint moved by up to +-3 pixels; rows permuted.  Two rows leave the unit sphere to reach the
distance's clamps: one anchor rescaled so that a_i.p_i = 1.5 (u = -1: the low clamp, pos_i = 1e-4, no gradient
through it) and one set to -1.6 p_j (u = 5.2: the high clamp).  Keypoints are drawn again while any pair of a
set lies at exactly C (the 3-4-5 and 5-0 offsets); the loss with either mask left out differs by >= 1e-3.  C = 5, MARGIN = 1; the loss at C = 0 is recorded too.
A second case ("all/", N = 8) has every keypoint within C of every other: every entry is masked, every
minimum exceeds 10, the loss and both gradients are exactly 0.

The generator asserts that the reference alone is unambiguous on these inputs and takes the next seed if it is
not, so that an implementation with another rounding must reproduce its selections: in fp64 every row's and
column's gap between the smallest and the second-smallest dn >= 1e-5, every |row min - column min| >= 1e-5,
every hinge argument >= 1e-5 from 0, every u_ij >= 1e-5 from both clamp bounds (the two hand-made entries
apart, which are far inside), no coordinate distance within 1e-3 of C, fp32 and fp64 argmins equal.  The fp32
rounding of D on these inputs is recorded as E_ref (1.6e-6 at its largest entry, the margins are 6 to 300 times
that), with the reference's own fp32-vs-fp64 error of the loss and of the gradients (L2-relative), from which the
tests take their tolerances.
"""
from __future__ import annotations

import ast
import json
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HN_REFERENCE", "/root/reference")
NASNET = os.path.join(REF, "FDLNet-master", "latency", "NASNet")

FIRST_SEED = 2025
N, CLUSTERS, PER = 200, 40, 5
FRAME_H, FRAME_W = 240, 320
MARGIN, C = 1.0, 5.0
GAP = 1e-5


def _functions(path, names, cls=None):
    body = ast.parse(open(path).read()).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    keep = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in keep} == set(names), (path, names)
    return ast.unparse(ast.Module(body=keep, type_ignores=[]))


def reference_functions():
    ns = {"torch": torch, "np": np}
    exec(_functions(os.path.join(NASNET, "utils", "math_utils.py"), ["distance_matrix_vector", "pairwise_distances"]),
         ns)
    exec(_functions(os.path.join(NASNET, "model", "des.py"), ["loss"], cls="HardNetNeiMask"), ns)
    return ns


def _place(g, base, reach, others):
    """base [2] moved by up to +-reach pixels each way, drawn again while it lies at exactly C of a row of others."""
    while True:
        kp = base + torch.randint(-reach, reach + 1, (2,), generator=g)
        if not len(others) or not (((torch.stack(others) - kp) ** 2).sum(1) == int(C * C)).any():
            return kp


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    unit = torch.nn.functional.normalize
    centre_d = unit(torch.randn(CLUSTERS, 128, generator=g), dim=1)
    centre_k = torch.stack([torch.randint(8, FRAME_H - 8, (CLUSTERS,), generator=g),
                            torch.randint(8, FRAME_W - 8, (CLUSTERS,), generator=g)], 1)
    which = torch.arange(N) // PER
    a = unit(centre_d[which] + 0.5 * unit(torch.randn(N, 128, generator=g), dim=1), dim=1)
    p = unit(a + 0.3 * unit(torch.randn(N, 128, generator=g), dim=1), dim=1)
    ak, pk = [], []
    for i in range(N):
        ak.append(_place(g, centre_k[which[i]], 2, ak))
        pk.append(_place(g, ak[-1], 3, pk))
    perm = torch.randperm(N, generator=g)
    a, p = a[perm].clone(), p[perm].clone()
    akp, pkp = torch.zeros(N, 4, dtype=torch.int64), torch.zeros(N, 4, dtype=torch.int64)
    akp[:, 1:3], pkp[:, 1:3] = torch.stack(ak)[perm], torch.stack(pk)[perm]
    akp[:, 0] = pkp[:, 0] = torch.arange(N) % 2  # the image index: present, not used by the loss
    lo, hi, hj = 17, 141, 66
    a[lo] *= 1.5 / float(a[lo] @ p[lo])  # a.p = 1.5: u = -1, the low clamp on the diagonal
    a[hi] = -1.6 * p[hj]                 # a.p = -1.6: u = 5.2, the high clamp at (hi, hj)
    return a, p, akp, pkp, (lo, hi, hj)


def masked(R, a, p, akp, pkp, c):
    """(D, dn) as des.py:68-87 builds them with the reference's two functions, in the dtype of a."""
    d = R["distance_matrix_vector"](a, p)
    dn = d + torch.eye(d.size(1)) * 10
    for kp in (akp, pkp):
        dn = dn + R["pairwise_distances"](kp[:, 1:3].to(torch.float), kp[:, 1:3].to(torch.float)).lt(c).to(torch.float) * 10
    return d, dn


def run(R, a, p, akp, pkp, c, dtype):
    a, p = a.clone().to(dtype).requires_grad_(True), p.clone().to(dtype).requires_grad_(True)
    loss = R["loss"](types.SimpleNamespace(MARGIN=MARGIN, C=c), a, p, akp, pkp)
    loss.backward()
    return loss.detach(), a.grad, p.grad


def record(R, seed):
    """The reference's results on one seed's inputs as (arrays, metadata), or the reason to take the next seed."""
    a, p, akp, pkp, (lo, hi, hj) = inputs(seed)
    l32, ga32, gp32 = run(R, a, p, akp, pkp, C, torch.float32)
    l64, ga64, gp64 = run(R, a, p, akp, pkp, C, torch.float64)
    l64_c0 = run(R, a, p, akp, pkp, 0.0, torch.float64)[0]
    d32, dn32 = masked(R, a, p, akp, pkp, C)
    d64, dn64 = masked(R, a.double(), p.double(), akp, pkp, C)
    # the restated dn is the reference's: it gives the reference's loss bit for bit
    mn32 = torch.min(dn32.min(1)[0], dn32.min(0)[0])
    assert torch.equal(torch.clamp(MARGIN + d32.diag() - mn32, min=0.0).mean(), l32)
    row, col = dn64.sort(dim=1), dn64.sort(dim=0)
    mn64 = torch.min(row[0][:, 0], col[0][0])
    margins = {
        "row_gap": float((row[0][:, 1] - row[0][:, 0]).min()), "col_gap": float((col[0][1] - col[0][0]).min()),
        "row_col_gap": float((row[0][:, 0] - col[0][0]).abs().min()),
        "hinge": float((MARGIN + d64.diag() - mn64).abs().min())}
    u = 2 - 2 * a.double() @ p.double().t()
    free = torch.ones(N, N, dtype=torch.bool)
    free[lo, lo] = free[hi, hj] = False
    margins["clamp"] = float(torch.minimum((u - 1e-8).abs(), (u - 4.0).abs())[free].min())
    assert u[lo, lo] < -0.9 and u[hi, hj] > 5.0 and d32[lo, lo] == torch.tensor(1e-8).sqrt() and d32[hi, hj] == 2.0
    assert ga64[lo].abs().max() > 0 and l64 > 0
    for k, v in margins.items():
        if v < GAP:
            return None, f"{k} margin {v:.2e}"
    coo = min(float((R["pairwise_distances"](kp[:, 1:3].double(), kp[:, 1:3].double()) - C).abs().min())
              for kp in (akp, pkp))
    assert coo >= 1e-3, coo
    margins["COO_THRSH"] = coo
    if not (torch.equal(dn32.argmin(1), row[1][:, 0]) and torch.equal(dn32.argmin(0), col[1][0])):
        return None, "fp32 and fp64 argmins differ"
    # the masks matter: most unmasked hardest negatives lie inside a mask, and each mask alone masks entries
    plain = d64 + torch.eye(N, dtype=torch.float64) * 10
    m1, m2 = (R["pairwise_distances"](kp[:, 1:3].float(), kp[:, 1:3].float()).lt(C) for kp in (akp, pkp))
    hardest_masked = int((m1 | m2)[torch.arange(N), plain.argmin(1)].sum())
    only1, only2 = int((m1 & ~m2).sum()), int((m2 & ~m1).sum())
    assert hardest_masked > N // 2 and only1 > 0 and only2 > 0, (hardest_masked, only1, only2)

    def loss_of(dn):  # each mask alone decides selected minima: leaving either out moves the loss by >= 1e-3
        return float(torch.clamp(MARGIN + d64.diag() - torch.min(dn.min(1)[0], dn.min(0)[0]), min=0.0).mean())
    alone = {"anchor_kp_mask_only": loss_of(plain + 10 * m1), "positive_kp_mask_only": loss_of(plain + 10 * m2)}
    assert abs(loss_of(plain + 10 * m1 + 10 * m2) - float(l64)) < 1e-12
    assert min(abs(v - float(l64)) for v in alone.values()) >= 1e-3, alone
    assert float(l64_c0) > 2 * float(l64)
    g64 = torch.cat([ga64, gp64])
    meta = {"seed": seed, "N": N, "MARGIN": MARGIN, "C": C, "low_clamp": [lo, lo], "high_clamp": [hi, hj],
            "E_ref": float((d32.double() - d64).abs().max()),
            "loss_err32": abs(float(l32) - float(l64)),
            "grad_err32": float((torch.cat([ga32, gp32]).double() - g64).norm() / g64.norm()),
            "margins": margins, "hardest_negative_masked_rows": hardest_masked,
            "masked_by_anchor_kp_only": only1, "masked_by_positive_kp_only": only2, "loss64_with": alone}
    out = {"a": a.numpy(), "p": p.numpy(), "akp": akp.numpy(), "pkp": pkp.numpy(),
           "loss32": l32.numpy(), "loss64": l64.numpy(), "loss64_C0": l64_c0.numpy(),
           "ga64": ga64.numpy().astype(np.float32), "gp64": gp64.numpy().astype(np.float32),
           "pos64": d64.diag().numpy(), "min_neg64": mn64.numpy(),
           "row_argmin": row[1][:, 0].numpy(), "col_argmin": col[1][0].numpy()}
    return (out, meta), None


def all_masked(R):
    g = torch.Generator().manual_seed(FIRST_SEED)
    unit = torch.nn.functional.normalize
    a = unit(torch.randn(8, 128, generator=g), dim=1)
    p = unit(a + 0.3 * unit(torch.randn(8, 128, generator=g), dim=1), dim=1)
    akp, pkp = torch.zeros(8, 4, dtype=torch.int64), torch.zeros(8, 4, dtype=torch.int64)
    akp[:, 1:3] = 100 + torch.randint(0, 3, (8, 2), generator=g)   # at most sqrt(8) apart
    pkp[:, 1:3] = 100 + torch.randint(0, 3, (8, 2), generator=g)
    l32, ga, gp = run(R, a, p, akp, pkp, C, torch.float32)
    assert float(l32) == 0.0 and not ga.any() and not gp.any()
    assert float(masked(R, a, p, akp, pkp, C)[1].min()) > 10
    return {"all/a": a.numpy(), "all/p": p.numpy(), "all/akp": akp.numpy(), "all/pkp": pkp.numpy()}


def main():
    R = reference_functions()
    seed, skipped = FIRST_SEED, []
    while True:
        got, why = record(R, seed)
        if got:
            break
        skipped.append({"seed": seed, "why": why})
        seed += 1
        assert seed < FIRST_SEED + 50
    out, meta = got
    out.update(all_masked(R))
    meta.update({"source": "FDLNet-master/latency/NASNet/model/des.py:57-96 over utils/math_utils.py:8-40, fp32 and "
                           "fp64 on the CPU", "skipped_seeds": skipped})
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "neimask_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
