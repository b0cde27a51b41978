"""The fused nearest / second-nearest matcher (hn_match_nn2) on the MI355X against an fp64 brute force, its tie,
partition and bounds guarantees, and the drop-in match scores of hardnetnas_amd/matching.py against the
reference's recorded results (tests/golden/fdl_match.npz).

Tolerances.  The matcher SELECTS on key(i,j) = c_j - 2 a_i.b_j with the dot product in bf16x3 split precision.
With every key off by at most E, the picked first (second) row's true key exceeds the true first (second)
minimum by at most 2 E.  E_sel is the largest key error of a CPU emulation of the split on the test's own
inputs (hi = bf16(v), lo = bf16(v - hi), hi.hi + hi.lo + lo.hi summed in fp64); the MFMA's fp32 accumulation,
which the emulation leaves out, is two orders below it.  The reported VALUES are plain fp32: their sqrt / clamp
argument must lie within 4 E_ref of the fp64 one, E_ref being the reference formulation's own fp32-vs-fp64
error on the same inputs (both are fp32 roundings of the same 128-term sum in different orders).
"""
import ctypes

import numpy as np
import pytest
import torch

from fixtures import build_module, golden_inputs
from hardnetnas_amd import _native as N
from hardnetnas_amd import matching as MT
from test_match import COUNT_KEYS, match_case, six_counts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (31, 63), (33, 65), (129, 64), (257, 1000), (1000, 257), (64, 70001), (65537, 193)]


def _descriptors(n, m, seed, scale=1.0, vary=0.0):
    """n queries and m database rows: unit vectors, half of the smaller side copied into the database as noisy
    copies (normalize(q + 0.3 randn)) at permuted rows; then every row times ``scale`` (database rows times
    scale (1 + vary u), u uniform in [-1, 1])."""
    g = torch.Generator().manual_seed(seed)
    unit = torch.nn.functional.normalize
    q = unit(torch.randn(n, 128, generator=g), dim=1)
    db = unit(torch.randn(m, 128, generator=g), dim=1)
    k = min(n, m) // 2
    if k:
        src, dst = torch.randperm(n, generator=g)[:k], torch.randperm(m, generator=g)[:k]
        db[dst] = unit(q[src] + 0.3 * torch.randn(k, 128, generator=g), dim=1)
    rows = scale * (1 + vary * (2 * torch.rand(m, 1, generator=g) - 1))
    return (q * scale).contiguous(), (db * rows).contiguous()


def _split(v):
    hi = v.bfloat16().float()
    return hi.double(), (v - hi).bfloat16().double()


def _brute_force(q, db, metric):
    """(x64 [n,m]: the fp64 clamp / sqrt argument; E_sel; E_ref) on the CPU."""
    a, b = q.double(), db.double()
    dot = a @ b.t()
    ah, al = _split(q)
    bh, bl = _split(db)
    dot3 = ah @ (bh + bl).t() + al @ bh.t()  # hi.hi + hi.lo + lo.hi, fp64 sums
    if metric == "unit":
        x64 = 2 - 2 * dot
        e_sel = (2 * (dot3 - dot)).abs().max().item()
        x32 = 2 - 2 * torch.mm(q, db.t())
    else:
        asq, bsq = (a * a).sum(1), (b * b).sum(1)
        x64 = asq[:, None] + bsq[None, :] - 2 * dot + 1e-6
        c32 = (db * db).sum(1).double()  # the key's c_j is an fp32 sum
        e_sel = ((c32[None, :] - 2 * dot3) - (bsq[None, :] - 2 * dot)).abs().max().item()
        x32 = (q * q).sum(1)[:, None] + (db * db).sum(1)[None, :] - 2.0 * torch.mm(q, db.t()) + 1e-6
    e_ref = (x32.double() - x64).abs().max().item()
    return x64, e_sel, e_ref


def _argument_of(dist, metric):
    d = dist.double()
    return d * d if metric == "unit" else (d - 1e-8) ** 2


def _check_against_brute_force(q, db, metric, dev, tag):
    n, m = q.shape[0], db.shape[0]
    dist, idx = N.match_nn2(q.to(dev), db.to(dev), metric)
    assert dist.shape == (n, 2) and idx.shape == (n, 2) and dist.dtype == torch.float32 and idx.dtype == torch.int32
    dist, idx = dist.cpu(), idx.cpu().long()
    x64, e_sel, e_ref = _brute_force(q, db, metric)
    tol_sel, tol_val = 2 * e_sel, 4 * e_ref
    places = 2 if m > 1 else 1
    best = x64.topk(places, dim=1, largest=False).values
    excess = val_err = 0.0
    for p in range(places):
        assert idx[:, p].min().item() >= 0 and idx[:, p].max().item() < m
        got = x64.gather(1, idx[:, p:p + 1])[:, 0]
        excess = max(excess, (got - best[:, p]).max().item())
        val_err = max(val_err, (_argument_of(dist[:, p], metric) - got).abs().max().item())
    print(f"match {tag} {metric} {n}x{m}: worst excess over the fp64 minimum {excess:.3e} (tol {tol_sel:.3e}, "
          f"E_sel {e_sel:.3e}), worst value error {val_err:.3e} (tol {tol_val:.3e}, E_ref {e_ref:.3e})")
    assert excess <= tol_sel
    assert val_err <= tol_val
    if m > 1:
        assert (dist[:, 0] <= dist[:, 1]).all()
        assert (idx[:, 0] != idx[:, 1]).all()
    else:
        assert torch.isinf(dist[:, 1]).all() and (dist[:, 1] > 0).all() and (idx[:, 1] == -1).all()


@pytest.mark.parametrize("metric", ["unit", "l2"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_match_against_fp64_brute_force(n, m, metric, cuda_device):
    q, db = _descriptors(n, m, 100 + n + m, scale=1.0 if metric == "unit" else 3.0)
    _check_against_brute_force(q, db, metric, cuda_device, "shapes")


def test_match_l2_with_unequal_database_norms(cuda_device):
    """|b_j|^2 decides: database rows of norm 3 (1 +- 0.2), so the nearest row by angle is often not the nearest."""
    q, db = _descriptors(257, 1000, 7, scale=3.0, vary=0.2)
    x64 = _brute_force(q, db, "l2")[0]
    by_angle = (q.double() @ torch.nn.functional.normalize(db.double(), dim=1).t()).argmax(1)
    assert (by_angle != x64.argmin(1)).float().mean().item() > 0.2
    _check_against_brute_force(q, db, "l2", cuda_device, "norms")


@pytest.mark.parametrize("m,rows", [(400, (7, 300, 301)), (4097, (7, 4000))])
def test_equal_rows_come_out_in_index_order(m, rows, cuda_device):
    q, db = _descriptors(40, m, 11)
    g = torch.Generator().manual_seed(12)
    v = torch.nn.functional.normalize(q[0] + 0.05 * torch.randn(128, generator=g), dim=0)
    for j in rows:
        db[j] = v
    for metric in ("unit", "l2"):
        dist, idx = N.match_nn2(q.to(cuda_device), db.to(cuda_device), metric)
        assert tuple(idx[0].tolist()) == rows[:2]
        assert dist[0, 0].item() == dist[0, 1].item() and torch.equal(dist[0, 0], dist[0, 1])
        assert dist[0, 0].item() < 0.6


@pytest.mark.parametrize("metric", ["unit", "l2"])
def test_row_partitions_reassemble_the_single_call(metric, cuda_device):
    q, db = _descriptors(3001, 777, 13, scale=1.0 if metric == "unit" else 3.0)
    q, db = q.to(cuda_device), db.to(cuda_device)
    dist_f, idx_f = N.match_nn2(q, db, metric)
    cuts = [0, 100, 1000, 3001]
    parts = [N.match_nn2(q[s:e], db, metric) for s, e in zip(cuts, cuts[1:])]
    assert torch.equal(torch.cat([p[0] for p in parts]), dist_f)
    assert torch.equal(torch.cat([p[1] for p in parts]), idx_f)


def _raw_call(q, db, metric, dist, idx, ws):
    lib = N.load_library()
    stream = torch.cuda.current_stream(q.device).cuda_stream
    rc = lib.hn_match_nn2(q.data_ptr(), q.shape[0], db.data_ptr(), db.shape[0], 128, N.MATCH_METRICS[metric],
                          dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, lib.hn_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("metric", ["unit", "l2"])
def test_outputs_and_workspace_stay_in_bounds(metric, cuda_device):
    n, m = 333, 257
    q, db = _descriptors(n, m, 17, scale=1.0 if metric == "unit" else 3.0)
    q, db = q.to(cuda_device), db.to(cuda_device)
    need = max(N.match_workspace_bytes(n, m), N.match_workspace_bytes(m, n))
    pad = 4096
    ws = torch.full((need + pad,), 0xA5, dtype=torch.uint8, device=cuda_device)
    dist = torch.full((n + 1, 2), -7.0, device=cuda_device)
    idx = torch.full((n + 1, 2), -7, dtype=torch.int32, device=cuda_device)
    sz = ctypes.c_size_t()
    assert N.load_library().hn_match_workspace_bytes(n, m, ctypes.byref(sz)) == 0
    _raw_call(q, db, metric, dist, idx, ws[:sz.value + pad])
    assert (dist[n] == -7.0).all() and (idx[n] == -7).all()
    assert (ws[sz.value:sz.value + pad] == 0xA5).all()
    want_d, want_i = N.match_nn2(q, db, metric)
    assert torch.equal(dist[:n], want_d) and torch.equal(idx[:n], want_i)
    # the swapped problem (another size) on the workspace the first call left behind == on a fresh one
    dist2 = torch.empty((m, 2), device=cuda_device)
    idx2 = torch.empty((m, 2), dtype=torch.int32, device=cuda_device)
    _raw_call(db, q, metric, dist2, idx2, ws)
    fresh_d, fresh_i = N.match_nn2(db, q, metric, workspace=torch.zeros(need, dtype=torch.uint8, device=cuda_device))
    assert torch.equal(dist2, fresh_d) and torch.equal(idx2, fresh_i)


@pytest.mark.parametrize("case", ["", "close/"])
def test_match_scores_reproduce_the_reference_on_the_gpu(case, cuda_device):
    t, ref, meta = match_case(case)
    t = {k: v.to(cuda_device) for k, v in t.items()}
    nn_value, nn_idx = MT._nearest(t["des1"], t["des2"])
    da, db, ia = MT._nearest2(t["des1"], t["des2"])
    assert nn_value.is_cuda and torch.equal(nn_idx.cpu(), ref["nn_idx"]) and torch.equal(ia.cpu(), ref["Ia"])
    tol = 4 * meta["E_ref"]
    for name, got, want in (("nn_value", nn_value, ref["nn_value"]), ("Da", da, ref["Da"]), ("Db", db, ref["Db"])):
        err = (got.cpu().double() ** 2 - want.double() ** 2).abs().max().item()
        print(f"match fixture {case or 'noise 0.3'} {name}: clamp-argument error {err:.3e} (tol {tol:.3e})")
        assert err <= tol
    label, nn_kp2 = MT.nearest_neighbor_distance_ratio_match(t["des1"], t["des2"], t["kp2"], meta["ratio_threshold"])
    assert torch.equal(label.cpu(), ref["predict_label"]) and torch.equal(nn_kp2.cpu(), t["kp2"].cpu()[ref["Ia"]])
    assert six_counts(t, meta) == tuple(meta["counts"][k] for k in COUNT_KEYS)


def test_descriptors_to_match_score_end_to_end(cuda_device):
    """HardNetNeiMask (NASNet) descriptors of 64 patches and of their slightly perturbed copies, on the GPU, into
    nearest_neighbor_match_score: the counts of the torch formulation on the same descriptors."""
    m, fx, _ = build_module("fdl_NASNet")
    x = torch.from_numpy(golden_inputs(fx)[:64])
    g = torch.Generator().manual_seed(3)
    x2 = x + 0.05 * x.std() * torch.randn(x.shape, generator=g)
    m = m.to(cuda_device)
    with torch.no_grad():
        d1, d2 = m(x.to(cuda_device)), m(x2.to(cuda_device))
    kp = torch.zeros(64, 4, dtype=torch.int64)
    kp[:, 1], kp[:, 2] = 16 * (torch.arange(64) // 8), 16 * (torch.arange(64) % 8)
    visible = torch.arange(64) % 7 != 3
    got = MT.nearest_neighbor_match_score(d1, d2, kp.to(cuda_device), kp.to(cuda_device), visible.to(cuda_device), 5.0)
    want = MT.nearest_neighbor_match_score(d1.cpu(), d2.cpu(), kp, kp, visible, 5.0)
    assert got == want and got[1] == int(visible.sum()) and got[0] > 0
