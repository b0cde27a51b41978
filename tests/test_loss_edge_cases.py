"""The builders of loss_edge_cases.py meet their preconditions, and their reference is the loss the project means.

test_gpu_loss_edges.py holds the fused loss to per-row bounds against ``reference`` on these inputs.  Those bounds
judge arithmetic only if fp32 and fp64 select the same entries, so the stability band, the 40-60 % mixed clamp,
the exact fan-in counts and the tie-free FPR95 distances are re-derived here from the returned tensors (not read
back from the builder's own verdict), on the CPU, and ``stable`` is shown to reject inputs just inside the band."""
import numpy as np
import pytest
import torch

import loss_edge_cases as C
from oracle import hardnet_oracle as O

CASES = [(f, b) for f in C.FAMILIES for b in C.SIZES if f != "close3" or b in C.CLOSE3_SIZES]


@pytest.mark.parametrize("family,b", CASES)
def test_case_is_stable_and_mixed(family, b):
    c = C.case(family, b)
    assert c.seed >= 1000 * b and c.tries <= 2
    noise, scale = C.FAMILIES[family]
    a, p = C.pairs(b, noise, scale, c.seed)
    assert torch.equal(a, c.a) and torch.equal(p, c.p)
    assert torch.allclose(a.norm(dim=1), torch.full((b,), scale), rtol=1e-6)
    assert c.mixed == C.mixed_margins(a, p)
    st, frac = C.check_case(a, p, c.mixed)
    assert C.BAND_MIN <= st.band == max(2e-6, 8 * st.E) <= 6.4e-6
    assert all(v >= st.band for v in st.worst.values()), st.worst
    s = C.selections(a, p)
    for (lt, swap), m in c.mixed.items():
        if m is None:
            assert b == 1 and lt == "triplet_margin"  # min_neg - pos is 10 for any input: no stable median
            continue
        mn = torch.minimum(s.row_min, s.col_min) if swap else s.row_min
        t = (m + s.pos - mn) if lt == "triplet_margin" else (m - mn)
        assert float(t.abs().min()) >= st.band
        assert torch.equal(t > 0, C.active_rows(a, p, swap, m, lt))
        if b >= 63:
            assert 0.40 <= float((t > 0).double().mean()) <= 0.60, (lt, swap, frac)
    if b >= 63 and family == "far":  # the existing tests' generator: margin 1.0 is all-or-nothing, hence the mixed one
        for swap in (False, True):
            assert bool(C.active_rows(a, p, swap, 1.0, "triplet_margin").all())
            assert not bool(C.active_rows(a, p, swap, 1.0, "contrastive").any())
    if b == 1:
        assert float(s.row_min) == float(s.col_min) == float(s.pos) + 10.0  # the exempt bit-equal tie


def test_stable_rejects_what_it_should():
    c = C.case("far", 65)
    a, p = c.a.clone(), c.p.clone()
    assert C.stable(a, p, [1.0]).ok
    s = C.selections(a, p)
    mn = torch.minimum(s.row_min, s.col_min)
    # a margin 1e-6 off one row's clamp, for each of the two expressions, with and without swap
    for on_clamp in (float(mn[5] - s.pos[5]), float(mn[9]), float(s.row_min[11] - s.pos[11]), float(s.row_min[2])):
        st = C.stable(a, p, [1.0, on_clamp + 1e-6])
        assert not st.ok and st.worst["clamp"] < st.band
        assert C.stable(a, p, [1.0, on_clamp + 1e-3]).worst["clamp"] >= 1e-6
    # a row's hardest negative duplicated: its two smallest entries equal
    q = p.clone()
    q[40 if int(s.row_argmin[0]) != 40 else 41] = q[int(s.row_argmin[0])]
    st = C.stable(a, q, [1.0])
    assert not st.ok and st.worst["row_gap"] == 0.0
    # a duplicated anchor: a column's two smallest entries equal
    b = a.clone()
    b[50] = b[int(s.col_argmin[4])]
    st = C.stable(b, p, [1.0])
    assert not st.ok and st.worst["col_gap"] == 0.0
    # an off-diagonal distance 1e-6 from the 0.008 mask
    q = p.clone()
    v = torch.nn.functional.normalize(torch.randn(128, generator=torch.Generator().manual_seed(1)), dim=0)
    v = torch.nn.functional.normalize(v - (v @ a[8]) * a[8], dim=0)
    q[30] = a[8] + (0.008 - 1e-8) * 0.9922 * v   # sqrt(x^2 + 1e-6) + 1e-8 = 0.008 near x = 0.0079373
    st = C.stable(a, q, [1.0])
    assert not st.ok and st.worst["mask"] < 5e-6, st.worst
    # the one exemption: B = 1, where the row and the column minimum are the same entry in fp64 and fp32 alike
    one = C.case("far", 1)
    st = C.stable(one.a, one.p, [1.0])
    assert st.ok and st.worst["row_col"] == float("inf")
    assert not C.stable(one.a, one.p, [10.0]).ok     # the triplet margin on the B = 1 clamp (module docstring)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("loss_type", C.LOSS_TYPES)
def test_reference_agrees_with_the_oracle(loss_type, swap):
    """``reference`` (losses.loss_HardNet, fused=False, fp64) against oracle.loss_hardnet, the reference's own
    lines, at unit and non-unit margins; and its by-products against the oracle's pos / min_neg."""
    for family, b in (("far", 65), ("close", 129), ("close3", 65), ("far", 1), ("close", 2)):
        c = C.case(family, b)
        for margin in set(C.margins_of(c, loss_type, swap)) | {0.5, 1.7}:
            r = C.reference(c.a, c.p, swap, margin, loss_type)
            want = O.loss_hardnet(c.a.double(), c.p.double(), swap, margin=margin, loss_type=loss_type).item()
            assert abs(r.loss - want) <= 1e-12 * max(1.0, abs(want)), (family, b, margin)
            assert abs(r.loss32 - want) <= 1e-4
            assert r.grad.shape == (2 * b, 128) and r.grad.dtype == torch.float64
            pos, mn = O.hardest_negative(c.a.double(), c.p.double(), swap)
            act = (margin + pos - mn > 0) if loss_type == "triplet_margin" else (
                (margin - mn > 0) if loss_type == "contrastive" else torch.ones(b, dtype=torch.bool))
            assert torch.equal(r.active, act)
            # a clamped triplet row passes nothing to its own anchor unless a column selected it
            if loss_type == "triplet_margin" and not swap:
                assert not r.grad[:b][~act].any()
            if b > 1 and r.grad.any():   # (margin 0.5 clamps every triplet row of 'far')
                assert r.g32err < 1e-4 and float(r.e32_row.max()) > 0
    c = C.case("far", 65)
    r1 = C.reference(c.a, c.p, swap, 1.0, loss_type)
    r2 = C.reference(c.a, c.p, swap, 1.0, loss_type, upstream=-3.0)
    assert r1.loss == r2.loss and float((r2.grad + 3.0 * r1.grad).abs().max()) <= 1e-12 * float(r1.grad.abs().max())


def test_reference_argmins_are_the_formulations():
    c = C.case("close", 129)
    r = C.reference(c.a, c.p, True, 1.0, "triplet_margin")
    d = O.distance_matrix_vector(c.a.double(), c.p.double()) + 1e-8
    dn = d + 10 * torch.eye(129, dtype=torch.float64)
    dn = dn + 10 * (dn < 0.008)
    assert torch.equal(r.row_argmin, dn.argmin(dim=1)) and torch.equal(r.col_argmin, dn.argmin(dim=0))


@pytest.mark.parametrize("m", C.FAN_M)
def test_fan_in_counts_are_exact(m):
    f = C.fan_in(m)
    assert f.a.shape == (C.FAN_B, 128) and len(f.rows) == len(f.cols) == m
    assert not set(f.rows) & set(f.cols) and not {f.t, f.s} & (set(f.rows) | set(f.cols))
    assert C.check_fan_in(f.a, f.p, m, f.rows, f.cols) == []
    for form in ("hardnet", "unit"):
        s = C.selections(f.a, f.p, form)
        assert int((s.row_argmin == f.t).sum()) == m
        won = (s.col_argmin == f.s) & (s.col_min < s.row_min)
        assert int(won.sum()) == m
        # the source lists the gather kernel sees: positive t has m sources without and with swap, anchor s has m
        # with swap; no other target comes near the 64-source switch
        for swap in (False, True):
            row_wins = (s.row_min < s.col_min) if swap else torch.ones(C.FAN_B, dtype=torch.bool)
            cnt_p = torch.bincount(s.row_argmin[row_wins], minlength=C.FAN_B)
            assert int(cnt_p[f.t]) == m and int(cnt_p[torch.arange(C.FAN_B) != f.t].max()) < 32
            if swap:
                cnt_a = torch.bincount(s.col_argmin[~row_wins], minlength=C.FAN_B)
                assert int(cnt_a[f.s]) == m and int(cnt_a[torch.arange(C.FAN_B) != f.s].max()) < 32
        st = C.stable(f.a, f.p, [1.0], form)
        assert st.ok and st.band >= 2e-6
    # one row fewer around c and the count check notices
    a = f.a.clone()
    a[f.rows[0]] = -a[f.rows[0]]
    assert any("rows select column" in x for x in C.check_fan_in(a, f.p, m, f.rows, f.cols))


def test_tied_case_splits_row_i_in_halves():
    """The reference gives entries (i, j) and (k, i) half of row i's weight each: anchor k's gradient holds a term
    along p_i that only the column half can put there."""
    t = C.tied()
    r = C.reference(t.a, t.p, True, 1.0, "triplet_margin")
    assert torch.equal(r.row_argmin[[t.i, t.k]], torch.tensor([t.j, min(t.i, t.j)]))
    assert int(r.col_argmin[t.i]) == t.k
    s = C.selections(t.a, t.p)
    u = t.a[t.k].double() - t.p[t.i].double()
    half = -0.5 / 65 / (float(s.dn[t.k, t.i]) - 1e-8) * u   # -g / 2 * d sqrt(u) / d a_k at entry (k, i)
    others = r.grad[t.k] - half
    r0 = C.reference(t.a, t.p, False, 1.0, "triplet_margin")  # without swap: no column half
    assert float(half.norm()) > 1e-3 and float((others - r0.grad[t.k]).norm()) <= 1e-11
    assert float((r.grad[t.i] - r0.grad[t.i]).norm()) > 1e-3


def test_reference_neimask_is_the_plain_loss_at_c0():
    f = C.fan_in(64)
    r = C.reference_neimask(f.a, f.p)
    s = C.selections(f.a, f.p, "unit")
    want = torch.clamp(1.0 + s.pos - torch.minimum(s.row_min, s.col_min), min=0).mean().item()
    assert abs(r.loss - want) <= 1e-12 and torch.equal(r.row_argmin, s.row_argmin)
    assert bool(r.active[f.rows + f.cols].all())


def test_saved_argmin_accessor_decodes_a_hand_packed_buffer():
    from hardnetnas_amd._native import hardnet_loss_saved_argmins
    for b in (1, 37, 64, 65):
        al = lambda n: (n + 255) // 256 * 256  # noqa: E731
        rng = np.random.RandomState(b)
        rows, cols = rng.randint(0, b, b), rng.randint(0, b, b)
        vals = rng.rand(2, b).astype(np.float32) + 10.0 * (rng.rand(2, b) < 0.3)
        buf = np.full(al(8 * b) + 2 * al(8 * b) + 64, 0xA5, np.uint8)
        for k, (v, idx) in enumerate(((vals[0], rows), (vals[1], cols))):
            keys = (v.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
            o = al(8 * b) + k * al(8 * b)
            buf[o:o + 8 * b] = keys.view(np.uint8)
        r, c = hardnet_loss_saved_argmins(torch.from_numpy(buf), b)
        assert r.dtype == torch.int64 and r.shape == (b,) and c.shape == (b,)
        assert np.array_equal(r.numpy(), rows) and np.array_equal(c.numpy(), cols)
        assert bool((torch.from_numpy(buf)[-64:] == 0xA5).all())


@pytest.mark.parametrize("n,dim", [(1, 128), (2, 128), (100, 128), (255, 128), (256, 128), (257, 128), (257, 1),
                                   (257, 65), (257, 130)])
def test_fpr_cases_cannot_tie(n, dim):
    a, p, labels, d = C.fpr_case(n, max(1, n // 5), 70 + n, dim)
    C.check_fpr_distances(d)
    assert len(np.unique(d)) == n and len(np.unique(C.fpr_key32(d))) == n
    assert int(labels.sum()) == max(1, n // 5)
    assert torch.equal((a - p).norm(dim=1), torch.from_numpy(d)) and int((p != 0).sum()) == n
    col = 0 if dim == 128 else dim - 1
    assert bool((p[:, col] != 0).all())
    with pytest.raises(AssertionError):
        C.check_fpr_distances(np.array([0.5, 0.5 * (1 + 5e-4), 0.7], np.float32))
    if n > 1:
        # the fp32 distance order decides the result: the fp32 key order and the fp64 score order are the same
        want = C.fpr_expected(labels, d)
        lab = labels[np.argsort(C.fpr_key32(d), kind="stable")]
        t = int(np.argmax(np.cumsum(lab) >= 0.95 * lab.sum()))
        fp, tn = int((lab[:t] == 0).sum()), int((lab[t:] == 0).sum())
        assert want == fp / (fp + tn)


def test_fpr_threshold_on_an_integer():
    _, _, labels, d = C.fpr_case(100, 20, 173)
    assert 0.95 * int(labels.sum()) == 19.0      # the 19th match reaches it exactly, not the 20th
    lab = labels[np.argsort(d)]
    t = int(np.argmax(np.cumsum(lab) >= 19.0))
    assert int(lab[:t + 1].sum()) == 19
    fp = int((lab[:t] == 0).sum())
    assert C.fpr_expected(labels, d) == fp / 80.0
    # the case can tell >= from >: stopping at the 20th match instead counts other false positives
    assert int((lab[:int(np.argmax(np.cumsum(lab) >= 20))] == 0).sum()) != fp


def test_loss_bound_inputs_are_mixed():
    for n in (1023, 3001):
        pos, rmin, cmin = C.loss_inputs(n)
        for margin in (0.5, 1.0):
            for mn in (rmin, torch.minimum(rmin, cmin)):
                for lt in ("triplet_margin", "contrastive"):
                    frac = float((C.loss_terms64(pos, mn, margin, lt) > (pos.double() if lt == "contrastive" else 0))
                                 .double().mean())
                    assert 0.05 < frac < 0.95, (n, margin, lt, frac)
    t = C.loss_terms64(*C.loss_inputs(1025)[:2], 1.0, "softmax")
    assert C.loss_bound(1025, 1 / 1025, t) == (2 + 40) * 2.0 ** -24 / 1025 * float(t.sum())
