"""The hardest-in-batch loss kernels (hn_loss.hip, hn_loss_gather.h, hn_pairdist.hip's k_loss and row shards) and
hn_fpr95 at their edges, against fp64, on the checked inputs of loss_edge_cases.py.

Fused train loss, per case, in this order (so that a failure names its cause):
  1. HardNetLossFunction is the grad_fn (the fused kernels ran);
  2. the saved row argmins -- with anchor_swap also the column argmins -- equal the fp64 ones exactly;
  3. |loss - ref64| <= max(1e-6, |ref32 - ref64|);
  4. every gradient row the fp64 reference leaves exactly zero is exactly zero;
  5. per row, |g_row - ref_row|_2 <= max(3 e32_row, 1e-5 |ref_row|_2), e32_row the fp32 CPU formulation's own
     error on that row (a row whose formulation cancels in fp32 shows it there);
  6. over the matrix, L2-relative <= max(1e-5, 3 g32err) (test_gpu_pairs.py's rule).
Rules 2 and 4 are exact because the inputs are *stable* (asserted here, never skipped): no selection, clamp or
mask decision lies within max(2e-6, 8 E) of flipping.  Every step prints its observed / allowed ratios; the worst
ones measured are in DESIGN.md.

B = 1 has no mixed triplet margin (min_neg - pos is 10 for any input; loss_edge_cases.py), margin 1.0 only."""
import ctypes
import math

import numpy as np
import pytest
import torch

import loss_edge_cases as C
from oracle import hardnet_oracle as O

pytestmark = pytest.mark.gpu


def _fused_step(a, p, swap, margin, loss_type, dev, upstream=1.0, positive_grad=True):
    """One loss_HardNet step on dev: (loss, [grad_a; grad_p] or grad_a alone, grad_fn name, row argmin, column
    argmin)."""
    from hardnetnas_amd import _native as N
    from hardnetnas_amd.losses import loss_HardNet
    x = a.detach().clone().to(dev).requires_grad_(True)
    y = p.detach().clone().to(dev).requires_grad_(positive_grad)
    loss = loss_HardNet(x, y, anchor_swap=swap, margin=margin, loss_type=loss_type)
    name = type(loss.grad_fn).__name__
    rows = cols = None
    if "HardNetLossFunction" in name:
        r, c = N.hardnet_loss_saved_argmins(loss.grad_fn.saved_tensors[2], a.shape[0])
        rows, cols = r.cpu(), c.cpu()
    (upstream * loss).backward()
    assert positive_grad or y.grad is None
    g = torch.cat([x.grad, y.grad]) if positive_grad else x.grad
    return loss.item(), g.cpu(), name, rows, cols


def _hold(tag, got, ref, swap, fn_name="HardNetLossFunction", rows=None):
    """Rules 1-6 on a step ``got`` = (loss, grad, grad_fn name, row argmin, column argmin) against the namespace
    ``ref`` of loss_edge_cases.reference; ``rows``: compare these gradient rows only.  Returns the ratios."""
    loss, g, name, rarg, carg = got
    assert fn_name in name, f"{tag}: grad_fn {name}"                                              # 1
    assert torch.equal(rarg, ref.row_argmin), f"{tag}: row argmins differ at " \
        f"{(rarg != ref.row_argmin).nonzero().flatten().tolist()[:8]}"                            # 2
    if swap:
        assert torch.equal(carg, ref.col_argmin), f"{tag}: column argmins differ at " \
            f"{(carg != ref.col_argmin).nonzero().flatten().tolist()[:8]}"
    el, al = abs(loss - ref.loss), max(1e-6, abs(ref.loss32 - ref.loss))
    assert el <= al, f"{tag}: loss {loss!r} vs {ref.loss!r}: {el:.2e} > {al:.2e}"                 # 3
    g = g.double()
    rg, e32 = (ref.grad, ref.e32_row) if rows is None else (ref.grad[rows], ref.e32_row[rows])
    zero = ~rg.any(dim=1)
    assert not g[zero].any(), f"{tag}: rows {(g.any(dim=1) & zero).nonzero().flatten().tolist()[:8]} " \
        f"are zero in fp64 and not here"                                                          # 4
    err, allow = (g - rg).norm(dim=1), torch.maximum(3 * e32, 1e-5 * rg.norm(dim=1))
    r5 = float((err[~zero] / allow[~zero]).max()) if (~zero).any() else 0.0
    worst = int((err - allow).argmax())
    assert bool((err <= allow).all()), f"{tag}: row {worst}: {float(err[worst]):.3e} > {float(allow[worst]):.3e} " \
        f"(e32_row {float(e32[worst]):.3e}, |ref| {float(rg[worst].norm()):.3e}); ratio {r5:.2f}"  # 5
    r6 = 0.0
    if float(rg.norm()) > 0:
        rel, a6 = float((g - rg).norm() / rg.norm()), max(1e-5, 3 * ref.g32err)
        r6 = rel / a6
        assert rel <= a6, f"{tag}: gradient L2-relative {rel:.3e} > {a6:.3e}"                     # 6
    return el / al, r5, r6


def _assert_stable(c):
    st, frac = C.check_case(c.a, c.p, c.mixed)
    assert st.ok, (c.family, c.b, st.worst, st.band)
    assert c.b < 63 or all(0.40 <= f <= 0.60 for f in frac.values()), frac


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("b", C.SIZES)
def test_fused_train_loss_edges(b, swap, cuda_device):
    """B = 1, 2, 3, the 64-row / 64-column tile edge, 257 (past k_lmin_bwd_src's block) and 1031 (k_lmin_finish's
    partial second pass, k_lmin_bwd_scan's ragged chunks) x every loss type at margin 1.0 and at the mixed margin
    (about half the rows clamped: zero coefficients, targets without sources), on 'far', 'close' and -- at
    B = 65 and 257 -- 'close3' pairs."""
    worst = {}
    for family in C.FAMILIES:
        if family == "close3" and b not in C.CLOSE3_SIZES:
            continue
        c = C.case(family, b)
        _assert_stable(c)
        for lt in C.LOSS_TYPES:
            for margin in C.margins_of(c, lt, swap):
                ref = C.reference(c.a, c.p, swap, margin, lt)
                got = _fused_step(c.a, c.p, swap, margin, lt, cuda_device)
                tag = f"{family} B={b} swap={int(swap)} {lt} margin={margin}"
                r = _hold(tag, got, ref, swap)
                print(f"RATIOS {tag}: active {float(ref.active.double().mean()):.2f} "
                      f"rule3 {r[0]:.3f} rule5 {r[1]:.3f} rule6 {r[2]:.3f}")
                worst[family] = [max(x, y) for x, y in zip(worst.get(family, (0, 0, 0)), r)]
                if b == 1 and lt == "triplet_margin":
                    # the only entry is the masked diagonal: nothing for the clamp to pass
                    assert not ref.active.any() and got[0] == 0.0 and not got[1].any()
                if b == 1 and lt == "softmax" and swap:
                    # the 0.5 / 0.5 split of torch.minimum(row, col), both halves landing on the one entry
                    assert ref.grad.abs().max() > 0 and got[1].abs().max() > 0
    for family, w in worst.items():
        print(f"WORST {family} B={b} swap={int(swap)}: rule3 {w[0]:.3f} rule5 {w[1]:.3f} rule6 {w[2]:.3f}")


@pytest.mark.parametrize("b", [65, 1031])
def test_upstream_gradient(b, cuda_device):
    """g = dloss / B with dloss != 1: (0.2 loss).backward() -- SupernetLoss's factor -- and (-3 loss).backward(),
    anchor_swap on, the triplet loss at the mixed margin; and a step where only the anchor requires grad."""
    for family in ("far", "close"):
        c = C.case(family, b)
        _assert_stable(c)
        margin = c.mixed[("triplet_margin", True)]
        for up in (0.2, -3.0):
            ref = C.reference(c.a, c.p, True, margin, "triplet_margin", upstream=up)
            got = _fused_step(c.a, c.p, True, margin, "triplet_margin", cuda_device, upstream=up)
            r = _hold(f"{family} B={b} upstream={up}", got, ref, True)
            print(f"RATIOS {family} B={b} upstream={up}: rule3 {r[0]:.3f} rule5 {r[1]:.3f} rule6 {r[2]:.3f}")
        ref = C.reference(c.a, c.p, True, margin, "triplet_margin")
        got = _fused_step(c.a, c.p, True, margin, "triplet_margin", cuda_device, positive_grad=False)
        _hold(f"{family} B={b} anchor only", got, ref, True, rows=slice(0, b))


LOSS_MARGIN_1 = [("triplet_margin", 1.0), ("contrastive", 1.0), ("softmax", 1.0)]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("m", C.FAN_M)
def test_fan_in_around_the_64_source_switch(m, swap, cuda_device):
    """A positive selected by exactly m = 63 / 64 / 65 rows and, with anchor_swap, an anchor selected by exactly m
    columns: k_lmin_bwd_gather orders a list of n <= 64 sources in-wave and rescans every source for n > 64.
    Rules 1-6 against fused=False in fp64; twice, bit-identical (the lists are filled in atomic order)."""
    f = C.fan_in(m)
    assert C.check_fan_in(f.a, f.p, m, f.rows, f.cols) == []
    for lt, margin in LOSS_MARGIN_1:
        ref = C.reference(f.a, f.p, swap, margin, lt)
        got = [_fused_step(f.a, f.p, swap, margin, lt, cuda_device) for _ in range(2)]
        assert int((got[0][3] == f.t).sum()) == m
        r = _hold(f"fan-in {m} swap={int(swap)} {lt}", got[0], ref, swap)
        print(f"RATIOS fan-in {m} swap={int(swap)} {lt}: rule3 {r[0]:.3f} rule5 {r[1]:.3f} rule6 {r[2]:.3f}")
        assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])


@pytest.mark.parametrize("m", C.FAN_M)
def test_fan_in_through_the_neighbour_mask_loss(m, cuda_device):
    """hn_neimask.hip compiles the same gather template: the same descriptors through loss_neimask with C = 0
    (any keypoints), against its own fused=False in fp64."""
    from hardnetnas_amd import _native as N
    from hardnetnas_amd.losses import loss_neimask
    f = C.fan_in(m)
    assert C.check_fan_in(f.a, f.p, m, f.rows, f.cols) == []
    ref = C.reference_neimask(f.a, f.p)
    kp = C.fan_keypoints(C.FAN_B).to(cuda_device)
    got = []
    for _ in range(2):
        x = f.a.clone().to(cuda_device).requires_grad_(True)
        y = f.p.clone().to(cuda_device).requires_grad_(True)
        loss = loss_neimask(x, y, kp, kp, margin=1.0, C=0.0)
        name = type(loss.grad_fn).__name__
        r, c = N.neimask_saved_argmins(loss.grad_fn.saved_tensors[2], C.FAN_B)
        r, c = r.cpu(), c.cpu()
        loss.backward()
        got.append((loss.item(), torch.cat([x.grad, y.grad]).cpu(), name, r, c))
    assert int((got[0][3] == f.t).sum()) == m and int((got[0][4] == f.s).sum()) >= m
    r = _hold(f"neimask fan-in {m}", got[0], ref, True, fn_name="NeiMaskLossFunction")
    print(f"RATIOS neimask fan-in {m}: rule3 {r[0]:.3f} rule5 {r[1]:.3f} rule6 {r[2]:.3f}")
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])


def test_row_column_tie_on_two_entries_splits_in_halves(cuda_device, swap=True):
    """loss_edge_cases.tied: row 9's minimum (9, 40) and column 9's minimum (52, 9) are bit-equal, in different
    rows and columns and without a mirror image, so the 0.5 / 0.5 share of k_lmin_bwd_src decides four gradient
    rows (a duplicated pair, as in test_gpu_pairs.py's ties test, gives every row the same sum for any share).
    Ties inside row 52 and column 40 go to the first index, as torch.min's.  Rules 1-6, with anchor_swap only:
    without it there is no tie to split, and positive 9's two terms -- its own pair and row 52's negative, the same
    entry's derivative with opposite signs -- cancel to a true gradient of 0 (fp64 2e-18, the fp32 CPU formulation
    1.2e-9, the kernels 8.1e-9 measured: the positive's derivative is taken in the difference form, the negative's in
    the expanded one), a row rule 5 has no scale for."""
    t = C.tied()
    assert C.stable(t.a, t.p, [1.0], ties=True).ok
    for lt, margin in LOSS_MARGIN_1:
        ref = C.reference(t.a, t.p, swap, margin, lt)
        got = _fused_step(t.a, t.p, swap, margin, lt, cuda_device)
        r = _hold(f"tied swap={int(swap)} {lt}", got, ref, swap)
        print(f"RATIOS tied swap={int(swap)} {lt}: rule3 {r[0]:.3f} rule5 {r[1]:.3f} rule6 {r[2]:.3f}")


@pytest.mark.parametrize("swap", [False, True])
def test_sparse_lists_do_not_depend_on_atomic_order(swap, cuda_device):
    """B = 1031 at the mixed margin, twice: about half the sources have no term, the rest fill 2,062 short lists
    through atomicAdd; loss and gradients are bit-identical."""
    c = C.case("far", 1031)
    for lt in ("triplet_margin", "contrastive"):
        margin = c.mixed[(lt, swap)]
        one, two = (_fused_step(c.a, c.p, swap, margin, lt, cuda_device) for _ in range(2))
        assert one[0] == two[0] and torch.equal(one[1], two[1])
        assert torch.equal(one[3], two[3]) and (not swap or torch.equal(one[4], two[4]))


@pytest.mark.parametrize("swap", [False, True])
def test_workspace_guards_through_the_c_abi(swap, cuda_device):
    """hn_hardnet_loss_train_forward / hn_hardnet_loss_backward at B = 130 (two row tiles and a ragged third, a
    partial k_lmin_bwd_src block): d_saved inside 512-byte 0xA5 pads, the loss and both gradients inside -777
    pads -- all pads intact, the inputs unchanged; and d_saved pre-filled with 0x00 and with 0xFF gives
    bit-identical results (nothing reads what the forward did not write: without anchor_swap colbest is never
    initialised, so it must never be read)."""
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    n, pad = 130, 512
    a, p = (t.to(cuda_device) for t in C.pairs(n, 0.3, 1.0, 130))
    keep = [a.clone(), p.clone()]
    nb = ctypes.c_size_t()
    assert lib.hn_hardnet_loss_train_workspace_bytes(n, ctypes.byref(nb)) == 0
    dl = torch.ones(1, device=cuda_device)
    res = []
    for lt, margin in ((0, 1.0), (2, 1.25), (1, 1.0)):
        for fill in (0xA5, 0x00, 0xFF):
            ws = torch.full((pad + nb.value + pad,), 0xA5, dtype=torch.uint8, device=cuda_device)
            ws[pad:pad + nb.value] = fill
            out = torch.full((64 + 1 + 64,), -777.0, device=cuda_device)
            grads = torch.full((64 * 128 + 2 * n * 128 + 64 * 128,), -777.0, device=cuda_device)
            base = ws.data_ptr() + pad
            assert base % 16 == 0
            rc = lib.hn_hardnet_loss_train_forward(a.data_ptr(), p.data_ptr(), n, 128, int(swap), margin, lt,
                                                   out.data_ptr() + 4 * 64, base, nb.value, None)
            assert rc == 0, lib.hn_last_error()
            gbase = grads.data_ptr() + 4 * 64 * 128
            rc = lib.hn_hardnet_loss_backward(a.data_ptr(), p.data_ptr(), n, 128, int(swap), margin, lt, dl.data_ptr(),
                                              gbase, gbase + 4 * n * 128, base, nb.value, None)
            assert rc == 0, lib.hn_last_error()
            torch.cuda.synchronize(cuda_device)
            assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nb.value:] == 0xA5).all())
            assert bool((out[:64] == -777.0).all()) and bool((out[65:] == -777.0).all())
            assert bool((grads[:64 * 128] == -777.0).all()) and bool((grads[-64 * 128:] == -777.0).all())
            body = grads[64 * 128:-64 * 128]
            assert math.isfinite(out[64].item()) and bool(torch.isfinite(body).all())
            assert torch.equal(a, keep[0]) and torch.equal(p, keep[1])
            res.append((lt, out[64].item(), body.clone()))
    for k in range(0, len(res), 3):
        for other in res[k + 1:k + 3]:
            assert other[1] == res[k][1] and torch.equal(other[2], res[k][2]), f"loss_type {res[k][0]}"
    # and the values are the loss's
    ref = C.reference(a.cpu(), p.cpu(), swap, 1.0, "triplet_margin")
    assert abs(res[0][1] - ref.loss) <= max(1e-6, abs(ref.loss32 - ref.loss))
    rel = float((res[0][2].cpu().double() - ref.grad.reshape(-1)).norm() / ref.grad.norm())
    assert rel <= max(1e-5, 3 * ref.g32err)


@pytest.mark.parametrize("n", [1, 1023, 1025, 3001])
def test_hardnet_loss_kernel_bound(n, cuda_device):
    """hn_hardnet_loss (k_loss) on synthetic fp32 pos / row_min / col_min: n = 1, either side of its 1024-thread
    block and three stride passes; margins 0.5 and 1.0; scale 1 / n and the 1 / (2 n) of a sharded batch;
    col_min present and absent; the min_neg output present and NULL.  Against the fp64 evaluation of the same fp32
    inputs, within (ceil(n / 1024) + 40) 2^-24 scale sum |l_i| (loss_edge_cases.loss_bound); min_neg is
    min(row_min, col_min) bit for bit."""
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    pos, rmin, cmin = C.loss_inputs(n)
    dp, dr, dc = (t.to(cuda_device) for t in (pos, rmin, cmin))
    worst = 0.0
    for with_col in (False, True):
        mn = torch.minimum(rmin, cmin) if with_col else rmin
        for lt in C.LOSS_TYPES:
            for margin in (0.5, 1.0):
                terms = C.loss_terms64(pos, mn, margin, lt)
                for scale in (1.0 / n, 1.0 / (2 * n)):
                    want = scale * float(terms.sum())
                    allow = C.loss_bound(n, scale, terms)
                    loss, gmn = N.hardnet_loss(dp, dr, dc if with_col else None, margin=margin, loss_type=lt,
                                               scale=scale)
                    assert torch.equal(gmn.cpu(), mn)
                    # the same call without the min_neg output
                    l2 = torch.full((3,), -777.0, device=cuda_device)
                    rc = lib.hn_hardnet_loss(dp.data_ptr(), dr.data_ptr(), dc.data_ptr() if with_col else None, n,
                                             margin, N.LOSS_TYPES[lt], scale, None, l2.data_ptr() + 4, None)
                    assert rc == 0, lib.hn_last_error()
                    torch.cuda.synchronize(cuda_device)
                    assert l2[0].item() == -777.0 and l2[2].item() == -777.0 and l2[1].item() == loss.item()
                    err = abs(float(loss.item()) - want)
                    worst = max(worst, err / allow if allow else (0.0 if err == 0 else math.inf))
                    assert err <= allow, f"n={n} {lt} margin={margin} scale={scale} col={with_col}: " \
                        f"{loss.item()!r} vs {want!r}: {err:.3e} > {allow:.3e}"
    print(f"RATIOS k_loss n={n}: worst observed / allowed {worst:.3f}")


@pytest.mark.parametrize("swap", [False, True])
def test_row_shards_at_ragged_cuts(swap, cuda_device):
    """hn_pairdist_rows at B = 300 (no multiple of 64) cut at [0, 1, 64, 65, 235, 299, 300]: a one-row shard at
    either end, the last one ending on the batch's ragged row, row0 = 65 / 235 / 299 no multiple of 64 --
    reassembled as test_gpu_pairs.py::test_row_shards_reassemble_the_full_result does: bit-identical to the
    single call, and within 1e-4 of the fp64 oracle."""
    from hardnetnas_amd._native import hardnet_loss, pairdist_hardneg, pairdist_rows
    a, p = C.pairs(300, 0.3, 1.0, 300)
    p[17] = a[250] + 1e-4 * torch.randn(128, generator=torch.Generator().manual_seed(3))  # dm < 0.008 off the diagonal
    ad, pd = a.to(cuda_device), p.to(cuda_device)
    pos_f, mn_f = pairdist_hardneg(ad, pd, swap)
    cuts = [0, 1, 64, 65, 235, 299, 300]
    parts, cmins = [], []
    for s, e in zip(cuts, cuts[1:]):
        pos, rmin, cmin = pairdist_rows(ad[s:e], s, pd, col_min=swap)
        assert pos.shape == (e - s,) and rmin.shape == (e - s,)
        parts.append((pos, rmin))
        cmins.append(cmin)
    pos = torch.cat([x[0] for x in parts])
    if swap:
        cm = torch.stack(cmins).min(dim=0)[0]
        mn = torch.cat([hardnet_loss(x[0], x[1], cm[s:e])[1] for x, s, e in zip(parts, cuts, cuts[1:])])
    else:
        mn = torch.cat([x[1] for x in parts])
    assert torch.equal(pos, pos_f)
    assert torch.equal(mn, mn_f)
    rpos, rmn = O.hardest_negative(a.double(), p.double(), swap)
    assert (pos.cpu().double() - rpos).abs().max().item() < 1e-4
    assert (mn.cpu().double() - rmn).abs().max().item() < 1e-4


def _fpr(a, p, labels, dev):
    from hardnetnas_amd._native import fpr95
    return fpr95(a.to(dev), p.to(dev), torch.as_tensor(labels).to(dev))


@pytest.mark.parametrize("n,dim", [(2, 128), (255, 128), (256, 128), (257, 128), (257, 1), (257, 65), (257, 130)])
def test_fpr95_exact_at_block_and_lane_edges(n, dim, cuda_device):
    """n on either side of the 256-thread blocks of k_gather_labels / k_threshold, dim below, past and no multiple
    of the 64 lanes k_pair_dist strides over the descriptor (the distance on the last element): the builder's
    distances cannot tie, so the result equals the oracle exactly, not within 2 / n."""
    a, p, labels, d = C.fpr_case(n, max(1, n // 5), 70 + n, dim)
    got, dd = _fpr(a, p, labels, cuda_device)
    assert torch.allclose(dd.cpu(), torch.from_numpy(d), rtol=1e-6, atol=0)
    assert got == C.fpr_expected(labels, d)


def test_fpr95_threshold_on_an_integer(cuda_device):
    """20 matches among 100: 0.95 * total = 19 exactly, reached by the 19th match (>=, not >)."""
    a, p, labels, d = C.fpr_case(100, 20, 173)
    assert 0.95 * float(labels.sum()) == 19.0
    got, dd = _fpr(a, p, labels, cuda_device)
    assert torch.allclose(dd.cpu(), torch.from_numpy(d), rtol=1e-6, atol=0)
    assert got == C.fpr_expected(labels, d)
    lab = labels[np.argsort(d)]
    t = int(np.argmax(np.cumsum(lab) >= 19))
    assert got == int((lab[:t] == 0).sum()) / 80.0
    assert got != int((lab[:int(np.argmax(np.cumsum(lab) >= 20))] == 0).sum()) / 80.0  # (the case can tell)


def test_fpr95_degenerate_labels(cuda_device):
    """All-zero labels give 0.0 (the threshold is met at the first pair: no false positive); no negatives --
    n = 1 with label 1, all labels 1 -- give the documented NaN (the reference divides 0 by 0).

    Labels other than 0 / 1: the kernel counts ``label != 0`` as a match, so 2 and -1 are matches.  The
    reference's np.cumsum would add them raw (a 2 twice, a -1 negatively) and its ``== 0`` counts would agree
    only on the zeros; the expected value here is the oracle on ``labels != 0``."""
    a, p, labels, d = C.fpr_case(257, 50, 9)
    assert _fpr(a, p, np.zeros(257, np.int32), cuda_device)[0] == 0.0
    assert C.fpr_expected(np.zeros(257, np.int32), d) == 0.0
    assert math.isnan(_fpr(a, p, np.ones(257, np.int32), cuda_device)[0])
    a1, p1, _, _ = C.fpr_case(1, 1, 1)
    got, dd = _fpr(a1, p1, np.ones(1, np.int32), cuda_device)
    assert math.isnan(got) and dd.shape == (1,)
    assert _fpr(a1, p1, np.zeros(1, np.int32), cuda_device)[0] == 0.0
    odd = labels.copy()
    ones = np.flatnonzero(labels)
    odd[ones[::2]] = 2
    odd[ones[1::3]] = -1
    assert set(np.unique(odd)) == {-1, 0, 1, 2}
    want = C.fpr_expected(labels, d)
    assert C.fpr_expected(odd, d) == want
    assert _fpr(a, p, odd, cuda_device)[0] == want == _fpr(a, p, labels, cuda_device)[0]
