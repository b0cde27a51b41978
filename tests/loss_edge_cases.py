"""Inputs for the hardest-in-batch loss and FPR95 edge tests, each with a precondition that is checked, not hoped for.

The fused loss (hn_loss.hip) selects: one hardest negative per row (and per column with anchor_swap), the smaller
of the two, a clamp that is active or not, a < 0.008 mask.  A test that compares its gradients with an fp64
reference says something about the arithmetic only if both sides made the same selections, and random inputs do
not promise that: a B = 63 draw had a row whose two smallest negatives differ by 6e-7, less than the fp32 error
of one distance.  So every input built here is *stable*:

  E    = the largest |d_fp32 - d_fp64| over the off-diagonal entries of the CPU formulation
         (hardnetnas_amd.losses.distance_matrix_vector + 1e-8)
  band = max(2e-6, 8 E)
  and at least ``band`` separates, in fp64: every row's and every column's smallest masked distance from its
  second smallest; every row's row minimum from its column minimum; every off-diagonal distance from 0.008;
  every row's margin + pos - min_neg and margin - min_neg from 0, for every margin the tests use and for min_neg
  with and without anchor_swap.

Only |row_min - col_min| has an exemption: a difference that is exactly 0 in fp64 and in fp32 (B = 1, where both
are the one masked diagonal entry) is a bit-equal tie, which fp32 reproduces bit for bit and which
torch.minimum splits 0.5 / 0.5 in either precision.  Builders search seeds upward from 1000 B and return the
first stable one; the GPU tests assert the precondition, they never skip and never drop a row.

Families (``pairs``): 'far' noise 0.3, 'close' noise 0.03, 'close3' noise 0.03 at |a| = |p| = 3.  Margins: 1.0,
where every triplet row of the 'far' pairs is active and no contrastive one, and a *mixed* margin per (loss type,
anchor_swap) -- the median over rows of min_neg - pos (triplet) or of min_neg (contrastive), rounded to 3
decimals -- at which 40-60 % of the rows are clamped (asserted for B >= 63).  At B = 1 min_neg - pos is 10 for
any input (the masked diagonal against itself), so a triplet margin from that median sits on the clamp by
construction and cannot be stable: B = 1 has no mixed triplet margin (``case(...).mixed`` holds None there).

``fan_in`` builds B = 200 with one positive selected by exactly m rows and one anchor selected by exactly m
columns, m around the gather kernel's 64-source switch.  ``tied`` duplicates one anchor and one positive so that a
row's and its column's minimum are bit-equal on two different entries (``stable(..., ties=True)`` exempts exactly
those bit-equal gaps, nothing else).  The fpr95 cases carry distances that cannot tie.
No GPU, no file I/O; the reference is the autograd formulation (``fused=False``) in fp64 on the CPU."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from hardnetnas_amd import losses as L
from hardnetnas_amd import matching as M

FAMILIES = {"far": (0.3, 1.0), "close": (0.03, 1.0), "close3": (0.03, 3.0)}
SIZES = (1, 2, 3, 63, 64, 65, 127, 129, 257, 1031)
CLOSE3_SIZES = (65, 257)
LOSS_TYPES = ("triplet_margin", "softmax", "contrastive")
BAND_MIN = 2e-6
ACTIVE_LO, ACTIVE_HI = 0.40, 0.60
MAX_TRIES = 16
FAN_B, FAN_T, FAN_S = 200, 3, 7
FAN_M = (63, 64, 65)

_unit = functools.partial(torch.nn.functional.normalize, dim=-1)


def pairs(b, noise, scale, seed):
    """Unit anchors, p = normalize(a + noise * randn), both multiplied by scale (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    a = _unit(torch.randn(b, 128, generator=g))
    p = _unit(a + noise * torch.randn(b, 128, generator=g))
    return a * scale, p * scale


def masked_distances(a, p, form="hardnet"):
    """(d, dn) in a's dtype.  'hardnet': loss_HardNet's d + 1e-8, with 10 added on the diagonal and then wherever
    the result is < 0.008; 'unit': loss_neimask's with C = 0 (10 on the diagonal only)."""
    if form == "hardnet":
        d = L.distance_matrix_vector(a, p) + 1e-8
        dn = d + 10.0 * torch.eye(d.size(1), dtype=d.dtype)
        return d, dn + 10.0 * (dn < 0.008).to(dn.dtype)
    d = M.distance_matrix_vector(a, p)
    return d, d + 10.0 * torch.eye(d.size(1), dtype=d.dtype)


def selections(a, p, form="hardnet"):
    """The fp64 selections: pos, row / column minima of dn and their argmins."""
    d, dn = masked_distances(a.double(), p.double(), form)
    rmin, rarg = dn.min(dim=1)
    cmin, carg = dn.min(dim=0)
    return SimpleNamespace(d=d, dn=dn, pos=torch.diagonal(d), row_min=rmin, row_argmin=rarg, col_min=cmin,
                           col_argmin=carg)


def _gap(dn, dim):
    """second smallest - smallest along dim (inf where there is no second)."""
    if dn.size(dim) < 2:
        return torch.full((dn.size(1 - dim),), math.inf, dtype=dn.dtype)
    two = torch.topk(dn, 2, dim=dim, largest=False)[0]
    return (two.select(dim, 1) - two.select(dim, 0))


def stable(a, p, margins, form="hardnet", ties=False):
    """The precondition of the module docstring on fp32 CPU inputs.  Returns a namespace: ok, band, E and
    ``worst``, the smallest separation found per kind (for messages).  ``ties``: also exempt a row's or column's
    two smallest entries when they are exactly equal in fp64 and in fp32 (``tied``: duplicated vectors; the kernels
    and torch.min both keep the first index)."""
    s = selections(a, p, form)
    d32, dn32 = masked_distances(a.float(), p.float(), form)
    b = a.shape[0]
    off = ~torch.eye(b, dtype=torch.bool)
    err = (d32.double() - s.d).abs()
    e = float(err[off].max()) if b > 1 else 0.0
    band = max(BAND_MIN, 8.0 * e)
    worst = {}
    for name, dim in (("row_gap", 1), ("col_gap", 0)):
        gap = _gap(s.dn, dim)
        if ties:
            gap = torch.where((gap == 0) & (_gap(dn32, dim) == 0), torch.full_like(gap, math.inf), gap)
        worst[name] = float(gap.min())
    rc = (s.row_min - s.col_min).abs()
    rc32 = dn32.min(dim=1)[0] - dn32.min(dim=0)[0]
    rc = torch.where((rc == 0) & (rc32 == 0), torch.full_like(rc, math.inf), rc)  # bit-equal ties are exempt
    worst["row_col"] = float(rc.min())
    if form == "hardnet":
        worst["mask"] = float((s.d[off] - 0.008).abs().min()) if b > 1 else math.inf
    clamp = math.inf
    for mn in (s.row_min, torch.minimum(s.row_min, s.col_min)):
        for m in margins:
            clamp = min(clamp, float((m + s.pos - mn).abs().min()), float((m - mn).abs().min()))
    worst["clamp"] = clamp
    return SimpleNamespace(ok=all(v >= band for v in worst.values()), band=band, E=e, worst=worst)


def active_rows(a, p, swap, margin, loss_type, form="hardnet"):
    """Per row: does the clamp pass a gradient (fp64)?  softmax has no clamp."""
    s = selections(a, p, form)
    mn = torch.minimum(s.row_min, s.col_min) if swap else s.row_min
    if loss_type == "triplet_margin":
        return margin + s.pos - mn > 0
    if loss_type == "contrastive":
        return margin - mn > 0
    return torch.ones_like(mn, dtype=torch.bool)


def mixed_margins(a, p):
    """{(loss type, swap): margin} from the fp64 selections: the median of min_neg - pos (triplet) / of min_neg
    (contrastive), rounded to 3 decimals; None for the triplet at B = 1 (module docstring)."""
    s = selections(a, p)
    out = {}
    for swap in (False, True):
        mn = torch.minimum(s.row_min, s.col_min) if swap else s.row_min
        out[("triplet_margin", swap)] = round(float((mn - s.pos).median()), 3) if a.shape[0] > 1 else None
        out[("contrastive", swap)] = round(float(mn.median()), 3)
    return out


def check_case(a, p, mixed):
    """(stability namespace, {key: active fraction at the mixed margin}) -- what ``case`` requires of a seed."""
    st = stable(a, p, [1.0] + [m for m in mixed.values() if m is not None])
    frac = {k: float(active_rows(a, p, k[1], m, k[0]).double().mean()) for k, m in mixed.items() if m is not None}
    return st, frac


@functools.lru_cache(maxsize=None)
def case(family, b):
    """The first stable seed >= 1000 b of a family at batch b: a, p (fp32 CPU), seed, band, E, ``mixed`` (the mixed
    margins) and ``frac`` (their active fractions, 40-60 % for b >= 63)."""
    noise, scale = FAMILIES[family]
    for seed in range(1000 * b, 1000 * b + MAX_TRIES):
        a, p = pairs(b, noise, scale, seed)
        mixed = mixed_margins(a, p)
        st, frac = check_case(a, p, mixed)
        if st.ok and (b < 63 or all(ACTIVE_LO <= f <= ACTIVE_HI for f in frac.values())):
            return SimpleNamespace(family=family, b=b, a=a, p=p, seed=seed, tries=seed - 1000 * b + 1, band=st.band,
                                   E=st.E, mixed=mixed, frac=frac)
    raise AssertionError(f"no stable seed for {family} at B = {b} in {MAX_TRIES} tries")


def margins_of(c, loss_type, swap):
    """The margins a test runs for one loss type: (1.0, mixed), (1.0,) where there is no mixed one; softmax takes
    no margin."""
    if loss_type == "softmax":
        return (1.0,)
    m = c.mixed[(loss_type, swap)]
    return (1.0,) if m is None else (1.0, m)


def _step(fn, a, p, dtype, upstream):
    x = a.detach().clone().to(dtype).requires_grad_(True)
    y = p.detach().clone().to(dtype).requires_grad_(True)
    loss = fn(x, y)
    (upstream * loss).backward()
    return loss.item(), torch.cat([x.grad, y.grad])


def _reference(fn, a, p, swap, margin, loss_type, upstream, form):
    s = selections(a, p, form)
    l64, g64 = _step(fn, a, p, torch.float64, upstream)
    l32, g32 = _step(fn, a, p, torch.float32, upstream)
    g32 = g32.double()
    n64 = float(g64.norm())
    return SimpleNamespace(loss=l64, grad=g64, row_argmin=s.row_argmin, col_argmin=s.col_argmin,
                           active=active_rows(a, p, swap, margin, loss_type, form), loss32=l32, grad32=g32,
                           e32_row=(g32 - g64).norm(dim=1), g32err=float((g32 - g64).norm()) / n64 if n64 else 0.0)


def reference(a, p, swap, margin, loss_type, upstream=1.0):
    """One step of losses.loss_HardNet(..., fused=False) on fp64 CPU copies: ``loss`` (without the upstream
    factor), ``grad`` = [grad_a; grad_p] of upstream * loss, the row and column argmins of dn, the per-row active
    flags, and the same step in fp32 on the CPU (``loss32``, ``grad32``, per-row ``e32_row`` and matrix-wide
    ``g32err``: the formulation's own fp32 error)."""
    fn = lambda x, y: L.loss_HardNet(x, y, anchor_swap=swap, margin=margin, loss_type=loss_type, fused=False)  # noqa: E731
    return _reference(fn, a, p, swap, margin, loss_type, upstream, "hardnet")


def fan_keypoints(b):
    """Any keypoints: with C = 0 no mask but the diagonal's applies."""
    kp = torch.zeros(b, 4, dtype=torch.int64)
    kp[:, 1], kp[:, 2] = 7 * (torch.arange(b) // 20), 7 * (torch.arange(b) % 20)
    return kp


def reference_neimask(a, p, margin=1.0):
    """The same for losses.loss_neimask(..., C=0, fused=False): anchor_swap always on, the triplet clamp."""
    kp = fan_keypoints(a.shape[0])
    fn = lambda x, y: L.loss_neimask(x, y, kp, kp, margin=margin, C=0.0, fused=False)  # noqa: E731
    return _reference(fn, a, p, True, margin, "triplet_margin", 1.0, "unit")


def _fan_pairs(b, m, seed, t=FAN_T, s=FAN_S):
    g = torch.Generator().manual_seed(seed)
    a, p = pairs(b, 0.05, 1.0, seed + 7919)
    c, e = _unit(torch.randn(128, generator=g)), _unit(torch.randn(128, generator=g))
    free = [i for i in range(b) if i not in (t, s)]
    perm = torch.randperm(len(free), generator=g).tolist()
    rows = sorted(free[i] for i in perm[:m])            # anchors around c: their hardest negative is column t
    cols = sorted(free[i] for i in perm[m:2 * m])       # positives around e: their column's minimum is row s
    noise = lambda n: torch.randn(n, 128, generator=g)  # noqa: E731
    # the clusters at 0.5 * unit noise; their partners by the rule of every other pair (``pairs``: 0.05 * randn, a
    # distance of about 0.5).  Partners at 0.05 * unit noise (d = 0.05) would put loss_neimask's u = 2 - 2 a.b at
    # 0.0025, where two fp32 summation orders of a.b differ by 1e-4 relative in 1 / (2 D): rule 5 would then weigh
    # the kernel's FMA chain against the CPU's blocked product, not the gather
    a[rows] = _unit(c + 0.5 * _unit(noise(m)))
    p[rows] = _unit(a[rows] + 0.05 * noise(m))
    p[cols] = _unit(e + 0.5 * _unit(noise(m)))
    a[cols] = _unit(p[cols] + 0.05 * noise(m))
    p[t], a[s] = c, e
    return a.contiguous(), p.contiguous(), rows, cols


def check_fan_in(a, p, m, rows, cols, t=FAN_T, s=FAN_S):
    """The fan-in preconditions as a list of failures (empty: met), for both distance forms."""
    bad = []
    for form in ("hardnet", "unit"):
        sel = selections(a, p, form)
        hit_r = (sel.row_argmin == t).nonzero().flatten().tolist()
        won = (sel.col_argmin == s) & (sel.col_min < sel.row_min)
        if hit_r != rows or len(hit_r) != m:
            bad.append(f"{form}: {len(hit_r)} rows select column {t}, want {m}")
        if won.nonzero().flatten().tolist() != cols or int(won.sum()) != m:
            bad.append(f"{form}: {int(won.sum())} columns select row {s} below their row minimum, want {m}")
        # with swap a row of `rows` keeps its row entry (t): the list of positive t has m sources either way
        if not bool((sel.row_min[rows] < sel.col_min[rows]).all()):
            bad.append(f"{form}: a row around c prefers its column minimum")
        for swap, idx in ((False, rows), (True, rows + cols)):
            for lt in ("triplet_margin", "contrastive"):
                if form == "hardnet" or lt == "triplet_margin":
                    if not bool(active_rows(a, p, swap, 1.0, lt, form)[idx].all()):
                        bad.append(f"{form}: a fan-in row is clamped ({lt}, swap {swap})")
        st = stable(a, p, [1.0], form)
        if not st.ok:
            bad.append(f"{form}: not stable {st.worst} (band {st.band:.1e})")
    return bad


@functools.lru_cache(maxsize=None)
def fan_in(m, b=FAN_B, seed=None):
    """B = 200: p[3] = c with exactly m anchors normalize(c + 0.5 unit noise) (those rows' hardest negative is
    column 3: positive 3's source list has m entries), a[7] = e with exactly m positives around e (with
    anchor_swap those columns' minimum is row 7, below their rows' own: anchor 7's list has m entries); every
    other pair random at noise 0.05.  The first seed >= 1000 m (or the given one) meeting ``check_fan_in``."""
    for sd in ([seed] if seed is not None else range(1000 * m, 1000 * m + MAX_TRIES)):
        a, p, rows, cols = _fan_pairs(b, m, sd)
        bad = check_fan_in(a, p, m, rows, cols)
        if not bad:
            return SimpleNamespace(a=a, p=p, m=m, rows=rows, cols=cols, seed=sd, t=FAN_T, s=FAN_S,
                                   band=stable(a, p, [1.0]).band)
    raise AssertionError(f"no fan-in case for m = {m}: {bad}")


@functools.lru_cache(maxsize=None)
def tied(b=65, i=9, j=40, k=52):
    """An exact row / column tie on two different entries, without a mirror image: the 'close' case at b with
    a[k] = a[i] and p[j] = p[i].  Row i's minimum is entry (i, j) and column i's is entry (k, i), both the bits of
    d(a_i, p_i) in fp64 and fp32 alike, so torch.minimum gives each half of row i's gradient: anchors i and k and
    positives j and i get different halves (a duplicated *pair* would hand every row the same sum either way).
    Row k ties over columns i and j and column j over rows i and k: first index, here and in the kernels."""
    c = case("close", b)
    a, p = c.a.clone(), c.p.clone()
    a[k], p[j] = a[i], p[i]
    s = selections(a, p)
    dn32 = masked_distances(a, p)[1]
    for dn in (s.dn, dn32):
        assert float(dn[i, j]) == float(dn[k, i]) == float(dn[k, j])
    assert float(s.row_min[i]) == float(s.col_min[i]) == float(s.dn[i, j])
    assert (int(s.row_argmin[i]), int(s.col_argmin[i])) == (j, k)
    assert (int(s.row_argmin[k]), int(s.col_argmin[j])) == (min(i, j), min(i, k))
    st = stable(a, p, [1.0], ties=True)
    assert st.ok and not stable(a, p, [1.0]).ok, st.worst
    for lt in ("triplet_margin", "contrastive"):
        assert bool(active_rows(a, p, True, 1.0, lt)[[i, j, k]].all())
    return SimpleNamespace(a=a, p=p, i=i, j=j, k=k, band=st.band)


# ---- hn_hardnet_loss -------------------------------------------------------------------------------------------
def loss_inputs(n, seed=0):
    """Synthetic fp32 pos / row_min / col_min of n rows: the triplet and the contrastive clamp are each active on
    some rows and not on others at margins 0.5 and 1.0, with and without col_min."""
    g = torch.Generator().manual_seed(5000 + n + seed)
    pos = 0.1 + 0.9 * torch.rand(n, generator=g)
    rmin = 0.3 + 2.0 * torch.rand(n, generator=g)
    cmin = 0.3 + 2.0 * torch.rand(n, generator=g)
    return pos, rmin, cmin


def loss_terms64(pos, mn, margin, loss_type):
    """The per-row loss of Losses.py:142-153 in fp64 on fp32 inputs."""
    pos, mn = pos.double(), mn.double()
    if loss_type == "triplet_margin":
        return torch.clamp(margin + pos - mn, min=0.0)
    if loss_type == "softmax":
        ep = torch.exp(2.0 - pos)
        return -torch.log(ep / (ep + torch.exp(2.0 - mn) + 1e-8))
    return torch.clamp(margin - mn, min=0.0) + pos


def loss_bound(n, scale, terms):
    """(ceil(n / 1024) + 40) 2^-24 scale sum |l_i|: k_loss's thread sums ceil(n / 1024) terms serially, then 6
    wave steps and 16 partials; 8 ulp for expf / logf per term."""
    return (math.ceil(n / 1024) + 40) * 2.0 ** -24 * scale * float(terms.abs().sum())


# ---- hn_fpr95 --------------------------------------------------------------------------------------------------
def fpr_key32(d):
    """The kernel's fp32 key 1 / (1 / (d + 1e-8) + 1e-8) on a float32 array."""
    one, eps = np.float32(1.0), np.float32(1e-8)
    return one / (one / (d + eps) + eps)


def fpr_case(n, n_match, seed, dim=128):
    """n pairs whose distances are distinct fp32 values 0.1 * 1.002^k (k a permutation of 0..n-1: spaced 2e-3
    relative), ``n_match`` of them labelled 1 at random.  Returns a, p ([n,dim] fp32, the distance on the first
    element, on the last one when dim != 128), labels (int32) and d (fp32)."""
    rng = np.random.RandomState(seed)
    d = (0.1 * 1.002 ** rng.permutation(n).astype(np.float64)).astype(np.float32)
    labels = np.zeros(n, np.int32)
    labels[rng.permutation(n)[:n_match]] = 1
    check_fpr_distances(d)
    a, p = torch.zeros(n, dim), torch.zeros(n, dim)
    p[:, 0 if dim == 128 else dim - 1] = torch.from_numpy(d)
    return a, p, labels, d


def check_fpr_distances(d):
    """No tie ambiguity: sorted, the distances are >= 1e-3 relative apart, and both the fp32 key transform of the
    kernel and the fp64 one of the reference keep them distinct and in that order."""
    assert d.dtype == np.float32
    order = np.argsort(d, kind="stable")
    ds = d[order].astype(np.float64)
    assert len(d) < 2 or (np.diff(ds) / ds[:-1]).min() >= 1e-3
    k32 = fpr_key32(d)[order]
    k64 = 1.0 / (1.0 / (d.astype(np.float64)[order] + 1e-8) + 1e-8)
    assert (np.diff(k32) > 0).all() and (np.diff(k64) > 0).all()


def fpr_expected(labels, d):
    """oracle.hardnet_oracle.error_rate_at_95_recall on the labels as the kernel counts them (!= 0 is a match;
    the reference's cumsum would add a label 2 or -1 raw) and the scores 1 / (d + 1e-8) in fp64."""
    from oracle import hardnet_oracle as O
    return O.error_rate_at_95_recall((np.asarray(labels) != 0).astype(np.int64), 1.0 / (d.astype(np.float64) + 1e-8))
