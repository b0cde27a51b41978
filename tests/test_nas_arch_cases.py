"""The architecture sets of nas_arch_cases.py cover what they claim, and their reference is fit to judge by.

The GPU file (test_gpu_nas_arch_pairs.py) holds the kernels to NAS_TOL = 2e-5 against the fp64 oracle on these
weights and patches.  That bar means something only if (a) the oracle's own rounding is far below it and (b)
the activations keep the fp16x3 split of the 1x1 convs in its normal range, so a failure is
the kernel's and a pass is not luck.  Both are checked here, on the CPU, for every architecture of C and every
8th of A and B (both oracles for all 400 take over a minute)."""
import itertools

import numpy as np
import pytest
import torch

import nas_arch_cases as C
from hardnetnas_amd import arch as A

REF_TOL = 1e-6            # fp32 oracle vs fp64 oracle: 1/20 of NAS_TOL
RMS_MIN, PEAK_MAX = 1e-2, 100.0
SAMPLED = sorted(set(C.IDX_C) | set(range(0, C.C10, 8)))


def test_set_sizes_and_names():
    assert C.OPS[0] == "skip" and len(C.OPS) == 17
    assert (len(C.SET_A), len(C.SET_B), len(C.SET_C1), len(C.SET_C2)) == (289, 63, 32, 16)
    assert (C.A0, C.B0, C.C10, C.C20, len(C.ARCHS)) == (0, 289, 352, 384, 400)
    for ops in C.ARCHS:
        assert A.arch_ops(ops) == ops
    assert len({tuple(o) for o in C.ARCHS}) >= 395  # (a few of B / C may repeat one of A)
    assert [C.set_of(i) for i in (0, 288, 289, 351, 352, 383, 384, 399)] == ["A", "A", "B", "B", "C1", "C1", "C2", "C2"]
    assert C.seed_of(0) == 1000 and all(0 <= i < len(C.ARCHS) for i in C.SEED_OVERRIDE)


def test_a_has_every_ordered_op_pair_at_every_slot_pair():
    slot_pairs = list(itertools.combinations(range(6), 2))
    assert len(slot_pairs) == 15
    for l1, l2 in slot_pairs:
        seen = {(ops[l1], ops[l2]) for ops in C.SET_A}
        assert len(seen) == 17 * 17, (l1, l2)
    # the five layer boundaries: 5 x 289 = 1,445 ordered (op, next op) pairs
    assert sum(len({(o[l], o[l + 1]) for o in C.SET_A}) for l in range(5)) == 1445


def test_a_and_b_have_all_64_skip_patterns():
    pat = {tuple(o == "skip" for o in ops) for ops in C.SET_A + C.SET_B}
    assert len(pat) == 64
    for mask, ops in zip(range(1, 64), C.SET_B):
        assert [o == "skip" for o in ops] == [bool(mask >> l & 1) for l in range(6)]


def test_c_seams():
    assert len(C.X_OPS) == 8 and all(not A.OP_SPECS[o].se for o in C.X_OPS)
    assert sorted(C.PAIR_L) == ["ir_k3_e1", "ir_k3_s2", "ir_k5_e1", "ir_k5_s2"]
    assert {(o[3], o[4]) for o in C.SET_C1} == set(C.PAIRS_LN) and len(set(C.PAIRS_LN)) == 32
    for ops in C.SET_C1:
        assert ops[:2] == ["skip", "skip"] and ops[2] in C.X_OPS
        st = C.expected_stages(ops)
        assert st["front+irf"] == 1 and st["irf2"] == 1 and "front" not in st
    for x in C.X_OPS:  # four per X, with every L
        mine = [o for o in C.SET_C1 if o[2] == x]
        assert len(mine) == 4 and {o[3] for o in mine} == set(C.PAIR_L)
    assert {o[5] for o in C.SET_C1} == set(C.OPS)
    for x in C.X_OPS:
        assert sum(o[2] == x for o in C.SET_C2) == 2
    c2 = [C.expected_stages(o) for o in C.SET_C2]
    assert all(o[3:5] == ["skip", "skip"] for o in C.SET_C2)
    # every way of reaching (or pre-empting) k_irf_skip: behind the generic and the max-pool front, with layer 2
    # taken by k_mpfront_irf, with layer 2 taken by k_irf2
    assert sum("irf+skip" in s for s in c2) >= 8
    assert any("irf+skip" in s and o[0] == "skip" for s, o in zip(c2, C.SET_C2))
    assert any("irf+skip" in s and o[0] != "skip" and o[1] == "skip" for s, o in zip(c2, C.SET_C2))
    assert any("front+irf" in s for s in c2) and any("irf2" in s for s in c2)


def test_expected_stages_of_the_registry_archs():
    """The launch prediction on architectures whose stages the GPU suite already pins."""
    assert C.expected_stages(A.MODEL_ARCH["wang2"]) == {"front": 1, "irf2": 2, "head": 1}
    assert C.expected_stages(A.MODEL_ARCH["wang3"]) == {"front": 1, "irf+skip": 1, "head": 1}
    assert C.expected_stages(A.MODEL_ARCH["wang4"]) == {"front+irf": 1, "irf2": 1, "irf": 1, "head": 1}
    assert C.expected_stages(["ir_k3_e1_se"] * 6) == {"front": 1, "se": 6, "irf": 5, "head": 1}
    assert C.expected_stages(["ir_k3_e1"] * 3 + ["ir_k5_s2", "ir_k3_s2_se", "skip"]) == \
        {"front": 1, "irf2": 2, "se": 1, "head": 1}


def test_inputs_are_reproducible():
    x = C.patches()
    assert tuple(x.shape) == (37, 1, 32, 32) and x.dtype == torch.float32
    u = C.u8_patches()
    assert tuple(u.shape) == (37, 32, 32) and u.dtype == torch.uint8 and len(torch.unique(u)) == 256
    m, p = C.model(352)
    m2, p2 = C._synth_nas(C.ARCHS[352], seed=1352)
    assert all(torch.equal(p[k], p2[k]) for k in p)


@pytest.mark.parametrize("group", range(4))
def test_reference_conditions(group):
    """fp32 oracle within 1e-6 of the fp64 oracle; every non-depthwise conv's input with rms >= 1e-2 and
    peak <= 100; unit-norm, finite descriptors."""
    bad, worst, lo, hi = [], 0.0, np.inf, 0.0
    for i in SAMPLED[group::4]:
        _, p = C.model(i)
        y64, stats = C.reference_with_conv_inputs(i, p, torch.float64)
        y32 = C.reference(i, p, torch.float32)
        assert len(stats) == C.n_dense_convs(C.ARCHS[i]), (i, len(stats))
        e = float(np.abs(y32.astype(np.float64) - y64).max())
        rms, peak = min(s[0] for s in stats), max(s[1] for s in stats)
        worst, lo, hi = max(worst, e), min(lo, rms), max(hi, peak)
        ok = (np.isfinite(y64).all() and e <= REF_TOL and rms >= RMS_MIN and peak <= PEAK_MAX
              and np.abs(np.linalg.norm(y64, axis=1) - 1.0).max() <= 1e-12)
        if not ok:
            bad.append((i, C.set_of(i), C.ARCHS[i], e, rms, peak))
    print(f"group {group}: fp32 vs fp64 oracle max {worst:.2e}; smallest rms {lo:.3g}, largest peak {hi:.3g}")
    assert not bad, bad
