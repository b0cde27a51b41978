"""The NAS eval forward over the architecture sets of nas_arch_cases.py: every ordered pair of ops at every pair
of slots (A), every skip / non-skip pattern (B) and the seams of the fused kernels (C), 400 architectures at the
ragged batch 37, against the fp64 oracle at the project's NAS bar (NAS_TOL = 2e-5 max abs).

Which kernels run, how the four activation buffers rotate, where the head's split-K scratch lies and how large
the workspace is all depend on what is adjacent to what, so for every architecture of B and C the invariants the
project claims bit for bit are checked too: a poisoned workspace, guard bands, chunking, the uint8 entry, and the
layerwise kernels against the same reference (which tells a fused kernel's error from an unfused one's).
test_dispatch_coverage then checks, from the stage counts the other tests recorded, that the sets reached the
launches they were built for."""
import numpy as np
import pytest
import torch

import nas_arch_cases as C
from hardnetnas_amd import arch as A
from test_gpu_parity import NAS_TOL

pytestmark = pytest.mark.gpu

# |row norm - 1|: the head normalises in fp32 -- a 128-term sum of squares, a square root and a division, each
# term within 2^-24 relative: (128 + 2) * 2^-24 = 7.7e-6 at the very worst
NORM_TOL = 1e-5
FUSED_STAGES = ("front", "front+irf", "irf", "irf2", "irf+skip", "skip")

CENSUS = {}  # architecture index -> {stage: launches} of one default-knob fp32 forward
ERRS = {}    # architecture index -> max |y - y64| of that forward


def _native(m, dev, monkeypatch=None, **env):
    """NativeModel of module m created under the environment knobs ``env`` (hn_create reads them)."""
    from hardnetnas_amd._native import NativeModel
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    nm = NativeModel.from_module(m, dev)
    for k in env:
        monkeypatch.delenv(k)
    return nm


def _profiled(nm, x):
    """(descriptors, {stage: launches}) of one forward."""
    nm.set_profiling(True)
    y = nm.forward(x)
    torch.cuda.synchronize()
    st = {k: int(c) for k, (_, c) in nm.stage_times().items() if c}
    nm.set_profiling(False)
    return y, st


def _err(y, y64):
    return float(np.abs(y.cpu().numpy().astype(np.float64) - y64).max())


def _default_forward(i, dev):
    """Architecture i at the default knobs: (module, NativeModel, descriptors, fp64 reference, error); records the
    stage counts and the error."""
    m, p = C.model(i)
    y64 = C.reference(i, p)
    nm = _native(m, dev)
    y, st = _profiled(nm, C.patches().to(dev))
    CENSUS[i], ERRS[i] = st, _err(y, y64)
    return m, nm, y, y64, ERRS[i]


def _assert_descriptors(i, y, err, what="default knobs", more=""):
    tag = f"arch {i} (set {C.set_of(i)}) {C.ARCHS[i]}, {what}"
    assert torch.isfinite(y).all(), tag
    assert err <= NAS_TOL, f"{tag}: max|y - y64| = {err:.3e} > {NAS_TOL:g}{more}"
    norm = float((y.double().norm(dim=1) - 1.0).abs().max())
    assert norm <= NORM_TOL, f"{tag}: |row norm - 1| = {norm:.3e}"


def _report(name, idx):
    w = max(idx, key=lambda i: ERRS[i])
    print(f"{name}: worst max|y - y64| = {ERRS[w]:.3e} at arch {w} {C.ARCHS[w]}")


def _check_invariants(i, m, nm, y, dev, monkeypatch):
    """The bit-for-bit claims on architecture i (nm: its default-knob model, y: its descriptors at b = 37)."""
    tag = f"arch {i} (set {C.set_of(i)}) {C.ARCHS[i]}"
    b = C.BATCH
    x = C.patches().to(dev)
    ws_bytes = nm.workspace_bytes(b)
    # a workspace of 0x00 bytes and one of 0xFF bytes (every float a NaN)
    for fill in (0x00, 0xFF):
        yw = nm.forward(x, workspace=torch.full((ws_bytes,), fill, dtype=torch.uint8, device=dev))
        assert torch.equal(yw, y), f"{tag}: workspace pre-filled with {fill:#04x} changes the descriptors"
    # 1 MiB guard bands around exactly workspace_bytes(b) bytes, 8 guard rows around the output
    G = 1 << 20
    buf = torch.full((G + ws_bytes + G,), 0xA5, dtype=torch.uint8, device=dev)
    ws = buf[G:G + ws_bytes]
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and ws.numel() == ws_bytes
    sentinel = -12345.0
    outbuf = torch.full((b + 16, 128), sentinel, device=dev)
    out = outbuf[8:8 + b]
    yg = nm.forward(x, out=out, workspace=ws)
    assert yg.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + ws_bytes:] == 0xA5).all()), f"{tag}: workspace guard"
    assert bool((outbuf[:8] == sentinel).all()) and bool((outbuf[8 + b:] == sentinel).all()), f"{tag}: output guard"
    assert torch.equal(out, y), tag
    # chunks of 64 at b = 165 (64 + 64 + 37: the last chunk smaller than the one the buffers are laid out for)
    x165 = C.patches(165, 11).to(dev)
    full = nm.forward(x165)
    chunked = _native(m, dev, monkeypatch, HN_CHUNK=64)
    assert chunked.workspace_bytes(165) == nm.workspace_bytes(64)
    assert torch.equal(chunked.forward(x165), full), f"{tag}: HN_CHUNK=64 at 165 patches"
    # uint8 patches: preprocessing fused into the front's patch load (k_mpfront_irf is bypassed) against
    # preprocess + forward
    from hardnetnas_amd._native import preprocess
    u = C.u8_patches().to(dev)
    assert torch.equal(nm.forward_u8(u, resize="none"), nm.forward(preprocess(u, resize="none"))), f"{tag}: forward_u8"


def _layerwise(i, m, y64, dev, monkeypatch):
    """(descriptors, error, stage counts) of the layer-by-layer kernels on architecture i."""
    lw = _native(m, dev, monkeypatch, HN_NO_FRONT=1, HN_NO_IRF=1, HN_NO_SKIPFUSE=1)
    y, st = _profiled(lw, C.patches().to(dev))
    return y, _err(y, y64), st


def _run_group(name, idx, dev, monkeypatch=None):
    for i in idx:
        m, nm, y, y64, err = _default_forward(i, dev)
        if monkeypatch is None:
            _assert_descriptors(i, y, err)
            continue
        ylw, elw, stlw = _layerwise(i, m, y64, dev, monkeypatch)
        _assert_descriptors(i, y, err, more=f" (layerwise kernels: {elw:.3e}; stages {CENSUS[i]})")
        _assert_descriptors(i, ylw, elw, what="layerwise kernels")
        assert not set(stlw) & set(FUSED_STAGES), (i, stlw)
        _check_invariants(i, m, nm, y, dev, monkeypatch)
    _report(name, idx)


@pytest.mark.parametrize("a", range(17))
def test_set_a_every_op_pair(a, cuda_device):
    """The 17 architectures ops[l] = OPS[(a + l*b) % 17], b = 0..16."""
    _run_group(f"A[a={a}]", C.IDX_A[17 * a:17 * a + 17], cuda_device)


@pytest.mark.parametrize("g", range(8))
def test_set_b_every_skip_pattern(g, cuda_device, monkeypatch):
    """Skip masks 8g + 1 .. 8g + 8 (the last group: 7), with the bit-for-bit invariants."""
    _run_group(f"B[{g}]", C.IDX_B[8 * g:8 * g + 8], cuda_device, monkeypatch)


@pytest.mark.parametrize("g", range(6))
def test_set_c_fused_kernel_seams(g, cuda_device, monkeypatch):
    """C1 (groups 0-3: k_mpfront_irf before k_irf2) and C2 (groups 4, 5: k_irf_skip behind every front), with the
    bit-for-bit invariants."""
    _run_group(f"C[{g}]", C.IDX_C[8 * g:8 * g + 8], cuda_device, monkeypatch)


def test_dispatch_coverage(cuda_device):
    """What the sets were built to reach was launched.  The expectations come from arch.OP_SPECS / arch.ir_mid
    (nas_arch_cases.expected_stages), not from the library's shape tables."""
    x = C.patches().to(cuda_device)
    for i in range(len(C.ARCHS)):  # (whatever the tests above have not run, e.g. under -k)
        if i not in CENSUS:
            CENSUS[i] = _profiled(_native(C.model(i)[0], cuda_device), x)[1]
    seen = set().union(*CENSUS.values())
    assert {"front", "front+irf", "irf", "irf2", "irf+skip", "skip", "se", "head"} <= seen, seen
    for i in C.IDX_C1:
        ops, st = C.ARCHS[i], CENSUS[i]
        n_se = sum(A.OP_SPECS[o].se for o in ops if o != "skip")
        assert st.get("front+irf") == 1 and st.get("irf2") == 1 and "front" not in st, (i, ops, st)
        assert st.get("se", 0) == n_se and n_se >= A.OP_SPECS[ops[4]].se, (i, ops, st)
    for i in C.IDX_C2:
        ops, st = C.ARCHS[i], CENSUS[i]
        # (k_irf_skip runs unless layer 2 went to k_irf2 with layer 1, or to k_mpfront_irf behind two skips)
        if not C._pair_ok(ops, 1) and "front+irf" not in C.expected_stages(ops):
            assert st.get("irf+skip") == 1 and "skip" not in st, (i, ops, st)
    # A alone launches k_irf2 on all 32 (L, N) pairs at slots (1, 2) and at slots (3, 4): all eight (ka, kb) kernels
    for l in (1, 3):
        got = {(C.ARCHS[i][l], C.ARCHS[i][l + 1]) for i in C.IDX_A if C._pair_ok(C.ARCHS[i], l)
               and CENSUS[i].get("irf2", 0) >= 1}
        assert got == set(C.PAIRS_LN), (l, sorted(set(C.PAIRS_LN) - got))
    # every architecture: exactly the predicted launches (no fall-back to the layerwise pw / dw / pwl kernels)
    wrong = [(i, C.ARCHS[i], CENSUS[i], C.expected_stages(C.ARCHS[i])) for i in range(len(C.ARCHS))
             if CENSUS[i] != C.expected_stages(C.ARCHS[i])]
    assert not wrong, wrong[:5]
    for name, idx in (("A", C.IDX_A), ("B", C.IDX_B), ("C1", C.IDX_C1), ("C2", C.IDX_C2)):
        if all(i in ERRS for i in idx):
            _report(f"set {name}", idx)
    for k in sorted(seen):
        print(f"stage {k!r}: in {sum(k in s for s in CENSUS.values())} of {len(CENSUS)} architectures, "
              f"{sum(s.get(k, 0) for s in CENSUS.values())} launches")
