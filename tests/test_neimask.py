"""FDLNet's neighbour-mask descriptor loss without a GPU: the torch formulation of hardnetnas_amd.losses and
``HardNetNeiMask.loss`` against the reference's recorded results (tests/golden/neimask_loss.npz, made by
tests/golden/make_neimask_golden.py from FDLNet-master/latency/NASNet/model/des.py:57-96), and the argument
checks of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from fixtures import load
from hardnetnas_amd import _native as N
from hardnetnas_amd import losses as L


@pytest.fixture(scope="module")
def fx():
    return load("neimask_loss")


def _inputs(fx, dtype, pre=""):
    a, p = (torch.from_numpy(fx[pre + k]).to(dtype).requires_grad_(True) for k in ("a", "p"))
    return a, p, torch.from_numpy(fx[pre + "akp"]), torch.from_numpy(fx[pre + "pkp"])


@pytest.mark.parametrize("via", ["function", "module"])
def test_formulation_matches_reference(via, fx):
    """fp32: the reference's fp32 loss bit for bit (the same torch operations in the same order); fp64: its fp64
    loss, gradients, pos, min_neg and argmins."""
    from hardnetnas_amd.model import HardNetNeiMask
    m = fx["meta"]
    des = HardNetNeiMask(MARGIN=m["MARGIN"], C=m["C"])

    def loss_of(a, p, akp, pkp):
        if via == "module":
            return des.loss(a, p, akp, pkp)
        return L.loss_neimask(a, p, akp, pkp, margin=m["MARGIN"], C=m["C"])

    a, p, akp, pkp = _inputs(fx, torch.float32)
    assert loss_of(a, p, akp, pkp).item() == float(fx["loss32"])
    a, p, akp, pkp = _inputs(fx, torch.float64)
    loss = loss_of(a, p, akp, pkp)
    loss.backward()
    assert abs(loss.item() - float(fx["loss64"])) <= 1e-12
    for g, k in ((a.grad, "ga64"), (p.grad, "gp64")):
        ref = fx[k].astype(np.float64)
        assert np.linalg.norm(g.numpy() - ref) / np.linalg.norm(ref) <= 1e-6  # (stored as fp32)
    d, dn = L.neimask_masked_distances(a.detach(), p.detach(), akp, pkp, m["C"])
    assert np.abs(d.diag().numpy() - fx["pos64"]).max() <= 1e-12
    assert np.abs(torch.min(dn.min(1)[0], dn.min(0)[0]).numpy() - fx["min_neg64"]).max() <= 1e-12
    assert np.array_equal(dn.argmin(1).numpy(), fx["row_argmin"])
    assert np.array_equal(dn.argmin(0).numpy(), fx["col_argmin"])
    lo, hi = m["low_clamp"], m["high_clamp"]
    assert abs(d[lo[0], lo[1]].item() - 1e-4) <= 1e-12  # the low clamp: sqrt(1e-8)
    assert d[hi[0], hi[1]].item() == 2.0


def test_all_masked_is_exactly_zero(fx):
    a, p, akp, pkp = _inputs(fx, torch.float32, "all/")
    loss = L.loss_neimask(a, p, akp, pkp, margin=1.0, C=5.0)
    loss.backward()
    assert loss.item() == 0.0 and not a.grad.any() and not p.grad.any()


def test_c_zero_is_the_plain_hardest_in_batch_loss(fx):
    """C = 0 masks nothing, the diagonal included (kd = 1e-4 there): des.py:61."""
    a, p, akp, pkp = _inputs(fx, torch.float64)
    loss = L.loss_neimask(a, p, akp, pkp, margin=1.0, C=0.0)
    assert abs(loss.item() - float(fx["loss64_C0"])) <= 1e-12
    from hardnetnas_amd.matching import distance_matrix_vector
    d = distance_matrix_vector(a, p)
    dn = d + 10 * torch.eye(d.size(0), dtype=d.dtype)
    plain = torch.clamp(1.0 + d.diag() - torch.minimum(dn.min(1)[0], dn.min(0)[0]), min=0.0).mean()
    assert abs(loss.item() - plain.item()) <= 1e-12
    assert loss.item() > 2 * float(fx["loss64"])  # the masks matter on these inputs


def test_pair_distance_loss_is_the_matrix_diagonal(fx):
    from hardnetnas_amd.matching import distance_matrix_vector
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-6)):
        a, p, _, _ = _inputs(fx, dtype)
        got = L.pair_distance_loss(a, p)
        ref = distance_matrix_vector(a, p).diag().mean()
        assert abs(got.item() - ref.item()) <= tol
        got.backward()
        assert a.grad is not None and torch.isfinite(a.grad).all()
    with pytest.raises(ValueError):
        L.pair_distance_loss(torch.zeros(3, 128), torch.zeros(4, 128))


def test_shape_mismatches_raise(fx):
    a, p, akp, pkp = (t.detach() for t in _inputs(fx, torch.float32))
    with pytest.raises(ValueError):
        L.loss_neimask(a, p[:-1], akp, pkp)
    with pytest.raises(ValueError):
        L.loss_neimask(a[0], p[0], akp, pkp)
    with pytest.raises(ValueError):
        L.loss_neimask(a, p, akp[:-1], pkp)
    with pytest.raises(ValueError):
        L.loss_neimask(a, p, akp, pkp[:, :2])
    with pytest.raises(ValueError):
        L.loss_neimask(a, p, akp.reshape(-1), pkp)


PTR = 0x1000  # a non-NULL, 16-byte aligned value: every check below fails before a pointer is followed


def _fwd(lib, **kw):
    a = dict(a=PTR, p=PTR, akp=PTR, pkp=PTR, batch=8, dim=128, loss=PTR, pos=None, mn=None, saved=PTR, nbytes=1 << 20)
    a.update(kw)
    return lib.hn_neimask_loss_forward(a["a"], a["p"], a["akp"], a["pkp"], a["batch"], a["dim"], 1.0, 5.0, a["loss"],
                                       a["pos"], a["mn"], a["saved"], a["nbytes"], None)


def _bwd(lib, **kw):
    a = dict(a=PTR, p=PTR, batch=8, dim=128, dloss=PTR, ga=PTR, gp=PTR, saved=PTR, nbytes=1 << 20)
    a.update(kw)
    return lib.hn_neimask_loss_backward(a["a"], a["p"], a["batch"], a["dim"], 1.0, a["dloss"], a["ga"], a["gp"],
                                        a["saved"], a["nbytes"], None)


def test_c_entry_points_check_their_arguments():
    lib = N.load_library()
    n = ctypes.c_size_t()
    assert lib.hn_neimask_loss_workspace_bytes(200, ctypes.byref(n)) == 0
    # keys 2 x 8 B, pos 4 B, coef 12 B, idx 8 B and four lists of 8 B per row, each block padded to 256 B
    assert 200 * 72 <= n.value <= 200 * 72 + 9 * 256 and n.value % 256 == 0
    assert lib.hn_neimask_loss_workspace_bytes(0, ctypes.byref(n)) == 1 and b"batch" in lib.hn_last_error()
    assert lib.hn_neimask_loss_workspace_bytes((1 << 22) + 1, ctypes.byref(n)) == 1
    assert lib.hn_neimask_loss_workspace_bytes(8, None) == 1
    for call in (_fwd, _bwd):
        assert call(lib, dim=64) == 1 and b"dim must be 128" in lib.hn_last_error()
        assert call(lib, batch=0) == 1 and b"batch" in lib.hn_last_error()
        assert call(lib, a=None) == 1 and b"NULL" in lib.hn_last_error()
        assert call(lib, p=None) == 1 and b"NULL" in lib.hn_last_error()
        assert call(lib, saved=None) == 1 and b"NULL" in lib.hn_last_error()
        assert call(lib, a=PTR + 4) == 1 and b"aligned" in lib.hn_last_error()
        assert call(lib, saved=PTR + 8) == 1 and b"aligned" in lib.hn_last_error()
        assert call(lib, nbytes=8 * 72) == 4 and b"workspace" in lib.hn_last_error()  # HN_ERR_WORKSPACE
    assert _fwd(lib, akp=None) == 1 and b"NULL" in lib.hn_last_error()
    assert _fwd(lib, pkp=None) == 1 and b"NULL" in lib.hn_last_error()
    assert _fwd(lib, loss=None) == 1 and b"NULL" in lib.hn_last_error()
    assert _fwd(lib, akp=PTR + 4) == 1 and b"8-byte" in lib.hn_last_error()
    assert _fwd(lib, pos=PTR + 2) == 1 and b"4-byte" in lib.hn_last_error()
    for k in ("dloss", "ga", "gp"):
        assert _bwd(lib, **{k: None}) == 1 and b"NULL" in lib.hn_last_error()
    assert _bwd(lib, ga=PTR + 4) == 1 and b"8-byte" in lib.hn_last_error()


def test_cpu_tensors_never_reach_the_kernels(fx, monkeypatch):
    """CPU, fp64 and fused=False run the torch formulation: the native Function is not entered."""
    def boom(*a, **k):
        raise AssertionError("native path taken")
    monkeypatch.setattr(N.NeiMaskLossFunction, "apply", boom)
    a, p, akp, pkp = _inputs(fx, torch.float32)
    assert L.loss_neimask(a, p, akp, pkp).grad_fn is not None
