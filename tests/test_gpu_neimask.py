"""FDLNet's neighbour-mask descriptor loss on the GPU (hn_neimask_loss_forward / hn_neimask_loss_backward through
``losses.loss_neimask`` and ``HardNetNeiMask.loss``) against the reference's recorded results
(tests/golden/neimask_loss.npz) and against the torch formulation (``fused=False``).

Bounds.  Fixture: |loss - fp64 reference| <= max(1e-6, the reference's own fp32 error), gradients L2-relative
<= max(1e-5, 3x the reference's own fp32 gradient error) -- the margins of
test_gpu_pairs.py::test_fused_train_loss_matches_reference_backward, for the same reason: the kernels round as an
fp32 implementation of the formulation does, in another summation order.  pos / min_neg: 3x E_ref, the
reference's own fp32 error of D.  Same-GPU comparisons (two fp32 implementations, u of order 1 with an error of a
few 1e-7, 1 / (2 D) of order 1): loss 1e-5, gradients L2-relative 1e-4, as the stock loss's same-GPU test."""
import ctypes

import numpy as np
import pytest
import torch

from fixtures import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load("neimask_loss")


def _clustered(n, seed, frame=(240, 320)):
    """The fixture's kind of input at any size: clusters of 5 keypoints within +-2 pixels with similar
    descriptors, positives moved by up to +-3 pixels, rows permuted (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    unit = torch.nn.functional.normalize
    k = (n + 4) // 5
    which = torch.arange(n) // 5
    cd = unit(torch.randn(k, 128, generator=g), dim=1)
    ck = torch.stack([torch.randint(8, frame[0] - 8, (k,), generator=g),
                      torch.randint(8, frame[1] - 8, (k,), generator=g)], 1)
    a = unit(cd[which] + 0.5 * unit(torch.randn(n, 128, generator=g), dim=1), dim=1)
    p = unit(a + 0.3 * unit(torch.randn(n, 128, generator=g), dim=1), dim=1)
    akp, pkp = torch.zeros(n, 4, dtype=torch.int64), torch.zeros(n, 4, dtype=torch.int64)
    akp[:, 1:3] = ck[which] + torch.randint(-2, 3, (n, 2), generator=g)
    pkp[:, 1:3] = akp[:, 1:3] + torch.randint(-3, 4, (n, 2), generator=g)
    perm = torch.randperm(n, generator=g)
    return a[perm].clone(), p[perm].clone(), akp[perm].clone(), pkp[perm].clone()


def _step(a, p, akp, pkp, dev, dtype=torch.float32, **kw):
    """(loss, [grad_anchor; grad_positive], grad_fn name) of one loss_neimask step on dev."""
    from hardnetnas_amd.losses import loss_neimask
    x = a.detach().clone().to(device=dev, dtype=dtype).requires_grad_(True)   # (fresh leaves on every call)
    y = p.detach().clone().to(device=dev, dtype=dtype).requires_grad_(True)
    loss = loss_neimask(x, y, akp.to(dev), pkp.to(dev), **kw)
    loss.backward()
    return loss.item(), torch.cat([x.grad, y.grad]), type(loss.grad_fn).__name__


def test_fixture_parity(fx, cuda_device):
    from hardnetnas_amd import _native as N
    m = fx["meta"]
    a, p, akp, pkp = (torch.from_numpy(fx[k]) for k in ("a", "p", "akp", "pkp"))
    res = [_step(a, p, akp, pkp, cuda_device, margin=m["MARGIN"], C=m["C"]) for _ in range(2)]
    assert "NeiMaskLossFunction" in res[0][2]
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])  # bit-identical run to run
    el = abs(res[0][0] - float(fx["loss64"]))
    ref = np.concatenate([fx["ga64"], fx["gp64"]]).astype(np.float64)
    eg = np.linalg.norm(res[0][1].cpu().numpy() - ref) / np.linalg.norm(ref)
    print(f"loss {res[0][0]:.7f}: err {el:.2e} (reference fp32 {m['loss_err32']:.2e}), "
          f"grad L2-rel {eg:.2e} (reference fp32 {m['grad_err32']:.2e})")
    assert el <= max(1e-6, m["loss_err32"])
    assert eg <= max(1e-5, 3 * m["grad_err32"])
    # the selections themselves, and pos / min_neg
    loss, pos, mn, saved = N.neimask_loss_forward(a.to(cuda_device), p.to(cuda_device), akp.to(cuda_device),
                                                  pkp.to(cuda_device), m["MARGIN"], m["C"])
    assert loss.item() == res[0][0]
    r, c = N.neimask_saved_argmins(saved, a.shape[0])
    assert np.array_equal(r.cpu().numpy(), fx["row_argmin"]) and np.array_equal(c.cpu().numpy(), fx["col_argmin"])
    ep = np.abs(pos.cpu().numpy() - fx["pos64"]).max()
    em = np.abs(mn.cpu().numpy() - fx["min_neg64"]).max()
    print(f"pos {ep:.2e}, min_neg {em:.2e} (E_ref {m['E_ref']:.2e})")
    assert ep <= 3 * m["E_ref"] and em <= 3 * m["E_ref"]
    lo = m["low_clamp"][0]
    assert pos[lo].item() == float(np.sqrt(np.float32(1e-8)))  # the low clamp on the diagonal ...
    ga = res[0][1][:a.shape[0]]
    assert ga[lo].abs().max().item() > 0  # ... (row lo still gets its negative's gradient)
    # without the masks the same kernels give the plain hardest-in-batch loss
    l0 = _step(a, p, akp, pkp, cuda_device, margin=m["MARGIN"], C=0.0)[0]
    assert abs(l0 - float(fx["loss64_C0"])) <= 1e-6


def test_all_masked_is_exactly_zero(fx, cuda_device):
    a, p, akp, pkp = (torch.from_numpy(fx["all/" + k]) for k in ("a", "p", "akp", "pkp"))
    loss, g, fn = _step(a, p, akp, pkp, cuda_device, margin=1.0, C=5.0)
    assert "NeiMaskLossFunction" in fn
    assert loss == 0.0 and not g.any()


def test_ties(cuda_device):
    """Hand-built exact ties at N = 200, as test_gpu_pairs.py::test_fused_train_loss_ties: duplicated positives
    (two equal columns in different column tiles), duplicated anchors in different 64-row workgroups, a duplicated
    pair (the row and the column minimum of a row equal: the 0.5 / 0.5 split), and one positive that is every
    row's hardest negative (the gather's long-list path); the lowest index wins.  Keypoints on a 7-pixel grid (no
    mask but the diagonal's) in the first case, clustered in the second.  Against fused=False in fp64."""
    g = torch.Generator().manual_seed(7)
    b = 200
    unit = lambda v: torch.nn.functional.normalize(v, dim=-1)  # noqa: E731
    c = unit(torch.randn(128, generator=g))
    a = unit(c + 0.5 * unit(torch.randn(b, 128, generator=g)))   # anchors clustered around c
    p = unit(a + 0.3 * unit(torch.randn(b, 128, generator=g)))
    p[150] = p[20]          # equal columns 20 / 150 for every row (tie across column tiles)
    a[130] = a[10]          # equal rows 10 / 130 (different 64-row workgroups)
    a[77], p[77] = a[5].clone(), p[5].clone()  # a duplicated pair: row / column minima tie
    a2, p2 = a.clone(), p.clone()
    p2[3] = c               # case 2: the cluster centre is every anchor's hardest negative (long list)
    grid = torch.zeros(b, 4, dtype=torch.int64)
    grid[:, 1], grid[:, 2] = 7 * (torch.arange(b) // 20), 7 * (torch.arange(b) % 20)
    _, _, akp, pkp = _clustered(b, 5)
    pkp[3, 1:3] = 1000      # (the centre's keypoint far from every other, so that no mask hides it)
    for aa, pp, ka, kp in ((a, p, grid, grid), (a2, p2, akp, pkp)):
        loss, gg, _ = _step(aa, pp, ka, kp, cuda_device, margin=1.0, C=5.0)
        ref, gr, _ = _step(aa, pp, ka, kp, torch.device("cpu"), dtype=torch.float64, margin=1.0, C=5.0, fused=False)
        assert abs(loss - ref) <= 1e-5
        err = float((gg.cpu().double() - gr).norm() / gr.norm())
        assert err <= 1e-4, err


@pytest.mark.parametrize("n", [1, 63, 65, 512])
def test_matches_torch_formulation_on_gpu(n, cuda_device):
    """The tile-remainder edges (one row; one short of a tile; one over) and the reference's own size
    (B * TOPK = 512) against fused=False on the same GPU."""
    a, p, akp, pkp = _clustered(n, 100 + n)
    loss, g, fn = _step(a, p, akp, pkp, cuda_device, margin=1.0, C=5.0)
    ref, gr, rfn = _step(a, p, akp, pkp, cuda_device, margin=1.0, C=5.0, fused=False)
    assert "NeiMaskLossFunction" in fn and "NeiMaskLossFunction" not in rfn
    eg = (g - gr).norm().item()
    print(f"N={n}: loss {loss:.6f} vs {ref:.6f}, grad diff {eg:.2e} of {gr.norm().item():.2e}")
    assert abs(loss - ref) <= 1e-5
    assert eg <= 1e-4 * gr.norm().item()
    if n == 1:
        assert loss == 0.0 and not g.any()  # the only entry is the masked diagonal


def test_keypoint_values_never_index_memory(cuda_device):
    """Keypoints are compared, never used as indices: int64 extremes and negative coordinates leave the
    canary-padded workspace, the padded outputs and the inputs untouched, and a later call is unaffected.
    Small negative coordinates still give the formulation's result."""
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    n, pad = 130, 512
    a, p, akp, pkp = (t.to(cuda_device) for t in _clustered(n, 9))
    want = N.neimask_loss_forward(a, p, akp, pkp, 1.0, 5.0)[0].item()
    wild_a, wild_p = akp.clone(), pkp.clone()
    lim = torch.iinfo(torch.int64)
    wild_a[0, 1:3] = torch.tensor([lim.min, lim.max])
    wild_a[1, 1:3] = torch.tensor([lim.max, lim.max])
    wild_a[64] = lim.min
    wild_p[2, 1:3] = torch.tensor([-7, 1 << 40])
    wild_p[129] = lim.max
    nb = ctypes.c_size_t()
    assert lib.hn_neimask_loss_workspace_bytes(n, ctypes.byref(nb)) == 0
    ws = torch.full((pad + nb.value + pad,), 0xA5, dtype=torch.uint8, device=cuda_device)
    out = torch.full((64 + 1 + 64 + n + 64 + n + 64,), -777.0, device=cuda_device)   # loss | pos | min_neg
    grads = torch.full((64 * 128 + 2 * n * 128 + 64 * 128,), -777.0, device=cuda_device)
    dl = torch.ones(1, device=cuda_device)
    keep = [t.clone() for t in (a, p, wild_a, wild_p)]
    base, o = ws.data_ptr() + pad, out.data_ptr()
    assert base % 16 == 0
    rc = lib.hn_neimask_loss_forward(a.data_ptr(), p.data_ptr(), wild_a.data_ptr(), wild_p.data_ptr(), n, 128, 1.0, 5.0,
                                     o + 4 * 64, o + 4 * 129, o + 4 * (129 + n + 64), base, nb.value, None)
    assert rc == 0, lib.hn_last_error()
    gbase = grads.data_ptr() + 4 * 64 * 128
    rc = lib.hn_neimask_loss_backward(a.data_ptr(), p.data_ptr(), n, 128, 1.0, dl.data_ptr(), gbase,
                                      gbase + 4 * n * 128, base, nb.value, None)
    assert rc == 0, lib.hn_last_error()
    torch.cuda.synchronize(cuda_device)
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nb.value:] == 0xA5).all())
    canary = torch.ones_like(out, dtype=torch.bool)
    canary[64] = False
    canary[129:129 + n] = False
    canary[129 + n + 64:129 + n + 64 + n] = False
    assert bool((out[canary] == -777.0).all()) and bool(torch.isfinite(out[~canary]).all())
    assert bool((grads[:64 * 128] == -777.0).all()) and bool((grads[-64 * 128:] == -777.0).all())
    assert bool(torch.isfinite(grads[64 * 128:-64 * 128]).all())
    assert all(torch.equal(x, y) for x, y in zip(keep, (a, p, wild_a, wild_p)))
    assert N.neimask_loss_forward(a, p, akp, pkp, 1.0, 5.0)[0].item() == want
    # negative coordinates inside the exact range: the formulation's result
    shift = torch.tensor([0, -150, -200, 0], device=cuda_device)
    l1, g1, _ = _step(a, p, akp + shift, pkp + shift, cuda_device, margin=1.0, C=5.0)
    l2, g2, _ = _step(a, p, akp + shift, pkp + shift, cuda_device, margin=1.0, C=5.0, fused=False)
    assert abs(l1 - l2) <= 1e-5 and (g1 - g2).norm().item() <= 1e-4 * g2.norm().item()
    assert abs(l1 - want) <= 1e-6  # (a translation changes no distance)


def test_fdl_train_step_with_its_own_loss(cuda_device):
    """One FDLNet descriptor train step at 48 pairs as Network.criterion runs it: HardNetNeiMask("NASNet").train()
    on the native train path, two forwards, des.loss(...) on the fused kernels, backward -- against the same step
    on the module's torch layers with the torch loss.  Weight gradients together L2-relative 5e-3, the project's
    bar for train-mode gradients (test_gpu_train.py)."""
    from fixtures import build_module
    from hardnetnas_amd import synth
    from hardnetnas_amd.losses import loss_neimask
    x = torch.from_numpy(synth.synth_patches(96, seed=43)).to(cuda_device)
    _, _, akp, pkp = _clustered(48, 3)
    akp, pkp = akp.to(cuda_device), pkp.to(cuda_device)
    res = {}
    for native in (True, False):
        m, _, _ = build_module("fdl_NASNet")
        m.MARGIN, m.C = 1.0, 5.0
        m = m.to(cuda_device).train()
        m.native_train = native
        oa, op_ = m(x[:48]), m(x[48:])
        assert ("NasTrainFunction" in type(oa.grad_fn).__name__) == native
        if native:
            loss = m.loss(oa, op_, akp, pkp)
            assert "NeiMaskLossFunction" in type(loss.grad_fn).__name__
        else:
            loss = loss_neimask(oa, op_, akp, pkp, margin=m.MARGIN, C=m.C, fused=False)
        loss.backward()
        res[native] = (loss.item(), torch.cat([t.grad.reshape(-1) for _, t in sorted(m.named_parameters())]))
    eg = ((res[True][1] - res[False][1]).norm() / res[False][1].norm()).item()
    print(f"loss {res[True][0]:.6f} vs {res[False][0]:.6f}, weight gradients L2-rel {eg:.2e}")
    assert res[False][0] > 0 and eg <= 5e-3
