"""loss_HardNet's 'average' and 'random' reductions on the GPU (hn_loss_dense.hip, hn_loss.hip through
``_native.HardNetLossReduceFunction``) against the reference's recorded results (tests/golden/loss_reduce.npz), the
fp64 references of tests/loss_reduce_ref.py and the torch formulation (``fused=False``) on the same GPU.

Bounds: against the fixture, loss <= max(1e-6, the reference's own fp32 loss error) and gradient L2-relative <=
max(1e-5, 3 g32err) (test_gpu_pairs.py's rule); against an fp64 reference computed here, max(1e-5, 3 x the error of
the fp32 torch formulation on the CPU against the same fp64) on the loss and on the gradient's L2-relative error.
Every test prints what it measured before it asserts."""
import copy
import ctypes

import pytest
import torch

import loss_reduce_ref as R

pytestmark = pytest.mark.gpu

FX = R.fixture()
FN = "HardNetLossReduceFunction"


def _step(a, p, idx, reduce, swap, margin, loss_type, dev):
    """One step on dev through the autograd function: (loss, [grad_a; grad_p] on the CPU, grad_fn name)."""
    from hardnetnas_amd import _native as N
    x = a.detach().clone().to(dev).requires_grad_(True)
    y = p.detach().clone().to(dev).requires_grad_(True)
    loss = N.HardNetLossReduceFunction.apply(x, y, idx if reduce == "random" else None, reduce, swap, margin,
                                             loss_type)
    name = type(loss.grad_fn).__name__
    loss.backward()
    return loss.item(), torch.cat([x.grad, y.grad]).cpu(), name


def _hold(tag, got, ref):
    """The fp64-reference bound on a step ``got`` against ``ref`` = loss_reduce_ref.reference(...)."""
    loss, g, name = got
    assert FN in name, f"{tag}: grad_fn {name}"
    el, al = abs(loss - ref.loss), max(1e-5, 3 * abs(ref.loss32 - ref.loss))
    gn = float(ref.grad.norm())
    eg = float((g.double() - ref.grad).norm())
    ag = max(1e-5, 3 * ref.g32err)
    print(f"{tag}: loss {loss!r} vs {ref.loss!r}: {el:.2e} (allowed {al:.2e}); gradient L2-rel "
          f"{eg / gn if gn else eg:.2e} (allowed {ag:.2e}, fp32 formulation {ref.g32err:.2e})")
    assert el <= al, f"{tag}: loss {loss!r} vs {ref.loss!r}"
    if gn == 0.0:
        assert eg == 0.0, f"{tag}: the fp64 gradient is zero, this one is not"
    else:
        assert eg / gn <= ag, f"{tag}: gradient L2-relative {eg / gn:.3e} > {ag:.3e}"


# 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FX["meta"]["cases"])
def test_fixture_parity(name, cuda_device):
    reduce, swap, lt, margin = R.parse_case(name)
    a, p, idx = torch.from_numpy(FX["a"]), torch.from_numpy(FX["p"]), torch.from_numpy(FX["idx"])
    loss, g, fn = _step(a, p, idx, reduce, swap, margin, lt, cuda_device)
    assert FN in fn, fn
    l64, l32 = float(FX[f"loss64_{name}"]), float(FX[f"loss32_{name}"])
    want = torch.from_numpy(FX[f"g_{name}"]).double()
    rel = float((g.double() - want).norm() / want.norm())
    allow = max(1e-5, 3 * float(FX[f"g32err_{name}"]))
    print(f"{name}: loss error {abs(loss - l64):.2e} (allowed {max(1e-6, abs(l32 - l64)):.2e}); gradient L2-rel "
          f"{rel:.2e} (allowed {allow:.2e})")
    assert abs(loss - l64) <= max(1e-6, abs(l32 - l64))
    assert rel <= allow
    loss2, g2, _ = _step(a, p, idx, reduce, swap, margin, lt, cuda_device)
    assert loss2 == loss and torch.equal(g2, g)  # bit-identical call to call


# 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", R.RAGGED_SIZES + R.SPLIT_SIZES)
def test_ragged_sizes(b, cuda_device):
    a, p, idx = R.ragged_case(b)
    for reduce in R.REDUCES:
        for swap in (False, True):
            for lt, margin in (("softmax", 1.0), ("triplet_margin", 0.2)):
                ref = R.reference(a, p, swap, margin, reduce, lt, idx)
                _hold(f"B={b} {reduce} swap={int(swap)} {lt}", _step(a, p, idx, reduce, swap, margin, lt, cuda_device),
                      ref)


# 3 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", R.REDUCES)
@pytest.mark.parametrize("loss_type", R.LOSS_TYPES)
def test_exact_tie_halves_the_gradient(reduce, loss_type, cuda_device):
    a, p, idx = R.tie_case()
    ref = R.reference(a, p, True, 1.0, reduce, loss_type, idx)
    loss, g, fn = _step(a, p, idx, reduce, True, 1.0, loss_type, cuda_device)
    assert FN in fn
    rel = float((g.double() - ref.grad).norm() / ref.grad.norm())
    print(f"tie {reduce} {loss_type}: loss {loss!r} vs {ref.loss!r}, gradient L2-rel {rel:.2e}")
    assert abs(loss - ref.loss) <= 1e-6 and rel <= 1e-5


# 4 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup_row,dup_col,zero_row", [(5, 129, 64), (129, 64, 63)])
def test_masked_duplicate_and_zero_positive(dup_row, dup_col, zero_row, cuda_device):
    """B = 130: three splits of one 64-row tile, the last ragged (2 rows).  The near-duplicate negative lies in the
    ragged tile / in the first column of another split than its row's, the zero positive at a split's edge."""
    a, p, idx = R.masking_case(130, dup_row, dup_col, zero_row)
    idx = idx.clone()
    idx[dup_row] = dup_col  # 'random' selects the masked entry too
    for reduce in R.REDUCES:
        for swap in (False, True):
            for lt, margin in (("softmax", 1.0), ("triplet_margin", 0.2), ("contrastive", 1.4)):
                ref = R.reference(a, p, swap, margin, reduce, lt, idx)
                _hold(f"mask ({dup_row},{dup_col}) {reduce} swap={int(swap)} {lt}",
                      _step(a, p, idx, reduce, swap, margin, lt, cuda_device), ref)


# 5 -------------------------------------------------------------------------------------------------
def test_random_index_lists(cuda_device):
    """The kernel clamps every loaded index to [0, B-1] before anything else is done with it (k_lrand_keys)."""
    b = 130
    a, p, perm = R.ragged_case(b)
    lists = {"identity": torch.arange(b), "zeros": torch.zeros(b, dtype=torch.int64)}  # zeros: 130 > 64 sources
    for tag, idx in lists.items():
        for swap in (False, True):
            for lt, margin in (("softmax", 1.0), ("triplet_margin", 0.2)):
                ref = R.reference(a, p, swap, margin, "random", lt, idx)
                _hold(f"random {tag} swap={int(swap)} {lt}", _step(a, p, idx, "random", swap, margin, lt, cuda_device),
                      ref)
    wild = perm.clone()
    wild[3], wild[64], wild[129] = -1, b, 1 << 40
    wild[7], wild[100] = -(1 << 62), (1 << 63) - 1
    clamped = wild.clamp(0, b - 1)
    for swap in (False, True):
        got = _step(a, p, wild, "random", swap, 1.0, "softmax", cuda_device)
        want = _step(a, p, clamped, "random", swap, 1.0, "softmax", cuda_device)
        assert got[0] == want[0] and torch.equal(got[1], want[1])
        _hold(f"random clamped swap={int(swap)}", got, R.reference(a, p, swap, 1.0, "random", "softmax", clamped))


# 6 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", R.REDUCES)
def test_saved_buffer_canaries(reduce, cuda_device):
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    b, guard = 130, 4096
    kind = N.BATCH_REDUCES[reduce]
    a, p, idx = (t.to(cuda_device) for t in R.ragged_case(b))
    nb = ctypes.c_size_t()
    assert lib.hn_hardnet_loss_reduce_workspace_bytes(kind, b, ctypes.byref(nb)) == 0
    need = nb.value
    assert need % 16 == 0
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=cuda_device)
    loss = torch.zeros(1, device=cuda_device)
    dl = torch.ones(1, device=cuda_device)
    ga, gp = torch.empty_like(a), torch.empty_like(p)
    stream = torch.cuda.current_stream(cuda_device).cuda_stream
    with torch.cuda.device(cuda_device):
        rc = lib.hn_hardnet_loss_reduce_forward(a.data_ptr(), p.data_ptr(), idx.data_ptr(), b, 128, kind, 1, 1.0, 1,
                                                loss.data_ptr(), buf.data_ptr(), need, stream)
        assert rc == 0, lib.hn_last_error()
        torch.cuda.synchronize(cuda_device)
        assert bool((buf[need:] == 0xA5).all()), "the forward wrote past saved_bytes"
        rc = lib.hn_hardnet_loss_reduce_backward(a.data_ptr(), p.data_ptr(), idx.data_ptr(), b, 128, kind, 1, 1.0, 1,
                                                 dl.data_ptr(), ga.data_ptr(), gp.data_ptr(), buf.data_ptr(), need,
                                                 stream)
        assert rc == 0, lib.hn_last_error()
        torch.cuda.synchronize(cuda_device)
    assert bool((buf[need:] == 0xA5).all()), "the backward wrote past saved_bytes"
    want = _step(a.cpu(), p.cpu(), idx.cpu(), reduce, True, 1.0, "softmax", cuda_device)
    assert loss.item() == want[0] and torch.equal(torch.cat([ga, gp]).cpu(), want[1])


# 7 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", R.REDUCES)
def test_against_the_torch_formulation_on_the_gpu(reduce, cuda_device):
    """loss_HardNet's dispatch at B = 512, swap on: a seeded run selects what fused=False selects."""
    from hardnetnas_amd.losses import loss_HardNet
    a, p, _ = R.ragged_case(512, scale=False)
    res = {}
    for fused in (True, False):
        x = a.to(cuda_device).requires_grad_(True)
        y = p.to(cuda_device).requires_grad_(True)
        torch.manual_seed(5)
        loss = loss_HardNet(x, y, anchor_swap=True, batch_reduce=reduce, loss_type="softmax", fused=fused)
        assert (FN in type(loss.grad_fn).__name__) == fused
        loss.backward()
        res[fused] = (loss.item(), torch.cat([x.grad, y.grad]).double().cpu())
    el = abs(res[True][0] - res[False][0]) / abs(res[False][0])
    eg = float((res[True][1] - res[False][1]).norm() / res[False][1].norm())
    print(f"{reduce} B=512 vs fused=False: loss rel {el:.2e}, gradient L2-rel {eg:.2e}")
    assert el <= 1e-5 and eg <= 1e-4


# 8 -------------------------------------------------------------------------------------------------
def test_hardnet_train_step_with_the_average_loss(cuda_device):
    """One train() step of the stock HardNet at 64 pairs: weight gradients under the HIP 'average' loss against the
    same step under the fused=False loss."""
    from fixtures import train_start
    from hardnetnas_amd.losses import loss_HardNet
    m, _, a, p = train_start("golden")
    x = torch.as_tensor(a[:64]).to(cuda_device), torch.as_tensor(p[:64]).to(cuda_device)
    grads = {}
    for fused in (True, False):
        mm = copy.deepcopy(m).to(cuda_device).train()
        out = mm(torch.cat(x))
        loss = loss_HardNet(out[:64], out[64:], anchor_swap=True, batch_reduce="average", fused=fused)
        assert (FN in type(loss.grad_fn).__name__) == fused
        loss.backward()
        grads[fused] = [q.grad.double().cpu() for q in mm.parameters() if q.grad is not None]
    assert len(grads[True]) == len(grads[False]) >= 7
    for k, (g, w) in enumerate(zip(grads[True], grads[False])):
        rel = float((g - w).norm() / w.norm())
        print(f"train step, parameter {k}: weight gradient L2-rel {rel:.2e}")
        assert rel <= 1e-4, k
