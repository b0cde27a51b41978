"""The references of loss_HardNet's 'average' and 'random' reductions (tests/loss_reduce_ref.py) against the
reference's recorded results (tests/golden/loss_reduce.npz, made by make_loss_reduce_golden.py), the closed form of
the kernels against the formulation's fp64 autograd, and the three torch losses beside loss_HardNet (no GPU)."""
import numpy as np
import pytest
import torch

import loss_reduce_ref as R
from hardnetnas_amd import losses as L

FX = R.fixture()
CASES = FX["meta"]["cases"]


def _inputs():
    return torch.from_numpy(FX["a"]), torch.from_numpy(FX["p"]), torch.from_numpy(FX["idx"])


def test_fixture_covers_the_cases_the_kernels_need():
    assert len(CASES) == 20 and FX["a"].shape == (129, 128) and sorted(FX["idx"]) == list(range(129))
    for reduce in R.REDUCES:
        for swap in (False, True):
            for lt in R.LOSS_TYPES:
                assert R.case_name(reduce, swap, lt, 1.0) in CASES
    second = [c for c in CASES if not c.endswith("_m1")]
    assert len(second) == 8 and {R.parse_case(c)[2] for c in second} == {"triplet_margin", "contrastive"}
    for c in second:  # a second margin puts the clamp on both sides
        assert 0.1 <= float(FX[f"active_{c}"]) <= 0.9, c


@pytest.mark.parametrize("name", CASES)
def test_formulation_equals_the_recorded_reference(name):
    reduce, swap, lt, margin = R.parse_case(name)
    a, p, idx = _inputs()
    loss, g = R.autograd_step(a, p, swap, margin, reduce, lt, idx, torch.float64)
    assert abs(loss - float(FX[f"loss64_{name}"])) <= 1e-12
    want = torch.from_numpy(FX[f"g_{name}"])
    assert torch.equal(g.float(), want)  # (the fixture stores the fp64 gradients rounded to fp32)
    # the package's own torch formulation (fused=False) is the same function
    torch.manual_seed(FX["meta"]["seed"])
    got = L.loss_HardNet(a.double(), p.double(), anchor_swap=swap, margin=margin, batch_reduce=reduce, loss_type=lt,
                         fused=False)
    assert abs(float(got.detach()) - float(FX[f"loss64_{name}"])) <= 1e-12


def _closed_vs_autograd(a, p, idx, swap, margin, reduce, lt):
    loss, g = R.autograd_step(a, p, swap, margin, reduce, lt, idx, torch.float64)
    cl, ga, gp = R.closed_form(a, p, swap, margin, reduce, lt, idx)
    assert abs(float(cl) - loss) <= 1e-10
    err = float((torch.cat([ga, gp]) - g).abs().max())
    assert err <= 1e-10, err


@pytest.mark.parametrize("b", [1, 2, 3, 33, 65, 129])
@pytest.mark.parametrize("reduce", R.REDUCES)
def test_closed_form_equals_fp64_autograd(b, reduce):
    if b == 129:
        a, p, idx = _inputs()
    else:
        a, p, idx = R.ragged_case(b)
    for swap in (False, True):
        for lt, margin in (("triplet_margin", 0.2), ("softmax", 1.0), ("contrastive", 1.4), ("triplet_margin", 1.0)):
            _closed_vs_autograd(a, p, idx, swap, margin, reduce, lt)


@pytest.mark.parametrize("reduce", R.REDUCES)
def test_closed_form_halves_across_the_exact_tie(reduce):
    a, p, idx = R.tie_case()
    u = (a * a).sum(1)[:, None] + (p * p).sum(1)[None, :] - 2 * a @ p.t()
    assert float(u[0, 1]) == 0.5 and float(u[1, 0]) == 0.5  # exact in fp32
    for lt in R.LOSS_TYPES:
        _closed_vs_autograd(a, p, idx, True, 1.0, reduce, lt)


def test_random_sampling_gor_and_decorrelation_equal_the_reference():
    a, p, _ = _inputs()
    n = torch.from_numpy(FX["n"])

    def step(fn, *ts):
        xs = [t.double().clone().requires_grad_(True) for t in ts]
        v = fn(*xs)
        v.backward()
        return float(v.detach()), torch.cat([x.grad for x in xs]).float()

    for tag, fn, ts in (
            ("random_sampling", lambda x, y, z: L.loss_random_sampling(x, y, z, anchor_swap=True, margin=1.0,
                                                                       loss_type="triplet_margin"), (a, p, n)),
            ("gor", L.global_orthogonal_regularization, (a, n)),
            ("decor", L.CorrelationPenaltyLoss(), (a,))):
        v, g = step(fn, *ts)
        assert abs(v - float(FX[f"{tag}_value"])) <= 1e-12, tag
        assert np.allclose(g.numpy(), FX[f"{tag}_grad"], rtol=1e-6, atol=1e-9), tag
    d = L.distance_vectors_pairwise(a.double(), p.double())
    assert d.shape == (129,) and abs(float(d[9]) - 1e-4) < 1e-6  # the zero positive distance: sqrt(1e-8)
    with pytest.raises(ValueError):
        L.loss_random_sampling(a, p, n, loss_type="hinge")
    with pytest.raises(ValueError):
        L.loss_random_sampling(a, p, n[:5])
    for lt in ("softmax", "contrastive"):
        assert torch.isfinite(L.loss_random_sampling(a, p, n, loss_type=lt))
