"""The conditions under which tests/test_gpu_hardnet_layers.py's bars mean something, on the CPU references alone
(tests/hardnet_layer_ref.py; no GPU): every mutant of every case misses the case's widest bar by a factor of 10 or
more in at least one metric, the fp32 yardstick itself is below 1e-5, and the fp64 reference of a convolution case
is the matching layer of ``hardnetnas_amd.model.HardNet``."""
import pytest
import torch

import hardnet_layer_ref as R
from hardnetnas_amd import _native as N
from hardnetnas_amd.model import HardNet

MUTANT_MARGIN = 10.0
E32_MAX = 1e-5


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_every_mutant_misses_the_bar(case):
    ref64, e32, bar = R.first_output(case)
    muts = R.mutants_of(case)
    assert muts, "a case without a mutant has no justification for its bar"
    for name, wrong in muts.items():
        assert wrong.shape == ref64.shape, name
        l2, mx = R.metrics(wrong, ref64)
        print(f"{R.case_id(case)} mutant '{name}': L2 {l2:.2e} / bar {bar[0]:.2e}, max {mx:.2e} / bar {bar[1]:.2e}")
        assert l2 >= MUTANT_MARGIN * bar[0] or mx >= MUTANT_MARGIN * bar[1], name


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_the_fp32_yardstick_is_small(case):
    c = R.case_of(case)
    e32 = c["e32"] if isinstance(c["e32"], list) else [c["e32"]]
    for e in e32:
        assert 0.0 <= e[0] < E32_MAX and 0.0 <= e[1] < E32_MAX, e
    if "e_split" in c:  # the bf16x3 split: 2^-16-relative products at worst
        assert c["e_split"][0] < 2.0 ** -14 and c["e_split"][1] < 2.0 ** -14, c["e_split"]


def test_every_kind_of_mutant_is_exercised():
    names = set()
    for case in R.ALL_CASES:
        names |= set(R.mutants_of(case))
    assert names >= {"last patch dropped", "last segment dropped NS=2", "last segment dropped NS=4",
                     "halo row missing", "pad column reads its flat neighbour", "input ReLU left out",
                     "ky and kx swapped", "unflipped weights", "parity classes swapped", "second chunk at offset 0",
                     "statistics without the last slice"}
    # the slice mutant is there on the shapes that have more than one slice
    for case in [("bn_fwd", 4, 70), ("bn_bwd", 5, 70), ("bn_fwd", 1, 37), ("bn_bwd", 0, 5)]:
        assert "statistics without the last slice" in R.mutants_of(case), case
    assert R.bn_slices(128, 70 * 64) == (2, 2240) and R.bn_slices(32, 37 * 1024)[0] == 10
    assert R.bn_slices(128, 64 * 64)[0] == 1


@pytest.mark.parametrize("layer", range(7))
def test_ref64_is_the_models_layer(layer):
    """conv_fwd's fp64 reference against features[conv] of HardNet in fp64, fed the same activation."""
    case = ("conv_fwd", layer, 5)
    c = R.conv_case(case)
    net = HardNet().double()
    conv = net.features[N.HARDNET_CONV_IDX[layer]]
    cin, cout, h, k, s, p = R.LAYERS[layer]
    assert tuple(conv.weight.shape) == (cout, cin, k, k) and conv.bias is None
    z = c["x"]["z"].double()
    with torch.no_grad():
        conv.weight.copy_(c["x"]["w"].double())
        y = conv(z if layer == 0 else torch.relu(z))
    assert y.shape == c["ref64"].shape and torch.equal(y, c["ref64"])
    bn = net.features[N.HARDNET_BN_IDX[layer]]
    assert not bn.affine and bn.eps == R.BN_EPS and bn.momentum == R.MOMENTUM and bn.num_features == cout


def test_bn_ref64_is_torchs_batch_norm():
    """bn_fwd's written-out fp64 statistics against torch's train-mode batch_norm in fp64."""
    for case in [("bn_fwd", 5, 5), ("bn_fwd", 6, 5)]:
        c = R.bn_case(case)
        y, rm, rv = (c["x"][k].double().clone() for k in ("y", "rmean", "rvar"))
        z = torch.nn.functional.batch_norm(y, rm, rv, training=True, momentum=R.MOMENTUM, eps=R.BN_EPS)
        for got, want in zip((z, rm, rv), (c["ref64"][0], c["ref64"][2], c["ref64"][3])):
            assert float((got - want).abs().max()) < 1e-12
    # and bn_bwd's formula against autograd through it
    c = R.bn_case(("bn_bwd", 3, 5))
    b, ch = c["x"]["z"].shape[:2]
    y = R.normal(("bn_bwd", 3, 5), "probe", c["x"]["z"].shape).double().requires_grad_()
    z = torch.nn.functional.batch_norm(y, None, None, training=True, eps=R.BN_EPS)
    da = c["x"]["da"].double()
    (torch.relu(z) * da).sum().backward()
    rstd = 1.0 / (y.detach().transpose(0, 1).reshape(ch, -1).var(1, unbiased=False) + R.BN_EPS).sqrt()
    want = R.bn_bwd_eval(3, z.detach(), rstd, da)
    assert float((y.grad - want).abs().max()) < 1e-12
