"""Tile / stage loops of the persistent conv3..conv5 kernels (k_conv_ws, k_conv_w1) on batches that give their
workgroups different numbers of tiles.

The persistent grid is min(tiles, 256); a tile is one patch for conv3 and two for conv4 / conv5.  So 255 patches
give every conv3 workgroup one tile; 513 give one conv3 workgroup three tiles beside 255 with two, and one conv4 /
conv5 workgroup two tiles beside 255 with one; 771 mix one- and two-tile conv4 / conv5 workgroups with a half-empty
last tile.  1, 2 and 3 are the single workgroup with a full, and with a half-empty, two-patch tile.

Tolerances: 5e-5 against the direct kernels is test_winograd_1d_conv3_conv5_match_reference's bar (both sides
are bf16x3 forms of the same fp32 network); 1e-4 against hardnet.npz is test_gpu_parity's golden tolerance.
"""
import numpy as np
import pytest
import torch

from hardnetnas_amd import synth
from fixtures import build_module, golden_inputs

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 255, 513, 771)
GOLDEN_TOL = 1e-4   # test_gpu_parity.TOL["hardnet"]
DIRECT_TOL = 5e-5   # test_winograd_1d_conv3_conv5_match_reference


@pytest.fixture(scope="module")
def runs(cuda_device):
    """Descriptors of every batch under the default variant (twice), the direct kernels (605gfg) and conv4 with
    the MFMA waves' own stores / the producers' stores (f / i) -- computed once, read-only for the tests."""
    import os
    from hardnetnas_amd._native import NativeModel
    m, fx, _ = build_module("hardnet")
    gold = golden_inputs(fx)
    xs = synth.synth_patches(max(BATCHES), fx["meta"]["test_seed"])
    assert np.array_equal(xs[:gold.shape[0]], gold), "the seeded stream's prefix is the fixture's input"
    x = torch.from_numpy(xs).to(cuda_device)
    saved = os.environ.get("HN_VARIANT")
    out = {}
    try:
        for tag, variant, batches, reps in (("default", None, BATCHES, 2), ("direct", "605gfg", BATCHES, 1),
                                            ("f", "605qfl", (513, 771), 1), ("i", "605qil", (513, 771), 1)):
            if variant is None:
                os.environ.pop("HN_VARIANT", None)
            else:
                os.environ["HN_VARIANT"] = variant
            nm = NativeModel.from_module(m, cuda_device)
            for b in batches:
                out[tag, b] = [nm(x[:b]).clone() for _ in range(reps)]
    finally:
        if saved is None:
            os.environ.pop("HN_VARIANT", None)
        else:
            os.environ["HN_VARIANT"] = saved
    torch.cuda.synchronize()
    return fx, out


@pytest.mark.parametrize("b", BATCHES)
def test_default_matches_direct_kernels(b, runs):
    _, out = runs
    err = (out["default", b][0] - out["direct", b][0]).abs().max().item()
    print(f"b={b}: max |default - 605gfg| = {err:.2e}")
    assert err <= DIRECT_TOL


@pytest.mark.parametrize("b", BATCHES)
def test_default_matches_golden_rows(b, runs):
    fx, out = runs
    n = min(b, fx["y"].shape[0])
    err = np.abs(out["default", b][0][:n].cpu().numpy() - fx["y"][:n]).max()
    print(f"b={b}: max |default - golden| over {n} rows = {err:.2e}")
    assert err <= GOLDEN_TOL


@pytest.mark.parametrize("b", (513, 771))
def test_conv4_store_forms_are_bit_identical(b, runs):
    _, out = runs
    assert torch.equal(out["f", b][0], out["i", b][0])
    assert torch.equal(out["i", b][0], out["default", b][0])  # i is the default's conv4


@pytest.mark.parametrize("b", BATCHES)
def test_two_calls_are_bit_identical(b, runs):
    _, out = runs
    assert torch.equal(out["default", b][0], out["default", b][1])


@pytest.mark.parametrize("b", BATCHES[:-1])
def test_rows_do_not_depend_on_the_batch(b, runs):
    """A patch's descriptor is the same in every batch that holds it, whatever tile of whatever workgroup
    computes it."""
    _, out = runs
    for big in BATCHES:
        if big > b:
            assert torch.equal(out["default", big][0][:b], out["default", b][0])
