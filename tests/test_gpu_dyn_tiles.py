"""Dynamically claimed work tiles of the persistent conv3 / conv5 kernels (hn_tiles.h) against the static
assignment (HN_STATIC_TILES=1): the same patches go through the same arithmetic whichever workgroup takes a tile,
so every comparison here is torch.equal.

R is the number of CUs = the persistent grid.  A conv3 tile is one patch and a conv5 tile two, a workgroup's
first two tiles are fixed and the rest claimed, so the batch sizes give grids smaller than R, tiles fewer than,
equal to and more than the grid and twice the grid for both tile sizes, half-empty last tiles, and launches in
which nothing, one tile or most tiles are claimed.  The counters reset themselves: the graph, ring-wrap and
two-stream cases are the ones a counter that does not return to zero, or that two launches share, would fail.
"""
import numpy as np
import pytest
import torch

from hardnetnas_amd import synth
from fixtures import build_module, golden_inputs

pytestmark = pytest.mark.gpu

GOLDEN_TOL = 1e-4  # test_gpu_parity.TOL["hardnet"]
TILE_RING = 64     # include/hardnet_mi355x.h HN_TILE_RING


def _sizes(R):
    return (1, 2, 3, R - 1, R, R + 1, 2 * R - 1, 2 * R + 1, 2 * R + 2, 2 * R + 3, 3 * R + 77, 5 * R + 1)


def _u8_sizes(R):
    return (3, R + 1, 2 * R + 3, 3 * R + 77)


def _model(m, dev, **env):
    """A NativeModel created under the given environment knobs (hn_create reads them once)."""
    import os
    from hardnetnas_amd._native import NativeModel
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        return NativeModel.from_module(m, dev)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def runs(cuda_device):
    """The default and the HN_STATIC_TILES=1 model, and their descriptors of every batch size (fp32 and uint8
    input) -- computed once, read-only for the tests."""
    R = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    m, fx, _ = build_module("hardnet")
    gold = golden_inputs(fx)
    n = max(_sizes(R))
    xs = synth.synth_patches(n, fx["meta"]["test_seed"])
    assert np.array_equal(xs[:gold.shape[0]], gold), "the seeded stream's prefix is the fixture's input"
    x = torch.from_numpy(xs).to(cuda_device)
    u8 = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (max(_u8_sizes(R)), 32, 32), dtype=np.uint8)).to(
        cuda_device)
    dyn = _model(m, cuda_device, HN_STATIC_TILES=None, HN_DYN_TILES=None)
    sta = _model(m, cuda_device, HN_STATIC_TILES=1)
    out = {}
    for tag, nm in (("dyn", dyn), ("static", sta)):
        for b in _sizes(R):
            out[tag, b] = nm(x[:b]).clone()
        for b in _u8_sizes(R):
            out[tag, "u8", b] = nm.forward_u8(u8[:b], resize="none").clone()
    torch.cuda.synchronize()
    return {"R": R, "fx": fx, "m": m, "x": x, "dyn": dyn, "static": sta, "out": out}


# the sizes as multiples of R, resolved in the test (R is a property of the device)
SIZE_IDS = ("1", "2", "3", "R-1", "R", "R+1", "2R-1", "2R+1", "2R+2", "2R+3", "3R+77", "5R+1")
U8_IDS = ("3", "R+1", "2R+3", "3R+77")


@pytest.mark.parametrize("i", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_claimed_tiles_are_bit_identical_to_static(i, runs):
    b = _sizes(runs["R"])[i]
    assert torch.equal(runs["out"]["dyn", b], runs["out"]["static", b])


@pytest.mark.parametrize("i", range(len(U8_IDS)), ids=U8_IDS)
def test_claimed_tiles_are_bit_identical_to_static_u8(i, runs):
    b = _u8_sizes(runs["R"])[i]
    assert torch.equal(runs["out"]["dyn", "u8", b], runs["out"]["static", "u8", b])


def test_golden_rows_under_the_default(runs):
    fx = runs["fx"]
    n = fx["y"].shape[0]
    b = max(_sizes(runs["R"]))
    err = np.abs(runs["out"]["dyn", b][:n].cpu().numpy() - fx["y"]).max()
    print(f"max |default - golden| over {n} rows = {err:.2e}")
    assert err <= GOLDEN_TOL


def test_graph_replays_equal_eager(runs, cuda_device):
    """One captured forward replayed three times: a counter that a launch leaves non-zero shows in the second."""
    nm, R = runs["dyn"], runs["R"]
    b = 3 * R + 77
    x = runs["x"][:b]
    static_x = torch.zeros_like(x)
    out = torch.empty((b, 128), device=cuda_device)
    ws = torch.empty(nm.workspace_bytes(b), device=cuda_device, dtype=torch.uint8)
    nm.forward(static_x, out=out, workspace=ws)  # warm-up: one-time launch attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            nm.forward(static_x, out=out, workspace=ws)
    static_x.copy_(x)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, runs["out"]["dyn", b])


def test_ring_wrap(runs):
    """More back-to-back forwards than the model has counter blocks."""
    nm = runs["dyn"]
    x = runs["x"][:3]
    ys = [nm(x) for _ in range(TILE_RING + 6)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[-1])
    assert torch.equal(ys[0], runs["out"]["static", 3])


def _two_streams(nm, x, cuda_device, rounds=8):
    """`rounds` forwards of x on each of two streams, interleaved, each stream with its own workspace and outputs."""
    b = x.shape[0]
    streams = [torch.cuda.Stream(device=cuda_device) for _ in range(2)]
    wss = [torch.empty(nm.workspace_bytes(b), device=cuda_device, dtype=torch.uint8) for _ in range(2)]
    outs = [[torch.empty((b, 128), device=cuda_device) for _ in range(rounds)] for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(rounds):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                nm.forward(x, out=outs[k][r], workspace=wss[k])
    torch.cuda.synchronize()
    return outs


def test_two_streams_equal_serial(runs, cuda_device):
    nm, R = runs["dyn"], runs["R"]
    b = 3 * R + 77
    outs = _two_streams(nm, runs["x"][:b], cuda_device)
    for k in range(2):
        for y in outs[k]:
            assert torch.equal(y, runs["out"]["static", b])


def test_two_streams_equal_serial_pipelined(runs, cuda_device):
    """The same with HN_PIPELINE=1 over two chunks of a small HN_CHUNK (each call forks its second stream)."""
    R = runs["R"]
    chunk = R + 45
    b = 2 * chunk
    x = runs["x"][:b]
    nm = _model(runs["m"], cuda_device, HN_CHUNK=chunk, HN_PIPELINE=1)
    ref = _model(runs["m"], cuda_device, HN_CHUNK=chunk, HN_STATIC_TILES=1)(x)
    outs = _two_streams(nm, x, cuda_device)
    for k in range(2):
        for y in outs[k]:
            assert torch.equal(y, ref)
