"""What the library decides from the batch size and the memory knobs, at the batch sizes where the decision
changes, and what its kernels do with memory that is not theirs.

  A  the small-batch split-K head under odd HN_SUBCHUNK / HN_C12_GROUP (and in the chunk pipeline): the header
     promises bit-identical descriptors for any knob values;
  B  the train kernels' row-segment forms (4 / 2 / 1 segments per patch, chosen from batch x waves per patch)
     against fp64 gradients of the reference's layers (tests/golden/train_buckets.npz);
  C  a poisoned caller workspace (every float a NaN) and canaries around the workspace and the output rows;
  D  NaN / Inf patches: unspecified descriptors for themselves, no effect on another row or a later call.

Every test reads and writes only inside tensors it allocates itself."""
import numpy as np
import pytest
import torch

from fixtures import TRAIN_BN_IDX, TRAIN_CONV_IDX, build_module, golden_inputs, load, summary_errors, train_start
from hardnetnas_amd import synth
from test_gpu_parity import TOL, _tol
from test_gpu_train import L2_BAR

pytestmark = pytest.mark.gpu

ODD_KNOBS = {301: (100, 150), 16384: (7000, 8000)}  # batch -> (HN_SUBCHUNK, HN_C12_GROUP)


def _native(m, dev, monkeypatch=None, **env):
    """NativeModel of module m created under the environment knobs ``env`` (hn_create reads them)."""
    from hardnetnas_amd._native import NativeModel
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    nm = NativeModel.from_module(m, dev)
    for k in env:
        monkeypatch.delenv(k)
    return nm


def _tiled_golden(fx, b, dev, u8=False):
    """The golden patches tiled to b rows: fp32 [b,1,32,32], or the uint8 [b,32,32] they were quantised from
    (synth.synth_patches: (q / 255 - mean) / std), which forward_u8(resize="none") normalises back."""
    g = golden_inputs(fx)
    x = np.concatenate([g] * -(-b // len(g)))[:b]
    if u8:
        q = (x.astype(np.float64) * synth.STD_IMAGE + synth.MEAN_IMAGE) * 255.0
        assert np.abs(q - np.rint(q)).max() < 1e-3
        return torch.from_numpy(np.rint(q).astype(np.uint8).reshape(b, 32, 32)).to(dev)
    return torch.from_numpy(x).to(dev)


def _noisy(fx, b, dev, u8, seed=7):
    """The input of test_c12_group_and_subchunk_sizes_are_bitwise_neutral at b rows."""
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (b, 32, 32), generator=g, dtype=torch.uint8).to(dev)
    x = _tiled_golden(fx, b, dev)
    return x + 0.01 * torch.randn(x.shape, generator=g).to(dev)


def _fwd(nm, x, **kw):
    return nm.forward_u8(x, resize="none", **kw) if x.dtype == torch.uint8 else nm.forward(x, **kw)


# ---- A: knob neutrality of the small-batch head ---------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("b", [301, 16384])
def test_small_batch_head_is_knob_neutral(b, u8, cuda_device, monkeypatch):
    """Batches of up to 16,384 patches run the split-K head whatever HN_SUBCHUNK / HN_C12_GROUP say (its
    partials' scratch is sized for the chunk, not the sub-chunk): bit-identical to the default knobs at 301
    patches in sub-chunks of 100 and groups of 150 (where a sub-chunk's conv3 output alone cannot hold the
    partials) and at the largest split batch in 7,000 / 8,000; and under the odd knobs a patch's descriptor
    does not depend on the batch it comes in."""
    m, fx, _ = build_module("hardnet")
    x = _noisy(fx, b, cuda_device, u8)
    sub, grp = ODD_KNOBS[b]
    ref = _fwd(_native(m, cuda_device), x)
    odd = _native(m, cuda_device, monkeypatch, HN_SUBCHUNK=sub, HN_C12_GROUP=grp)
    y = _fwd(odd, x)
    assert torch.equal(y, ref)
    if b == 301:
        assert torch.equal(_fwd(odd, x[:37]), y[:37])


def test_pipelined_head_is_knob_neutral(cuda_device, monkeypatch):
    """forward_hardnet_pipe with sub-chunks of 1,000 in chunks of 4,096 (two full chunks and a ragged one):
    bit-identical to the sequential path at the default sub-chunk size."""
    m, fx, _ = build_module("hardnet")
    g = golden_inputs(fx)
    n = 2 * 4096 + 37
    x = torch.from_numpy(np.concatenate([g, synth.synth_patches(n - len(g), seed=41)])).to(cuda_device)
    ref = _native(m, cuda_device, monkeypatch, HN_CHUNK=4096)
    seq = _native(m, cuda_device, monkeypatch, HN_CHUNK=4096, HN_SUBCHUNK=1000)
    pipe = _native(m, cuda_device, monkeypatch, HN_CHUNK=4096, HN_SUBCHUNK=1000, HN_PIPELINE=1)
    assert pipe.workspace_bytes(n) == seq.workspace_bytes(n) + 4096 * 16384 * 4  # (the pipeline's second buffer)
    y = pipe(x)
    assert torch.equal(y, ref(x))
    assert torch.equal(seq(x), y)


def test_odd_knobs_match_reference_vectors(cuda_device, monkeypatch):
    """301 golden patches (tiled) in sub-chunks of 100 / groups of 150 against the reference's descriptors."""
    m, fx, _ = build_module("hardnet")
    sub, grp = ODD_KNOBS[301]
    nm = _native(m, cuda_device, monkeypatch, HN_SUBCHUNK=sub, HN_C12_GROUP=grp)
    y = nm(_tiled_golden(fx, 301, cuda_device))[:256].cpu().numpy()
    assert np.abs(y - fx["y"]).max() <= TOL["hardnet"]


# ---- B: gradients in every row-segment bucket ------------------------------------------------
@pytest.mark.parametrize("b", [640, 1031, 2051])
def test_train_gradients_in_every_row_segment_bucket(b, cuda_device):
    """The HIP train forward + backward of the smooth objective (y * c).sum() at fresh init against
    tests/golden/train_buckets.npz (the reference's layers on the CPU, fp32 and fp64).

    Row segments per patch (hn_train.hip): ns(w) = 1 if w >= 2,048, 2 if w >= 1,024, else 4, with
    w = batch x (waves sharing a patch's ring), capped by the layer's rows / rows per step.

      kernel family (the default HN_TRAIN_F32 = 17)       w         B = 640   1,031   2,051
      k_fwd3 conv1, k_fwd2 conv2 (one ring per wave)      B           4         2       1
      k_wgrad3 (conv1/3/5), k_wgrad2 (conv2/4)            B           4         2       1
      k_dgrad2 of conv2 (32 input channels: one wave)     B           4         2       1
      k_fwd3s conv3 (64 ch), k_fwd2 conv4, k_dgrad2 of
        conv4 (two waves per ring)                        2 B         2         1       1
      k_fwd3s conv5 (128 ch, four waves per ring)         4 B         1         1       1

    (the stride-1 data gradients run on the eval conv kernels at this default, which have no such forms).  The
    other train tests stop at 256 patches: 4 everywhere but the last row's 2.  1,031 and 2,051 are odd (a ragged
    last workgroup in every kernel that packs 2 or 4 units per workgroup, a ragged conv5 pair in the eval
    kernels).

    Bars: outputs 1e-4 max abs on 64 strided rows; running statistics 1e-5 relative; each gradient's error
    against fp64 (sampled entries, norm, +-1 projections) within max(L2_BAR, 3 x the torch-CPU fp32 run's own
    error recorded in the fixture) -- ReLU-kink flips cost fp32 up to 1.7e-3 here."""
    fx = load("train_buckets")
    meta, pre = fx["meta"], f"b{b}/"
    mb = meta[f"b{b}"]
    x = synth.synth_patches(b, mb["x_seed"])
    c = synth.normal(mb["c_seed"], b * 128).astype(np.float32).reshape(b, 128)
    assert synth.sha256_f32(x) == mb["x_sha256"] and synth.sha256_f32(c) == mb["c_sha256"]
    m = train_start("fresh")[0].to(cuda_device)
    xg = torch.from_numpy(x).to(cuda_device).requires_grad_(True)
    y = m(xg)
    assert "HardNetTrainFunction" in type(y.grad_fn).__name__
    (y * torch.from_numpy(c).to(cuda_device)).sum().backward()
    rows = fx[pre + "rows"]
    yr = y.detach().cpu().numpy()[rows]
    e32, e64 = np.abs(yr - fx[pre + "y_32"]).max(), np.abs(yr - fx[pre + "y_64"]).max()
    print(f"B={b}: max|hip - ref32| = {e32:.2e}, max|hip - ref64| = {e64:.2e} on {len(rows)} rows")
    assert e32 <= 1e-4 and e64 <= 1e-4
    for i in TRAIN_BN_IDX:
        bn = m.features[i]
        for got, key in ((bn.running_mean, "rm"), (bn.running_var, "rv")):
            ref = fx[f"{pre}{key}{i}_32"]
            e = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
            assert e <= 1e-5, (key, i, e)
    grads = {f"g{i}": (m.features[i].weight.grad, i) for i in TRAIN_CONV_IDX}
    grads["gx"] = (xg.grad, meta["gx_seed"])
    fp32_err = dict(zip(meta["grad_names"], fx[pre + "fp32_err"]))
    bad = []
    for k, (g, seed) in grads.items():
        errs = summary_errors(g.cpu().numpy(), fx, pre + k, seed, meta["cap"])
        e, bar = max(errs.values()), max(L2_BAR, 3.0 * float(fp32_err[k]))
        print(f"B={b}: {k} L2-rel err vs fp64: HIP {e:.2e} (torch-CPU fp32 {fp32_err[k]:.2e}, bar {bar:.2e})")
        if not e <= bar:
            bad.append((k, errs, bar))
    assert not bad, bad


# ---- C: poisoned workspace, canaries ---------------------------------------------------------
C_MODELS = ["hardnet", "wang2", "wang3", "wang4", "fdl_NASNet", "cov_a"]
C_CASES = [(n, b, "f32") for n in C_MODELS for b in (37, 301)] + [("hardnet", 37, "u8"), ("hardnet", 301, "u8"),
                                                                  ("hardnet", 301, "knobs")]


def _c_case(name, b, mode, dev, monkeypatch):
    """(model, fixture, input, workspace bytes of this call) of a C case."""
    m, fx, _ = build_module(name)
    if mode == "knobs":
        sub, grp = ODD_KNOBS[301]
        nm = _native(m, dev, monkeypatch, HN_SUBCHUNK=sub, HN_C12_GROUP=grp)
    else:
        nm = _native(m, dev)
    x = _tiled_golden(fx, b, dev, u8=mode == "u8")
    return nm, fx, x, nm.workspace_bytes_u8(b) if mode == "u8" else nm.workspace_bytes(b)


@pytest.mark.parametrize("name,b,mode", C_CASES)
def test_poisoned_workspace_changes_nothing(name, b, mode, cuda_device, monkeypatch):
    """The forward reads no scratch it has not written in the same call: a workspace of zero bytes and one of
    0xFF bytes (every float a NaN) give the same descriptors, bit for bit, and they are the reference's."""
    nm, fx, x, ws_bytes = _c_case(name, b, mode, cuda_device, monkeypatch)
    ys = [_fwd(nm, x, workspace=torch.full((ws_bytes,), fill, dtype=torch.uint8, device=cuda_device))
          for fill in (0x00, 0xFF)]
    assert torch.equal(ys[0], ys[1])
    k = min(b, 256)
    assert np.abs(ys[1][:k].cpu().numpy() - fx["y"][:k]).max() <= _tol(name)


@pytest.mark.parametrize("name,b,mode", C_CASES)
def test_workspace_and_output_canaries(name, b, mode, cuda_device, monkeypatch):
    """The forward writes nothing outside hn_workspace_bytes of the workspace and b rows of the output: 1 MiB
    guard regions on both sides of the workspace and 8 guard rows on both sides of the output keep their
    fill, and the descriptors equal those of an ordinary call."""
    nm, fx, x, ws_bytes = _c_case(name, b, mode, cuda_device, monkeypatch)
    G = 1 << 20
    buf = torch.full((G + ws_bytes + G,), 0xA5, dtype=torch.uint8, device=cuda_device)
    ws = buf[G:G + ws_bytes]
    assert ws.is_contiguous() and ws.data_ptr() % 256 == 0 and ws.numel() == ws_bytes
    sentinel = -12345.0
    outbuf = torch.full((b + 16, 128), sentinel, device=cuda_device)
    out = outbuf[8:8 + b]
    y = _fwd(nm, x, out=out, workspace=ws)
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + ws_bytes:] == 0xA5).all())
    assert bool((outbuf[:8] == sentinel).all()) and bool((outbuf[8 + b:] == sentinel).all())
    assert torch.equal(out, _fwd(nm, x))


# ---- D: non-finite patches -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hardnet", "wang2", "wang4", "fdl_NASNet"])
def test_non_finite_patches_do_not_leak(name, cuda_device):
    """One pixel of four of 255 patches set to +NaN, -NaN, +Inf and -Inf (the last patch: a ragged tile and
    a ragged conv5 pair).  The descriptor of such a patch is unspecified (the reference returns NaN); every
    other row is bit-equal to the clean run's, and a clean call right after, on the same model and the same
    caller workspace, is bit-equal to the first one."""
    from hardnetnas_amd._native import NativeModel
    m, fx, _ = build_module(name)
    nm = NativeModel.from_module(m, cuda_device)
    b = 255
    x = torch.from_numpy(golden_inputs(fx)[:b]).to(cuda_device)
    xb = x.clone()
    xb[0, 0, 13, 7] = float("nan")
    xb.view(torch.int32)[77, 0, 13, 7] = 0xFFC00000 - (1 << 32)
    xb[128, 0, 13, 7] = float("inf")
    xb[254, 0, 13, 7] = float("-inf")
    bits = xb.view(torch.int32)[[0, 77], 0, 13, 7].tolist()
    assert bits == [0x7FC00000, 0xFFC00000 - (1 << 32)], bits
    ws = torch.zeros(nm.workspace_bytes(b), dtype=torch.uint8, device=cuda_device)
    clean = nm.forward(x, workspace=ws).clone()
    dirty = nm.forward(xb, workspace=ws).clone()
    again = nm.forward(x, workspace=ws)
    bad = [0, 77, 128, 254]
    what = {r: ("finite" if bool(torch.isfinite(dirty[r]).all()) else "non-finite") +
            (", as clean" if torch.equal(dirty[r], clean[r]) else ", changed") for r in bad}
    print(f"{name}: corrupted rows (+NaN, -NaN, +Inf, -Inf) came out {what}")
    keep = torch.ones(b, dtype=torch.bool, device=cuda_device)
    keep[bad] = False
    assert torch.isfinite(clean).all()
    assert torch.equal(dirty[keep], clean[keep])
    assert torch.equal(again, clean)
