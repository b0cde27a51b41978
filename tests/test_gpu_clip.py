"""Keypoint patch extraction on the GPU: _native.clip_patch (k_clip_patch) and NativeModel.forward_keypoints
against the reference's recorded patches and fp64 evaluations, its geometry, determinism, bounds guarantee,
chunking and graph capture.

Tolerances.  Golden: 4 E_ref against the stored fp64 values, E_ref = the reference's own fp32 error on these
inputs (read from the fixture); the factor is the margin the matcher tests give to fp32 roundings of the same
expression in another order.  Generated sizes: 4 E with E the fp32 torch formulation's own error against its fp64
form on the same inputs (the CPU tests pin both to the reference).  Pixels whose fp64 coordinate lies within 1e-3
of a discontinuity line (x = 0, W - 1; y = 0, H - 1) are compared with the one-sided evaluations instead
(tests/clip_ref.py); their share is asserted <= 1 % for every case."""
import os
import subprocess
import sys
from functools import lru_cache

import pytest
import torch

from clip_kp_child import kp_inputs
from clip_ref import check_against_fp64, random_case
from fixtures import build_module, load
from hardnetnas_amd import _native as N
from hardnetnas_amd import patches as PT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_MODELS = {"fdl_NASNet": 2e-5, "hardnet": 1e-4, "wang2": 2e-5}  # the project's parity bars


def golden():
    fx = load("clip_patch")
    t = {k: torch.from_numpy(v) for k, v in fx.items() if k != "meta"}
    t["ref64"] = t["ref32"].double() + t["ref64_minus_ref32"].double()
    t["ratio"] = t["im_info"][:, 0].contiguous()
    return t, fx["meta"]


def native(dev, kpts, scale, ori, ratio, images, **kw):
    return N.clip_patch(images.to(dev), kpts.to(dev), scale.to(dev), ori.to(dev) if ori is not None else None,
                        ratio.to(dev), **kw)


def test_golden(cuda_device):
    t, meta = golden()
    got = native(cuda_device, t["kpts"], t["scale"], t["ori"], t["ratio"], t["images"]).cpu()
    _, share = check_against_fp64(got, t["kpts"], t["scale"], t["ori"], t["ratio"], t["images"], 4 * meta["E_ref"],
                                  want=t["ref64"])
    assert share <= 0.01
    # the public entry point takes the same path
    pub = PT.clip_patch(*(x.to(cuda_device) for x in (t["kpts"], t["scale"], t["ori"], t["im_info"], t["images"])), 32)
    assert torch.equal(pub.cpu(), got)


@lru_cache(maxsize=None)
def _images(B, H, W):
    return torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(B * 100003 + H * 131 + W))


@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (61, 83), (1031, 1543)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 257, 4097])
def test_sizes(n, B, hw, cuda_device):
    H, W = hw
    kpts, scale, ori, ratio, images = random_case(n, B, H, W, seed=n * 7 + B * 3 + H, images=_images(B, H, W))
    im_info = torch.stack([ratio, ratio], dim=1)
    want = PT.clip_patch(kpts, scale, ori, im_info, images.double(), 32)
    cpu32 = PT.clip_patch(kpts, scale, ori, im_info, images, 32)
    from clip_ref import coords64, near_lines
    keep = ~near_lines(*coords64(kpts, scale, ori, ratio), H, W).unsqueeze(1)
    E = float((cpu32.double() - want)[keep].abs().max())
    got = native(cuda_device, kpts, scale, ori, ratio, images).cpu()
    _, share = check_against_fp64(got, kpts, scale, ori, ratio, images, 4 * E, want=want)
    assert share <= 0.01


def test_windows_wholly_outside_are_zero(cuda_device):
    """A window that misses the image samples only clamped corners: weights built from them cancel to rounding.
    Half-width 1.5 px, centres 5 px beyond a border: every |corner - coordinate| <= 5 + 1.5 sqrt(2) < 7.2, so a
    term is below 64 and the three additions round by at most 3 x ulp(32) / 2 = 5.7e-6 < 4 E_ref."""
    t, meta = golden()
    H, W = meta["H"], meta["W"]
    d = 5  # centre distance from the border line, > 1.5 sqrt(2) + 1
    pts = [(-d, 40), (H - 1 + d, 40), (30, -d), (30, W - 1 + d), (-d, -d), (-d, W - 1 + d), (H - 1 + d, -d),
           (H - 1 + d, W - 1 + d)]
    kpts = torch.tensor([[i % 3, y, x, 0] for i, (y, x) in enumerate(pts)], dtype=torch.int64)
    ratio = torch.ones(3)
    scale = torch.full((len(pts),), 3.0)
    ang = torch.linspace(0, 3.0, len(pts))
    ori = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1)
    got = native(cuda_device, kpts, scale, ori, ratio, t["images"]).cpu()
    worst = float(got.abs().max())
    print(f"outside windows: max |value| {worst:.3e} (tol {4 * meta['E_ref']:.3e})")
    assert worst <= 4 * meta["E_ref"]


def test_unequal_counts_and_shuffled_order(cuda_device):
    t, _ = golden()
    base = native(cuda_device, t["kpts"], t["scale"], t["ori"], t["ratio"], t["images"])
    perm = torch.randperm(120, generator=torch.Generator().manual_seed(5))[:77]
    got = native(cuda_device, t["kpts"][perm], t["scale"][perm], t["ori"][perm], t["ratio"], t["images"])
    assert torch.equal(got, base[perm.to(cuda_device)])
    none = native(cuda_device, t["kpts"], t["scale"], None, t["ratio"], t["images"])
    one = torch.tensor([[1.0, 0.0]]).repeat(120, 1)
    assert torch.equal(none, native(cuda_device, t["kpts"], t["scale"], one, t["ratio"], t["images"]))


def test_determinism_and_partition(cuda_device):
    """A keypoint's patch is bit-identical alone, inside a batch of 4,097 (past the grid limit: the grid-stride
    loop's second round) and across two calls."""
    kpts, scale, ori, ratio, images = random_case(4097, 3, 61, 83, seed=11)
    a = native(cuda_device, kpts, scale, ori, ratio, images)
    b = native(cuda_device, kpts, scale, ori, ratio, images)
    assert torch.equal(a, b)
    for i in (0, 1234, 4095, 4096):
        alone = native(cuda_device, kpts[i:i + 1], scale[i:i + 1], ori[i:i + 1], ratio, images)
        assert torch.equal(alone[0], a[i]), i


def test_bounds(cuda_device):
    """The images are a view into the middle of a larger buffer of canaries; keypoints with a NaN scale, an Inf
    orientation and batch indices -1 and B sit beside finite ones.  (The address computation was swept on the
    host under the sanitizers first: tests/test_clip.py.)"""
    t, _ = golden()
    B, _, H, W = t["images"].shape
    pad, canary = 1 << 16, 12345.0
    buf = torch.full((2 * pad + B * H * W + 3,), canary, device=cuda_device)
    images = buf[pad + 3:pad + 3 + B * H * W].view(B, 1, H, W)  # 12 bytes off a 16-byte boundary
    images.copy_(t["images"])
    n = 40
    kpts, scale, ori = t["kpts"][:n].clone(), t["scale"][:n].clone(), t["ori"][:n].clone()
    bad = [5, 12, 20, 33]
    scale[5] = float("nan")
    ori[12, 0] = float("inf")
    kpts[20, 0] = -1
    kpts[33, 0] = B
    good = [i for i in range(n) if i not in bad]
    extra = 8
    out = torch.full((n + extra, 1, 32, 32), canary, device=cuda_device)
    native(cuda_device, kpts, scale, ori, t["ratio"], images, out=out[:n])
    clean = native(cuda_device, kpts[good], scale[good], ori[good], t["ratio"], images)
    torch.cuda.synchronize()
    assert torch.equal(out[good], clean)
    assert bool((out[n:] == canary).all())
    assert bool((buf[:pad + 3] == canary).all()) and bool((buf[pad + 3 + B * H * W:] == canary).all())
    assert torch.equal(images.cpu(), t["images"])


# ---- forward_keypoints -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("name", list(KP_MODELS))
def test_forward_keypoints(name, n, cuda_device):
    m, _, _ = build_module(name)
    args = kp_inputs(n, cuda_device)
    images, kpts, scale, ori, ratio = args
    nm = N.NativeModel.from_module(m, cuda_device)
    y = nm.forward_keypoints(*args)
    assert tuple(y.shape) == (n, 128)
    assert torch.equal(y, nm.forward(N.clip_patch(*args)))
    assert nm.workspace_bytes_kp(n) == nm.workspace_bytes(n) + n * 4096
    # the module-level call takes the same path
    im_info = torch.stack([ratio, ratio], dim=1)
    md = m.to(cuda_device)
    with torch.no_grad():
        assert torch.equal(PT.describe_keypoints(md, kpts, scale, ori, im_info, images), y)
    # against the CPU composition on reference-pinned patches
    m_cpu, _, _ = build_module(name)
    with torch.no_grad():
        want = m_cpu(PT.clip_patch(kpts.cpu(), scale.cpu(), ori.cpu(), im_info.cpu(), images.cpu(), 32))
    err = float((y.cpu() - want).abs().max())
    print(f"{name} n={n}: descriptor error vs the CPU composition {err:.3e} (bar {KP_MODELS[name]:g})")
    assert err <= KP_MODELS[name]


def test_forward_keypoints_argument_checks(cuda_device):
    m, _, _ = build_module("hardnet")
    nm = N.NativeModel.from_module(m, cuda_device)
    im, kp, sc, orr, ra = kp_inputs(4, cuda_device)
    out = torch.empty(4, 128, device=cuda_device)
    ws = torch.empty(nm.workspace_bytes_kp(4) - 1, dtype=torch.uint8, device=cuda_device)
    rc = nm.lib.hn_forward_kp(nm._h, im.data_ptr(), 3, im.shape[2], im.shape[3], kp.data_ptr(), sc.data_ptr(),
                              orr.data_ptr(), ra.data_ptr(), 4, out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 4 and b"workspace" in nm.lib.hn_last_error()  # HN_ERR_WORKSPACE
    ws = torch.empty(nm.workspace_bytes_kp(4) + 16, dtype=torch.uint8, device=cuda_device)
    rc = nm.lib.hn_forward_kp(nm._h, im.data_ptr(), 3, im.shape[2], im.shape[3], kp.data_ptr(), sc.data_ptr(),
                              orr.data_ptr(), ra.data_ptr(), 4, out.data_ptr(), ws.data_ptr() + 4, ws.numel() - 4, None)
    assert rc == 1 and b"16-byte" in nm.lib.hn_last_error()
    assert tuple(nm.forward_keypoints(im, kp[:0], sc[:0], orr[:0], ra).shape) == (0, 128)


def test_forward_keypoints_across_chunks(cuda_device, tmp_path):
    """130 keypoints in chunks of 100 (HN_CHUNK, with HN_SUBCHUNK 64 for the stock HardNet), set in a fresh
    process because hn_create reads them: equal to the one-chunk result bit for bit, for every model."""
    n, out = 130, str(tmp_path / "kp.pt")
    env = dict(os.environ, HN_CHUNK="100", HN_SUBCHUNK="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "clip_kp_child.py"), out, str(n), *KP_MODELS],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "CLIP_KP_OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    chunked = torch.load(out)
    args = kp_inputs(n, cuda_device)
    for name in KP_MODELS:
        m, _, _ = build_module(name)
        y = N.NativeModel.from_module(m, cuda_device).forward_keypoints(*args)
        assert torch.equal(y.cpu(), chunked[name]), name


def test_graph_capture(cuda_device):
    """forward_keypoints allocates and synchronises nothing: captured on a side stream (a single-branch graph)
    and replayed twice it gives the eager result."""
    m, _, _ = build_module("fdl_NASNet")
    nm = N.NativeModel.from_module(m, cuda_device)
    images, kpts, scale, ori, ratio = kp_inputs(130, cuda_device)
    ref = nm.forward_keypoints(images, kpts, scale, ori, ratio).clone()
    static_scale = torch.ones_like(scale)
    out = torch.empty((130, 128), device=cuda_device)
    ws = torch.empty(nm.workspace_bytes_kp(130), device=cuda_device, dtype=torch.uint8)
    nm.forward_keypoints(images, kpts, static_scale, ori, ratio, out=out, workspace=ws)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            nm.forward_keypoints(images, kpts, static_scale, ori, ratio, out=out, workspace=ws)
    static_scale.copy_(scale)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
