"""hn_clip_patch_backward on the GPU: the gradients of clip_patch with respect to the keypoints' scale and
orientation, through _native.clip_patch_backward and through patches.clip_patch(...).backward().

Reference: tests/clip_grad_ref.py -- the closed form in fp64 at the corner cells of the fp32 coordinates (which the
kernel reproduces bit for bit); no sample is excluded.  Tolerance: 4 E per output, max abs, E = the error of fp32
torch autograd over patches._clip_patch_torch on the CPU against that reference on the same case, measured here;
the factor is the one tests/test_gpu_clip.py gives to fp32 roundings of the same expression in another order."""
from functools import lru_cache

import pytest
import torch

from clip_grad_ref import grad64, torch_grads, upstream
from clip_ref import random_case
from fixtures import load
from hardnetnas_amd import _native as N
from hardnetnas_amd import patches as PT

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def _images(B, H, W):
    return torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(B * 100003 + H * 131 + W))


@lru_cache(maxsize=None)
def case(n, B, H, W):
    """Inputs, upstream gradient, fp64 reference and E (scale, orientation) of one size; computed once."""
    kpts, scale, ori, ratio, images = random_case(n, B, H, W, seed=n * 7 + B * 3 + H, images=_images(B, H, W))
    dout = upstream(n, seed=n + H)
    ref_s, ref_o = grad64(dout, kpts, scale, ori, ratio, images)
    t_s, t_o = torch_grads(dout, kpts, scale, ori, ratio, images, torch.float32)
    E = (float((t_s.double() - ref_s).abs().max()), float((t_o.double() - ref_o).abs().max()))
    return (kpts, scale, ori, ratio, images), dout, (ref_s, ref_o), E


def dev_args(dev, kpts, scale, ori, ratio, images):
    return (images.to(dev), kpts.to(dev), scale.to(dev), ori.to(dev) if ori is not None else None, ratio.to(dev))


def backward(dev, dout, kpts, scale, ori, ratio, images, **kw):
    return N.clip_patch_backward(dout.to(dev), *dev_args(dev, kpts, scale, ori, ratio, images), **kw)


SIZES = [(n, B, H, W) for (B, H, W) in ((1, 2, 2), (3, 3, 5), (3, 61, 83)) for n in (1, 2, 63, 257, 4097)]
SIZES.append((64, 2, 1031, 1543))


@pytest.mark.parametrize("n,B,H,W", SIZES)
def test_sizes(n, B, H, W, cuda_device):
    """2x2: every corner clamped; 4097: past one round of the 4,096-workgroup grid; 1 and 63: partial rounds."""
    args, dout, (ref_s, ref_o), (E_s, E_o) = case(n, B, H, W)
    kpts, scale, ori, ratio, images = args
    ds, do = backward(cuda_device, dout, *args)
    e_s, e_o = float((ds.cpu().double() - ref_s).abs().max()), float((do.cpu().double() - ref_o).abs().max())
    print(f"n {n} B {B} {H}x{W}: d_scale err {e_s:.3e} (E {E_s:.3e}, max |grad| {float(ref_s.abs().max()):.3g}); "
          f"d_ori err {e_o:.3e} (E {E_o:.3e}, max |grad| {float(ref_o.abs().max()):.3g})")
    # the public entry point: the kernel forward, the same kernel backward
    sc = scale.to(cuda_device).requires_grad_(True)
    orr = ori.to(cuda_device).requires_grad_(True)
    im_info = torch.stack([ratio, ratio], dim=1).to(cuda_device)
    out = PT.clip_patch(kpts.to(cuda_device), sc, orr, im_info, images.to(cuda_device), 32)
    assert type(out.grad_fn).__name__ == "ClipPatchFunctionBackward"
    assert torch.equal(out.detach(), N.clip_patch(*dev_args(cuda_device, *args)))
    out.backward(dout.to(cuda_device))
    assert torch.equal(sc.grad, ds) and torch.equal(orr.grad, do)
    assert e_s <= 4 * E_s and e_o <= 4 * E_o


def test_no_rotation_and_single_outputs(cuda_device):
    args, dout, _, _ = case(257, 3, 61, 83)
    kpts, scale, ori, ratio, images = args
    ds, do = backward(cuda_device, dout, *args)
    only_s, none_o = backward(cuda_device, dout, *args, want_ori=False)
    none_s, only_o = backward(cuda_device, dout, *args, want_scale=False)
    assert none_o is None and none_s is None
    assert torch.equal(only_s, ds) and torch.equal(only_o, do)
    # ori = None is the rotation (1, 0)
    one = torch.tensor([[1.0, 0.0]]).repeat(kpts.shape[0], 1)
    want, _ = backward(cuda_device, dout, kpts, scale, one, ratio, images)
    got, g_o = backward(cuda_device, dout, kpts, scale, None, ratio, images, want_ori=False)
    assert g_o is None and torch.equal(got, want)
    with pytest.raises(ValueError):
        backward(cuda_device, dout, kpts, scale, None, ratio, images)
    # through autograd: only the outputs that need a gradient are asked for
    dev = cuda_device
    im_info = torch.stack([ratio, ratio], dim=1).to(dev)
    sc = scale.to(dev).requires_grad_(True)
    out = PT.clip_patch(kpts.to(dev), sc, ori.to(dev), im_info, images.to(dev), 32)
    assert type(out.grad_fn).__name__ == "ClipPatchFunctionBackward"
    out.backward(dout.to(dev))
    assert torch.equal(sc.grad, ds)
    orr = ori.to(dev).requires_grad_(True)
    out = PT.clip_patch(kpts.to(dev), scale.to(dev), orr, im_info, images.to(dev), 32)
    out.backward(dout.to(dev))
    assert torch.equal(orr.grad, do)
    sc = scale.to(dev).requires_grad_(True)
    out = PT.clip_patch(kpts.to(dev), sc, None, im_info, images.to(dev), 32)
    out.backward(dout.to(dev))
    assert torch.equal(sc.grad, got)
    # nothing to record: the plain kernel, no graph
    assert PT.clip_patch(kpts.to(dev), scale.to(dev), ori.to(dev), im_info, images.to(dev), 32).grad_fn is None


def test_determinism_and_partition(cuda_device):
    """A keypoint's gradient is bit-identical alone, inside a batch of 4,097 (the grid-stride loop's second round)
    and across two calls."""
    args, dout, _, _ = case(4097, 3, 61, 83)
    kpts, scale, ori, ratio, images = args
    a = backward(cuda_device, dout, *args)
    b = backward(cuda_device, dout, *args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in (0, 1234, 4095, 4096):
        s, o = backward(cuda_device, dout[i:i + 1], kpts[i:i + 1], scale[i:i + 1], ori[i:i + 1], ratio, images)
        assert torch.equal(s[0], a[0][i]) and torch.equal(o[0], a[1][i]), i


def test_bounds(cuda_device):
    """The inputs of test_gpu_clip.py::test_bounds (the host sweep has shown them to address inside the images): a
    NaN scale, an Inf orientation and batch indices -1 and B beside finite keypoints; the images a view into a
    canary buffer, both outputs inside canary buffers."""
    fx = load("clip_patch")
    t = {k: torch.from_numpy(v) for k, v in fx.items() if k != "meta"}
    ratio = t["im_info"][:, 0].contiguous()
    B, _, H, W = t["images"].shape
    dev, pad, canary = cuda_device, 1 << 16, 12345.0
    buf = torch.full((2 * pad + B * H * W + 3,), canary, device=dev)
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
    dout = upstream(n, seed=7)
    front, back = 5, 9
    out_s = torch.full((front + n + back,), canary, device=dev)
    out_o = torch.full((front + n + back, 2), canary, device=dev)
    N.clip_patch_backward(dout.to(dev), images, kpts.to(dev), scale.to(dev), ori.to(dev), ratio.to(dev),
                          out_scale=out_s[front:front + n], out_ori=out_o[front:front + n])
    cs, co = N.clip_patch_backward(dout[good].to(dev), images, kpts[good].to(dev), scale[good].to(dev),
                                   ori[good].to(dev), ratio.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(out_s[front:front + n][good], cs) and torch.equal(out_o[front:front + n][good], co)
    assert bool(torch.isfinite(cs).all()) and bool(torch.isfinite(co).all())
    for o in (out_s, out_o):
        assert bool((o[:front] == canary).all()) and bool((o[front + n:] == canary).all())
    assert bool((buf[:pad + 3] == canary).all()) and bool((buf[pad + 3 + B * H * W:] == canary).all())
    assert torch.equal(images.cpu(), t["images"])


def test_argument_checks(cuda_device):
    args, dout, _, _ = case(2, 3, 3, 5)
    kpts, scale, ori, ratio, images = args
    im, kp, sc, orr, ra = dev_args(cuda_device, *args)
    d = dout.to(cuda_device)
    lib = N.load_library()
    # an orientation gradient without an orientation: HN_ERR_ARG, no launch
    out = torch.full((4,), 7.0, device=cuda_device)
    rc = lib.hn_clip_patch_backward(d.data_ptr(), im.data_ptr(), 3, 3, 5, kp.data_ptr(), sc.data_ptr(), None,
                                    ra.data_ptr(), 2, None, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 1 and b"d_dori" in lib.hn_last_error() and bool((out == 7.0).all())
    # n == 0
    ds, do = N.clip_patch_backward(d[:0], im, kp[:0], sc[:0], orr[:0], ra)
    assert tuple(ds.shape) == (0,) and tuple(do.shape) == (0, 2)
    # width 1, as the forward
    with pytest.raises(ValueError):
        N.clip_patch_backward(d, im[:, :, :, :1], kp, sc, orr, ra)
    rc = lib.hn_clip_patch_backward(d.data_ptr(), im.data_ptr(), 3, 3, 1, kp.data_ptr(), sc.data_ptr(), orr.data_ptr(),
                                    ra.data_ptr(), 2, out.data_ptr(), None, None)
    assert rc == 1 and b"width" in lib.hn_last_error()


def test_graph_capture(cuda_device):
    """The call allocates and synchronises nothing given its destinations: captured on a side stream (a
    single-branch graph) and replayed twice it gives the eager result."""
    args, dout, _, _ = case(257, 3, 61, 83)
    im, kp, sc, orr, ra = dev_args(cuda_device, *args)
    d = dout.to(cuda_device)
    ref_s, ref_o = N.clip_patch_backward(d, im, kp, sc, orr, ra)
    static_d = torch.ones_like(d)
    out_s, out_o = torch.empty_like(ref_s), torch.empty_like(ref_o)
    N.clip_patch_backward(static_d, im, kp, sc, orr, ra, out_scale=out_s, out_ori=out_o)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=cuda_device)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            N.clip_patch_backward(static_d, im, kp, sc, orr, ra, out_scale=out_s, out_ori=out_o)
    static_d.copy_(d)
    for _ in range(2):
        out_s.zero_()
        out_o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, ref_s) and torch.equal(out_o, ref_o)
