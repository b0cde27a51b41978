"""The descriptor's input gradient in train() on the GPU (hn_nas_train_backward_dx through NasTrainFunction) and
its composition with the clip_patch backward: des(clip_patch(...)) with native forward and backward, the chain the
FDLNet training step runs from the losses down to the keypoints' scale and orientation.

Bars: the input gradient's L2-relative error against the same module's torch layers in fp64 on the CPU <= 2e-2,
the bar tests/test_gpu_nas_train.py holds a single gradient tensor to (ReLU kinks included); everything that must
not change with the input gradient -- parameter gradients, running statistics, the old entry point -- bit for bit."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import gt_helpers as G
from clip_grad_ref import upstream
from clip_ref import random_case
from fixtures import build_module
from hardnetnas_amd import _native as N
from hardnetnas_amd import network as NW
from hardnetnas_amd import patches as PT
from hardnetnas_amd import synth
from nas_train_ref import raw_step

pytestmark = pytest.mark.gpu
FDL = ["fdl_NASNet", "fdl_NASNet_01"]


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", FDL)
def test_input_gradient_against_fp64(name, cuda_device):
    m, _, _ = build_module(name)
    m.train()
    m64 = copy.deepcopy(m).double()
    x = torch.from_numpy(synth.synth_patches(96, seed=23))
    v = seeded((96, 128), 5)
    xg = x.to(cuda_device).requires_grad_(True)
    y = m.to(cuda_device)(xg)
    assert "NasTrainFunction" in type(y.grad_fn).__name__
    y.backward(v.to(cuda_device))
    x64 = x.double().requires_grad_(True)
    y64 = m64(x64)
    y64.backward(v.double())
    e_y = float((y.detach().cpu().double() - y64.detach()).abs().max())
    rel = float((xg.grad.cpu().double() - x64.grad).norm() / x64.grad.norm())
    print(f"{name}: descriptors {e_y:.2e}; input gradient L2-rel vs fp64 {rel:.3e} (bar 2e-2), "
          f"|grad| {float(x64.grad.norm()):.3g}")
    assert tuple(xg.grad.shape) == (96, 1, 32, 32) and e_y <= 1e-4
    assert rel <= 2e-2


@pytest.mark.parametrize("name", FDL)
def test_parameter_gradients_and_statistics_do_not_change(name, cuda_device):
    x = torch.from_numpy(synth.synth_patches(64, seed=29)).to(cuda_device)
    v = seeded((64, 128), 6).to(cuda_device)
    res = []
    for need in (False, True):
        m = build_module(name)[0].to(cuda_device).train()
        xi = x.clone().requires_grad_(need)
        y = m(xi)
        assert "NasTrainFunction" in type(y.grad_fn).__name__
        y.backward(v)
        assert (xi.grad is not None) == need
        res.append((y.detach(), {k: t.grad for k, t in m.named_parameters()}, dict(m.state_dict())))
    assert torch.equal(res[0][0], res[1][0])
    for k, g in res[0][1].items():
        assert torch.equal(g, res[1][1][k]), k
    for k, t in res[0][2].items():
        assert torch.equal(t, res[1][2][k]), k


@pytest.mark.parametrize("name", FDL + ["wang2"])
@pytest.mark.parametrize("b", [2, 5])
def test_entry_points_and_bounds(name, b, cuda_device):
    """B = 2 (the smallest batch) and 5 (odd): the old entry point, the new one with NULL and the new one with an
    input gradient give the same parameter gradients bit for bit; d_din inside a canary buffer leaves the canaries
    intact and equals the plain call.  wang2: the C entry point forms the input gradient for the NAS kinds too
    (no input_norm: factor 1)."""
    dev = cuda_device
    m = build_module(name)[0].to(dev).train()
    x = torch.from_numpy(synth.synth_patches(b, seed=31)).to(dev)
    v = seeded((b, 128), 8).to(dev)
    old = raw_step(m, x, v, "hn_nas_train_backward")
    null = raw_step(m, x, v, "hn_nas_train_backward_dx", None)
    plain = torch.empty((b, 1, 32, 32), device=dev)
    with_dx = raw_step(m, x, v, "hn_nas_train_backward_dx", plain)
    for a, c, d in zip(old, null, with_dx):
        assert torch.equal(a, c) and torch.equal(a, d)
    canary, front = 12345.0, 2048
    buf = torch.full((front + (b + 3) * 1024,), canary, device=dev)
    raw_step(m, x, v, "hn_nas_train_backward_dx", buf[front:front + b * 1024])
    assert torch.equal(buf[front:front + b * 1024].view(b, 1, 32, 32), plain)
    assert bool((buf[:front] == canary).all()) and bool((buf[front + b * 1024:] == canary).all())
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    # a misaligned d_din is refused before any launch
    lib = N.load_library()
    desc = N.desc_for_module(m)
    p = ctypes.c_void_p(4096)
    ts = N.train_tensors(m)[1]
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = lib.hn_nas_train_backward_dx(ctypes.byref(desc), p, p, b, ptrs, None, ptrs, None, ctypes.c_void_p(4096 + 4), p,
                                      1 << 40, p, 1 << 40, None)
    assert rc == 1 and b"d_din" in lib.hn_last_error()


def test_input_gradient_of_the_nas_stem_against_fp64(cuda_device):
    """The NAS kinds through the C entry point (no module dispatches to it): conv0's data gradient without
    input_norm, against the module's torch layers in fp64."""
    dev = cuda_device
    m = build_module("wang2")[0].train()
    m64 = copy.deepcopy(m).double()
    x = torch.from_numpy(synth.synth_patches(96, seed=37))
    v = seeded((96, 128), 9)
    din = torch.empty((96, 1, 32, 32), device=dev)
    raw_step(m.to(dev), x.to(dev), v.to(dev), "hn_nas_train_backward_dx", din)
    x64 = x.double().requires_grad_(True)
    m64(x64).backward(v.double())
    rel = float((din.cpu().double() - x64.grad).norm() / x64.grad.norm())
    print(f"wang2: input gradient L2-rel vs fp64 {rel:.3e} (bar 2e-2)")
    assert rel <= 2e-2


@pytest.mark.parametrize("name", ["fdl_NASNet", "hardnet"])
def test_composition_with_clip_patch(name, cuda_device):
    """des(clip_patch(...)) in train(), orientation and scale requiring grad: both native grad_fns, and the
    keypoints' gradients are hn_clip_patch_backward of the patches' gradient, bit for bit."""
    dev = cuda_device
    n, B, H, W = 64, 3, 61, 83
    kpts, scale, ori, ratio, images = random_case(n, B, H, W, seed=77)
    des = build_module(name)[0].to(dev).train()
    im_info = torch.stack([ratio, ratio], dim=1).to(dev)
    kp, im, ra = kpts.to(dev), images.to(dev), ratio.to(dev)
    sc, orr = scale.to(dev).requires_grad_(True), ori.to(dev).requires_grad_(True)
    patches = PT.clip_patch(kp, sc, orr, im_info, im, 32)
    patches.retain_grad()
    y = des(patches)
    assert type(patches.grad_fn).__name__ == "ClipPatchFunctionBackward"
    want_fn = "HardNetTrainFunction" if name == "hardnet" else "NasTrainFunction"
    assert want_fn in type(y.grad_fn).__name__
    y.backward(seeded((n, 128), 10).to(dev))
    assert patches.grad is not None and bool(torch.isfinite(patches.grad).all())
    ds, do = N.clip_patch_backward(patches.grad, im, kp, sc.detach(), orr.detach(), ra)
    assert torch.equal(sc.grad, ds) and torch.equal(orr.grad, do)
    assert float(do.abs().max()) > 0 and float(ds.abs().max()) > 0
    # describe_keypoints reaches the same two functions through its des(clip_patch(...)) fallback
    sc2, or2 = scale.to(dev).requires_grad_(True), ori.to(dev).requires_grad_(True)
    y2 = PT.describe_keypoints(des, kp, sc2, or2, im_info, im)
    assert want_fn in type(y2.grad_fn).__name__


def test_pair_under_autograd(cuda_device):
    """network.pair with orientation maps requiring grad: the patches are the no-grad pair(..., topk=K)'s bit for
    bit (hn_clip_patch on the same rows), backward runs, and the maps' gradients are finite and zero away from
    the keypoint pixels."""
    dev = cuda_device
    H, W, B, K = 61, 83, 3, 48
    c = G.case_inputs(H, W, B, seed=12, K=K)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)  # noqa: E731
    ori, scale, h12, h21 = f(c["ori"]), f(c["scale"]), f(c["homo12"]), f(c["homo21"])
    mask = torch.from_numpy(c["mask"]).to(dev)
    g = torch.Generator().manual_seed(3)
    raw1, raw2 = torch.rand(B, 1, H, W, generator=g).to(dev), torch.rand(B, 1, H, W, generator=g).to(dev)
    info = torch.ones(B, 2, device=dev)
    with torch.no_grad():
        gs, go = NW.gt_scale_orin(scale.unsqueeze(-1), ori, h12, h21)
        want, limc0, rimc0 = NW.pair(mask.unsqueeze(-1), None, scale.unsqueeze(-1), ori, info, raw1, h12, gs, go, info,
                                     raw2, 32, topk=K)
    ori_l, ori_r = ori.clone().requires_grad_(True), go.clone().requires_grad_(True)
    got, limc, rimc = NW.pair(mask.unsqueeze(-1), None, scale.unsqueeze(-1), ori_l, info, raw1, h12, gs, ori_r, info,
                              raw2, 32, topk=K)
    assert torch.equal(limc, limc0) and torch.equal(rimc, rimc0)
    assert got.requires_grad and torch.equal(got.detach(), want)
    got.backward(torch.cat((upstream(B * K, 1), upstream(B * K, 2)), 1).to(dev))
    for grad, rows in ((ori_l.grad.reshape(B, H, W, 2), limc), (ori_r.grad.reshape(B, H, W, 2), rimc)):
        assert bool(torch.isfinite(grad).all())
        at = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        at[rows[:, 0], rows[:, 1], rows[:, 2]] = True
        assert float(grad[~at].abs().max()) == 0.0
        assert float(grad[at].abs().max()) > 0.0
