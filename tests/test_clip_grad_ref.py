"""The yardstick of the clip_patch gradient tests on the CPU: the fp64 closed form of tests/clip_grad_ref.py against
fp64 autograd over patches._clip_patch_torch, on cases where the fp32 and the fp64 coordinates fall into the same
cells (small images), and the CPU dispatch of patches.clip_patch under autograd, which the native backward must
not change."""
import pytest
import torch

from clip_grad_ref import grad64, torch_grads, upstream
from clip_ref import random_case
from hardnetnas_amd import patches as PT


@pytest.mark.parametrize("n,B,H,W", [(2, 3, 3, 5), (63, 3, 61, 83)])
@pytest.mark.parametrize("rotate", [True, False])
def test_closed_form_equals_fp64_autograd(n, B, H, W, rotate):
    kpts, scale, ori, ratio, images = random_case(n, B, H, W, seed=n * 7 + B * 3 + H)
    ori = ori if rotate else None
    dout = upstream(n, seed=n + H)
    ds, do = grad64(dout, kpts, scale, ori, ratio, images)
    ws, wo = torch_grads(dout, kpts, scale, ori, ratio, images, torch.float64)
    rel_s = float((ds - ws).abs().max() / ws.abs().max())
    print(f"n {n} {H}x{W}: d_scale rel {rel_s:.3e} (max |grad| {float(ws.abs().max()):.3g})")
    assert rel_s <= 1e-10
    if rotate:
        rel_o = float((do - wo).abs().max() / wo.abs().max())
        print(f"n {n} {H}x{W}: d_ori rel {rel_o:.3e} (max |grad| {float(wo.abs().max()):.3g})")
        assert rel_o <= 1e-10
    else:
        assert do is None


def test_cpu_dispatch_under_autograd_is_unchanged():
    """CPU tensors with grad recorded keep the torch formulation: same grad_fn type as before the native backward
    existed, gradients equal to calling the formulation directly."""
    kpts, scale, ori, ratio, images = random_case(5, 2, 9, 11, seed=3)
    im_info = torch.stack([ratio, ratio], dim=1)
    sc, orr = scale.clone().requires_grad_(True), ori.clone().requires_grad_(True)
    assert not PT._native_grad_ok(kpts, sc, orr, im_info, images, 32)
    assert not PT._native_ok(kpts, sc, orr, im_info, images, 32)
    out = PT.clip_patch(kpts, sc, orr, im_info, images, 32)
    assert type(out.grad_fn).__name__ == "UnsqueezeBackward0"
    dout = upstream(5, seed=1)
    out.backward(dout)
    ws, wo = torch_grads(dout, kpts, scale, ori, ratio, images, torch.float32)
    assert torch.equal(sc.grad, ws) and torch.equal(orr.grad, wo)
