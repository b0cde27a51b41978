"""Reference of the clip_patch gradient tests (test_clip_grad_ref.py, test_gpu_clip_grad.py): the closed form of
the gradients with respect to the keypoints' scale and orientation, evaluated in fp64 sample by sample.

The derivative is discontinuous where a sample coordinate crosses an integer, and the fp32 coordinate and its fp64
value fall into different cells for a few samples per thousand at real image sizes.  So the corner cells are those of
the fp32 torch formulation's own coordinates (``cells32``: patches._clip_patch_torch's operations in its order, which
the kernel reproduces bit for bit -- tests/test_gpu_clip.py pins that), while the coordinates inside the cell, the
pixel differences and the sums are fp64 (``clip_ref.coords64``).  No sample is excluded.

With the corners detached (the reference's ``.floor().long()``), per sample
    gX = (y1 - ys)(Ic - Ia) + (ys - y0)(Id - Ib),   gY = (x1 - xs)(Ib - Ia) + (xs - x0)(Id - Ic),
and per keypoint, d the upstream gradient, gx / gy the grid values of the sample's column / row:
    a = sum d (gX gx + gY gy),   b = sum d (-gX gy + gY gx),
    d_scale = (a cos + b sin) / r / 2,   d_ori = (a s, b s),   s = (scale / r) / 2."""
import torch

from clip_ref import coords64


def _corner32(v, hi):
    f = torch.nan_to_num(v.floor(), nan=-1.0)
    return f.clamp(0, hi).long(), (f + 1).clamp(0, hi).long()


def cells32(kpts, scale, ori, ratio, H, W, P=32):
    """(x0, x1, y0, y1) int64 [N,P,P]: the clamped corners of the fp32 coordinates, computed operation by operation
    as patches._clip_patch_torch computes them."""
    n, B = kpts.shape[0], ratio.numel()
    g = torch.linspace(-1, 1, P, dtype=torch.float32)
    gx, gy = g.view(1, 1, P), g.view(1, P, 1)
    r = ratio.float()[kpts[:, 0].clamp(0, B - 1)]
    s = ((scale.reshape(-1).float() / r) / 2.0).view(n, 1, 1)
    if ori is not None:
        sc, ss = s * ori[:, 0].float().view(n, 1, 1), s * ori[:, 1].float().view(n, 1, 1)
    else:
        sc, ss = s, s * 0
    kx = (kpts[:, 2].float() / r).view(n, 1, 1)
    ky = (kpts[:, 1].float() / r).view(n, 1, 1)
    x = sc * gx + (-ss) * gy + kx
    y = ss * gx + sc * gy + ky
    return (*_corner32(x, W - 1), *_corner32(y, H - 1))


def grad64(dout, kpts, scale, ori, ratio, images, P=32):
    """(d_scale [N], d_ori [N,2] or None) in fp64 from the upstream gradient ``dout`` [N,1,P,P]; CPU tensors."""
    B, _, H, W = images.shape
    n = kpts.shape[0]
    x0, x1, y0, y1 = cells32(kpts, scale, ori, ratio, H, W, P)
    xs, ys = coords64(kpts, scale, ori, ratio, P)
    im = images.double().reshape(-1)
    base = (kpts[:, 0].clamp(0, B - 1) * (H * W)).view(-1, 1, 1)

    def px(yv, xv):
        return im[base + yv * W + xv]

    Ia, Ib, Ic, Id = px(y0, x0), px(y1, x0), px(y0, x1), px(y1, x1)
    gX = (y1 - ys) * (Ic - Ia) + (ys - y0) * (Id - Ib)
    gY = (x1 - xs) * (Ib - Ia) + (xs - x0) * (Id - Ic)
    g = torch.linspace(-1, 1, P, dtype=torch.float32).double()
    gx, gy = g.view(1, 1, P), g.view(1, P, 1)
    d = dout.double().reshape(n, P, P)
    a = (d * (gX * gx + gY * gy)).sum(dim=(1, 2))
    b = (d * (-gX * gy + gY * gx)).sum(dim=(1, 2))
    r = ratio.double()[kpts[:, 0].clamp(0, B - 1)]
    s = scale.double().reshape(-1) / r / 2.0
    if ori is None:
        return a / r / 2.0, None
    c, sn = ori[:, 0].double(), ori[:, 1].double()
    return (a * c + b * sn) / r / 2.0, torch.stack((a * s, b * s), dim=1)


def upstream(n, seed, P=32):
    """The seeded normal upstream gradient [N,1,P,P] fp32 of the tests."""
    return torch.randn(n, 1, P, P, generator=torch.Generator().manual_seed(seed))


def torch_grads(dout, kpts, scale, ori, ratio, images, dtype):
    """(d_scale, d_ori or None) of torch autograd over patches._clip_patch_torch on the CPU in ``dtype`` (the grid
    values stay the fp32 linspace values)."""
    from hardnetnas_amd import patches as PT
    sc = scale.to(dtype).clone().requires_grad_(True)
    orr = ori.to(dtype).clone().requires_grad_(True) if ori is not None else None
    im_info = torch.stack([ratio, ratio], dim=1).to(dtype)
    out = PT._clip_patch_torch(kpts, sc, orr, im_info, images.to(dtype), 32)
    out.backward(dout.to(dtype))
    return sc.grad, orr.grad if orr is not None else None
