"""Keypoint patch extraction of FDLNet's inference path on the GPU kernel.

``clip_patch`` is a drop-in replacement, with the reference's signature and return value, for
FDLNet-master/latency/NASNet/utils/image_utils.py:11-158: a rotated, scaled PSIZE x PSIZE window around every
keypoint, sampled from its image by bilinear interpolation with clamped indices.  It is the step between the
detector's keypoints and the descriptor in ``Network.inference`` (model/network.py:148-183):

    detector -> topk_map -> clip_patch -> self.des(patches) -> NN / NNT / NNDR matching

The reference runs some 60 small kernels and twenty [N * PSIZE^2] temporaries; here fp32 HIP ``images``
[B,1,H,W] with int64 keypoints on the same device and PSIZE == 32 go through ``_native.clip_patch`` (one kernel,
hn_clip.hip).  With autograd recording on fp32 ``kpts_scale`` / ``kpts_ori`` (the training step: both come from
the detector's maps) the same inputs go through ``_native.ClipPatchFunction``: that kernel forward and
``hn_clip_patch_backward`` backward, gradients to scale and orientation only, once differentiable.  Everything
else -- CPU tensors, fp64, another PSIZE, or ``images`` / ``im_info`` requiring grad -- runs the torch formulation
below in the dtype of ``images``; in fp64 (grid values still the fp32 ``linspace`` values) it is the ground truth
of the tests.

``describe_keypoints`` is ``des(clip_patch(..., 32))`` in one call; with one of this package's descriptor
modules in eval mode on a HIP device it runs ``NativeModel.forward_keypoints`` and the patches never leave the
forward's workspace.

One deliberate difference from the reference.  The reference maps keypoint i to ``im_info`` row i // (N / B)
(through ``.view(B, -1)``) but to its image through ``kpts_byxc[:, 0]``.  The two agree only when every image
has the same number of keypoints, listed in batch order; otherwise the reference raises or silently scales a
keypoint by another image's ratio.  Here ``kpts_byxc[:, 0]`` selects both, so unequal counts per image and any
keypoint order work, and on inputs where the reference is consistent the results are the same.  A batch index
outside [0, B - 1] is clamped for addressing and non-finite coordinates are made safe (the reference raises);
the patch of such a keypoint is unspecified.
"""
from __future__ import annotations

import torch

NATIVE_PSIZE = 32


def _records_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _native_shapes_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE) -> bool:
    dev = images.device
    return (PSIZE == NATIVE_PSIZE and images.is_cuda and images.dtype == torch.float32 and images.dim() == 4
            and images.shape[1] == 1 and kpts_byxc.dtype == torch.int64 and kpts_byxc.device == dev
            and kpts_byxc.dim() == 2 and kpts_byxc.shape[1] == 4
            and kpts_scale.device == dev and im_info.device == dev
            and (kpts_ori is None or kpts_ori.device == dev))


def _native_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE) -> bool:
    """The kernel alone: no autograd graph to record."""
    return (_native_shapes_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)
            and not _records_grad(images, kpts_scale, kpts_ori))


def _native_grad_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE) -> bool:
    """The kernel with its backward (``_native.ClipPatchFunction``): ``_native_ok``'s conditions with autograd
    recording on the fp32 ``kpts_scale`` and / or ``kpts_ori`` -- the training step, where the detector's maps give
    both -- while ``images`` and ``im_info``, which the kernel does not differentiate, require no grad."""
    return (_native_shapes_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)
            and _records_grad(kpts_scale, kpts_ori) and not _records_grad(images, im_info)
            and kpts_scale.dtype == torch.float32 and (kpts_ori is None or kpts_ori.dtype == torch.float32))


def _native_args(kpts_scale, kpts_ori, im_info):
    """(scale [N], ori [N,2] or None, ratio [B]) as the fp32 tensors of the C ABI."""
    return (kpts_scale.detach().reshape(-1).float(),
            kpts_ori.detach().float() if kpts_ori is not None else None,
            im_info.detach()[:, 0].float().contiguous())


def _corner(v, hi):
    """floor(v) and floor(v) + 1, clamped to [0, hi], as floats of v's dtype (exact: hi < 2^24)."""
    f = torch.nan_to_num(v.detach().floor(), nan=-1.0)
    return f.clamp(0, hi), (f + 1).clamp(0, hi)


def _clip_patch_torch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
    """image_utils.py:11-158 operation by operation in the dtype of ``images``, with the keypoint's own column 0
    selecting its ratio.  The only [N * PSIZE^2] int64 tensors are the four flat indices."""
    dt, dev = images.dtype, images.device
    B, _, H, W = images.shape
    n = kpts_byxc.size(0)
    g = torch.linspace(-1, 1, PSIZE, dtype=torch.float, device=dev).to(dt)
    gx, gy = g.view(1, 1, PSIZE), g.view(1, PSIZE, 1)
    b = kpts_byxc[:, 0].clamp(0, B - 1)
    r = im_info[:, 0].to(dt)[b]
    s = ((kpts_scale.reshape(-1).to(dt) / r) / 2.0).view(n, 1, 1)
    if kpts_ori is not None:
        sc, ss = s * kpts_ori[:, 0].to(dt).view(n, 1, 1), s * kpts_ori[:, 1].to(dt).view(n, 1, 1)
    else:
        sc, ss = s, s * 0
    kx = (kpts_byxc[:, 2].to(dt) / r).view(n, 1, 1)
    ky = (kpts_byxc[:, 1].to(dt) / r).view(n, 1, 1)
    x = sc * gx + (-ss) * gy + kx
    y = ss * gx + sc * gy + ky
    x0, x1 = _corner(x, W - 1)
    y0, y1 = _corner(y, H - 1)
    base = (b * (H * W)).view(n, 1, 1)
    im_flat = images.reshape(-1)

    def pixel(yf, xf):  # flat index through fp64 (exact below 2^53), then the one int64 tensor
        return im_flat[(yf.double() * W + xf.double()).long().add_(base)]

    Ia, Ib, Ic, Id = pixel(y0, x0), pixel(y1, x0), pixel(y0, x1), pixel(y1, x1)
    wa = (x1 - x) * (y1 - y)
    wb = (x1 - x) * (y - y0)
    wc = (x - x0) * (y1 - y)
    wd = (x - x0) * (y - y0)
    return (wa * Ia + wb * Ib + wc * Ic + wd * Id).unsqueeze(1)


def clip_patch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
    """[N,1,PSIZE,PSIZE] patches around the keypoints ``kpts_byxc`` [N,4] (b, y, x, .) of ``images`` [B,1,H,W]:
    ``kpts_scale`` [N] and ``kpts_ori`` [N,2] (cos, sin; or None) give the window, ``im_info`` [B,2] the
    rescale ratio of each image (column 0).  image_utils.py:11-158."""
    assert kpts_byxc.size(0) == kpts_scale.reshape(-1).size(0)
    if _native_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
        from . import _native
        return _native.clip_patch(images.detach(), kpts_byxc, *_native_args(kpts_scale, kpts_ori, im_info))
    if _native_grad_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
        from . import _native
        return _native.ClipPatchFunction.apply(images.detach(), kpts_byxc, kpts_scale, kpts_ori,
                                               im_info.detach()[:, 0].float().contiguous())
    return _clip_patch_torch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)


def describe_keypoints(des, kpts_byxc, kpts_scale, kpts_ori, im_info, images):
    """``des(clip_patch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, 32))`` -> [N,128] (network.py:163-176).
    With ``des`` one of this package's descriptor modules in eval mode and everything on one HIP device with no
    autograd graph to record, the clipping runs inside ``NativeModel.forward_keypoints``; otherwise it is
    literally that composition (a ``strict=True`` module raises in its forward as it always does)."""
    from .model import _NativeMixin, _native_blocker
    if (isinstance(des, _NativeMixin) and kpts_byxc.size(0) > 0
            and _native_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, NATIVE_PSIZE)):
        probe = torch.empty((0, 1, NATIVE_PSIZE, NATIVE_PSIZE), device=images.device)  # stands for the patches
        if _native_blocker(des, probe) is None:
            from . import _native
            nm = _native._BY_ID[des._native_handle(probe)]
            scale, ori, ratio = _native_args(kpts_scale, kpts_ori, im_info)
            return nm.forward_keypoints(images.detach(), kpts_byxc, scale, ori, ratio)
    return des(clip_patch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, NATIVE_PSIZE))
