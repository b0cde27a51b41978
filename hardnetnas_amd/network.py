"""FDLNet's homography ground-truth stage and ``Network`` (FDLNet-master/latency/NASNet/model/network.py).

``Network.forward`` takes a pair of images and the two homographies between them, warps the score maps, builds
ground-truth scale and orientation maps, projects keypoints, cuts patch pairs and describes them; ``criterion``
evaluates the three losses on that endpoint:

    det(im1), det(im2) -> gt_scale_orin x 2 -> gtscore x 2 (filter_border, warp, warp(ones), det.process)
                       -> pair x 4 (nonzero / masked_select, clip_patch, ptCltoCr, clip_patch) -> des x 8 -> criterion

Drop-in replacements, with the reference's signatures, return shapes and dtypes:

    warp            utils/image_utils.py:161-194   (``align_corners`` added, see below)
    filter_border   utils/image_utils.py:197-213
    gt_scale_orin   model/network.py:200-264
    ptCltoCr        utils/math_utils.py:43-106
    pair            utils/net_utils.py:10-53
    Network         model/network.py:12-324

Each function has a torch restatement, operation by operation, in the dtype of its inputs; it is differentiable, runs
on any device and in fp64 is the ground truth of the tests.  It is written so that B = 1 behaves as B > 1 (the
reference's ``.squeeze()`` calls do not).  On HIP fp32 tensors with no autograd graph to record, the native path runs
instead: ``_native.warp_score`` / ``gt_scale_orin`` / ``mask_keypoints`` / ``project_keypoints`` (one kernel each,
hn_gt.hip).  A native ``Network.forward`` makes no host synchronisation and runs no torch kernel on the ground-truth
side; it computes each left patch set and its descriptors once (``im*_lpredpatch`` is the same tensor as
``im*_lpatch`` in the reference) and calls ``hn_project_keypoints`` twice per direction, once per map pair gathered.

``align_corners``: the reference calls ``grid_sample`` without the argument, which in today's torch means ``False``;
that is the default here and "what the reference's code does".  Under ``False`` the identity homography is not an
identity warp; ``True`` is the behaviour the reference's ``(W - 1)`` normalisation was written for.

Deliberate differences from the reference: ``ptCltoCr`` lets the keypoint's own column 0 select its homography (the
reference's ``.view(B, -1)`` agrees with it only for equal counts in batch order), as ``clip_patch`` does for the
ratio; and ``pair`` takes an optional ``topk`` -- the native path needs the row count without reading it back, so it
runs when ``topk`` is given (``Network.forward`` passes its TOPK) and then always returns B * topk rows (an image
whose mask has fewer set pixels gets rows (b, 0, 0, 0) for the rest).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .detector import BORDER
from . import patches as _patches
from .patches import NATIVE_PSIZE, _records_grad, clip_patch


def _hip32(*ts) -> bool:
    """Every given tensor is fp32 (or an integer / mask type) on one HIP device and no autograd graph would be
    recorded."""
    ts = [t for t in ts if t is not None]
    dev = ts[0].device
    return (all(t.is_cuda and t.device == dev and (t.dtype == torch.float32 or not t.is_floating_point()) for t in ts)
            and not _records_grad(*ts))


# ---------------------------------------------------------------------------------------------------------------
# warp / filter_border
# ---------------------------------------------------------------------------------------------------------------
def _pixel_grid(B, H, W, like):
    """imgBatchXYZ (utils/common_utils.py:45-53) in the dtype and on the device of ``like``: [B,H,W,3] (x, y, 1)."""
    gy, gx = torch.meshgrid([torch.arange(H), torch.arange(W)], indexing="ij")
    gx, gy = gx.float().unsqueeze(-1), gy.float().unsqueeze(-1)
    grid = torch.cat((gx, gy, gy.new_full(gy.size(), fill_value=1)), -1).unsqueeze(0).repeat(B, 1, 1, 1)
    return grid.to(device=like.device, dtype=like.dtype)


def _project(batchXYZ, homo):
    """transXYZ_2_to_1 (utils/common_utils.py:56-75): [B,H,W,3] points through [B,3,3] -> [B,H,W,2] (x, y)."""
    B, H, W, C = batchXYZ.size()
    grid = batchXYZ.contiguous().view(B, H * W, C).contiguous().permute(0, 2, 1)
    grid = grid.type_as(homo).to(homo.device)
    grid_w = torch.matmul(homo, grid).contiguous().permute(0, 2, 1)
    grid_w = torch.div(grid_w, torch.unsqueeze(grid_w[:, :, 2], -1) + 1e-8)
    return grid_w.contiguous().view(B, H, W, -1)[:, :, :, :2]


def filter_border(imscore, radius=BORDER):
    """[B,H,W,C] with everything within ``radius`` pixels of an edge multiplied by 0 (image_utils.py:197-213)."""
    _, height, width, _ = imscore.size()
    mask = imscore.new_full((1, height - 2 * radius, width - 2 * radius, 1), fill_value=1)
    mask = F.pad(input=mask, pad=(0, 0, radius, radius, radius, radius, 0, 0), mode="constant", value=0)
    return imscore * mask


def _warp_torch(im1_data, homo21, align_corners):
    B, imH, imW, C = im1_data.size()
    grid_w = _project(_pixel_grid(B, imH, imW, homo21), homo21)
    xn = grid_w[:, :, :, 0].div(imW - 1) * 2 - 1
    yn = grid_w[:, :, :, 1].div(imH - 1) * 2 - 1
    out = F.grid_sample(im1_data.permute(0, 3, 1, 2), torch.stack((xn, yn), dim=-1), mode="bilinear",
                        padding_mode="zeros", align_corners=bool(align_corners))
    return out.permute(0, 2, 3, 1)


def warp(im1_data, homo21, align_corners=False):
    """``im1_data`` [B,H,W,C] seen through ``homo21`` [B,3,3]: output pixel p samples the input bilinearly at
    proj(homo21, p), zeros outside (image_utils.py:161-194).  C = 1 on HIP fp32 runs ``hn_warp_score``."""
    if im1_data.dim() == 4 and im1_data.shape[3] == 1 and im1_data.shape[1] >= 2 and im1_data.shape[2] >= 2 \
            and im1_data.shape[0] > 0 and _hip32(im1_data, homo21) and homo21.dtype == torch.float32:
        from . import _native
        warped, _ = _native.warp_score(im1_data.detach().squeeze(-1), homo21.detach(), border=0,
                                       align_corners=align_corners, want_visible=False)
        return warped.unsqueeze(-1)
    return _warp_torch(im1_data, homo21, align_corners)


# ---------------------------------------------------------------------------------------------------------------
# gt_scale_orin
# ---------------------------------------------------------------------------------------------------------------
def _msd(x, y):
    """MSD (utils/math_utils.py:114-125) of two int64 [B,H,W,2] point maps: an fp32 [B,H,W,1] map, as there."""
    sm = ((x - y) ** 2).sum(keepdim=True, dim=-1)
    return torch.sqrt((sm + 1e-8).float()) * 2


def _gt_scale_orin_torch(im2_scale, im2_orin, homo12, homo21):
    B, H, W, _ = im2_scale.size()
    im2_cos, im2_sin = im2_orin.reshape(B, H, W, 2).chunk(chunks=2, dim=-1)
    centX, centY, centZ = _pixel_grid(B, H, W, im2_scale.new_zeros(1, dtype=torch.float)).chunk(3, dim=3)

    half_scale = im2_scale // 2
    centXYZ = torch.cat((centX, centY, centZ), dim=3)
    upXYZ = torch.cat((centX, centY - half_scale, centZ), dim=3)
    bottomXYZ = torch.cat((centX, centY + half_scale, centZ), dim=3)
    rightXYZ = torch.cat((centX + half_scale, centY, centZ), dim=3)
    leftXYZ = torch.cat((centX - half_scale, centY, centZ), dim=3)

    centXYw = _project(centXYZ, homo21)
    centXw, centYw = centXYw.chunk(chunks=2, dim=-1)
    centXYw = centXYw.long()
    upScale = _msd(_project(upXYZ, homo21).long(), centXYw)
    rightScale = _msd(_project(rightXYZ, homo21).long(), centXYw)
    bottomScale = _msd(_project(bottomXYZ, homo21).long(), centXYw)
    leftScale = _msd(_project(leftXYZ, homo21).long(), centXYw)
    centScale = (upScale + rightScale + bottomScale + leftScale) / 4

    offset_x, offset_y = im2_scale * im2_cos, im2_scale * im2_sin
    offsetXYw = _project(torch.cat((centX + offset_x, centY + offset_y, centZ), dim=3), homo21)
    offsetXw, offsetYw = offsetXYw.chunk(chunks=2, dim=-1)
    offset_ww, offset_hw = offsetXw - centXw, offsetYw - centYw
    offset_rw = (offset_ww ** 2 + offset_hw ** 2 + 1e-8).sqrt()
    cos_w = offset_ww / (offset_rw + 1e-8)
    sin_w = offset_hw / (offset_rw + 1e-8)

    map_xy = _project(centXYZ, homo12).round().long()
    x = map_xy[..., 0].clamp(min=0, max=W - 1)
    y = map_xy[..., 1].clamp(min=0, max=H - 1)
    q = (y * W + x).view(B, H * W)

    def at_q(m):  # m[b, y, x] for every output pixel: the reference's advanced-index gather
        return m.reshape(B, H * W).gather(1, q).view(B, H, W, 1)

    im1w_scale = at_q(centScale).view(im2_scale.size())
    im1w_orin = torch.cat((at_q(cos_w), at_q(sin_w)), dim=-1)
    im1w_orin = im1w_orin / torch.norm(im1w_orin, p=2, dim=-1, keepdim=True)
    return im1w_scale, im1w_orin.unsqueeze(0)


def _scale_map(scale, shape):
    """The scale map as the contiguous [B,H,W] tensor of the C ABI.  A map that is one expanded scalar (what RFDet's
    native forward returns) is materialised here; ``Network.forward`` passes the detector's scale as a value instead."""
    return scale.detach().reshape(shape).contiguous()


def gt_scale_orin(im2_scale, im2_orin, homo12, homo21):
    """Ground-truth scale [B,H,W,1] and orientation [1,B,H,W,2] maps of image 1 from image 2's maps ``im2_scale``
    [B,H,W,1] and ``im2_orin`` [B,H,W,2] (any shape with those elements) and the two homographies
    (network.py:200-264).  HIP fp32 runs ``hn_gt_scale_orin``."""
    B, H, W, _ = im2_scale.size()
    if B > 0 and H >= 2 and W >= 2 and _hip32(im2_scale, im2_orin, homo12, homo21) \
            and all(t.dtype == torch.float32 for t in (im2_scale, im2_orin, homo12, homo21)):
        from . import _native
        gt_scale, gt_ori = _native.gt_scale_orin(_scale_map(im2_scale, (B, H, W)),
                                                 im2_orin.detach().reshape(B, H, W, 2), homo12.detach(),
                                                 homo21.detach())
        return gt_scale.unsqueeze(-1), gt_ori.unsqueeze(0)
    return _gt_scale_orin_torch(im2_scale, im2_orin, homo12, homo21)


# ---------------------------------------------------------------------------------------------------------------
# ptCltoCr / pair
# ---------------------------------------------------------------------------------------------------------------
def _ptCltoCr_torch(leftC, homolr, right_imscale, right_imorint, clamp):
    B, maxh, maxw, _ = right_imscale.size()
    dt = homolr.dtype
    b = leftC[:, 0].clamp(0, B - 1)
    h = homolr.reshape(B, 9)[b]
    x, y = leftC[:, 2].to(dt), leftC[:, 1].to(dt)
    u = h[:, 0] * x + h[:, 1] * y + h[:, 2]
    v = h[:, 3] * x + h[:, 4] * y + h[:, 5]
    w = h[:, 6] * x + h[:, 7] * y + h[:, 8]
    xr = (u / (w + 1e-8)).round().long()
    yr = (v / (w + 1e-8)).round().long()
    if clamp:
        xr = xr.clamp(min=0, max=maxw - 1)
        yr = yr.clamp(min=0, max=maxh - 1)
    rightC = torch.stack((b, yr, xr, torch.zeros_like(b)), dim=1)
    idx = (b * (maxh * maxw) + yr * maxw + xr).clamp(min=0, max=maxh * maxw * B - 1)
    right_imS = right_imscale.reshape(-1).gather(0, idx)
    if right_imorint is None:
        return rightC, right_imS, None
    return rightC, right_imS, right_imorint.reshape(-1, 2)[idx]


def ptCltoCr(leftC, homolr, right_imscale, right_imorint=None, clamp=True):
    """Keypoints ``leftC`` [N,4] rows (b, y, x, 0) projected into the right image by ``homolr`` [B,3,3] and rounded:
    ``(rightC [N,4] rows (b, y', x', 0), right_imS [N], right_imO [N,2] or None)``, scale and orientation gathered
    from ``right_imscale`` [B,H,W,1] and ``right_imorint`` (B H W pairs in any shape) at the index
    b H W + y' W + x' clamped to the maps (math_utils.py:43-106).  HIP fp32 runs ``hn_project_keypoints``."""
    B, H, W, _ = right_imscale.size()
    if (B > 0 and H >= 2 and W >= 2 and leftC.dtype == torch.int64 and leftC.dim() == 2 and leftC.shape[1] == 4
            and homolr.dtype == torch.float32 and right_imscale.dtype == torch.float32
            and (right_imorint is None or right_imorint.dtype == torch.float32)
            and _hip32(leftC, homolr, right_imscale, right_imorint)):
        from . import _native
        om = right_imorint.detach().reshape(B, H, W, 2) if right_imorint is not None else None
        return _native.project_keypoints(leftC, homolr.detach(), (B, H, W),
                                         scale_map=_scale_map(right_imscale, (B, H, W)), ori_map=om, clamp=clamp)
    return _ptCltoCr_torch(leftC, homolr, right_imscale, right_imorint, clamp)


def _mask_keypoints(left_imtopk, left_imscale, left_imorint, topk):
    """(left_imC, left_imS, left_imO): nonzero() and the masked_selects of pair (net_utils.py:27-37)."""
    B, H, W, _ = left_imtopk.size()
    if (topk is not None and B > 0 and H >= 2 and W >= 2 and left_imtopk.dtype == torch.uint8
            and left_imscale.dtype == torch.float32
            and (left_imorint is None or left_imorint.dtype == torch.float32)
            and _hip32(left_imtopk, left_imscale, left_imorint)):
        from . import _native
        om = left_imorint.detach().reshape(B, H, W, 2) if left_imorint is not None else None
        kpts, kscale, kori, _ = _native.mask_keypoints(left_imtopk.reshape(B, H, W), int(topk),
                                                       scale_map=_scale_map(left_imscale, (B, H, W)), ori_map=om)
        return kpts, kscale, kori
    sel = left_imtopk.to(torch.bool)
    left_imC = left_imtopk.nonzero()
    left_imS = left_imscale.masked_select(sel)
    if left_imorint is None:
        return left_imC, left_imS, None
    left_cos, left_sim = left_imorint.reshape(B, H, W, 2).chunk(chunks=2, dim=-1)
    left_imO = torch.cat((left_cos.masked_select(sel).unsqueeze(-1), left_sim.masked_select(sel).unsqueeze(-1)), dim=-1)
    return left_imC, left_imS, left_imO


def _clip_patch_matmul(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
    """clip_patch (utils/image_utils.py:11-158) in the reference's own operation order -- the 3x3 affine built as
    scale . rotation by one batched matmul and applied to the [3, PSIZE^2] grid by another -- in the dtype of
    ``images``, with the keypoint's own column 0 selecting its ratio.  ``patches.clip_patch``'s torch formulation
    applies the same affine term by term (the order of the kernel, hn_clip.h); the two differ by the rounding of a
    sample coordinate (at most 2 E_ref of clip_patch.npz), and ``pair`` is held to the reference's fp32 patches more
    tightly than that, so its torch path runs this form."""
    dt, dev = images.dtype, images.device
    B, _, H, W = images.shape
    n = kpts_byxc.size(0)
    g = torch.linspace(-1, 1, PSIZE, dtype=torch.float, device=dev)
    y_t, x_t = torch.meshgrid([g, g], indexing="ij")
    x_t, y_t = x_t.contiguous().view(-1), y_t.contiguous().view(-1)
    grid = torch.stack((x_t, y_t, torch.ones_like(x_t))).view(-1).repeat(n).view(n, 3, -1).to(dt)
    b = kpts_byxc[:, 0].clamp(0, B - 1)
    r = im_info[:, 0].to(dt)[b]
    s = (kpts_scale.reshape(-1).to(dt) / r) / 2.0
    thetas = torch.eye(2, 3, dtype=dt, device=dev).unsqueeze(0).repeat(n, 1, 1) * s[:, None, None]
    thetas = torch.cat((thetas, torch.tensor([[[0, 0, 1]]], dtype=dt, device=dev).repeat(n, 1, 1)), 1)
    if kpts_ori is not None:
        cos, sin = kpts_ori[:, 0].to(dt).unsqueeze(-1), kpts_ori[:, 1].to(dt).unsqueeze(-1)
        zeros, ones = torch.zeros_like(cos), torch.ones_like(cos)
        R = torch.cat((cos, -sin, zeros, sin, cos, zeros, zeros, zeros, ones), dim=-1).view(-1, 3, 3)
        thetas = torch.matmul(thetas, R)
    T_g = torch.matmul(thetas, grid)
    x = (T_g[:, 0, :] + (kpts_byxc[:, 2].to(dt) / r).view(-1, 1)).reshape(-1)
    y = (T_g[:, 1, :] + (kpts_byxc[:, 1].to(dt) / r).view(-1, 1)).reshape(-1)
    x0, y0 = x.detach().floor().long(), y.detach().floor().long()
    x1, y1 = (x0 + 1).clamp(min=0, max=W - 1), (y0 + 1).clamp(min=0, max=H - 1)
    x0, y0 = x0.clamp(min=0, max=W - 1), y0.clamp(min=0, max=H - 1)
    base = b.unsqueeze(-1).repeat(1, PSIZE * PSIZE).view(-1) * (H * W)
    im_flat = images.reshape(-1)
    Ia, Ib = im_flat[base + y0 * W + x0], im_flat[base + y1 * W + x0]
    Ic, Id = im_flat[base + y0 * W + x1], im_flat[base + y1 * W + x1]
    x0_f, x1_f, y0_f, y1_f = x0.to(dt), x1.to(dt), y0.to(dt), y1.to(dt)
    wa, wb = (x1_f - x) * (y1_f - y), (x1_f - x) * (y - y0_f)
    wc, wd = (x - x0_f) * (y1_f - y), (x - x0_f) * (y - y0_f)
    return (wa * Ia + wb * Ib + wc * Ic + wd * Id).view(n, PSIZE, PSIZE).unsqueeze(1)


def _pair_patches(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE):
    """The patches of ``pair``: ``hn_clip_patch`` where ``patches.clip_patch`` would run it -- alone, or under autograd
    on the keypoints' scale / orientation with ``hn_clip_patch_backward`` behind it -- else the reference's operation
    order (``_clip_patch_matmul``)."""
    if (_patches._native_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)
            or _patches._native_grad_ok(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)):
        return clip_patch(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE=PSIZE)
    return _clip_patch_matmul(kpts_byxc, kpts_scale, kpts_ori, im_info, images, PSIZE)


def pair(left_imtopk, left_topkvalue, left_imscale, left_imorint, left_iminfo, left_imraw, homolr, right_imscale,
         right_imorint, right_iminfo, right_imraw, PSIZE, topk=None):
    """Patch pairs of the left image's top-K mask (net_utils.py:10-53): ``(left_impair [N,2,PSIZE,PSIZE], left_imC
    [N,4], right_imC [N,4])`` -- the patches around the mask's pixels in the left image and around their clamped
    projections in the right image.  With ``topk`` given, HIP fp32 inputs and PSIZE = 32 every step runs on the
    library's kernels and N = B topk.  Where ``hn_clip_patch`` does not run, the patches are cut in the reference's
    operation order (``_clip_patch_matmul``)."""
    native = topk if PSIZE == NATIVE_PSIZE else None
    left_imC, left_imS, left_imO = _mask_keypoints(left_imtopk, left_imscale, left_imorint, native)
    left_imP = _pair_patches(left_imC, left_imS, left_imO, left_iminfo, left_imraw, PSIZE)
    right_imC, right_imS, right_imO = ptCltoCr(left_imC, homolr, right_imscale, right_imorint)
    right_imP = _pair_patches(right_imC, right_imS, right_imO, right_iminfo, right_imraw, PSIZE)
    return torch.cat((left_imP, right_imP), 1), left_imC, right_imC


# ---------------------------------------------------------------------------------------------------------------
# Network
# ---------------------------------------------------------------------------------------------------------------
ENDPOINT_KEYS = ("im1_score", "im1_gtsc", "im1_visible", "im2_score", "im2_gtsc", "im2_visible", "im1_limc",
                 "im1_rimcw", "im2_limc", "im2_rimcw", "im1_lpdes", "im1_rpdes", "im2_lpdes", "im2_rpdes",
                 "im1_lpreddes", "im1_rpreddes", "im2_lpreddes", "im2_rpreddes")


class Network(nn.Module):
    """model/network.py:12-324: detector + descriptor with the homography ground-truth stage between them."""

    def __init__(self, det, des, SCORE_W, PAIR_W, PSIZE, TOPK):
        super().__init__()
        self.det = det
        self.des = des
        self.PSIZE = PSIZE
        self.TOPK = TOPK
        self.SCORE_W = SCORE_W
        self.PAIR_W = PAIR_W

    # ---- native path -------------------------------------------------------------------------------------------
    def _native_ok(self, batch) -> bool:
        from .model import _NativeMixin, _native_blocker
        im1_data, im1_info, homo12, im2_data, im2_info, homo21, im1_raw, im2_raw = batch
        det = self.det
        if not (self.PSIZE == NATIVE_PSIZE and hasattr(det, "_native_ok") and hasattr(det, "forward_maps")
                and isinstance(self.des, _NativeMixin) and int(det.TOPK) >= 1):
            return False
        if det.scale_list.numel() != 1:
            # _forward_native passes the one constant scale to the ground-truth stage; a detector with a scale map
            # (RFDetSO) takes the reference-order path below, which carries the maps
            return False
        if not (det._native_ok(im1_data) and det._native_ok(im2_data) and im1_data.shape == im2_data.shape
                and im1_data.shape[2] > 2 * BORDER and im1_data.shape[3] > 2 * BORDER
                and int(det.TOPK) <= im1_data.shape[2] * im1_data.shape[3]):
            return False
        dev = im1_data.device
        for t in (im1_info, homo12, im2_info, homo21, im1_raw, im2_raw):
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32):
                return False
        if im1_raw.shape != im1_data.shape or im2_raw.shape != im2_data.shape:
            return False
        if _records_grad(im1_info, homo12, im2_info, homo21, im1_raw, im2_raw):
            return False
        probe = torch.empty((0, 1, NATIVE_PSIZE, NATIVE_PSIZE), device=dev)
        return _native_blocker(self.des, probe) is None

    def _forward_native(self, batch):
        """The endpoint as a composition of the library's calls: no torch kernel, no host synchronisation."""
        from . import _native
        im1_data, im1_info, homo12, im2_data, im2_info, homo21, im1_raw, im2_raw = batch
        det, K = self.det, int(self.det.TOPK)
        sv = float(det.scale_list[0])
        sel = det._select_args()
        probe = torch.empty((0, 1, NATIVE_PSIZE, NATIVE_PSIZE), device=im1_data.device)
        nm = _native._BY_ID[self.des._native_handle(probe)]
        score1, ori1 = det.forward_maps(im1_data)
        score2, ori2 = det.forward_maps(im2_data)
        raw1, raw2 = im1_raw.detach(), im2_raw.detach()
        ratio1, ratio2 = im1_info.detach()[:, 0].contiguous(), im2_info.detach()[:, 0].contiguous()
        h12, h21 = homo12.detach(), homo21.detach()
        shape = tuple(score1.shape)
        end = {}

        def side(tag, score_l, ori_l, score_r, ori_r, hlr, hrl, raw_l, raw_r, ratio_l, ratio_r, gt_r):
            # gtscore(right score, homolr): the right score seen from the left image, then det.process
            warped, visible = _native.warp_score(score_r, hlr, border=BORDER, align_corners=False)
            gt = _native.select_keypoints(warped, *sel, dense=True)
            own = _native.select_keypoints(score_l, *sel, dense=True)
            end[tag + "_score"] = own["score_proc"].unsqueeze(-1)
            end[tag + "_gtsc"] = gt["score_proc"].unsqueeze(-1)
            end[tag + "_visible"] = visible.unsqueeze(-1)
            # pair: the gtscore mask's pixels in the left image, projected into the right image
            limc, ls, lo, _ = _native.mask_keypoints(gt["topk_mask"], K, scale_value=sv, ori_map=ori_l)
            rimcw, rs, ro = _native.project_keypoints(limc, hlr, shape, scale_map=gt_r[0], ori_map=gt_r[1], clamp=True)
            _, ps, po = _native.project_keypoints(limc, hlr, shape, scale_value=sv, ori_map=ori_r, clamp=True)
            end[tag + "_limc"], end[tag + "_rimcw"] = limc, rimcw
            lpdes = nm.forward_keypoints(raw_l, limc, ls, lo, ratio_l)
            end[tag + "_lpdes"] = end[tag + "_lpreddes"] = lpdes
            end[tag + "_rpdes"] = nm.forward_keypoints(raw_r, rimcw, rs, ro, ratio_r)
            end[tag + "_rpreddes"] = nm.forward_keypoints(raw_r, rimcw, ps, po, ratio_r)

        gt1 = _native.gt_scale_orin(None, ori2, h12, h21, scale_value=sv)  # image 1's ground truth, from image 2
        gt2 = _native.gt_scale_orin(None, ori1, h21, h12, scale_value=sv)
        side("im1", score1, ori1, score2, ori2, h12, h21, raw1, raw2, ratio1, ratio2, gt2)
        side("im2", score2, ori2, score1, ori1, h21, h12, raw2, raw1, ratio2, ratio1, gt1)
        return {k: end[k] for k in ENDPOINT_KEYS}

    # ---- the reference's methods -------------------------------------------------------------------------------
    def forward(self, batch):
        if self._native_ok(batch):
            return self._forward_native(batch)
        im1_data, im1_info, homo12, im2_data, im2_info, homo21, im1_raw, im2_raw = batch
        im1_rawsc, im1_scale, im1_orin = self.det(im1_data)
        im2_rawsc, im2_scale, im2_orin = self.det(im2_data)
        im1_gtscale, im1_gtorin = self.gt_scale_orin(im2_scale, im2_orin, homo12, homo21)
        im2_gtscale, im2_gtorin = self.gt_scale_orin(im1_scale, im1_orin, homo21, homo12)
        im1_gtsc, im1_topkmask, im1_topkvalue, im1_visiblemask = self.gtscore(im2_rawsc, homo12)
        im2_gtsc, im2_topkmask, im2_topkvalue, im2_visiblemask = self.gtscore(im1_rawsc, homo21)
        im1_score = self.det.process(im1_rawsc)[0]
        im2_score = self.det.process(im2_rawsc)[0]

        def pairs(topkmask, topkvalue, l_scale, l_orin, l_info, l_raw, homolr, r_gtscale, r_gtorin, r_scale, r_orin,
                  r_info, r_raw):
            """The two pair calls of one side: (limc, rimcw, lpdes, rpdes, lpreddes, rpreddes); the left patches,
            which both calls cut identically, are cut and described once."""
            ppair, limc, rimcw = pair(topkmask, topkvalue, l_scale, l_orin, l_info, l_raw, homolr, r_gtscale,
                                      r_gtorin, r_info, r_raw, self.PSIZE)
            lpatch, rpatch = ppair.chunk(chunks=2, dim=1)
            _, predS, predO = ptCltoCr(limc, homolr, r_scale, r_orin)
            rpredpatch = _pair_patches(rimcw, predS, predO, r_info, r_raw, self.PSIZE)
            lpdes = self.des(lpatch)
            return limc, rimcw, lpdes, self.des(rpatch), lpdes, self.des(rpredpatch)

        im1 = pairs(im1_topkmask, im1_topkvalue, im1_scale, im1_orin, im1_info, im1_raw, homo12, im2_gtscale,
                    im2_gtorin, im2_scale, im2_orin, im2_info, im2_raw)
        im2 = pairs(im2_topkmask, im2_topkvalue, im2_scale, im2_orin, im2_info, im2_raw, homo21, im1_gtscale,
                    im1_gtorin, im1_scale, im1_orin, im1_info, im1_raw)
        return {
            "im1_score": im1_score, "im1_gtsc": im1_gtsc, "im1_visible": im1_visiblemask,
            "im2_score": im2_score, "im2_gtsc": im2_gtsc, "im2_visible": im2_visiblemask,
            "im1_limc": im1[0], "im1_rimcw": im1[1], "im2_limc": im2[0], "im2_rimcw": im2[1],
            "im1_lpdes": im1[2], "im1_rpdes": im1[3], "im2_lpdes": im2[2], "im2_rpdes": im2[3],
            "im1_lpreddes": im1[4], "im1_rpreddes": im1[5], "im2_lpreddes": im2[4], "im2_rpreddes": im2[5],
        }

    def inference(self, im_data, im_info, im_raw):
        """``(im_scale, kpts, im_des, scale, ori, score)`` (network.py:148-183): ``detector.detect_and_describe``."""
        from .detector import detect_and_describe
        return detect_and_describe(self.det, self.des, im_data, im_info, im_raw)

    def gtscore(self, right_score, homolr):
        """(processed warped score, its top-K mask, its NMS'd score, visible mask), each [B,H,W,1]
        (network.py:185-198)."""
        if (right_score.dim() == 4 and right_score.shape[3] == 1 and right_score.shape[0] > 0
                and right_score.shape[1] > 2 * BORDER and right_score.shape[2] > 2 * BORDER
                and right_score.dtype == torch.float32 and homolr.dtype == torch.float32
                and _hip32(right_score, homolr)):
            from . import _native
            warped, visible = _native.warp_score(right_score.detach().squeeze(-1), homolr.detach(), border=BORDER)
            return (*self.det.process(warped.unsqueeze(-1)), visible.unsqueeze(-1))
        im2_score = filter_border(right_score)
        im1w_score = warp(im2_score, homolr)
        im1visible_mask = warp(im2_score.new_full(im2_score.size(), fill_value=1), homolr)
        return (*self.det.process(im1w_score), im1visible_mask)

    gt_scale_orin = staticmethod(gt_scale_orin)

    def criterion(self, endpoint):
        """``(PLT, det_loss, des_loss)`` (network.py:266-324): the score loss (``det.loss``) and the pair loss
        (``losses.pair_distance_loss``) weighted into the detector's loss, the hard loss (``des.loss``) the
        descriptor's."""
        from .losses import pair_distance_loss
        e = endpoint
        im1_scloss = self.det.loss(e["im1_score"], e["im1_gtsc"], e["im1_visible"])
        im2_scloss = self.det.loss(e["im2_score"], e["im2_gtsc"], e["im2_visible"])
        score_loss = (im1_scloss + im2_scloss) / 2.0 * self.SCORE_W
        im1_pairloss = pair_distance_loss(e["im1_lpreddes"], e["im1_rpreddes"])
        im2_pairloss = pair_distance_loss(e["im2_lpreddes"], e["im2_rpreddes"])
        pair_loss = (im1_pairloss + im2_pairloss) / 2.0 * self.PAIR_W
        im1_hardloss = self.des.loss(e["im1_lpdes"], e["im1_rpdes"], e["im1_limc"], e["im1_rimcw"])
        im2_hardloss = self.des.loss(e["im2_lpdes"], e["im2_rpdes"], e["im2_limc"], e["im2_rimcw"])
        hard_loss = (im1_hardloss + im2_hardloss) / 2.0
        det_loss = score_loss + pair_loss
        des_loss = hard_loss
        PLT = {"scalar": {"score_loss": score_loss, "pair_loss": pair_loss, "hard_loss": hard_loss}}
        return PLT, det_loss.mean(), des_loss.mean()
