"""FDLNet's keypoint detector and keypoint selection: the first two steps of ``Network.inference``
(FDLNet-master/latency/NASNet/model/network.py:148-183)

    detector -> process / topk_map -> clip_patch -> des(patches) -> NN / NNT / NNDR matching

``RFDet`` is a drop-in for the NASNet variant's detector (model/det.py): the reference's constructor arguments,
attributes and ``state_dict`` keys, so a reference checkpoint loads with ``strict=True``.  In eval mode on HIP fp32
``[B,1,H,W]`` images with no autograd graph to record, ``forward`` runs ``hn_det_forward`` (two kernels, hn_det.hip)
and ``process`` / ``detect`` run ``hn_select_keypoints`` (hn_select.hip).  In train mode under autograd, on HIP fp32
images that need no gradient, ``forward`` runs ``hn_det_train_forward`` and records a ``DetTrainFunction`` node whose
backward is ``hn_det_train_backward`` (hn_det_train.hip).  Everywhere else -- CPU tensors, fp64, train mode under
``no_grad``, eval mode under autograd -- the torch layers below run; they restate the reference formulas operation
by operation and in fp64 are the ground truth of the tests.

``select_keypoints_torch`` restates the selection with the C ABI's tie rule: both top-K steps order pixels by
(value descending, flat index ascending) -- a stable descending sort -- where the reference leaves ties to
``torch.sort``; a NaN score counts as 0.  Where no cut falls inside a group of equal values the two agree.

``RFDetSO`` is RF-Net's detector (rfnet/model/rf_det_so.py), the one with real scale selection: ten levels, a scale
and an orientation per pixel; in eval mode on HIP fp32 images its ``forward`` runs ``hn_rfdet_forward``
(hn_rfdet.hip) and everywhere else its torch layers.  It shares ``process``, ``loss`` and the initialisers with ``RFDet``.

``detect`` is image -> keypoints and ``detect_and_describe`` image -> descriptors (the reference ``inference``
tuple), with no torch kernel and no host synchronisation between the image and the descriptors on the native path.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

BORDER = 8          # filter_border's radius (utils/image_utils.py:211)
SOFT_NMS_KSIZE = 15  # soft_nms_3d's arguments in RFDet.forward (model/det.py:83)
SOFT_NMS_STRENGTH = 7.0


def channel_shuffle(x, groups):
    """model/operations.py:437-447: new channel j * groups + g is old channel g * (C / groups) + j."""
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).contiguous().view(b, c, h, w)


class InvertedResidual(nn.Module):
    """model/operations.py:449-511 with benchmodel 1, stride 1 (the only form the detector uses)."""

    def __init__(self, inp, oup, stride, benchmodel):
        super().__init__()
        if benchmodel != 1 or stride != 1:
            raise ValueError("the detector uses InvertedResidual(benchmodel=1, stride=1) only")
        self.benchmodel, self.stride = benchmodel, stride
        c = oup // 2
        self.banch2 = nn.Sequential(
            nn.Conv2d(c, c, 1, 1, 0, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True),
            nn.Conv2d(c, c, 3, stride, 1, groups=c, bias=False), nn.BatchNorm2d(c),
            nn.Conv2d(c, c, 1, 1, 0, bias=False), nn.BatchNorm2d(c), nn.ReLU(inplace=True))

    def forward(self, x):
        h = x.shape[1] // 2
        return channel_shuffle(torch.cat((x[:, :h], self.banch2(x[:, h:])), 1), 2)


def soft_nms_3d(scale_logits, ksize, com_strength):
    """utils/image_utils.py:298-329 on [B,H,W,C] logits."""
    x = scale_logits.permute(0, 3, 1, 2)
    m = F.max_pool2d(x, kernel_size=ksize, padding=ksize // 2, stride=1).max(dim=1, keepdim=True)[0]
    e = torch.exp(com_strength * (x - m))
    s = F.conv2d(e, e.new_full([1, x.shape[1], ksize, ksize], 1.0), stride=1, padding=ksize // 2)
    return (e / (s + 1e-8)).permute(0, 2, 3, 1)


def soft_max_and_argmax_1d(input, scale_list, com_strength1, com_strength2, orint_maps=None):
    """utils/image_utils.py:332-367 (dim -1, keepdim): (score_map, scale_map); with ``orint_maps`` [..., C, 2] the
    three-output form of rfnet/utils/image_utils.py:332-375: (score_map, scale_map, orint_map [..., 1, 2])."""
    mx = input.max(dim=-1, keepdim=True)[0]
    e1 = torch.exp(com_strength1 * (input - mx))
    e2 = torch.exp(com_strength2 * (input - mx))
    s1 = e1 / (e1.sum(dim=-1, keepdim=True) + 1e-8)
    s2 = e2 / (e2.sum(dim=-1, keepdim=True) + 1e-8)
    scale_list = scale_list.view(*([1] * (input.dim() - 1)), -1).to(device=input.device, dtype=input.dtype)
    score_map, scale_map = (input * s1).sum(dim=-1, keepdim=True), (scale_list * s2).sum(dim=-1, keepdim=True)
    if orint_maps is None:
        return score_map, scale_map
    orint_map = (orint_maps * s1.unsqueeze(-1)).sum(dim=-2, keepdim=True)
    return score_map, scale_map, orint_map / torch.norm(orint_map, p=2, dim=-1, keepdim=True)


def gauss_filter_weight(ksize, sig):
    """utils/image_utils.py:277-295 (fp32, not normalised; sigma 0 is a delta)."""
    mu = ksize // 2
    if sig == 0:
        psf = torch.zeros((ksize, ksize)).float()
        psf[mu, mu] = 1.0
        return psf
    sig = torch.tensor(sig).float()
    x = torch.arange(ksize)[None, :].repeat(ksize, 1).float()
    y = torch.arange(ksize)[:, None].repeat(1, ksize).float()
    return torch.exp(-((x - mu) ** 2 / (2 * sig ** 2) + (y - mu) ** 2 / (2 * sig ** 2)))


def gauss_taps_abi(ksize, sig):
    """The blur weights as hn_select_keypoints computes them: the reference's fp32 exponent, the exponential
    evaluated in fp64 and rounded to fp32 (equal to ``gauss_filter_weight`` up to the last bit of torch's fp32 exp)."""
    import math
    import numpy as np
    mu, f = ksize // 2, np.float32
    if sig == 0:
        return gauss_filter_weight(ksize, 0)
    two_s2 = f(2.0) * (f(sig) * f(sig))
    rows = [[f(math.exp(float(-((f(x - mu) * f(x - mu)) / two_s2 + (f(y - mu) * f(y - mu)) / two_s2))))
             for x in range(ksize)] for y in range(ksize)]
    return torch.tensor(rows, dtype=torch.float32)


def _blur_abi(g, psf):
    """clamp(conv(g, psf), 0, 1) on fp32 [B,H,W] in hn_select_keypoints' arithmetic: taps in row-major order, each a
    fused multiply-add -- emulated as the exact fp64 product plus the accumulator, rounded to fp32 (a true FMA but
    for a double rounding of probability ~2^-29 per operation)."""
    k = psf.shape[0]
    pad = k // 2
    b, h, w = g.shape
    gp = F.pad(g, (pad, pad, pad, pad)).double()
    acc = torch.zeros_like(g)
    for ky in range(k):
        for kx in range(k):
            acc = (gp[:, ky:ky + h, kx:kx + w] * float(psf[ky, kx]) + acc.double()).float()
    return acc.clamp(0.0, 1.0)


def _nms_value(score, border, nms_thresh, nms_ksize):
    """Steps 1-2 of the selection on [B,H,W]: f (border filtered, NaN as 0) and v = f keep."""
    b, h, w = score.shape
    s = torch.nan_to_num(score, nan=0.0) if torch.isnan(score).any() else score
    f = torch.zeros_like(s)
    f[:, border:h - border, border:w - border] = s[:, border:h - border, border:w - border]
    t = torch.where(f < nms_thresh, torch.zeros_like(f), f)
    pad = nms_ksize // 2
    mx = F.max_pool2d(F.pad(t.unsqueeze(1), (pad, pad, pad, pad), value=0.0), nms_ksize, stride=1).squeeze(1)
    v = f * (t >= mx).to(f.dtype)
    return torch.where(v == 0, torch.zeros_like(v), v)  # -0 -> +0


def _topk_mask(maps, k):
    """[B,H,W] bool mask of the k largest per image, ties by lowest flat index (stable descending sort)."""
    b = maps.shape[0]
    flat = maps.reshape(b, -1)
    idx = flat.sort(dim=-1, descending=True, stable=True)[1][:, :k]
    mask = torch.zeros_like(flat, dtype=torch.bool)
    mask.scatter_(1, idx, True)
    return mask.view_as(maps)


def select_keypoints_torch(score, border, nms_thresh, nms_ksize, topk, gauss_ksize, gauss_sigma, scale_map=None,
                           scale_value=32.0, ori_map=None, abi_blur=False):
    """The selection of ``hn_select_keypoints`` in torch, in the dtype of ``score`` [B,H,W]:
    (kpts [B K,4] int64, kscore, kscale, kori or None, q [B,H,W], topk_mask [B,H,W] uint8, v [B,H,W]).
    The blur is the reference's ``F.conv2d``; with ``abi_blur`` (fp32 only) it is the C ABI's, bit for bit (its
    weights, tap order and fused multiply-adds), so that near-equal blurred values order as they do on the GPU."""
    v = _nms_value(score, border, nms_thresh, nms_ksize)
    mask = _topk_mask(v, topk)
    g = v * mask.to(v.dtype)
    if abi_blur:
        q = _blur_abi(g, gauss_taps_abi(gauss_ksize, gauss_sigma))
    else:
        psf = gauss_filter_weight(gauss_ksize, gauss_sigma).to(device=score.device, dtype=score.dtype)
        q = F.conv2d(g.unsqueeze(1), psf[None, None], stride=1, padding=gauss_ksize // 2).squeeze(1).clamp(0.0, 1.0)
    top = _topk_mask(q, topk)
    kp = top.nonzero()
    kpts = torch.cat((kp, torch.zeros_like(kp[:, :1])), dim=1)
    kscore = score[top]
    kscale = scale_map[top] if scale_map is not None else score.new_full((kpts.shape[0],), scale_value)
    kori = ori_map[top] if ori_map is not None else None
    return kpts, kscore, kscale, kori, q, mask.to(torch.uint8), v


class _DetectorBase(nn.Module):
    """What RFDet and RFDetSO share (model/det.py:96-166 is rfnet/model/rf_det_module.py:182-244): ``process``,
    ``loss``, the initialisers and the selection arguments, over the attributes both constructors set."""

    def _select_args(self):
        return (BORDER, float(self.NMS_THRESH), int(self.NMS_KSIZE), int(self.TOPK), int(self.GAUSSIAN_KSIZE),
                float(self.GAUSSIAN_SIGMA))

    def process(self, im1w_score):
        """nms, top-K and Gaussian blur of a [B,H,W,1] score map (model/det.py:96-133):
        (processed score, top-K mask uint8, NMS'd score), each [B,H,W,1]."""
        s = im1w_score.squeeze(-1)
        if (s.is_cuda and s.dtype == torch.float32 and s.shape[0] > 0
                and not (torch.is_grad_enabled() and s.requires_grad)):
            from . import _native
            out = _native.select_keypoints(s.detach(), *self._select_args(), dense=True)
            # the NMS'd score is no output of the C ABI (inference never reads it): a pad and a max-pool in torch
            v = _nms_value(s.detach(), BORDER, float(self.NMS_THRESH), int(self.NMS_KSIZE))
            return out["score_proc"].unsqueeze(-1), out["topk_mask"].unsqueeze(-1), v.unsqueeze(-1)
        _, _, _, _, q, mask, v = select_keypoints_torch(s, *self._select_args())
        return q.unsqueeze(-1), mask.unsqueeze(-1), v.unsqueeze(-1)

    @staticmethod
    def loss(left_score, im1gt_score, im1visible_mask):
        l2_element_diff = (left_score - im1gt_score) ** 2
        Nvi = torch.clamp(im1visible_mask.sum(dim=(3, 2, 1)), min=2.0)
        return (torch.sum(l2_element_diff * im1visible_mask, dim=(3, 2, 1)) / (Nvi + 1e-8)).mean()

    @staticmethod
    def weights_init(m):
        if isinstance(m, nn.Conv2d):
            nn.init.xavier_uniform_(m.weight.data, gain=nn.init.calculate_gain("leaky_relu"))
            try:
                nn.init.xavier_uniform_(m.bias.data)
            except Exception:
                pass

    @staticmethod
    def convO_init(m):
        if isinstance(m, nn.Conv2d):
            nn.init.zeros_(m.weight.data)
            try:
                nn.init.ones_(m.bias.data)
            except Exception:
                pass


class RFDet(_DetectorBase):
    """model/det.py:14-166 (NASNet variant: one scale, 32)."""

    def __init__(self, score_com_strength, scale_com_strength, nms_thresh, nms_ksize, topk, gauss_ksize, gauss_sigma):
        super().__init__()
        self.score_com_strength = score_com_strength
        self.scale_com_strength = scale_com_strength
        self.NMS_THRESH = nms_thresh
        self.NMS_KSIZE = nms_ksize
        self.TOPK = topk
        self.GAUSSIAN_KSIZE = gauss_ksize
        self.GAUSSIAN_SIGMA = gauss_sigma
        self.features = nn.Sequential(nn.Conv2d(1, 16, kernel_size=3, stride=1, padding=1),
                                      InvertedResidual(16, 16, 1, 1), InvertedResidual(16, 16, 1, 1))
        self.conv = nn.Conv2d(in_channels=16, out_channels=1, kernel_size=3, stride=1, padding=1)
        self.insnorm = nn.InstanceNorm2d(1, affine=True)
        self.conv_ori = nn.Conv2d(in_channels=16, out_channels=2, kernel_size=3, stride=1, padding=1)
        self.insnorm_ori = nn.InstanceNorm2d(2, affine=True)
        self.scale_list = torch.tensor([32.0])
        self._native = None  # (key, NativeDetector)

    # ---- native path -------------------------------------------------------------------------------------------
    def _native_ok(self, photos) -> bool:
        return (not self.training and photos.is_cuda and photos.dtype == torch.float32 and photos.dim() == 4
                and photos.shape[1] == 1 and photos.shape[0] > 0 and photos.shape[2] * photos.shape[3] >= 2
                and self.conv.weight.device == photos.device
                and not (torch.is_grad_enabled() and (photos.requires_grad
                                                      or any(p.requires_grad for p in self.parameters()))))

    def _native_train_ok(self, photos) -> bool:
        """train() under autograd on HIP fp32 images that need no gradient: ``forward`` runs ``hn_det_train_forward``
        and records a ``DetTrainFunction`` node (every BatchNorm tracking running statistics with one float momentum
        and one eps, which the C ABI takes once)."""
        if not (self.training and torch.is_grad_enabled() and photos.is_cuda and photos.dtype == torch.float32
                and photos.dim() == 4 and photos.shape[1] == 1 and photos.is_contiguous()
                and photos.numel() >= 2 and not photos.requires_grad):
            return False
        tensors = [*self.parameters(), *self.buffers()]
        if not (all(t.device == photos.device and (t.dtype == torch.float32 or not t.is_floating_point())
                    for t in tensors) and any(p.requires_grad for p in self.parameters())):
            return False
        bns = self._batchnorms()
        return (all(m.track_running_stats and isinstance(m.momentum, float) and m.running_mean is not None
                    for m in bns)
                and len({m.momentum for m in bns}) == 1 and len({m.eps for m in bns}) == 1
                and self.insnorm.eps == self.insnorm_ori.eps and self.insnorm.affine and self.insnorm_ori.affine
                and not self.insnorm.track_running_stats and not self.insnorm_ori.track_running_stats)

    def _batchnorms(self):
        return [m for m in self.features.modules() if isinstance(m, nn.BatchNorm2d)]

    def forward_train_maps(self, photos):
        """(score [B,H,W,1], ori [B,H,W,2]) of the native train-mode forward, with its autograd node."""
        from . import _native
        tensors = _native.det_train_tensors(self)
        bns = self._batchnorms()
        return _native.DetTrainFunction.apply(photos, tensors, bns, bns[0].eps, self.insnorm.eps, bns[0].momentum,
                                              *[t for t in tensors if t.requires_grad])

    def native_detector(self, device):
        """The NativeDetector of the current weights on ``device`` (rebuilt when a tensor of the state changes)."""
        from . import _native
        key = (str(device),) + tuple((v.data_ptr(), v._version) for v in (*self.parameters(), *self.buffers()))
        if self._native is None or self._native[0] != key:
            self._native = (key, _native.NativeDetector(_native.state_dict_blob(self.state_dict()), device,
                                                        bn_eps=self.features[1].banch2[1].eps, in_eps=self.insnorm.eps))
        return self._native[1]

    def forward_maps(self, photos):
        """(score [B,H,W], ori [B,H,W,2]) of the native forward."""
        return self.native_detector(photos.device).forward(photos.detach())

    def _apply(self, fn, *a, **k):
        self._native = None
        return super()._apply(fn, *a, **k)

    # ---- the reference's methods -------------------------------------------------------------------------------
    def forward(self, photos):
        if self._native_train_ok(photos):
            # the scale map is the constant 32 with no graph: in the reference its gradient is exactly zero (the two
            # paths through input - max in soft_max_and_argmax_1d cancel)
            score, ori = self.forward_train_maps(photos)
            return score, torch.full((), float(self.scale_list[0]), device=score.device).expand_as(score), ori
        if self._native_ok(photos):
            score, ori = self.forward_maps(photos)
            score = score.unsqueeze(-1)
            return score, torch.full((), float(self.scale_list[0]), device=score.device).expand_as(score), ori
        return self.forward_torch(photos)

    def forward_torch(self, photos):
        """The torch layers (model/det.py:57-94), whatever the device: the CPU / fp64 / training path."""
        feature_map = self.features(photos)
        feature_map_1 = F.leaky_relu(self.insnorm(self.conv(feature_map)))
        ori_map = self.insnorm_ori(self.conv_ori(feature_map))
        ori_map = (ori_map / torch.norm(ori_map, p=2, dim=1, keepdim=True)).permute(0, 2, 3, 1)
        score_maps = feature_map_1.permute(0, 2, 3, 1)
        scale_probs = soft_nms_3d(score_maps, ksize=SOFT_NMS_KSIZE, com_strength=SOFT_NMS_STRENGTH)
        score_map, scale_map = soft_max_and_argmax_1d(scale_probs, self.scale_list, self.score_com_strength,
                                                      self.scale_com_strength)
        return score_map, scale_map, ori_map


RF_LEVELS = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21)  # the receptive fields that name RFDetSO's heads
RF_SOFT_NMS_STRENGTH = 3.0                        # soft_nms_3d's com_strength in RFDetSO.forward (rf_det_so.py:220)


class RFDetSO(_DetectorBase):
    """RF-Net's detector (rfnet/model/rf_det_so.py over rf_det_module.py): ten receptive-field levels 3 .. 21, a
    score head and an orientation head at each, scale selection by a 3-D soft NMS over (y, x, level).  The
    reference's constructor arguments, attributes and ``state_dict`` keys.  ``forward`` returns ``score [B,H,W,1]``,
    ``scale [B,H,W,1]``, ``ori [B,H,W,1,2]`` on every path: in eval mode on HIP fp32 ``[B,1,H,W]`` images with no
    autograd graph to record and ksize / padding / dilation 3 / 1 / 1 it runs ``hn_rfdet_forward`` (hn_rfdet.hip);
    everywhere else -- CPU, fp64, ``train()``, autograd -- the torch layers."""

    def __init__(self, score_com_strength, scale_com_strength, nms_thresh, nms_ksize, topk, gauss_ksize, gauss_sigma,
                 ksize, padding, dilation, scale_list):
        super().__init__()
        self.score_com_strength = score_com_strength
        self.scale_com_strength = scale_com_strength
        self.NMS_THRESH = nms_thresh
        self.NMS_KSIZE = nms_ksize
        self.TOPK = topk
        self.GAUSSIAN_KSIZE = gauss_ksize
        self.GAUSSIAN_SIGMA = gauss_sigma
        self._conv_geometry = (ksize, padding, dilation)
        for k, rf in enumerate(RF_LEVELS, start=1):  # registration order = the reference's state_dict order
            setattr(self, f"conv{k}", nn.Conv2d(1 if k == 1 else 16, 16, kernel_size=ksize, stride=1, padding=padding,
                                                dilation=dilation))
            setattr(self, f"insnorm{k}", nn.InstanceNorm2d(16, affine=True))
            setattr(self, f"conv_s{rf}", nn.Conv2d(16, 1, kernel_size=1, stride=1, padding=0))
            setattr(self, f"insnorm_s{rf}", nn.InstanceNorm2d(1, affine=True))
        self.scale_list = torch.tensor(scale_list)
        for rf in RF_LEVELS:
            setattr(self, f"conv_o{rf}", nn.Conv2d(16, 2, kernel_size=1, stride=1, padding=0))
        self._native = None  # (key, NativeRFDetector)

    # ---- native path -------------------------------------------------------------------------------------------
    def _native_ok(self, photos) -> bool:
        return (not self.training and photos.is_cuda and photos.dtype == torch.float32 and photos.dim() == 4
                and photos.shape[1] == 1 and photos.shape[0] > 0 and photos.shape[2] * photos.shape[3] >= 2
                and self._conv_geometry == (3, 1, 1) and self.scale_list.numel() == len(RF_LEVELS)
                and self.conv1.weight.device == photos.device
                and all(p.dtype == torch.float32 for p in self.parameters())
                and len({getattr(self, n).eps for n in self._insnorm_names()}) == 1
                and not (torch.is_grad_enabled() and (photos.requires_grad
                                                      or any(p.requires_grad for p in self.parameters()))))

    @staticmethod
    def _insnorm_names():
        return [f"insnorm{k}" for k in range(1, 11)] + [f"insnorm_s{rf}" for rf in RF_LEVELS]

    def native_detector(self, device):
        """The NativeRFDetector of the current weights on ``device`` (rebuilt when a tensor of the state changes)."""
        from . import _native
        key = ((str(device), float(self.score_com_strength), float(self.scale_com_strength),
                tuple(self.scale_list.tolist()))
               + tuple((v.data_ptr(), v._version) for v in (*self.parameters(), *self.buffers())))
        if self._native is None or self._native[0] != key:
            self._native = (key, _native.NativeRFDetector(
                _native.state_dict_blob(self.state_dict()), self.scale_list.float().cpu().numpy(), device,
                in_eps=self.insnorm1.eps, score_com_strength=float(self.score_com_strength),
                scale_com_strength=float(self.scale_com_strength)))
        return self._native[1]

    def forward_maps(self, photos):
        """(score [B,H,W], scale [B,H,W], ori [B,H,W,2]) of the native forward."""
        return self.native_detector(photos.device).forward(photos.detach())

    def _apply(self, fn, *a, **k):
        self._native = None
        return super()._apply(fn, *a, **k)

    # ---- the reference's methods -------------------------------------------------------------------------------
    def forward(self, photos):
        if self._native_ok(photos):
            score, scale, ori = self.forward_maps(photos)
            return score.unsqueeze(-1), scale.unsqueeze(-1), ori.unsqueeze(-2)
        return self.forward_torch(photos)

    def forward_torch(self, photos):
        """The torch layers (rf_det_so.py:74-234), whatever the device: the CPU / fp64 / training path."""
        feat, scores, orints = photos, [], []
        for k, rf in enumerate(RF_LEVELS, start=1):
            h = F.leaky_relu(getattr(self, f"insnorm{k}")(getattr(self, f"conv{k}")(feat)))
            scores.append(getattr(self, f"insnorm_s{rf}")(getattr(self, f"conv_s{rf}")(h)).permute(0, 2, 3, 1))
            o = getattr(self, f"conv_o{rf}")(h)
            orints.append((o / torch.norm(o, p=2, dim=1, keepdim=True)).permute(0, 2, 3, 1).unsqueeze(-2))
            feat = h if k == 1 else h + feat  # the heads read h before the residual; feat_10 is never read
        score_maps = torch.cat(scores, -1)    # [B,H,W,10]
        orint_maps = torch.cat(orints, -2)    # [B,H,W,10,2]
        scale_probs = soft_nms_3d(score_maps, ksize=SOFT_NMS_KSIZE, com_strength=RF_SOFT_NMS_STRENGTH)
        return soft_max_and_argmax_1d(scale_probs, self.scale_list, self.score_com_strength, self.scale_com_strength,
                                      orint_maps=orint_maps)


def randomise_rfdet_(det, seed):
    """Seeded, non-degenerate weights for the tests and the benchmark -- the distributions of the fixture
    tests/golden/rfdet.npz -- on a module with RFDetSO's attribute names (the reference's or this
    package's): ``weights_init`` under ``torch.manual_seed(seed)``; then from a generator seeded ``seed + 1`` the
    InstanceNorm affine parameters weight 0.75 + 0.5 U, bias 0.2 N, and the conv_o* heads weight 0.3 N, bias
    +-(0.5 + U) (convO_init's zeros and ones would make every orientation the same constant).  The two signs are
    drawn once for the detector, not per level: the final orientation is close to the mean of the ten unit vectors
    (the softmax over levels is nearly flat), and with independent signs per level that mean cancels to a norm
    below the exclusion floor on ~3 % of the pixels.  Returns det.eval()."""
    torch.manual_seed(seed)
    det.apply(det.weights_init)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in det.modules():
            if isinstance(m, nn.InstanceNorm2d):
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
        sign = torch.where(torch.rand(2, generator=g) < 0.5, -1.0, 1.0)
        for rf in RF_LEVELS:
            conv = getattr(det, f"conv_o{rf}")
            conv.weight.copy_(0.3 * torch.randn(conv.weight.shape, generator=g))
            conv.bias.copy_(sign * (0.5 + torch.rand(2, generator=g)))
    return det.eval()


def detect(det, im_data):
    """Image -> keypoints (model/network.py:155-162, 181-182; rfnet/model/rf_net_so.py:160-168): ``(kpts [B K,4]
    int64 rows (b, y, x, 0) in raster order per image, kscale [B K], kori [B K,2], kscore [B K], im_scale
    [B,H,W,1])``, K = ``det.TOPK``.  On the native path this is ``hn_det_forward`` (``RFDet``: one constant scale)
    or ``hn_rfdet_forward`` (``RFDetSO``: its scale map, so ``kscale`` varies per keypoint) followed by
    ``hn_select_keypoints``, bit for bit.  An orientation map ``[B,H,W,1,2]`` is taken as ``[B,H,W,2]``."""
    if det._native_ok(im_data):
        from . import _native
        maps = det.forward_maps(im_data)
        if len(maps) == 3:  # a detector with a scale map
            score, scale, ori = maps
            out = _native.select_keypoints(score, *det._select_args(), scale_map=scale, ori_map=ori)
            return out["kpts"], out["kscale"], out["kori"], out["kscore"], scale.unsqueeze(-1)
        score, ori = maps
        scale_value = float(det.scale_list[0])
        out = _native.select_keypoints(score, *det._select_args(), scale_value=scale_value, ori_map=ori)
        im_scale = torch.full((), scale_value, device=score.device).expand(*score.shape, 1)
        return out["kpts"], out["kscale"], out["kori"], out["kscore"], im_scale
    im_rawsc, im_scale, im_orint = det(im_data)
    kpts, kscore, kscale, kori, _, _, _ = select_keypoints_torch(
        im_rawsc.squeeze(-1), *det._select_args(), scale_map=im_scale.squeeze(-1),
        ori_map=im_orint.reshape(*im_rawsc.shape[:3], 2))
    return kpts, kscale, kori, kscore, im_scale


def detect_and_describe(det, des, im_data, im_info, im_raw):
    """``Network.inference`` (model/network.py:148-183): ``(im_scale, kpts, im_des, scale, ori, score)`` --
    ``detect`` chained into ``describe_keypoints``."""
    from .patches import describe_keypoints
    kpts, kscale, kori, kscore, im_scale = detect(det, im_data)
    im_des = describe_keypoints(des, kpts, kscale, kori, im_info, im_raw)
    return im_scale, kpts, im_des, kscale, kori, kscore
