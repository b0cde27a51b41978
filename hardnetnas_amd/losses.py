"""Differentiable ``loss_HardNet`` for training loops (hardnet/Losses.py:87-154, batch_reduce 'min',
'average' and 'random'), with ``distance_matrix_vector`` (Losses.py:5-13) in the reference's formulation.

The training loop calls it as HardNet.py:408-413.  On HIP fp32 [B,128] descriptors every reduction runs on
HIP kernels, forward and backward, without the B x B matrix: 'min' and 'random' on hn_loss.hip, 'average'
(B <= 65,536) on the f32-input MFMA kernels of hn_loss_dense.hip.  The autograd formulation below (the B x B
matrix materialised, as in the reference) serves CPU / fp64 tensors, other widths and ``fused=False``.  The
other losses HardNet.py:399-419 can call -- ``loss_random_sampling`` with ``distance_vectors_pairwise``,
``global_orthogonal_regularization``, ``CorrelationPenaltyLoss`` -- are torch formulations (O(B * 128) row
work with nothing to fuse away).  ``loss_L2Net`` is left out: Losses.py:70 subtracts an int from a bool
tensor, which current torch refuses, so the reference cannot pin it.  For inference-time mining at
large B (65,536 pairs) ``hardnetnas_amd._native.pairdist_rows`` / ``hardnet_loss`` and
``hardnetnas_amd.distributed.sharded_hardnet_loss`` run the bf16x3 MFMA pair kernel (forward only).

``loss_neimask`` is FDLNet's descriptor training loss (FDLNet-master/latency/NASNet/model/des.py:57-96): another
distance (``matching.distance_matrix_vector``), two keypoint-neighbourhood masks in place of the < 0.008 rule,
anchor swap always on; on HIP fp32 [N,128] descriptors it runs the fused kernels of hn_neimask.hip.
``pair_distance_loss`` is the mean positive distance ``Network.criterion`` reports beside it (network.py:300-301).
"""
from __future__ import annotations

import torch

__all__ = ["distance_matrix_vector", "loss_HardNet", "SupernetLoss", "loss_neimask", "pair_distance_loss",
           "distance_vectors_pairwise", "loss_random_sampling", "global_orthogonal_regularization",
           "CorrelationPenaltyLoss"]


def distance_matrix_vector(anchor: torch.Tensor, positive: torch.Tensor) -> torch.Tensor:
    """sqrt(|a_i|^2 + |p_j|^2 - 2 a_i . p_j + 1e-6) (Losses.py:5-13)."""
    a2 = (anchor * anchor).sum(dim=1, keepdim=True)
    p2 = (positive * positive).sum(dim=1, keepdim=True)
    return torch.sqrt(a2 + p2.t() - 2.0 * anchor @ positive.t() + 1e-6)


def loss_HardNet(anchor: torch.Tensor, positive: torch.Tensor, anchor_swap: bool = False,
                 anchor_ave: bool = False, margin: float = 1.0, batch_reduce: str = "min",
                 loss_type: str = "triplet_margin", fused: bool = True) -> torch.Tensor:
    """Hardest-in-batch margin loss (Losses.py:87-154); anchor_ave is accepted and unused, as there.

    'average' (:124-130) takes every masked entry as a negative, paired -- as in the reference -- with the
    positive distance of its column; 'random' (:131-138) one negative per row at torch.randperm(B), drawn once
    from the CPU generator as the reference draws it, on either path: a seeded run selects the same negatives
    fused or not.

    Dispatch, with no knob but ``fused``: [B,128] fp32 tensors on one HIP device run the HIP kernels, forward
    and backward without the B x B matrix -- 'min' (the training default, HardNet.py:74) through
    ``_native.HardNetLossFunction``, 'average' (B <= 65,536) and 'random' through
    ``_native.HardNetLossReduceFunction``.  ``fused=False``, CPU / fp64 tensors, other widths and 'average'
    beyond 65,536 rows run the reference's autograd formulation here."""
    if anchor.size() != positive.size() or anchor.dim() != 2:
        raise ValueError("anchor and positive must be 2-D tensors of the same shape")
    if batch_reduce not in ("min", "average", "random"):
        raise ValueError(f"unknown batch_reduce {batch_reduce!r} (min, average or random)")
    if loss_type not in ("triplet_margin", "softmax", "contrastive"):
        raise ValueError(f"unknown loss_type {loss_type!r}")
    native = (fused and anchor.is_cuda and positive.is_cuda and anchor.dtype == torch.float32
              and positive.dtype == torch.float32 and anchor.shape[1] == 128)
    if native and batch_reduce == "min":
        from . import _native
        return _native.HardNetLossFunction.apply(anchor, positive, anchor_swap, margin, loss_type)
    if native and anchor.device == positive.device and anchor.shape[0] >= 1:
        from . import _native
        if batch_reduce == "random":
            idxs = torch.randperm(anchor.size(0)).long()
            return _native.HardNetLossReduceFunction.apply(anchor, positive, idxs, "random", anchor_swap, margin,
                                                           loss_type)
        if anchor.shape[0] <= _native.AVERAGE_MAX_BATCH:
            return _native.HardNetLossReduceFunction.apply(anchor, positive, None, "average", anchor_swap, margin,
                                                           loss_type)
    eps = 1e-8
    d = distance_matrix_vector(anchor, positive) + eps
    b = d.size(1)
    eye = torch.eye(b, device=d.device, dtype=d.dtype)
    pos1 = torch.diagonal(d)
    dn = d + 10.0 * eye
    dn = dn + 10.0 * (dn < 0.008).to(dn.dtype)  # near-duplicate "negatives" pushed out
    if batch_reduce == "min":
        pos = pos1
        min_neg = dn.min(dim=1)[0]
        if anchor_swap:
            min_neg = torch.minimum(min_neg, dn.min(dim=0)[0])
    elif batch_reduce == "average":
        pos = pos1.repeat(anchor.size(0))          # entry k pairs with pos1[k % B]
        min_neg = dn.reshape(-1)                   # entry k = dn[k // B][k % B]
        if anchor_swap:
            min_neg = torch.minimum(min_neg, dn.t().contiguous().reshape(-1))
    else:
        idxs = torch.randperm(anchor.size(0)).long().to(d.device)
        min_neg = dn.gather(1, idxs.view(-1, 1)).reshape(-1)
        if anchor_swap:
            min_neg = torch.minimum(min_neg, dn.t().gather(1, idxs.view(-1, 1)).reshape(-1))
        pos = pos1
    if loss_type == "triplet_margin":
        loss = torch.clamp(margin + pos - min_neg, min=0.0)
    elif loss_type == "softmax":
        e_pos = torch.exp(2.0 - pos)
        loss = -torch.log(e_pos / (e_pos + torch.exp(2.0 - min_neg) + eps))
    else:
        loss = torch.clamp(margin - min_neg, min=0.0) + pos
    return loss.mean()


def distance_vectors_pairwise(anchor, positive, negative=None):
    """Row-wise distances sqrt(|x_i|^2 + |y_i|^2 - 2 x_i.y_i + 1e-8) (Losses.py:15-28): d(a, p), and with a
    negative also d(a, n) and d(p, n)."""
    a_sq = torch.sum(anchor * anchor, dim=1)
    p_sq = torch.sum(positive * positive, dim=1)
    eps = 1e-8
    d_a_p = torch.sqrt(a_sq + p_sq - 2 * torch.sum(anchor * positive, dim=1) + eps)
    if negative is not None:
        n_sq = torch.sum(negative * negative, dim=1)
        d_a_n = torch.sqrt(a_sq + n_sq - 2 * torch.sum(anchor * negative, dim=1) + eps)
        d_p_n = torch.sqrt(p_sq + n_sq - 2 * torch.sum(positive * negative, dim=1) + eps)
        return d_a_p, d_a_n, d_p_n
    return d_a_p


def loss_random_sampling(anchor, positive, negative, anchor_swap=False, margin=1.0, loss_type="triplet_margin"):
    """The triplet loss over given negatives (Losses.py:29-55; batch_reduce 'random_global', HardNet.py:402-406):
    no mining in the batch."""
    if anchor.size() != positive.size() or anchor.size() != negative.size() or anchor.dim() != 2:
        raise ValueError("anchor, positive and negative must be 2-D tensors of the same shape")
    eps = 1e-8
    pos, d_a_n, d_p_n = distance_vectors_pairwise(anchor, positive, negative)
    min_neg = torch.min(d_a_n, d_p_n) if anchor_swap else d_a_n
    if loss_type == "triplet_margin":
        loss = torch.clamp(margin + pos - min_neg, min=0.0)
    elif loss_type == "softmax":
        exp_pos = torch.exp(2.0 - pos)
        loss = -torch.log(exp_pos / (exp_pos + torch.exp(2.0 - min_neg) + eps))
    elif loss_type == "contrastive":
        loss = torch.clamp(margin - min_neg, min=0.0) + pos
    else:
        raise ValueError(f"unknown loss_type {loss_type!r} (triplet_margin, softmax or contrastive)")
    return torch.mean(loss)


def global_orthogonal_regularization(anchor, negative):
    """mean(a_i.n_i)^2 + max(mean((a_i.n_i)^2) - 1/dim, 0) (Losses.py:156-162; --gor, HardNet.py:418-419)."""
    neg_dis = torch.sum(torch.mul(anchor, negative), 1)
    dim = anchor.size(1)
    return torch.pow(torch.mean(neg_dis), 2) + torch.clamp(torch.mean(torch.pow(neg_dis, 2)) - 1.0 / dim, min=0.0)


class CorrelationPenaltyLoss(torch.nn.Module):
    """The Frobenius norm of the off-diagonal of the descriptors' scatter matrix over the batch size
    (HardNet.py:42-53; --decor, HardNet.py:415-416)."""

    def forward(self, input):
        zeroed = input - torch.mean(input, dim=0).expand_as(input)
        cor_mat = torch.t(zeroed) @ zeroed
        no_diag = cor_mat - torch.diag(torch.diag(cor_mat))
        return torch.sqrt((no_diag * no_diag).sum()) / input.size(0)


class SupernetLoss(torch.nn.Module):
    """The supernet search loss (hardnetNAS/supernet_functions/model_supernet.py:88-110):
    alpha * (loss_HardNet(outs, targets) + clamp(log(latency^beta) * (log(((sample_latency - target)
    / target)^2) + 5) * 0.2, 0)), with the hardnetNAS loss_HardNet (general_functions/Losses.py:27-51:
    anchor swap always on, margin 1).  alpha 0.2, beta 0.6 (config_for_supernet.py)."""

    def __init__(self, alpha: float = 0.2, beta: float = 0.6):
        super().__init__()
        self.alpha, self.beta = alpha, beta

    def forward(self, outs, targets, latency, sample_latency, target):
        ce = loss_HardNet(outs, targets, anchor_swap=True)
        lat = torch.clamp(torch.log(latency ** self.beta) * (torch.log(((sample_latency - target) / target) ** 2) + 5)
                          * 0.2, 0)
        loss = self.alpha * (ce + lat)
        return loss, ce, lat


def _keypoint_distances(kp: torch.Tensor) -> torch.Tensor:
    """pairwise_distances(x, x) (utils/math_utils.py:22-40) on the (y, x) columns of [N,4] keypoint rows cast to
    fp32, as des.py:76-84 calls it: sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 1e-8))."""
    x = kp[:, 1:3].to(torch.float)
    n = (x ** 2).sum(1)
    return torch.sqrt((n.view(-1, 1) + n.view(1, -1) - 2.0 * torch.mm(x, x.t())).clamp(min=1e-8))


def neimask_masked_distances(anchor, positive, anchor_kp, positive_kp, C: float):
    """(D, dn) of des.py:68-87: the [N,N] descriptor distances and the same with 10 added on the diagonal and
    wherever the anchor keypoints, and again wherever the positive keypoints, lie closer than C."""
    from .matching import distance_matrix_vector as unit_distances
    d = unit_distances(anchor, positive)
    dn = d + torch.eye(d.size(1), device=d.device) * 10  # (an fp32 eye, as the reference builds it)
    dn = dn + _keypoint_distances(anchor_kp).lt(C).to(torch.float) * 10
    dn = dn + _keypoint_distances(positive_kp).lt(C).to(torch.float) * 10
    return d, dn


def loss_neimask(anchor: torch.Tensor, positive: torch.Tensor, anchor_kp: torch.Tensor, positive_kp: torch.Tensor,
                 margin: float = 1.0, C: float = 5.0, fused: bool = True) -> torch.Tensor:
    """FDLNet's neighbour-mask hardest-in-batch margin loss (``HardNetNeiMask.loss``, des.py:57-96):
    mean_i max(margin + D_ii - min(min_j dn_ij, min_k dn_ki), 0).  The keypoints are [N,4] rows (b, y, x, 0); the
    image index is not used, as in the reference; C = 0 gives the plain hardest-in-batch loss.

    fp32 [N,128] descriptors with int64 [N,4] keypoints on one HIP device run the fused kernels
    (``_native.NeiMaskLossFunction``: forward and backward, no N x N matrix, ties to the lowest index); CPU / fp64
    tensors, other widths or dtypes and ``fused=False`` run the reference's formulation here."""
    if anchor.size() != positive.size() or anchor.dim() != 2:
        raise ValueError("anchor and positive must be 2-D tensors of the same shape")
    for kp in (anchor_kp, positive_kp):
        if kp.dim() != 2 or kp.size(0) != anchor.size(0) or kp.size(1) < 3:
            raise ValueError("anchor_kp and positive_kp must be [N,4] keypoint rows (b, y, x, 0), one per descriptor")
    if (fused and anchor.is_cuda and anchor.shape[1] == 128 and anchor.shape[0] >= 1
            and anchor.dtype == torch.float32 and positive.dtype == torch.float32
            and all(kp.dtype == torch.int64 and kp.shape[1] == 4 for kp in (anchor_kp, positive_kp))
            and all(t.device == anchor.device for t in (positive, anchor_kp, positive_kp))):
        from . import _native
        return _native.NeiMaskLossFunction.apply(anchor, positive, anchor_kp, positive_kp, margin, C)
    d, dn = neimask_masked_distances(anchor, positive, anchor_kp, positive_kp, C)
    pos = d.diag()
    min_neg = torch.min(dn.min(dim=1)[0], dn.min(dim=0)[0])
    return torch.clamp(margin + pos - min_neg, min=0.0).mean()


def pair_distance_loss(anchor: torch.Tensor, positive: torch.Tensor) -> torch.Tensor:
    """``distance_matrix_vector(a, p).diag().mean()`` (network.py:300-301) row by row, without the matrix."""
    if anchor.size() != positive.size() or anchor.dim() != 2:
        raise ValueError("anchor and positive must be 2-D tensors of the same shape")
    return (2 - 2 * (anchor * positive).sum(1)).clamp(min=1e-8, max=4.0).sqrt().mean()
