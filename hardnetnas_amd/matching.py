"""Descriptor matching scores of FDLNet's evaluation on the fused GPU matcher.

Drop-in replacements, with the reference's signatures and return values, for the match-score functions
of FDLNet-master/latency/NASNet/utils/eval_utils.py:

    nearest_neighbor_match_score                  :112-126
    nearest_neighbor_threshold_match_score        :129-148
    nearest_neighbor_distance_ratio_match         :168-175
    nearest_neighbor_distance_ratio_match_score   :178-197
    eval_model                                    :85-109

and ``distance_matrix_vector`` of utils/math_utils.py:8-19.  The reference builds the N x M distance
matrix and takes its row ``min`` or ``sort``; here fp32 [., 128] descriptors on a HIP device go through
``_native.match_nn2`` once (nearest and second-nearest row, both distances and indices, no matrix), and
only the O(N) coordinate arithmetic that follows runs in torch, on the same device.  Everything else
(CPU tensors, fp64, other descriptor widths) runs the torch formulation below.

Where several database rows lie inside the distance's clamp (2 - 2 a.b < 1e-8) the reference sees equal
distances and returns whichever index torch picks; the GPU matcher orders them by the unclamped value
(include/hardnet_mi355x.h).
"""
from __future__ import annotations

import torch

DESC_DIM = 128


def distance_matrix_vector(anchor: torch.Tensor, positive: torch.Tensor) -> torch.Tensor:
    """[N,M] distances between unit descriptors: sqrt(clamp(2 - 2 a.b, 1e-8, 4)) (math_utils.py:8-19)."""
    x = 2 - 2 * torch.mm(anchor, positive.t())
    return torch.sqrt(x.clamp(min=1e-8, max=4.0))


def _native_ok(des1: torch.Tensor, des2: torch.Tensor) -> bool:
    return (des1.is_cuda and des2.is_cuda and des1.device == des2.device
            and des1.dtype == torch.float32 and des2.dtype == torch.float32
            and des1.dim() == 2 and des2.dim() == 2 and des1.shape[1] == DESC_DIM and des2.shape[1] == DESC_DIM
            and des1.shape[0] >= 1 and des2.shape[0] >= 1)


def _nearest(des1, des2):
    """(nn_value [N], nn_idx [N] int64): the row minimum of the distance matrix and its argmin."""
    if _native_ok(des1, des2):
        from ._native import match_nn2
        dist, idx = match_nn2(des1, des2, "unit")
        return dist[:, 0], idx[:, 0].long()
    return distance_matrix_vector(des1, des2).min(dim=-1)


def _nearest2(des1, des2):
    """(Da [N], Db [N], Ia [N] int64): the two smallest distances of every row and the nearest's index."""
    if _native_ok(des1, des2):
        from ._native import match_nn2
        dist, idx = match_nn2(des1, des2, "unit")
        return dist[:, 0], dist[:, 1], idx[:, 0].long()
    ordered, indices = distance_matrix_vector(des1, des2).sort(dim=-1)
    return ordered[:, 0], ordered[:, 1], indices[:, 0]


def _within_reach(kp1w, nn_kp2, COO_THRSH):
    """Row i: the (y, x) of warped keypoint i and of its matched keypoint are at most COO_THRSH apart.  The
    reference takes the diagonal of pairwise_distances (math_utils.py:22-40) between the two lists; this
    is that diagonal alone: sqrt(max(|p|^2 + |q|^2 - 2 p.q, 1e-8))."""
    p, q = kp1w[:, 1:3].float(), nn_kp2[:, 1:3].float()
    d2 = (p * p).sum(1) + (q * q).sum(1) - 2.0 * (p * q).sum(1)
    return torch.sqrt(d2.clamp(min=1e-8)).le(COO_THRSH)


def _count(label) -> int:
    return int(label.sum().item())


def nearest_neighbor_match_score(des1, des2, kp1w, kp2, visible, COO_THRSH):
    """(correct, predicted): visible keypoints whose nearest descriptor's keypoint lies within COO_THRSH of
    their warped position, out of the visible ones (at least 1).  eval_utils.py:112-126."""
    visible = visible.bool()
    _, nn_idx = _nearest(des1, des2)
    correct = _within_reach(kp1w, kp2.index_select(0, nn_idx), COO_THRSH) & visible
    return _count(correct), max(_count(visible), 1)


def nearest_neighbor_threshold_match_score(des1, des2, kp1w, kp2, visible, DES_THRSH, COO_THRSH):
    """(correct, predicted) where a match is predicted only if the nearest distance is below DES_THRSH.
    eval_utils.py:129-148."""
    visible = visible.bool()
    nn_value, nn_idx = _nearest(des1, des2)
    predicted = nn_value.lt(DES_THRSH) & visible
    correct = predicted & _within_reach(kp1w, kp2.index_select(0, nn_idx), COO_THRSH) & visible
    return _count(correct), max(_count(predicted), 1)


def nearest_neighbor_distance_ratio_match(des1, des2, kp2, threshold):
    """(predict_label [N] bool, nn_kp2 [N,4]): nearest / second-nearest distance below ``threshold``, and
    the nearest descriptor's keypoint row.  eval_utils.py:168-175."""
    da, db, ia = _nearest2(des1, des2)
    return (da / db).lt(threshold), kp2.index_select(0, ia.view(-1))


def nearest_neighbor_distance_ratio_match_score(des1, des2, kp1w, kp2, visible, COO_THRSH, threshold=0.7):
    """(correct, predicted) under the distance-ratio test.  eval_utils.py:178-197."""
    visible = visible.bool()
    predicted, nn_kp2 = nearest_neighbor_distance_ratio_match(des1, des2, kp2, threshold)
    predicted = predicted & visible
    correct = predicted & _within_reach(kp1w, nn_kp2, COO_THRSH) & visible
    return _count(correct), max(_count(predicted), 1)


def eval_model(model, parsed_batch, DES_THRSH, COO_THRSH):
    """``(TPNN, PNN, TPNNT, PNNT, TPNNDR, PNNDR)`` of one image pair (eval_utils.py:85-109; batch size 1, as there):
    ``model.inference`` on both images, image 1's keypoints projected into image 2 unclamped
    (``network.ptCltoCr(clamp=False)``), then the three match scores above.  With a ``network.Network`` on HIP
    tensors every step before the counts runs on the library's kernels."""
    from .network import ptCltoCr
    im1_data, im1_info, homo12, im2_data, im2_info, homo21, im1_raw, im2_raw = parsed_batch
    scale1, kp1, des1, _, _, _ = model.inference(im1_data, im1_info, im1_raw)
    scale2, kp2, des2, _, _, _ = model.inference(im2_data, im2_info, im2_raw)
    kp1w = ptCltoCr(kp1, homo12, scale2, right_imorint=None, clamp=False)[0]
    _, _, maxh, maxw = im2_data.size()
    visible = kp1w[:, 2].lt(maxw) * kp1w[:, 1].lt(maxh)
    TPNN, PNN = nearest_neighbor_match_score(des1, des2, kp1w, kp2, visible, COO_THRSH)
    TPNNT, PNNT = nearest_neighbor_threshold_match_score(des1, des2, kp1w, kp2, visible, DES_THRSH, COO_THRSH)
    TPNNDR, PNNDR = nearest_neighbor_distance_ratio_match_score(des1, des2, kp1w, kp2, visible, COO_THRSH)
    return TPNN, PNN, TPNNT, PNNT, TPNNDR, PNNDR
