/* loss_HardNet's 'average' and 'random' batch reductions on the MI355X: an extension of the C ABI of
 * hardnet_mi355x.h (which includes this file; include either).  Same conventions: device pointers, int status
 * (HN_OK or an HN_ERR_* code, the message through hn_last_error), every argument check before any launch. */
#ifndef HARDNET_MI355X_LOSS_REDUCE_H
#define HARDNET_MI355X_LOSS_REDUCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Train-mode loss_HardNet's other two reductions (hardnet/Losses.py:124-138) and their backwards, without a
 * B x B matrix (an addition to the ABI of hardnet_mi355x.h: HN_ABI_VERSION stays 2).  With
 * d_ij = sqrt((|a_i|^2 + |p_j|^2) - 2 a_i.p_j + 1e-6) + 1e-8, dn_ij = d_ij + 10 [i = j], dn_ij += 10 if dn_ij < 0.008
 * and pos_i = d_ii; loss types and error codes as in hardnet_mi355x.h:
 *   HN_REDUCE_AVERAGE: loss = (1 / B^2) sum_ij f(pos_j, m_ij), m_ij = dn_ij or, with anchor_swap,
 *             min(dn_ij, dn_ji): every masked entry, the diagonal (d_ii + 10) included, is a negative, paired -- as
 *             the reference's pos1.repeat(B) pairs it -- with the positive distance of its COLUMN.  The products
 *             run on the f32-input MFMA (exact fp32); per-entry terms are fp32, their sum fp64 in a fixed order.
 *             1 <= batch <= 65,536 (B^2 work beyond that would occupy the GPU for seconds per call).
 *   HN_REDUCE_RANDOM: loss = mean_i f(pos_i, mn_i), mn_i = dn[i][t_i] or, with anchor_swap,
 *             min(dn[i][t_i], dn[t_i][i]), t = d_idx ([batch] int64 on the device; the reference draws
 *             torch.randperm(B)).  The list need not be a permutation; every value is clamped to [0, batch - 1]
 *             as it is loaded, so no value of it can address memory outside the inputs.  1 <= batch <= 2^22.
 *   HN_REDUCE_MIN is rejected here: it runs on hn_hardnet_loss_train_forward / hn_hardnet_loss_backward.
 *   backward: d_dloss (one float on the device) -> d_grad_anchor, d_grad_positive [batch,128] (overwritten), as
 *             autograd differentiates the reference formulation: torch.minimum's halves on an exact dn_ij = dn_ji
 *             tie, nothing through the + 10 constants or an active clamp.  No float atomics; results are
 *             bit-identical call to call.
 * d_idx is required for HN_REDUCE_RANDOM (forward and backward) and ignored for HN_REDUCE_AVERAGE; dim must be 128.
 * d_saved (hn_hardnet_loss_reduce_workspace_bytes: O(batch) bytes) is written by the forward and read by the
 * backward with the same anchors, positives and arguments. */
enum hn_batch_reduce { HN_REDUCE_MIN = 0, HN_REDUCE_AVERAGE = 1, HN_REDUCE_RANDOM = 2 };
int hn_hardnet_loss_reduce_workspace_bytes(int32_t batch_reduce, int64_t batch, size_t* bytes_out);
int hn_hardnet_loss_reduce_forward(const float* d_anchor, const float* d_positive, const int64_t* d_idx,
                                   int64_t batch, int32_t dim, int32_t batch_reduce, int32_t anchor_swap,
                                   float margin, int32_t loss_type, float* d_loss, void* d_saved, size_t saved_bytes,
                                   void* hip_stream);
int hn_hardnet_loss_reduce_backward(const float* d_anchor, const float* d_positive, const int64_t* d_idx,
                                    int64_t batch, int32_t dim, int32_t batch_reduce, int32_t anchor_swap,
                                    float margin, int32_t loss_type, const float* d_dloss, float* d_grad_anchor,
                                    float* d_grad_positive, void* d_saved, size_t saved_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* HARDNET_MI355X_LOSS_REDUCE_H */
