// C ABI (include/hardnet_mi355x.h) of the model-less operations: keypoint patch extraction and its backward
// (hn_clip.hip), pair distances, matching, the eval loss, FPR95 and uint8 preprocessing.  Each entry point checks
// its arguments on the host and makes one launch call.
#include <string>

#include "hardnet_mi355x.h"
#include "hn_api_util.h"
#include "hn_internal.h"

extern "C" int hn_clip_patch(const float* d_images, int64_t n_images, int32_t height, int32_t width,
                             const int64_t* d_kpts, const float* d_scale, const float* d_ori, const float* d_ratio,
                             int64_t n, float* d_patches, void* hip_stream) {
  if (const char* e = clip_arg_error(n_images, height, width, n)) return fail(HN_ERR_ARG, e);
  if (n == 0) return HN_OK;
  if (!d_images || !d_kpts || !d_scale || !d_ratio || !d_patches)
    return fail(HN_ERR_ARG, "NULL device pointer (only d_ori may be NULL)");
  if (hn_misaligned(16, d_patches)) return fail(HN_ERR_ARG, "d_patches must be 16-byte aligned");
  HIPCHK(hn_launch_clip(d_images, n_images, height, width, d_kpts, d_scale, d_ori, d_ratio, n, d_patches,
                        static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_clip_patch_backward(const float* d_dpatches, const float* d_images, int64_t n_images, int32_t height,
                                      int32_t width, const int64_t* d_kpts, const float* d_scale, const float* d_ori,
                                      const float* d_ratio, int64_t n, float* d_dscale, float* d_dori,
                                      void* hip_stream) {
  if (const char* e = clip_arg_error(n_images, height, width, n)) return fail(HN_ERR_ARG, e);
  if (d_dori && !d_ori) return fail(HN_ERR_ARG, "d_dori needs d_ori (no rotation has no orientation gradient)");
  if (n == 0) return HN_OK;
  if (!d_dpatches || !d_images || !d_kpts || !d_scale || !d_ratio)
    return fail(HN_ERR_ARG, "NULL device pointer (only d_ori, d_dscale and d_dori may be NULL)");
  if (hn_misaligned(16, d_dpatches)) return fail(HN_ERR_ARG, "d_dpatches must be 16-byte aligned");
  HIPCHK(hn_launch_clip_backward(d_dpatches, d_images, n_images, height, width, d_kpts, d_scale, d_ori, d_ratio, n,
                                 d_dscale, d_dori, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_pairdist_workspace_bytes(int64_t batch, size_t* bytes_out) {
  if (!bytes_out || batch < 0) return fail(HN_ERR_ARG, "bad argument");
  // column minima (padded to 64 entries) + the row kernel's workspace (hn_pairdist_rows_ws_bytes)
  const long b = batch > 0 ? (long)batch : 1;
  *bytes_out = (size_t)((b + 63) / 64 * 64) * sizeof(float) + hn_pairdist_rows_ws_bytes(b, b);
  return HN_OK;
}

extern "C" int hn_pairdist_hardneg(const float* d_anchor, const float* d_positive, int64_t batch,
                                   int32_t dim, int32_t anchor_swap, float* d_pos,
                                   float* d_min_neg, void* d_workspace, size_t workspace_bytes,
                                   void* hip_stream) {
  if (!d_anchor || !d_positive || !d_pos || !d_min_neg || !d_workspace)
    return fail(HN_ERR_ARG, "NULL device pointer");
  if (batch < 2 || batch > (1 << 30)) return fail(HN_ERR_ARG, "batch out of range");
  if (dim != 128) return fail(HN_ERR_ARG, "dim must be 128");
  size_t need = 0;
  hn_pairdist_workspace_bytes(batch, &need);
  if (workspace_bytes < need) return fail(HN_ERR_WORKSPACE, "workspace too small");
  HIPCHK(hn_launch_pairdist(d_anchor, d_positive, (int)batch, dim, anchor_swap, d_pos, d_min_neg,
                            d_workspace, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_pairdist_rows_workspace_bytes(int64_t n_rows, int64_t batch, size_t* bytes_out) {
  if (!bytes_out || n_rows < 1 || batch < 2 || batch > (1 << 30) || n_rows > batch)
    return fail(HN_ERR_ARG, "bad n_rows / batch");
  *bytes_out = hn_pairdist_rows_ws_bytes((long)n_rows, (long)batch);
  return HN_OK;
}

extern "C" int hn_pairdist_rows(const float* d_anchor_rows, int64_t n_rows, int64_t row0,
                                const float* d_positive, int64_t batch, int32_t dim, float* d_pos,
                                float* d_row_min, float* d_col_min, void* d_workspace,
                                size_t workspace_bytes, void* hip_stream) {
  if (!d_anchor_rows || !d_positive || !d_pos || !d_row_min || !d_workspace)
    return fail(HN_ERR_ARG, "NULL device pointer");
  if (dim != 128) return fail(HN_ERR_ARG, "dim must be 128");
  size_t need = 0;
  int rc = hn_pairdist_rows_workspace_bytes(n_rows, batch, &need);
  if (rc) return rc;
  if (row0 < 0 || row0 + n_rows > batch) return fail(HN_ERR_ARG, "rows [row0, row0 + n_rows) outside the batch");
  if (workspace_bytes < need) return fail(HN_ERR_WORKSPACE, "workspace too small");
  if (hn_misaligned(16, d_anchor_rows, d_positive))
    return fail(HN_ERR_ARG, "descriptor pointers must be 16-byte aligned");
  HIPCHK(hn_launch_pairdist_rows(d_anchor_rows, (int)n_rows, (int)row0, d_positive, (int)batch, d_pos,
                                 d_row_min, d_col_min, d_workspace, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

static const char* match_size_error(int64_t n_query, int64_t n_db) {
  if (n_query < 1 || n_query > (1 << 22)) return "n_query must be 1 .. 2^22";
  if (n_db < 1 || n_db > (1 << 22)) return "n_db must be 1 .. 2^22";
  return nullptr;
}

extern "C" int hn_match_workspace_bytes(int64_t n_query, int64_t n_db, size_t* bytes_out) {
  if (!bytes_out) return fail(HN_ERR_ARG, "bytes_out is NULL");
  if (const char* e = match_size_error(n_query, n_db)) return fail(HN_ERR_ARG, e);
  *bytes_out = hn_match_ws_bytes((long)n_query, (long)n_db);
  return HN_OK;
}

extern "C" int hn_match_nn2(const float* d_query, int64_t n_query, const float* d_db, int64_t n_db, int32_t dim,
                            int32_t metric, float* d_dist, int32_t* d_idx, void* d_workspace,
                            size_t workspace_bytes, void* hip_stream) {
  if (dim != 128) return fail(HN_ERR_ARG, "dim must be 128, got " + std::to_string(dim));
  if (metric != HN_METRIC_UNIT && metric != HN_METRIC_L2)
    return fail(HN_ERR_ARG, "unknown metric " + std::to_string(metric) + " (HN_METRIC_UNIT, HN_METRIC_L2)");
  if (const char* e = match_size_error(n_query, n_db)) return fail(HN_ERR_ARG, e);
  if (int rc = hn_need_ws(workspace_bytes, hn_match_ws_bytes((long)n_query, (long)n_db))) return rc;
  if (!d_query || !d_db || !d_dist || !d_idx || !d_workspace) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(16, d_query, d_db, d_workspace))
    return fail(HN_ERR_ARG, "d_query / d_db / d_workspace must be 16-byte aligned");
  if (hn_misaligned(8, d_dist, d_idx)) return fail(HN_ERR_ARG, "d_dist / d_idx must be 8-byte aligned");
  HIPCHK(hn_launch_match_nn2(d_query, (int)n_query, d_db, (int)n_db, metric, d_dist, d_idx, d_workspace,
                             static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_hardnet_loss(const float* d_pos, const float* d_row_min, const float* d_col_min,
                               int64_t n, float margin, int32_t loss_type, float scale,
                               float* d_min_neg, float* d_loss, void* hip_stream) {
  if (!d_pos || !d_row_min || !d_loss) return fail(HN_ERR_ARG, "NULL device pointer");
  if (n < 1 || n > (1 << 30)) return fail(HN_ERR_ARG, "n out of range");
  if (loss_type < HN_LOSS_TRIPLET_MARGIN || loss_type > HN_LOSS_CONTRASTIVE)
    return fail(HN_ERR_ARG, "unknown loss_type " + std::to_string(loss_type) +
                                " (Losses.py:142-152: triplet_margin, softmax, contrastive)");
  HIPCHK(hn_launch_loss(d_pos, d_row_min, d_col_min, (int)n, margin, loss_type, scale, d_min_neg, d_loss,
                        static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_fpr95_workspace_bytes(int64_t n, size_t* bytes_out) {
  if (!bytes_out || n < 1 || n > (int64_t)1 << 30) return fail(HN_ERR_ARG, "n out of range");
  HIPCHK(hn_fpr95_ws_bytes(n, bytes_out));
  return HN_OK;
}

extern "C" int hn_fpr95(const float* d_anchor, const float* d_positive, const int32_t* d_labels,
                        int64_t n, int32_t dim, float* d_dists, double* d_fpr, void* d_workspace,
                        size_t workspace_bytes, void* hip_stream) {
  if (!d_anchor || !d_positive || !d_labels || !d_fpr || !d_workspace)
    return fail(HN_ERR_ARG, "NULL device pointer");
  if (n < 1 || n > (int64_t)1 << 30 || dim < 1) return fail(HN_ERR_ARG, "bad n / dim");
  size_t need = 0;
  HIPCHK(hn_fpr95_ws_bytes(n, &need));
  if (workspace_bytes < need) return fail(HN_ERR_WORKSPACE, "workspace too small");
  HIPCHK(hn_launch_fpr95(d_anchor, d_positive, d_labels, n, dim, d_dists, d_fpr, d_workspace,
                         workspace_bytes, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_preprocess(const uint8_t* d_in, int64_t n, int32_t in_hw, int32_t resize,
                             int32_t normalize, float mean, float stdv, float* d_out,
                             void* hip_stream) {
  if (n < 0) return fail(HN_ERR_ARG, "n < 0");
  if (int rc = hn_resize_args(resize, in_hw)) return rc;
  if (n == 0) return HN_OK;
  if (!d_in || !d_out) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(16, d_in, d_out)) return fail(HN_ERR_ARG, "d_in / d_out must be 16-byte aligned");
  if (normalize && !(stdv != 0.0f)) return fail(HN_ERR_ARG, "std must be nonzero");
  HIPCHK(hn_launch_preprocess(d_in, n, resize, normalize, mean, stdv, d_out,
                              static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}
