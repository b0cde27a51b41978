// C ABI (include/hardnet_mi355x.h) of the train steps: the stock HardNet (hn_train.hip), hardnetNAS and FDLNet's
// descriptor (hn_nas_train.hip), and the two train losses with their backwards (hn_loss.hip, hn_neimask.hip).
// Each entry point checks its arguments on the host and makes one call into the kernel file.
#include <string>

#include "hardnet_mi355x.h"
#include "hn_api_util.h"
#include "hn_internal.h"

// ---------------------------------------------------------------------------------------
// train-mode stock HardNet (hn_train.hip)
// ---------------------------------------------------------------------------------------
extern "C" int hn_hardnet_train_workspace_bytes(int64_t batch, size_t* saved_bytes_out, size_t* scratch_bytes_out) {
  if (!saved_bytes_out || !scratch_bytes_out || batch < 2 || batch > (1 << 24))
    return fail(HN_ERR_ARG, "batch must be 2 .. 2^24 (and both size pointers given)");
  const HnTrainWs L = hn_train_layout((long)batch);
  *saved_bytes_out = L.saved_total;
  *scratch_bytes_out = L.scratch_total;
  return HN_OK;
}

static int train_args(int64_t batch, const void* const* ptrs, int n, void* saved, size_t saved_bytes, void* scratch,
                      size_t scratch_bytes) {
  size_t need_sv = 0, need_sc = 0;
  int rc = hn_hardnet_train_workspace_bytes(batch, &need_sv, &need_sc);
  if (rc) return rc;
  if (!saved || !scratch) return fail(HN_ERR_ARG, "NULL workspace");
  return hn_train_buffers(saved_bytes, need_sv, scratch_bytes, need_sc, ptrs, n, "weight");
}

extern "C" int hn_hardnet_train_forward(const float* d_in, int64_t batch, const float* const* d_weights,
                                        float* const* d_running_mean, float* const* d_running_var, float momentum,
                                        float dropout_p, uint64_t seed, float* d_out, void* d_saved,
                                        size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                                        void* hip_stream) {
  int rc = train_args(batch, reinterpret_cast<const void* const*>(d_weights), 7, d_saved, saved_bytes, d_scratch,
                      scratch_bytes);
  if (rc) return rc;
  if (!d_in || !d_out) return fail(HN_ERR_ARG, "NULL device pointer");
  if (int rc = hn_pair_given(d_running_mean, d_running_var, "running_mean and running_var")) return rc;
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HN_ERR_ARG, "dropout_p must be in [0, 1)");
  HIPCHK(hn_train_forward(d_in, (long)batch, d_weights, d_running_mean, d_running_var, momentum, 1e-5f, 1e-7f,
                          1e-10f, dropout_p, (unsigned long long)seed, d_out, static_cast<char*>(d_saved),
                          static_cast<char*>(d_scratch), static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_hardnet_train_backward(const float* d_dout, int64_t batch, const float* const* d_weights,
                                         float* const* d_dweights, float* d_din, float dropout_p, uint64_t seed,
                                         void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                                         void* hip_stream) {
  int rc = train_args(batch, reinterpret_cast<const void* const*>(d_weights), 7, d_saved, saved_bytes, d_scratch,
                      scratch_bytes);
  if (rc) return rc;
  if (!d_dout) return fail(HN_ERR_ARG, "NULL device pointer");
  if ((rc = hn_ptr_table(d_dweights, 7, "gradient"))) return rc;
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HN_ERR_ARG, "dropout_p must be in [0, 1)");
  HIPCHK(hn_train_backward(d_dout, (long)batch, d_weights, d_dweights, d_din, 1e-10f, dropout_p,
                           (unsigned long long)seed, static_cast<char*>(d_saved), static_cast<char*>(d_scratch),
                           static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// one layer operation of the step alone (a test and diagnostic entry: the header's table gives each operation's
// buffers)
static int layer_op_config(int32_t bits, int32_t row_segments, int64_t batch) {
  if (batch < 2 || batch > (1 << 24)) return fail(HN_ERR_ARG, "batch must be 2 .. 2^24");
  if (bits < -1 || bits > 255) return fail(HN_ERR_ARG, "train_f32_bits must be -1 (the process's) or 0 .. 255");
  if (row_segments != 0 && row_segments != 1 && row_segments != 2 && row_segments != 4)
    return fail(HN_ERR_ARG, "row_segments must be 0, 1, 2 or 4");
  return HN_OK;
}

extern "C" int hn_hardnet_train_layer_op_workspace_bytes(int32_t train_f32_bits, int32_t row_segments, int64_t batch,
                                                         size_t* scratch_bytes_out) {
  if (!scratch_bytes_out) return fail(HN_ERR_ARG, "NULL scratch_bytes_out");
  if (int rc = layer_op_config(train_f32_bits, row_segments, batch)) return rc;
  *scratch_bytes_out = hn_train_layout((long)batch, train_f32_bits, row_segments).scratch_total;
  return HN_OK;
}

extern "C" int hn_hardnet_train_layer_op(int32_t op, int32_t layer, int32_t train_f32_bits, int32_t row_segments,
                                         int64_t dgrad_chunk, int64_t batch, const float* d_x, const float* d_w,
                                         float* d_y, float* d_aux0, float* d_aux1, float* d_aux2, float momentum,
                                         float dropout_p, uint64_t seed, void* d_scratch, size_t scratch_bytes,
                                         void* hip_stream) {
  size_t need = 0;
  if (int rc = hn_hardnet_train_layer_op_workspace_bytes(train_f32_bits, row_segments, batch, &need)) return rc;
  if (op < HN_TRAIN_OP_INPUT_NORM || op > HN_TRAIN_OP_INPUT_NORM_BWD)
    return fail(HN_ERR_ARG, "unknown op " + std::to_string(op));
  if (layer < 0 || layer > 6) return fail(HN_ERR_ARG, "layer must be 0 .. 6");
  const int form = hn_train_conv_form(op, layer, train_f32_bits < 0 ? hn_knobs().train_f32 : train_f32_bits);
  if (row_segments && form != kHnFormRing && form != kHnFormRingShared)
    return fail(HN_ERR_ARG, "row_segments: this op / layer / train_f32_bits has no row-segment kernel");
  if (dgrad_chunk < 0 || dgrad_chunk > batch) return fail(HN_ERR_ARG, "dgrad_chunk must be 0 .. batch");
  if (dgrad_chunk && !(op == HN_TRAIN_OP_CONV_DGRAD && form == kHnFormCol))
    return fail(HN_ERR_ARG, "dgrad_chunk: this op / layer / train_f32_bits is not the column-GEMM data gradient");
  const bool needs_x = op != HN_TRAIN_OP_BN_FWD;
  const bool needs_w = op == HN_TRAIN_OP_CONV_FWD || op == HN_TRAIN_OP_L2_BWD || op == HN_TRAIN_OP_BN_BWD ||
                       op == HN_TRAIN_OP_CONV_WGRAD || op == HN_TRAIN_OP_CONV_DGRAD;
  const bool needs_aux0 = op == HN_TRAIN_OP_INPUT_NORM || op == HN_TRAIN_OP_BN_FWD || op == HN_TRAIN_OP_INPUT_NORM_BWD;
  if (!d_y || (needs_x && !d_x) || (needs_w && !d_w) || (needs_aux0 && !d_aux0))
    return fail(HN_ERR_ARG, "NULL device pointer");
  if (op == HN_TRAIN_OP_BN_FWD)
    if (int rc = hn_pair_given(d_aux1, d_aux2, "running_mean and running_var")) return rc;
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(HN_ERR_ARG, "dropout_p must be in [0, 1)");
  if (hn_misaligned(16, d_x, d_w, d_y, d_aux0, d_aux1, d_aux2, static_cast<const char*>(d_scratch)))
    return fail(HN_ERR_ARG, "device pointers must be 16-byte aligned");
  if (!d_scratch) return fail(HN_ERR_ARG, "NULL workspace");
  if (int rc = hn_need_ws(scratch_bytes, need, "scratch ")) return rc;
  const HnTrainOpArgs o{op,    layer,  train_f32_bits, row_segments, (long)dgrad_chunk, (long)batch, d_x,   d_w,
                        d_y,   d_aux0, d_aux1,         d_aux2,       momentum,          dropout_p,   1e-5f, 1e-7f,
                        1e-10f, (unsigned long long)seed};
  HIPCHK(hn_train_layer_op(o, static_cast<char*>(d_scratch), static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// ---------------------------------------------------------------------------------------
// train-mode hardnetNAS (hn_nas_train.hip)
// ---------------------------------------------------------------------------------------
static int nas_train_desc_ok(const hn_arch_desc* d) {
  if (!d) return fail(HN_ERR_ARG, "NULL desc");
  const bool fdl = d->kind == HN_KIND_FDL_NASNET || d->kind == HN_KIND_FDL_NASNET01;
  if (d->kind != HN_KIND_NAS && d->kind != HN_KIND_NAS_SUPERNET && !fdl)
    return fail(HN_ERR_ARG, "train mode: desc kind must be HN_KIND_NAS, HN_KIND_NAS_SUPERNET or an FDL kind");
  if (d->n_layers < 1 || d->n_layers > HN_MAX_LAYERS) return fail(HN_ERR_ARG, "bad n_layers");
  if (fdl && !(d->input_norm_eps >= 0.f)) return fail(HN_ERR_ARG, "FDL: input_norm_eps must be >= 0");
  int hw = fdl ? 8 : 32, c = fdl ? 64 : 32;  // the FDL fronts leave 64 channels at 8x8
  for (int i = 0; i < d->n_layers; ++i) {
    if (d->kind != HN_KIND_NAS_SUPERNET && (d->op[i] < 0 || d->op[i] >= 17)) return fail(HN_ERR_ARG, "bad op index");
    if (d->c_in[i] != c || (d->stride[i] != 1 && d->stride[i] != 2) || hw % d->stride[i])
      return fail(HN_ERR_ARG, "layer " + std::to_string(i) + ": channels / stride do not chain");
    if (d->c_out[i] < 1 || d->c_out[i] > 128 || d->c_in[i] % 4 || d->c_out[i] % 4)
      return fail(HN_ERR_ARG, "layer " + std::to_string(i) + ": channel count");
    c = d->c_out[i];
    hw /= d->stride[i];
  }
  if (hw != 4) return fail(HN_ERR_ARG, "the layers must reduce the front's output to the 4x4 head input");
  return HN_OK;
}

extern "C" int hn_nas_train_tensor_count(const hn_arch_desc* desc, size_t* n_out) {
  int rc = nas_train_desc_ok(desc);
  if (rc) return rc;
  if (!n_out) return fail(HN_ERR_ARG, "NULL n_out");
  hn_nas_train_plan(*desc, 2, n_out, nullptr, nullptr);
  return HN_OK;
}

extern "C" int hn_nas_train_workspace_bytes(const hn_arch_desc* desc, int64_t batch, size_t* saved_bytes_out,
                                            size_t* scratch_bytes_out) {
  int rc = nas_train_desc_ok(desc);
  if (rc) return rc;
  if (!saved_bytes_out || !scratch_bytes_out || batch < 2 || batch > (1 << 22))
    return fail(HN_ERR_ARG, "batch must be 2 .. 2^22 (and both size pointers given)");
  hn_nas_train_plan(*desc, (long)batch, nullptr, saved_bytes_out, scratch_bytes_out);
  return HN_OK;
}

static int nas_train_args(const hn_arch_desc* desc, int64_t batch, float* const* tensors, void* saved,
                          size_t saved_bytes, void* scratch, size_t scratch_bytes, const float* soft) {
  size_t need_sv = 0, need_sc = 0, nt = 0;
  int rc = hn_nas_train_workspace_bytes(desc, batch, &need_sv, &need_sc);
  if (rc) return rc;
  hn_nas_train_plan(*desc, (long)batch, &nt, nullptr, nullptr);
  if (!saved || !scratch) return fail(HN_ERR_ARG, "NULL workspace");
  if ((rc = hn_train_buffers(saved_bytes, need_sv, scratch_bytes, need_sc, tensors, nt, "tensor"))) return rc;
  if (desc->kind == HN_KIND_NAS_SUPERNET && !soft) return fail(HN_ERR_ARG, "the supernet needs d_soft");
  return HN_OK;
}

extern "C" int hn_nas_train_forward(const hn_arch_desc* desc, const float* d_in, int64_t batch, float* const* d_tensors,
                                    float momentum, const float* d_soft, float* d_out, void* d_saved,
                                    size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  int rc = nas_train_args(desc, batch, d_tensors, d_saved, saved_bytes, d_scratch, scratch_bytes, d_soft);
  if (rc) return rc;
  if (!d_in || !d_out) return fail(HN_ERR_ARG, "NULL device pointer");
  HIPCHK(hn_nas_train_forward_impl(*desc, d_in, (long)batch, d_tensors, momentum, d_soft, d_out,
                                   static_cast<char*>(d_saved), static_cast<char*>(d_scratch),
                                   static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_nas_train_backward(const hn_arch_desc* desc, const float* d_dout, const float* d_in, int64_t batch,
                                     float* const* d_tensors, const float* d_soft, float* const* d_grads,
                                     float* d_dsoft, void* d_saved, size_t saved_bytes, void* d_scratch,
                                     size_t scratch_bytes, void* hip_stream) {
  return hn_nas_train_backward_dx(desc, d_dout, d_in, batch, d_tensors, d_soft, d_grads, d_dsoft, nullptr, d_saved,
                                  saved_bytes, d_scratch, scratch_bytes, hip_stream);
}

extern "C" int hn_nas_train_backward_dx(const hn_arch_desc* desc, const float* d_dout, const float* d_in,
                                        int64_t batch, float* const* d_tensors, const float* d_soft,
                                        float* const* d_grads, float* d_dsoft, float* d_din, void* d_saved,
                                        size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream) {
  int rc = nas_train_args(desc, batch, d_tensors, d_saved, saved_bytes, d_scratch, scratch_bytes, d_soft);
  if (rc) return rc;
  if (!d_dout || !d_in) return fail(HN_ERR_ARG, "NULL device pointer");
  if (!d_grads) return fail(HN_ERR_ARG, "NULL gradient pointer array");
  if (const int slot = hn_nas_train_null_grad_slot(*desc, d_grads); slot >= 0) {
    return fail(HN_ERR_ARG, "d_grads[" + std::to_string(slot) + "] is NULL: every weight slot needs a gradient buffer");
  }
  if (desc->kind == HN_KIND_NAS_SUPERNET && !d_dsoft) return fail(HN_ERR_ARG, "the supernet needs d_dsoft");
  if (hn_misaligned(16, d_din)) return fail(HN_ERR_ARG, "d_din must be 16-byte aligned");
  HIPCHK(hn_nas_train_backward_impl(*desc, d_dout, (long)batch, d_in, d_tensors, d_soft, d_grads, d_dsoft, d_din,
                                    static_cast<char*>(d_saved), static_cast<char*>(d_scratch),
                                    static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_hardnet_loss_train_workspace_bytes(int64_t batch, size_t* bytes_out) {
  if (!bytes_out || batch < 1 || batch > (1 << 22)) return fail(HN_ERR_ARG, "batch out of range");
  *bytes_out = hn_loss_train_saved_bytes((long)batch);
  return HN_OK;
}

// what both train losses check about the descriptors and the saved buffer (`need`: its bytes for a valid batch)
static int loss_args(const float* a, const float* p, int64_t batch, int32_t dim, int32_t loss_type, void* saved,
                     size_t saved_bytes, size_t (*need)(long)) {
  if (!a || !p || !saved) return fail(HN_ERR_ARG, "NULL device pointer");
  if (batch < 1 || batch > (1 << 22)) return fail(HN_ERR_ARG, "batch out of range");
  if (dim != 128) return fail(HN_ERR_ARG, "dim must be 128");
  if (loss_type < 0 || loss_type > 2) return fail(HN_ERR_ARG, "unknown loss_type");
  if (hn_misaligned(16, a, p, saved)) return fail(HN_ERR_ARG, "device pointers must be 16-byte aligned");
  if (saved_bytes < need((long)batch)) return fail(HN_ERR_WORKSPACE, "saved workspace too small");
  return HN_OK;
}
static int loss_train_args(const float* a, const float* p, int64_t batch, int32_t dim, int32_t loss_type,
                           void* saved, size_t saved_bytes) {
  return loss_args(a, p, batch, dim, loss_type, saved, saved_bytes, hn_loss_train_saved_bytes);
}

extern "C" int hn_hardnet_loss_train_forward(const float* d_anchor, const float* d_positive, int64_t batch,
                                             int32_t dim, int32_t anchor_swap, float margin, int32_t loss_type,
                                             float* d_loss, void* d_saved, size_t saved_bytes, void* hip_stream) {
  if (int rc = loss_train_args(d_anchor, d_positive, batch, dim, loss_type, d_saved, saved_bytes)) return rc;
  if (!d_loss) return fail(HN_ERR_ARG, "NULL device pointer");
  HIPCHK(hn_launch_loss_train_fwd(d_anchor, d_positive, (int)batch, anchor_swap ? 1 : 0, margin, loss_type, d_loss,
                                  d_saved, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_hardnet_loss_backward(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim,
                                        int32_t anchor_swap, float margin, int32_t loss_type, const float* d_dloss,
                                        float* d_grad_anchor, float* d_grad_positive, void* d_saved,
                                        size_t saved_bytes, void* hip_stream) {
  if (int rc = loss_train_args(d_anchor, d_positive, batch, dim, loss_type, d_saved, saved_bytes)) return rc;
  if (!d_dloss || !d_grad_anchor || !d_grad_positive) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_grad_anchor, d_grad_positive))
    return fail(HN_ERR_ARG, "gradient pointers must be 8-byte aligned");
  HIPCHK(hn_launch_loss_train_bwd(d_anchor, d_positive, (int)batch, anchor_swap ? 1 : 0, margin, loss_type, d_dloss,
                                  d_grad_anchor, d_grad_positive, d_saved, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// loss_HardNet's 'average' and 'random' reductions (hn_loss_dense.hip, hn_loss.hip)
static constexpr int64_t kAverageMaxBatch = 65536;  // B^2 work beyond it would occupy the GPU for seconds per call
static int reduce_kind(int32_t batch_reduce) {
  if (batch_reduce == HN_REDUCE_MIN)
    return fail(HN_ERR_ARG, "HN_REDUCE_MIN runs on hn_hardnet_loss_train_forward / hn_hardnet_loss_backward");
  if (batch_reduce != HN_REDUCE_AVERAGE && batch_reduce != HN_REDUCE_RANDOM)
    return fail(HN_ERR_ARG, "unknown batch_reduce " + std::to_string(batch_reduce));
  return HN_OK;
}
static size_t average_saved_bytes(long b) { return b <= kAverageMaxBatch ? hn_loss_dense_saved_bytes(b) : 0; }

extern "C" int hn_hardnet_loss_reduce_workspace_bytes(int32_t batch_reduce, int64_t batch, size_t* bytes_out) {
  if (int rc = reduce_kind(batch_reduce)) return rc;
  const int64_t cap = batch_reduce == HN_REDUCE_AVERAGE ? kAverageMaxBatch : (int64_t)1 << 22;
  if (!bytes_out || batch < 1 || batch > cap)
    return fail(HN_ERR_ARG, "batch out of range (1 .. " + std::to_string(cap) + " for this batch_reduce)");
  *bytes_out = batch_reduce == HN_REDUCE_AVERAGE ? hn_loss_dense_saved_bytes((long)batch)
                                                 : hn_loss_train_saved_bytes((long)batch);
  return HN_OK;
}

static int loss_reduce_args(const float* a, const float* p, const int64_t* idx, int64_t batch, int32_t dim,
                            int32_t batch_reduce, int32_t loss_type, void* saved, size_t saved_bytes) {
  if (int rc = reduce_kind(batch_reduce)) return rc;
  if (batch_reduce == HN_REDUCE_AVERAGE && batch > kAverageMaxBatch)
    return fail(HN_ERR_ARG, "batch out of range (1 .. " + std::to_string(kAverageMaxBatch) + " for HN_REDUCE_AVERAGE)");
  if (int rc = loss_args(a, p, batch, dim, loss_type, saved, saved_bytes,
                         batch_reduce == HN_REDUCE_AVERAGE ? average_saved_bytes : hn_loss_train_saved_bytes))
    return rc;
  if (batch_reduce == HN_REDUCE_RANDOM) {
    if (!idx) return fail(HN_ERR_ARG, "HN_REDUCE_RANDOM needs d_idx");
    if (hn_misaligned(8, idx)) return fail(HN_ERR_ARG, "d_idx must be 8-byte aligned");
  }
  return HN_OK;
}

extern "C" int hn_hardnet_loss_reduce_forward(const float* d_anchor, const float* d_positive, const int64_t* d_idx,
                                              int64_t batch, int32_t dim, int32_t batch_reduce, int32_t anchor_swap,
                                              float margin, int32_t loss_type, float* d_loss, void* d_saved,
                                              size_t saved_bytes, void* hip_stream) {
  if (int rc = loss_reduce_args(d_anchor, d_positive, d_idx, batch, dim, batch_reduce, loss_type, d_saved, saved_bytes))
    return rc;
  if (!d_loss) return fail(HN_ERR_ARG, "NULL device pointer");
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (batch_reduce == HN_REDUCE_AVERAGE)
    HIPCHK(hn_launch_loss_dense_fwd(d_anchor, d_positive, (int)batch, anchor_swap ? 1 : 0, margin, loss_type, d_loss,
                                    d_saved, st));
  else
    HIPCHK(hn_launch_loss_random_fwd(d_anchor, d_positive, reinterpret_cast<const long long*>(d_idx), (int)batch,
                                     anchor_swap ? 1 : 0, margin, loss_type, d_loss, d_saved, st));
  return HN_OK;
}

extern "C" int hn_hardnet_loss_reduce_backward(const float* d_anchor, const float* d_positive, const int64_t* d_idx,
                                               int64_t batch, int32_t dim, int32_t batch_reduce, int32_t anchor_swap,
                                               float margin, int32_t loss_type, const float* d_dloss,
                                               float* d_grad_anchor, float* d_grad_positive, void* d_saved,
                                               size_t saved_bytes, void* hip_stream) {
  if (int rc = loss_reduce_args(d_anchor, d_positive, d_idx, batch, dim, batch_reduce, loss_type, d_saved, saved_bytes))
    return rc;
  if (!d_dloss || !d_grad_anchor || !d_grad_positive) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_grad_anchor, d_grad_positive))
    return fail(HN_ERR_ARG, "gradient pointers must be 8-byte aligned");
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (batch_reduce == HN_REDUCE_AVERAGE)
    HIPCHK(hn_launch_loss_dense_bwd(d_anchor, d_positive, (int)batch, anchor_swap ? 1 : 0, margin, loss_type, d_dloss,
                                    d_grad_anchor, d_grad_positive, d_saved, st));
  else  // the selections lie in d_saved: the 'min' backward runs on them as it is
    HIPCHK(hn_launch_loss_train_bwd(d_anchor, d_positive, (int)batch, anchor_swap ? 1 : 0, margin, loss_type, d_dloss,
                                    d_grad_anchor, d_grad_positive, d_saved, st));
  return HN_OK;
}

extern "C" int hn_neimask_loss_workspace_bytes(int64_t batch, size_t* bytes_out) {
  if (!bytes_out || batch < 1 || batch > (1 << 22)) return fail(HN_ERR_ARG, "batch out of range");
  *bytes_out = hn_neimask_saved_bytes((long)batch);
  return HN_OK;
}

static int neimask_args(const float* a, const float* p, int64_t batch, int32_t dim, void* saved, size_t saved_bytes) {
  return loss_args(a, p, batch, dim, 0, saved, saved_bytes, hn_neimask_saved_bytes);
}

extern "C" int hn_neimask_loss_forward(const float* d_anchor, const float* d_positive, const int64_t* d_anchor_kp,
                                       const int64_t* d_positive_kp, int64_t batch, int32_t dim, float margin,
                                       float coo_thresh, float* d_loss, float* d_pos, float* d_min_neg, void* d_saved,
                                       size_t saved_bytes, void* hip_stream) {
  if (int rc = neimask_args(d_anchor, d_positive, batch, dim, d_saved, saved_bytes)) return rc;
  if (!d_anchor_kp || !d_positive_kp || !d_loss) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_anchor_kp, d_positive_kp)) return fail(HN_ERR_ARG, "keypoint pointers must be 8-byte aligned");
  if (hn_misaligned(4, d_loss, d_pos, d_min_neg)) return fail(HN_ERR_ARG, "output pointers must be 4-byte aligned");
  HIPCHK(hn_launch_neimask_fwd(d_anchor, d_positive, reinterpret_cast<const long long*>(d_anchor_kp),
                               reinterpret_cast<const long long*>(d_positive_kp), (int)batch, margin, coo_thresh, d_loss,
                               d_pos, d_min_neg, d_saved, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_neimask_loss_backward(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim,
                                        float margin, const float* d_dloss, float* d_grad_anchor,
                                        float* d_grad_positive, void* d_saved, size_t saved_bytes, void* hip_stream) {
  if (int rc = neimask_args(d_anchor, d_positive, batch, dim, d_saved, saved_bytes)) return rc;
  if (!d_dloss || !d_grad_anchor || !d_grad_positive) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_grad_anchor, d_grad_positive))
    return fail(HN_ERR_ARG, "gradient pointers must be 8-byte aligned");
  HIPCHK(hn_launch_neimask_bwd(d_anchor, d_positive, (int)batch, margin, d_dloss, d_grad_anchor, d_grad_positive,
                               d_saved, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}
