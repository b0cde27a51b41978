// C ABI (include/hardnet_mi355x.h) of FDLNet's keypoint side: the NASNet detector in eval() (hn_det.hip) and in
// train() (hn_det_train.hip), keypoint selection (hn_select.hip) and the homography ground-truth stage (hn_gt.hip).
// Each entry point checks its arguments on the host and makes one launch call.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "hardnet_mi355x.h"
#include "hn_api_util.h"
#include "hn_internal.h"

struct hn_detector {
  float* params = nullptr;  // hndet layout, BN folded
  float in_eps = 1e-5f;
};

extern "C" int hn_det_param_count(size_t* n_out) {
  if (!n_out) return fail(HN_ERR_ARG, "n_out is NULL");
  *n_out = hndet::kStateFloats;
  return HN_OK;
}

extern "C" int hn_det_create(const float* host_params, size_t n_params, float bn_eps, float in_eps,
                             hn_detector** out) {
  using namespace hndet;
  if (!out || !host_params) return fail(HN_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (n_params != (size_t)kStateFloats)
    return fail(HN_ERR_ARG, "host_params has " + std::to_string(n_params) + " floats, expected " +
                                std::to_string(kStateFloats));
  if (!(bn_eps > 0.f) || !(in_eps > 0.f)) return fail(HN_ERR_ARG, "bn_eps and in_eps must be > 0");
  for (size_t i = 0; i < n_params; ++i)
    if (!std::isfinite(host_params[i])) return fail(HN_ERR_ARG, "host_params holds a non-finite value");
  std::vector<float> f(kFolded);
  const float* p = host_params;
  std::memcpy(&f[kC0W], p, 160 * sizeof(float));  // features.0.weight, .bias
  p += 160;
  // conv weight [cout][per] without bias, then BatchNorm weight, bias, running_mean, running_var [cout]
  auto conv_bn = [&](int cout, int per, float* w, float* b) -> bool {
    const float *cw = p, *g = p + cout * per, *be = g + cout, *rm = be + cout, *rv = rm + cout;
    p = rv + cout;
    for (int o = 0; o < cout; ++o) {
      if (!((double)rv[o] + bn_eps > 0)) return false;
      const double s = (double)g[o] / std::sqrt((double)rv[o] + (double)bn_eps);
      for (int k = 0; k < per; ++k) w[o * per + k] = (float)((double)cw[o * per + k] * s);
      b[o] = (float)((double)be[o] - (double)rm[o] * s);
    }
    return true;
  };
  for (int k = 0; k < 2; ++k) {
    float* blk = &f[kBlk + k * kBlkSize];
    if (!conv_bn(8, 8, blk + kBlkPw1W, blk + kBlkPw1B) || !conv_bn(8, 9, blk + kBlkDwW, blk + kBlkDwB) ||
        !conv_bn(8, 8, blk + kBlkPw2W, blk + kBlkPw2B))
      return fail(HN_ERR_ARG, "a BatchNorm running_var + bn_eps is not positive");
  }
  std::memcpy(&f[kHeadW], p, 144 * sizeof(float));  // conv.weight
  f[kHeadB] = p[144];                               // conv.bias
  f[kInG] = p[145];                                 // insnorm.weight, .bias
  f[kInB] = p[146];
  p += 147;
  std::memcpy(&f[kHeadW + 144], p, 288 * sizeof(float));  // conv_ori.weight
  f[kHeadB + 1] = p[288];                                 // conv_ori.bias
  f[kHeadB + 2] = p[289];
  f[kInG + 1] = p[290];                                   // insnorm_ori.weight, .bias
  f[kInG + 2] = p[291];
  f[kInB + 1] = p[292];
  f[kInB + 2] = p[293];
  p += 294;
  if ((size_t)(p - host_params) != n_params) return fail(HN_ERR_ARG, "host_params not fully consumed");
  hn_detector* d = new hn_detector;
  d->in_eps = in_eps;
  if (hipMalloc(&d->params, kFolded * sizeof(float)) != hipSuccess) {
    delete d;
    return fail(HN_ERR_NOMEM, "hipMalloc of parameters failed");
  }
  const hipError_t e = hipMemcpy(d->params, f.data(), kFolded * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d->params);
    delete d;
    return fail(HN_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  *out = d;
  return HN_OK;
}

extern "C" void hn_det_destroy(hn_detector* d) {
  if (!d) return;
  (void)hipFree(d->params);
  delete d;
}

// what hn_det_workspace_bytes and hn_det_forward check about the images; null = fine
static const char* det_arg_error(int64_t n_images, int32_t height, int32_t width) {
  if (n_images < 0) return "n_images must be >= 0";
  if (height < 1 || width < 1 || (int64_t)height * width < 2)
    return "height and width must be >= 1 with at least 2 pixels (InstanceNorm)";
  if ((int64_t)height * width > INT32_MAX) return "height * width must be below 2^31";
  if (n_images > INT32_MAX || n_images * hn_det_parts(height, width) > INT32_MAX)
    return "n_images * tiles must be below 2^31";
  return nullptr;
}

extern "C" int hn_det_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* bytes_out) {
  if (!bytes_out) return fail(HN_ERR_ARG, "bytes_out is NULL");
  if (const char* e = det_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  *bytes_out = hn_det_ws_bytes(n_images, height, width);
  return HN_OK;
}

extern "C" int hn_det_forward(hn_detector* d, const float* d_images, int64_t n_images, int32_t height, int32_t width,
                              float* d_score, float* d_ori, void* d_workspace, size_t workspace_bytes,
                              void* hip_stream) {
  if (const char* e = det_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (!d) return fail(HN_ERR_ARG, "detector is NULL");
  if (n_images == 0) return HN_OK;
  if (!d_images || !d_score || !d_ori || !d_workspace) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_ori) || hn_misaligned(16, d_workspace))
    return fail(HN_ERR_ARG, "d_ori must be 8-byte and d_workspace 16-byte aligned");
  if (int rc = hn_need_ws(workspace_bytes, hn_det_ws_bytes(n_images, height, width))) return rc;
  HIPCHK(hn_launch_det(d->params, d->in_eps, d_images, n_images, height, width, d_score, d_ori, d_workspace,
                       static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// the detector in train() (hn_det_train.hip): what the three entry points check about the images; null = fine
static const char* det_train_arg_error(int64_t n_images, int32_t height, int32_t width) {
  if (n_images < 1) return "n_images must be >= 1";
  if (height < 1 || width < 1) return "height and width must be >= 1";
  if ((int64_t)height * width > INT32_MAX) return "height * width must be below 2^31";
  if (n_images > (1 << 24)) return "n_images must be at most 2^24";
  if (n_images * height * width < 2) return "n_images * height * width must be >= 2 (the unbiased batch variance)";
  return nullptr;
}

extern "C" int hn_det_train_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* saved_bytes_out,
                                            size_t* scratch_bytes_out) {
  if (!saved_bytes_out || !scratch_bytes_out) return fail(HN_ERR_ARG, "NULL size pointer");
  if (const char* e = det_train_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  hn_det_train_plan(n_images, height, width, saved_bytes_out, scratch_bytes_out);
  return HN_OK;
}

static int det_train_args(int64_t n_images, int32_t height, int32_t width, const float* images,
                          float* const* tensors, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes) {
  if (const char* e = det_train_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (!images || !saved || !scratch) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(16, images, saved, scratch))
    return fail(HN_ERR_ARG, "d_images, d_saved and d_scratch must be 16-byte aligned");
  size_t need_sv = 0, need_sc = 0;
  hn_det_train_plan(n_images, height, width, &need_sv, &need_sc);
  return hn_train_buffers(saved_bytes, need_sv, scratch_bytes, need_sc, tensors, HN_DET_TRAIN_TENSORS, "tensor");
}

extern "C" int hn_det_train_forward(const float* d_images, int64_t n_images, int32_t height, int32_t width,
                                    float* const* d_tensors, float bn_eps, float in_eps, float momentum,
                                    float* d_score, float* d_ori, void* d_saved, size_t saved_bytes, void* d_scratch,
                                    size_t scratch_bytes, void* hip_stream) {
  int rc = det_train_args(n_images, height, width, d_images, d_tensors, d_saved, saved_bytes, d_scratch,
                          scratch_bytes);
  if (rc) return rc;
  if (!(bn_eps > 0.f) || !(in_eps > 0.f)) return fail(HN_ERR_ARG, "bn_eps and in_eps must be > 0");
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(HN_ERR_ARG, "momentum must be in 0 .. 1");
  if (!d_score || !d_ori) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(16, d_score, d_ori)) return fail(HN_ERR_ARG, "d_score and d_ori must be 16-byte aligned");
  HIPCHK(hn_det_train_forward_impl(d_images, n_images, height, width, d_tensors, bn_eps, in_eps, momentum, d_score,
                                   d_ori, static_cast<char*>(d_saved), static_cast<char*>(d_scratch),
                                   static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_det_train_backward(const float* d_dscore, const float* d_dori, const float* d_images,
                                     int64_t n_images, int32_t height, int32_t width, float* const* d_tensors,
                                     float* const* d_grads, void* d_saved, size_t saved_bytes, void* d_scratch,
                                     size_t scratch_bytes, void* hip_stream) {
  int rc = det_train_args(n_images, height, width, d_images, d_tensors, d_saved, saved_bytes, d_scratch,
                          scratch_bytes);
  if (rc) return rc;
  if (hn_misaligned(16, d_dscore, d_dori)) return fail(HN_ERR_ARG, "d_dscore and d_dori must be 16-byte aligned");
  if (!d_grads) return fail(HN_ERR_ARG, "NULL gradient pointer array");
  for (int i = 0; i < HN_DET_TRAIN_TENSORS; ++i)
    if (hn_det_train_is_param(i) && !d_grads[i])
      return fail(HN_ERR_ARG, "d_grads[" + std::to_string(i) + "] is NULL: every parameter slot needs a gradient buffer");
  HIPCHK(hn_det_train_backward_impl(d_dscore, d_dori, d_images, n_images, height, width, d_tensors, d_grads,
                                    static_cast<char*>(d_saved), static_cast<char*>(d_scratch),
                                    static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// what hn_select_workspace_bytes and hn_select_keypoints check about the map and K; null = fine
static const char* select_arg_error(int64_t n_images, int32_t height, int32_t width, int32_t topk) {
  if (n_images < 0) return "n_images must be >= 0";
  if (height < 1 || width < 1) return "height and width must be >= 1";
  if ((int64_t)height * width > INT32_MAX) return "height * width must be below 2^31";
  if (n_images > INT32_MAX) return "n_images must be below 2^31";
  return hn_topk_error(topk, height, width);
}

extern "C" int hn_select_workspace_bytes(int64_t n_images, int32_t height, int32_t width, int32_t topk,
                                         size_t* bytes_out) {
  if (!bytes_out) return fail(HN_ERR_ARG, "bytes_out is NULL");
  if (const char* e = select_arg_error(n_images, height, width, topk)) return fail(HN_ERR_ARG, e);
  *bytes_out = hn_select_ws_bytes(n_images, height, width);
  return HN_OK;
}

extern "C" int hn_select_keypoints(const float* d_score, int64_t n_images, int32_t height, int32_t width,
                                   int32_t border, float nms_thresh, int32_t nms_ksize, int32_t topk,
                                   int32_t gauss_ksize, float gauss_sigma, const float* d_scale_map,
                                   float scale_value, const float* d_ori_map, int64_t* d_kpts, float* d_kscore,
                                   float* d_kscale, float* d_kori, float* d_score_proc, uint8_t* d_topk_mask,
                                   void* d_workspace, size_t workspace_bytes, void* hip_stream) {
  if (const char* e = select_arg_error(n_images, height, width, topk)) return fail(HN_ERR_ARG, e);
  if (const char* e = hn_border_error(border, height, width)) return fail(HN_ERR_ARG, e);
  if (nms_ksize < 1 || nms_ksize > 15 || !(nms_ksize & 1)) return fail(HN_ERR_ARG, "nms_ksize must be odd, 1 .. 15");
  if (gauss_ksize < 1 || gauss_ksize > 15 || !(gauss_ksize & 1))
    return fail(HN_ERR_ARG, "gauss_ksize must be odd, 1 .. 15");
  if (!(gauss_sigma >= 0.f) || !std::isfinite(gauss_sigma))
    return fail(HN_ERR_ARG, "gauss_sigma must be finite and >= 0");
  if (nms_thresh != nms_thresh) return fail(HN_ERR_ARG, "nms_thresh is NaN");
  if (int rc = hn_pair_given(d_kori, d_ori_map, "d_kori and d_ori_map")) return rc;
  if (n_images == 0) return HN_OK;
  if (!d_score || !d_kpts || !d_kscore || !d_kscale || !d_workspace)
    return fail(HN_ERR_ARG, "NULL device pointer (d_scale_map, d_ori_map / d_kori, d_score_proc, d_topk_mask may be)");
  if (hn_misaligned(16, d_workspace)) return fail(HN_ERR_ARG, "d_workspace must be 16-byte aligned");
  if (int rc = hn_need_ws(workspace_bytes, hn_select_ws_bytes(n_images, height, width))) return rc;
  // get_gauss_filter_weight (image_utils.py:277-295): the exponent in its fp32 operation order, the exponential as
  // the fp64 one rounded to fp32 (what any libm reproduces); not normalised; sigma 0: a delta
  float taps[225];
  const int c = gauss_ksize / 2;
  const float two_s2 = 2.0f * (gauss_sigma * gauss_sigma);
  for (int y = 0; y < gauss_ksize; ++y)
    for (int x = 0; x < gauss_ksize; ++x) {
      const float fx = (float)(x - c), fy = (float)(y - c);
      taps[y * gauss_ksize + x] = gauss_sigma == 0.f ? (x == c && y == c ? 1.f : 0.f)
                                                     : (float)std::exp((double)-((fx * fx) / two_s2 + (fy * fy) / two_s2));
    }
  HnSelectArgs a{};
  a.score = d_score;
  a.B = n_images;
  a.H = height;
  a.W = width;
  a.border = border;
  a.nms_thresh = nms_thresh;
  a.nms_ksize = nms_ksize;
  a.topk = topk;
  a.gauss_ksize = gauss_ksize;
  a.taps = taps;
  a.scale_map = d_scale_map;
  a.scale_value = scale_value;
  a.ori_map = d_ori_map;
  a.kpts = d_kpts;
  a.kscore = d_kscore;
  a.kscale = d_kscale;
  a.kori = d_kori;
  a.score_proc = d_score_proc;
  a.topk_mask = d_topk_mask;
  a.ws = d_workspace;
  HIPCHK(hn_launch_select(a, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

// homography ground-truth stage (hn_gt.hip): what the four calls check about the maps before the GPU is touched;
// null = fine.  height * width < 2^31 and n_images * height * width < 2^62 are hn_homo.h's conditions.
static const char* gt_arg_error(int64_t n_images, int32_t height, int32_t width) {
  if (n_images < 0) return "n_images must be >= 0";
  if (height < 2 || width < 2) return "height and width must be >= 2";
  if ((int64_t)height * width > INT32_MAX) return "height * width must be below 2^31";
  if (n_images > ((int64_t)1 << 62) / ((int64_t)height * width)) return "n_images * height * width must be below 2^62";
  return nullptr;
}

extern "C" int hn_warp_score(const float* d_score, const float* d_homo, int64_t n_images, int32_t height,
                             int32_t width, int32_t border, int32_t align_corners, float* d_warped, float* d_visible,
                             void* hip_stream) {
  if (const char* e = gt_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (const char* e = hn_border_error(border, height, width)) return fail(HN_ERR_ARG, e);
  if (align_corners != 0 && align_corners != 1) return fail(HN_ERR_ARG, "align_corners must be 0 or 1");
  if (n_images == 0 || (!d_warped && !d_visible)) return HN_OK;
  if (!d_homo || (d_warped && !d_score))
    return fail(HN_ERR_ARG, "NULL device pointer (d_warped or d_visible may be; d_score only without d_warped)");
  HIPCHK(hn_launch_warp_score(d_score, d_homo, n_images, height, width, border, align_corners, d_warped, d_visible,
                              static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_gt_scale_orin(const float* d_scale, float scale_value, const float* d_ori, const float* d_homo12,
                                const float* d_homo21, int64_t n_images, int32_t height, int32_t width,
                                float* d_gt_scale, float* d_gt_ori, void* hip_stream) {
  if (const char* e = gt_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (n_images == 0) return HN_OK;
  if (!d_ori || !d_homo12 || !d_homo21 || !d_gt_scale || !d_gt_ori)
    return fail(HN_ERR_ARG, "NULL device pointer (only d_scale may be NULL)");
  if (hn_misaligned(8, d_ori, d_gt_ori)) return fail(HN_ERR_ARG, "d_ori and d_gt_ori must be 8-byte aligned");
  HIPCHK(hn_launch_gt_scale_orin(d_scale, scale_value, d_ori, d_homo12, d_homo21, n_images, height, width, d_gt_scale,
                                 d_gt_ori, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_mask_keypoints(const uint8_t* d_mask, int64_t n_images, int32_t height, int32_t width, int32_t topk,
                                 const float* d_scale_map, float scale_value, const float* d_ori_map, int64_t* d_kpts,
                                 float* d_kscale, float* d_kori, int32_t* d_counts, void* hip_stream) {
  if (const char* e = gt_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (const char* e = hn_topk_error(topk, height, width)) return fail(HN_ERR_ARG, e);
  if (n_images > INT64_MAX / 8 / topk) return fail(HN_ERR_ARG, "n_images * topk too large");
  if (int rc = hn_pair_given(d_kori, d_ori_map, "d_kori and d_ori_map")) return rc;
  if (n_images == 0) return HN_OK;
  if (!d_mask || !d_kpts || !d_kscale)
    return fail(HN_ERR_ARG, "NULL device pointer (d_scale_map, d_ori_map / d_kori and d_counts may be)");
  HIPCHK(hn_launch_mask_keypoints(d_mask, n_images, height, width, topk, d_scale_map, scale_value, d_ori_map, d_kpts,
                                  d_kscale, d_kori, d_counts, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}

extern "C" int hn_project_keypoints(const int64_t* d_kpts, int64_t n, const float* d_homo, int64_t n_images,
                                    int32_t height, int32_t width, const float* d_scale_map, float scale_value,
                                    const float* d_ori_map, int32_t clamp, int64_t* d_kpts_r, float* d_scale_r,
                                    float* d_ori_r, void* hip_stream) {
  if (n < 0) return fail(HN_ERR_ARG, "n must be >= 0");
  if (const char* e = gt_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (n > 0 && n_images == 0) return fail(HN_ERR_ARG, "n_images must be >= 1 for n > 0 keypoints");
  if (clamp != 0 && clamp != 1) return fail(HN_ERR_ARG, "clamp must be 0 or 1");
  if (int rc = hn_pair_given(d_ori_r, d_ori_map, "d_ori_r and d_ori_map")) return rc;
  if (n == 0) return HN_OK;
  if (!d_kpts || !d_homo || !d_kpts_r || !d_scale_r)
    return fail(HN_ERR_ARG, "NULL device pointer (d_scale_map and d_ori_map / d_ori_r may be)");
  HIPCHK(hn_launch_project_kpts(d_kpts, n, d_homo, n_images, height, width, d_scale_map, scale_value, d_ori_map, clamp,
                                d_kpts_r, d_scale_r, d_ori_r, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}
