// C ABI (include/hardnet_mi355x_rfdet.h) of RF-Net's ten-scale detector (hn_rfdet.hip).  Each entry point checks
// its arguments on the host and makes one launch call.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "hardnet_mi355x.h"
#include "hn_api_util.h"
#include "hn_internal.h"
#include "hn_rfdet.h"

struct hn_rfdet {
  float* params = nullptr;  // hnrf layout
  float in_eps = 1e-5f, cs1 = 0.f, cs2 = 0.f;
};

extern "C" int hn_rfdet_param_count(size_t* n_out) {
  if (!n_out) return fail(HN_ERR_ARG, "n_out is NULL");
  *n_out = hnrf::kStateFloats;
  return HN_OK;
}

extern "C" int hn_rfdet_create(const float* host_params, size_t n_params, const float* scale_list, float in_eps,
                               float score_com_strength, float scale_com_strength, hn_rfdet** out) {
  using namespace hnrf;
  if (!out || !host_params || !scale_list) return fail(HN_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (n_params != (size_t)kStateFloats)
    return fail(HN_ERR_ARG, "host_params has " + std::to_string(n_params) + " floats, expected " +
                                std::to_string(kStateFloats));
  if (!(in_eps > 0.f) || !std::isfinite(in_eps)) return fail(HN_ERR_ARG, "in_eps must be > 0");
  if (!std::isfinite(score_com_strength) || !std::isfinite(scale_com_strength))
    return fail(HN_ERR_ARG, "score_com_strength and scale_com_strength must be finite");
  for (size_t i = 0; i < n_params; ++i)
    if (!std::isfinite(host_params[i])) return fail(HN_ERR_ARG, "host_params holds a non-finite value");
  for (int k = 0; k < kLevels; ++k)
    if (!std::isfinite(scale_list[k])) return fail(HN_ERR_ARG, "scale_list holds a non-finite value");
  std::vector<float> f(kDeviceFloats, 0.f);
  const float* p = host_params;
  for (int k = 0; k < kLevels; ++k) {
    float* L = &f[(size_t)k * kLevelStride];
    if (k == 0) {
      std::memcpy(L + kConvW, p, 144 * sizeof(float));  // conv1.weight [16][1][3][3]
      p += 144;
    } else {
      for (int co = 0; co < 16; ++co)  // conv_k.weight [16][16][3][3] into the MFMA B-operand order
        for (int ci = 0; ci < 16; ++ci)
          for (int tap = 0; tap < 9; ++tap) L[kConvW + mfma_weight_index(co, ci, tap)] = p[(co * 16 + ci) * 9 + tap];
      p += 2304;
    }
    std::memcpy(L + kConvB, p, 16 * sizeof(float));
    std::memcpy(L + kInG, p + 16, 16 * sizeof(float));
    std::memcpy(L + kInB, p + 32, 16 * sizeof(float));
    std::memcpy(L + kSW, p + 48, 16 * sizeof(float));
    L[kSB] = p[64];
    L[kSG] = p[65];
    L[kSBeta] = p[66];
    p += 67;
  }
  for (int k = 0; k < kLevels; ++k) {  // conv_o*.weight [2][16], .bias [2]
    float* L = &f[(size_t)k * kLevelStride];
    std::memcpy(L + kOW, p, 32 * sizeof(float));
    L[kOB] = p[32];
    L[kOB + 1] = p[33];
    p += 34;
  }
  if ((size_t)(p - host_params) != n_params) return fail(HN_ERR_ARG, "host_params not fully consumed");
  std::memcpy(&f[kScaleList], scale_list, kLevels * sizeof(float));
  hn_rfdet* d = new hn_rfdet;
  d->in_eps = in_eps;
  d->cs1 = score_com_strength;
  d->cs2 = scale_com_strength;
  if (hipMalloc(&d->params, kDeviceFloats * sizeof(float)) != hipSuccess) {
    delete d;
    return fail(HN_ERR_NOMEM, "hipMalloc of parameters failed");
  }
  const hipError_t e = hipMemcpy(d->params, f.data(), kDeviceFloats * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d->params);
    delete d;
    return fail(HN_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  *out = d;
  return HN_OK;
}

extern "C" void hn_rfdet_destroy(hn_rfdet* d) {
  if (!d) return;
  (void)hipFree(d->params);
  delete d;
}

// what hn_rfdet_workspace_bytes and hn_rfdet_forward check about the images (hn_det_forward's rules); null = fine
static const char* rfdet_arg_error(int64_t n_images, int32_t height, int32_t width) {
  if (n_images < 0) return "n_images must be >= 0";
  if (height < 1 || width < 1 || (int64_t)height * width < 2)
    return "height and width must be >= 1 with at least 2 pixels (InstanceNorm)";
  if ((int64_t)height * width > INT32_MAX) return "height * width must be below 2^31";
  if (n_images > INT32_MAX || n_images * hn_rfdet_parts(height, width) > INT32_MAX)
    return "n_images * tiles must be below 2^31";
  return nullptr;
}

extern "C" int hn_rfdet_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* bytes_out) {
  if (!bytes_out) return fail(HN_ERR_ARG, "bytes_out is NULL");
  if (const char* e = rfdet_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  *bytes_out = hn_rfdet_ws_bytes(n_images, height, width);
  return HN_OK;
}

extern "C" int hn_rfdet_forward(hn_rfdet* d, const float* d_images, int64_t n_images, int32_t height, int32_t width,
                                float* d_score, float* d_scale, float* d_ori, void* d_workspace,
                                size_t workspace_bytes, void* hip_stream) {
  if (const char* e = rfdet_arg_error(n_images, height, width)) return fail(HN_ERR_ARG, e);
  if (!d) return fail(HN_ERR_ARG, "detector is NULL");
  if (n_images == 0) return HN_OK;
  if (!d_images || !d_score || !d_scale || !d_ori || !d_workspace) return fail(HN_ERR_ARG, "NULL device pointer");
  if (hn_misaligned(8, d_ori) || hn_misaligned(16, d_workspace))
    return fail(HN_ERR_ARG, "d_ori must be 8-byte and d_workspace 16-byte aligned");
  if (int rc = hn_need_ws(workspace_bytes, hn_rfdet_ws_bytes(n_images, height, width))) return rc;
  HIPCHK(hn_launch_rfdet(d->params, d->in_eps, d->cs1, d->cs2, d_images, n_images, height, width, d_score, d_scale,
                         d_ori, d_workspace, static_cast<hipStream_t>(hip_stream)));
  return HN_OK;
}
