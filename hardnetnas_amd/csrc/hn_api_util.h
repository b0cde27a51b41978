// What the C ABI's translation units (hn_api.hip, hn_api_det.hip, hn_api_train.hip, hn_api_ops.hip) share, and no
// kernel file includes: the error record and the argument checks that several entry points apply.  The messages are
// observable through hn_last_error, and so is the order of an entry point's checks (the first failing one decides).
#pragma once
#include <cstdint>
#include <string>

#include "hardnet_mi355x.h"
#include "hn_internal.h"

// records msg for hn_last_error on the calling thread and returns code (defined in hn_api.hip)
int hn_fail(int code, const std::string& msg);
static inline int fail(int code, const std::string& msg) { return hn_fail(code, msg); }

// (the HN_ERR_HIP message quotes the expression: rewording a call inside HIPCHK changes an error text)
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      return fail(HN_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));             \
  } while (0)

// true when one of the pointers is not a multiple of align (a power of two); NULL passes
template <class... P>
static inline bool hn_misaligned(uintptr_t align, const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & (align - 1)) != 0;
}

// HN_OK, or HN_ERR_WORKSPACE "<prefix>workspace too small: need <need> bytes"
static inline int hn_need_ws(size_t have, size_t need, const char* prefix = "") {
  if (have >= need) return HN_OK;
  return fail(HN_ERR_WORKSPACE, std::string(prefix) + "workspace too small: need " + std::to_string(need) + " bytes");
}

// an optional output and the optional input it is computed from: HN_OK, or HN_ERR_ARG "<names> must both be ..."
static inline int hn_pair_given(const void* a, const void* b, const char* names) {
  if ((a == nullptr) == (b == nullptr)) return HN_OK;
  return fail(HN_ERR_ARG, std::string(names) + " must both be given or both NULL");
}

// the rules on `border` and `topk` of a height x width map; null = fine
static inline const char* hn_border_error(int32_t border, int32_t height, int32_t width) {
  if (border < 0 || height <= 2 * (int64_t)border || width <= 2 * (int64_t)border)
    return "border must be >= 0 with height, width > 2 * border";
  return nullptr;
}
static inline const char* hn_topk_error(int32_t topk, int32_t height, int32_t width) {
  if (topk < 1 || topk > (int64_t)height * width) return "topk must be in 1 .. height * width";
  return nullptr;
}

// uint8 patches (hn_preprocess, hn_forward_u8): the resize mode and the patch side it reads
static inline int hn_resize_args(int32_t resize, int32_t in_hw) {
  if (resize != HN_RESIZE_NONE && resize != HN_RESIZE_CV2_LINEAR && resize != HN_RESIZE_PIL_BILINEAR)
    return fail(HN_ERR_ARG, "unknown resize mode " + std::to_string(resize));
  const int want = resize == HN_RESIZE_NONE ? 32 : 64;
  if (in_hw != want)
    return fail(HN_ERR_ARG, "in_hw must be " + std::to_string(want) + " for this resize mode, got " +
                                std::to_string(in_hw));
  return HN_OK;
}

// a host table of n device pointers, all required (`what`: "tensor", "weight", "gradient")
template <class T>
static inline int hn_ptr_table(T* const* ptrs, size_t n, const char* what) {
  if (!ptrs) return fail(HN_ERR_ARG, std::string("NULL ") + what + " pointer array");
  for (size_t i = 0; i < n; ++i)
    if (!ptrs[i]) return fail(HN_ERR_ARG, std::string("NULL ") + what + " pointer " + std::to_string(i));
  return HN_OK;
}
// the train entry points' two workspaces, then their pointer table
template <class T>
static inline int hn_train_buffers(size_t saved_bytes, size_t need_sv, size_t scratch_bytes, size_t need_sc,
                                   T* const* ptrs, size_t n, const char* what) {
  if (int rc = hn_need_ws(saved_bytes, need_sv, "saved ")) return rc;
  if (int rc = hn_need_ws(scratch_bytes, need_sc, "scratch ")) return rc;
  return hn_ptr_table(ptrs, n, what);
}

// keypoint patch extraction (hn_clip.hip): what hn_clip_patch and hn_forward_kp check about the images and
// the keypoint list before the GPU is touched; null = fine
static const char* clip_arg_error(int64_t n_images, int32_t height, int32_t width, int64_t n) {
  if (n < 0) return "n must be >= 0";
  if (n_images < 0) return "n_images must be >= 0";
  if (height < 2 || width < 2) return "height and width must be >= 2";
  // n_images * height * width < 2^63: the flat index of every pixel fits an int64
  if (n_images > INT64_MAX / ((int64_t)height * (int64_t)width)) return "n_images * height * width must be below 2^63";
  if (n > 0 && n_images == 0) return "n_images must be >= 1 for n > 0 keypoints";
  return nullptr;
}
