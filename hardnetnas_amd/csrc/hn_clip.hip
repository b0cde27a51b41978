// Keypoint patch extraction on device: FDLNet's clip_patch (FDLNet-master/latency/NASNet/utils/
// image_utils.py:11-158), the step between the detector's keypoints and the descriptor forward
// (model/network.py:163-176).  A rotated, scaled 32x32 window around every keypoint is sampled from its image
// by bilinear interpolation with clamped indices; the arithmetic is hn_clip.h's, fp32 in the reference's
// operation order (this file is built without fast-math, -fno-honor-nans or contraction).
//
// One 256-thread workgroup per patch (grid-stride beyond kClipMaxGrid patches).  Thread 0 turns the keypoint's
// row, scale, orientation and ratio into the patch's affine once and hands it to the others through LDS (two
// slots, alternating, so that one barrier per patch suffices).  Thread t then owns output row t / 8, columns
// 4 (t % 8) .. + 3.  A pixel's x0 and x1 are neighbours, so each of its two image rows is one 8-byte read of a
// pixel pair (hn_clip.h): 8 gather instructions per thread through the vector cache (a patch's footprint is at
// most (2 sqrt(2) s + 2)^2 pixels, shared by its 1,024 samples).  The four pixels leave as one 16-byte store, so
// a wave writes 8 full output rows (1 KiB contiguous).  The time is set by the number of gather instructions,
// not by the 4 KiB written per patch nor by where the image lines come from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_clip.h"
#include "hn_internal.h"

namespace {

constexpr int kClipMaxGrid = 4096;  // 16 workgroups per CU: two rounds of the 8 resident ones

__global__ __launch_bounds__(256) void k_clip_patch(const float* __restrict__ images, int64_t B, int32_t H, int32_t W,
                                                    const int64_t* __restrict__ kpts, const float* __restrict__ scale,
                                                    const float* __restrict__ ori, const float* __restrict__ ratio,
                                                    int64_t n, float* __restrict__ out) {
  __shared__ hnclip::Keypoint s_kp[2];
  const int t = threadIdx.x;
  const int row = t >> 3, col = (t & 7) * 4;
  int slot = 0;
  for (int64_t p = blockIdx.x; p < n; p += gridDim.x, slot ^= 1) {
    if (t == 0) s_kp[slot] = hnclip::keypoint(kpts + p * 4, scale[p], ori ? ori + p * 2 : nullptr, ratio, B, H, W);
    __syncthreads();
    const hnclip::Keypoint k = s_kp[slot];
    hnclip::Sample s[4];
    hnclip::PixelPair top[4], bottom[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = hnclip::sample(k, row, col + j, H, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      top[j] = *reinterpret_cast<const hnclip::PixelPair*>(images + s[j].p0);
      bottom[j] = *reinterpret_cast<const hnclip::PixelPair*>(images + s[j].p1);
    }
    float4 v;
    v.x = hnclip::blend(s[0], top[0], bottom[0]);
    v.y = hnclip::blend(s[1], top[1], bottom[1]);
    v.z = hnclip::blend(s[2], top[2], bottom[2]);
    v.w = hnclip::blend(s[3], top[3], bottom[3]);
    *reinterpret_cast<float4*>(out + p * 1024 + t * 4) = v;
  }
}

}  // namespace

hipError_t hn_launch_clip(const float* images, int64_t B, int H, int W, const int64_t* kpts, const float* scale,
                          const float* ori, const float* ratio, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)std::min<int64_t>(n, kClipMaxGrid)), block(256);
  hipLaunchKernelGGL(k_clip_patch, grid, block, 0, st, images, B, (int32_t)H, (int32_t)W, kpts, scale, ori, ratio, n,
                     out);
  return hipGetLastError();
}
