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
//
// k_clip_patch_backward, below it, is the backward to the keypoints' scale and orientation in the same shape
// (DESIGN.md section 24).
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

// Backward to the keypoints' scale and orientation (hn_clip.h: sample_grad / accumulate_grad / keypoint_grad), in
// the forward's shape: one workgroup per keypoint, thread t owns the same four adjacent samples, reads their
// upstream gradient as one 16-byte load and gathers the same eight pixel pairs.  The 1,024 shares of (a, b) are
// summed in a fixed order: a thread's four left to right, a butterfly over the wave's 64 lanes, then the four
// waves' sums in wave order by thread 0, which applies the chain rule and writes the keypoint's three floats.  No
// atomics: a keypoint's gradient does not depend on the grid, the batch or the call.  Two barriers per keypoint
// (affine published; wave sums published) make one LDS slot of each enough.
__global__ __launch_bounds__(256) void k_clip_patch_backward(
    const float* __restrict__ dout, const float* __restrict__ images, int64_t B, int32_t H, int32_t W,
    const int64_t* __restrict__ kpts, const float* __restrict__ scale, const float* __restrict__ ori,
    const float* __restrict__ ratio, int64_t n, float* __restrict__ dscale, float* __restrict__ dori) {
  __shared__ hnclip::Keypoint s_kp;
  __shared__ float s_red[4][2];
  const int t = threadIdx.x;
  const int row = t >> 3, col = (t & 7) * 4;
  for (int64_t p = blockIdx.x; p < n; p += gridDim.x) {
    if (t == 0) s_kp = hnclip::keypoint(kpts + p * 4, scale[p], ori ? ori + p * 2 : nullptr, ratio, B, H, W);
    __syncthreads();
    const hnclip::Keypoint k = s_kp;
    const float4 d = *reinterpret_cast<const float4*>(dout + p * 1024 + t * 4);
    hnclip::SampleGrad g[4];
    hnclip::PixelPair top[4], bottom[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = hnclip::sample_grad(k, row, col + j, H, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      top[j] = *reinterpret_cast<const hnclip::PixelPair*>(images + g[j].s.p0);
      bottom[j] = *reinterpret_cast<const hnclip::PixelPair*>(images + g[j].s.p1);
    }
    float a = 0.0f, b = 0.0f;
    hnclip::accumulate_grad(g[0], top[0], bottom[0], d.x, &a, &b);
    hnclip::accumulate_grad(g[1], top[1], bottom[1], d.y, &a, &b);
    hnclip::accumulate_grad(g[2], top[2], bottom[2], d.z, &a, &b);
    hnclip::accumulate_grad(g[3], top[3], bottom[3], d.w, &a, &b);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
    }
    if ((t & 63) == 0) {
      s_red[t >> 6][0] = a;
      s_red[t >> 6][1] = b;
    }
    __syncthreads();
    if (t == 0) {
      const float sa = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
      const float sb = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
      hnclip::keypoint_grad(kpts + p * 4, scale[p], ori ? ori + p * 2 : nullptr, ratio, B, sa, sb,
                            dscale ? dscale + p : nullptr, dori ? dori + p * 2 : nullptr);
    }
  }
}

}  // namespace

hipError_t hn_launch_clip_backward(const float* dout, const float* images, int64_t B, int H, int W,
                                   const int64_t* kpts, const float* scale, const float* ori, const float* ratio,
                                   int64_t n, float* dscale, float* dori, hipStream_t st) {
  if (n <= 0 || (!dscale && !dori)) return hipSuccess;
  const dim3 grid((unsigned)std::min<int64_t>(n, kClipMaxGrid)), block(256);
  hipLaunchKernelGGL(k_clip_patch_backward, grid, block, 0, st, dout, images, B, (int32_t)H, (int32_t)W, kpts, scale,
                     ori, ratio, n, dscale, dori);
  return hipGetLastError();
}

hipError_t hn_launch_clip(const float* images, int64_t B, int H, int W, const int64_t* kpts, const float* scale,
                          const float* ori, const float* ratio, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)std::min<int64_t>(n, kClipMaxGrid)), block(256);
  hipLaunchKernelGGL(k_clip_patch, grid, block, 0, st, images, B, (int32_t)H, (int32_t)W, kpts, scale, ori, ratio, n,
                     out);
  return hipGetLastError();
}
