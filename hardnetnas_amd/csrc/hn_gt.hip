// The homography ground-truth stage of FDLNet's training step on device: what Network.forward does between the
// detector's maps of an image pair and the patch pairs (FDLNet-master/latency/NASNet/model/network.py:23-142,
// 185-264) -- gtscore's two warps, gt_scale_orin, pair's nonzero() / masked_select and ptCltoCr.  The arithmetic is
// hn_homo.h's, fp32 in the reference's operation order (this file is built without fast-math, -fno-honor-nans or
// contraction).  Four kernels, one launch each, no workspace, no float atomics:
//
//   k_warp_score      one thread per output pixel; blockIdx.y walks the images, so the nine homography entries are
//                     uniform per workgroup and live in scalar registers.  Four gathered reads per pixel.
//   k_gt_scale_orin   one thread per output pixel, the same layout: one projection by homo12 to find q, then the
//                     six projections by homo21 at q only (the reference evaluates them at every pixel of the other
//                     image and gathers).  Two map reads (scale, orientation pair) and two coalesced stores.
//   k_mask_keypoints  one 1,024-thread workgroup per image: every wave owns a contiguous 1/16 of the image, counts
//                     its set pixels, the 16 counts are scanned once (one barrier), then every wave walks its part
//                     again with a wave-level scan and writes the rows of rank < K.  Ranks follow the raster order
//                     by construction.
//   k_project_kpts    one thread per keypoint.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_homo.h"
#include "hn_internal.h"

namespace {

constexpr int kPix = 256;        // pixels per workgroup of the two map kernels
constexpr int kMaxImagesY = 65535;
constexpr int kMaskThreads = 1024, kMaskWaves = kMaskThreads / 64;
constexpr int kMaskPer = 8;      // pixels per lane and step

struct Homo9 {
  float h[9];
};

// the nine entries of image b through uniform (scalar) loads
__device__ __forceinline__ Homo9 load_homo(const float* __restrict__ homo, int64_t b) {
  Homo9 m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.h[i] = homo[b * 9 + i];
  return m;
}

__global__ __launch_bounds__(kPix) void k_warp_score(const float* __restrict__ score, const float* __restrict__ homo,
                                                     int64_t B, int32_t H, int32_t W, int32_t border, int align,
                                                     float* __restrict__ warped, float* __restrict__ visible) {
  const int32_t hw = H * W;
  const int32_t p = blockIdx.x * kPix + threadIdx.x;
  if (p >= hw) return;
  const int32_t y = p / W, x = p - y * W;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const Homo9 m = load_homo(homo, b);
    const hnhomo::Bilinear s = hnhomo::bilinear(m.h, x, y, H, W, align);
    const float* im = score + b * hw;
    float acc = 0.0f, vis = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (s.ok[k]) {
        if (warped) {
          const float v = hnhomo::in_border(s.idx[k], H, W, border) ? 0.0f : im[s.idx[k]];
          acc = acc + v * s.w[k];
        }
        vis = vis + s.w[k];
      }
    }
    if (warped) warped[b * hw + p] = acc;
    if (visible) visible[b * hw + p] = vis;
  }
}

__global__ __launch_bounds__(kPix) void k_gt_scale_orin(const float* __restrict__ scale, float scale_value,
                                                        const float* __restrict__ ori,
                                                        const float* __restrict__ homo12,
                                                        const float* __restrict__ homo21, int64_t B, int32_t H,
                                                        int32_t W, float* __restrict__ gt_scale,
                                                        float* __restrict__ gt_ori) {
  const int32_t hw = H * W;
  const int32_t p = blockIdx.x * kPix + threadIdx.x;
  if (p >= hw) return;
  const int32_t y = p / W, x = p - y * W;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const Homo9 m12 = load_homo(homo12, b), m21 = load_homo(homo21, b);
    int32_t qx, qy;
    const int32_t q = hnhomo::gt_source(m12.h, x, y, H, W, &qx, &qy);
    const float s = scale ? scale[b * hw + q] : scale_value;
    const float2 o = *reinterpret_cast<const float2*>(ori + (b * hw + q) * 2);
    hnhomo::Point centre;
    gt_scale[b * hw + p] = hnhomo::gt_scale_at(m21.h, qx, qy, s, &centre);
    const hnhomo::Point g = hnhomo::gt_ori_at(m21.h, qx, qy, s, o.x, o.y, centre);
    *reinterpret_cast<float2*>(gt_ori + (b * hw + p) * 2) = make_float2(g.x, g.y);
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kMaskThreads) void k_mask_keypoints(
    const uint8_t* __restrict__ mask, int64_t B, int32_t H, int32_t W, int32_t K, const float* __restrict__ scale_map,
    float scale_value, const float* __restrict__ ori_map, int64_t* __restrict__ kpts, float* __restrict__ kscale,
    float* __restrict__ kori, int32_t* __restrict__ counts) {
  __shared__ int s_wave[kMaskWaves];
  const int32_t hw = H * W;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // wave w owns pixels [w seg, min((w + 1) seg, hw)), seg a multiple of the wave's step
  const int32_t step = 64 * kMaskPer;
  const int64_t seg = ((((int64_t)hw + kMaskWaves - 1) / kMaskWaves + step - 1) / step) * step;
  const int64_t lo = wave * seg, hi = lo + seg < hw ? lo + seg : hw;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const uint8_t* m = mask + b * hw;
    int n = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += step) {  // uniform per wave
      const int64_t i = i0 + lane * kMaskPer;
#pragma unroll
      for (int j = 0; j < kMaskPer; ++j)
        if (i + j < hi) n += m[i + j] != 0;
    }
    const int wave_total = __shfl(wave_inclusive_scan(n, lane), 63, 64);
    __syncthreads();  // the previous image's readers of s_wave are done
    if (lane == 0) s_wave[wave] = wave_total;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kMaskWaves; ++w) {
      const int c = s_wave[w];
      base += w < wave ? c : 0;
      total += c;
    }
    if (t == 0 && counts) counts[b] = total;
    int64_t* rows = kpts + b * K * 4;
    // rows of rank >= total: (b, 0, 0, 0), scale and orientation of pixel (0, 0)
    for (int64_t r = (int64_t)total + t; r < K; r += kMaskThreads) {
      hnhomo::keypoint_row(rows + r * 4, b, 0, W);
      kscale[b * K + r] = scale_map ? scale_map[b * hw] : scale_value;
      if (kori) {
        kori[(b * K + r) * 2] = ori_map[b * hw * 2];
        kori[(b * K + r) * 2 + 1] = ori_map[b * hw * 2 + 1];
      }
    }
    if (base >= K) continue;  // uniform per wave
    for (int64_t i0 = lo; i0 < hi && base < K; i0 += step) {  // uniform per wave: every lane takes part in the scan
      const int64_t i = i0 + lane * kMaskPer;
      uint32_t bits = 0;
#pragma unroll
      for (int j = 0; j < kMaskPer; ++j)
        if (i + j < hi && m[i + j] != 0) bits |= 1u << j;
      const int c = __popc(bits);
      const int incl = wave_inclusive_scan(c, lane);
      int r = base + incl - c;
#pragma unroll
      for (int j = 0; j < kMaskPer; ++j)
        if (bits >> j & 1u) {
          if (r < K) {
            const int32_t idx = (int32_t)(i + j);
            hnhomo::keypoint_row(rows + (int64_t)r * 4, b, idx, W);
            kscale[b * K + r] = scale_map ? scale_map[b * hw + idx] : scale_value;
            if (kori) {
              kori[(b * K + r) * 2] = ori_map[(b * hw + idx) * 2];
              kori[(b * K + r) * 2 + 1] = ori_map[(b * hw + idx) * 2 + 1];
            }
          }
          ++r;
        }
      base += __shfl(incl, 63, 64);
    }
  }
}

__global__ __launch_bounds__(256) void k_project_kpts(const int64_t* __restrict__ kpts, int64_t n,
                                                      const float* __restrict__ homo, int64_t B, int32_t H, int32_t W,
                                                      const float* __restrict__ scale_map, float scale_value,
                                                      const float* __restrict__ ori_map, int clamp,
                                                      int64_t* __restrict__ kpts_r, float* __restrict__ scale_r,
                                                      float* __restrict__ ori_r) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t* kp = kpts + i * 4;
    const int64_t row[4] = {kp[0], kp[1], kp[2], kp[3]};
    const int64_t b = hnhomo::homography_of(row, B);
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = homo[b * 9 + k];
    const hnhomo::Projected r = hnhomo::project_keypoint(row, h, B, H, W, clamp);
    kpts_r[i * 4] = r.b;
    kpts_r[i * 4 + 1] = r.y;
    kpts_r[i * 4 + 2] = r.x;
    kpts_r[i * 4 + 3] = 0;
    scale_r[i] = scale_map ? scale_map[r.gather] : scale_value;
    if (ori_r) {
      ori_r[i * 2] = ori_map[r.gather * 2];
      ori_r[i * 2 + 1] = ori_map[r.gather * 2 + 1];
    }
  }
}

dim3 map_grid(int64_t B, int H, int W) {
  const int64_t hw = (int64_t)H * W;
  return dim3((unsigned)((hw + kPix - 1) / kPix), (unsigned)std::min<int64_t>(B, kMaxImagesY));
}

}  // namespace

hipError_t hn_launch_warp_score(const float* score, const float* homo, int64_t B, int H, int W, int border,
                                int align_corners, float* warped, float* visible, hipStream_t st) {
  if (B <= 0 || (!warped && !visible)) return hipSuccess;
  hipLaunchKernelGGL(k_warp_score, map_grid(B, H, W), dim3(kPix), 0, st, score, homo, B, (int32_t)H, (int32_t)W,
                     (int32_t)border, align_corners, warped, visible);
  return hipGetLastError();
}

hipError_t hn_launch_gt_scale_orin(const float* scale, float scale_value, const float* ori, const float* homo12,
                                   const float* homo21, int64_t B, int H, int W, float* gt_scale, float* gt_ori,
                                   hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gt_scale_orin, map_grid(B, H, W), dim3(kPix), 0, st, scale, scale_value, ori, homo12, homo21, B,
                     (int32_t)H, (int32_t)W, gt_scale, gt_ori);
  return hipGetLastError();
}

hipError_t hn_launch_mask_keypoints(const uint8_t* mask, int64_t B, int H, int W, int K, const float* scale_map,
                                    float scale_value, const float* ori_map, int64_t* kpts, float* kscale, float* kori,
                                    int32_t* counts, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mask_keypoints, dim3((unsigned)std::min<int64_t>(B, 1024)), dim3(kMaskThreads), 0, st, mask, B,
                     (int32_t)H, (int32_t)W, (int32_t)K, scale_map, scale_value, ori_map, kpts, kscale, kori, counts);
  return hipGetLastError();
}

hipError_t hn_launch_project_kpts(const int64_t* kpts, int64_t n, const float* homo, int64_t B, int H, int W,
                                  const float* scale_map, float scale_value, const float* ori_map, int clamp,
                                  int64_t* kpts_r, float* scale_r, float* ori_r, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_project_kpts, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, kpts,
                     n, homo, B, (int32_t)H, (int32_t)W, scale_map, scale_value, ori_map, clamp, kpts_r, scale_r, ori_r);
  return hipGetLastError();
}
