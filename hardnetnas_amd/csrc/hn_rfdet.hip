// RF-Net's ten-scale keypoint detector on device: eval-mode RFDetSO.forward
// (FDLNet-master/latency/rfnet/model/rf_det_so.py, rf_det_module.py) for [B,1,H,W] fp32 images with
// ksize 3, padding 1, dilation 1, in fp32 FMA arithmetic.
//
//   level k = 1..10   pre_k = conv_k(feat_{k-1}) + bias (3x3; conv1 1 -> 16, the others 16 -> 16; feat_0 the image)
//                     h_k = leaky_relu(InstanceNorm_k(pre_k))        (affine, whole-image biased variance, eps)
//                     s_k = conv_s_k(h_k) (1x1, 16 -> 1), o_k = conv_o_k(h_k) / |conv_o_k(h_k)| (1x1, 16 -> 2)
//                     feat_1 = h_1, feat_k = h_k + feat_{k-1}: the heads read h_k BEFORE the residual
//   tail              soft_nms_3d(15, 3.0) over the ten InstanceNorm'd score maps, then the three-output
//                     soft_max_and_argmax_1d: score, scale and the re-normalised orientation
//
// Every InstanceNorm needs its whole image before one output can be formed, so a level boundary is a kernel
// boundary.  23 launches: k_rf_first (image -> pre_1), nine k_rf_mid (step k: pre_k, feat_{k-1} -> feat_k, s_k, o_k,
// pre_{k+1}), k_rf_last (level 10's heads), k_rf_tail, and after each of the eleven layer kernels one k_rf_stats
// (one workgroup per image) that turns that step's per-workgroup fp64 partial sums into the mean and
// 1 / sqrt(var + eps) the next step reads -- in a fixed order that depends on the image alone, so an image's maps
// are the same bits alone or in any batch.  No float atomics.  (Combining the partials inside every workgroup of the
// next step, as k_det_post does for its 6 values, would re-read 34 doubles x tiles per workgroup: ~3 GB of L2
// traffic per level at 8 x 480 x 640.)
//
// k_rf_mid: one 256-thread workgroup per 16 x 16 tile forms feat_k for its 18 x 18 window (zero outside the
// image: the next conv's padding) channel-major in LDS, writes feat_k, s_k, o_k for its own pixels, then runs the
// 16 -> 16 3x3 conv as an implicit GEMM on v_mfma_f32_16x16x4_f32: M = 16 pixels of one tile row, N = 16 output
// channels, K = 144 = 9 taps x 16 channels in 36 steps; a lane's 36 B operands (weights, packed in that order by
// hn_rfdet_create) stay in registers; each wave owns 4 tile rows = 4 independent accumulators.  The MFMA is an
// fmaf chain in k order, so the arithmetic class is hn_det.hip's.  Intermediates are fp32 channels-last [B,H,W,16].
//
// Every index below goes through hn_rfdet.h (win_y / win_x / win_own / pixel / lds_a_index / mfma_weight_index / plan).
// hn_rfdet_host_check.cpp (`make rfdet_check`) is a hand-written mirror of these kernels' loops over those helpers
// under the sanitizers: a change to a loop bound, a window or a buffer here must be made there too, and an index
// formed here without the header is one the check cannot see.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_internal.h"
#include "hn_rfdet.h"

namespace {

using namespace hnrf;
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : 0.01f * v; }

// h = leaky_relu(InstanceNorm(pre)) of one pixel: st = mean[16], rstd[16]; L = the level's parameter record
__device__ __forceinline__ void form_h(const float* __restrict__ pre, const float* __restrict__ st,
                                       const float* __restrict__ L, float (&h)[16]) {
  const float4* p4 = reinterpret_cast<const float4*>(pre);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = p4[q];
    const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = q * 4 + j;
      h[c] = lrelu(fmaf((a[j] - st[c]) * st[16 + c], L[kInG + c], L[kInB + c]));
    }
  }
}

// the two 1x1 heads of one pixel: the raw score and the unit orientation
__device__ __forceinline__ float heads(const float (&h)[16], const float* __restrict__ L, float2& o) {
  float s = L[kSB], oc = L[kOB], os = L[kOB + 1];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    s = fmaf(L[kSW + c], h[c], s);
    oc = fmaf(L[kOW + c], h[c], oc);
    os = fmaf(L[kOW + 16 + c], h[c], os);
  }
  const float nrm = sqrtf(fmaf(oc, oc, os * os));
  o.x = oc / nrm;
  o.y = os / nrm;
  return s;
}

// the workgroup's sum and sum of squares of the raw score: -> part_s[2]
__device__ __forceinline__ void reduce_s(double ssum, double ssq, double (*s_reds)[2], double* __restrict__ part_s) {
  const int t = threadIdx.x;
  for (int d = 32; d >= 1; d >>= 1) {
    ssum += __shfl_down(ssum, d, 64);
    ssq += __shfl_down(ssq, d, 64);
  }
  if ((t & 63) == 0) {
    s_reds[t >> 6][0] = ssum;
    s_reds[t >> 6][1] = ssq;
  }
  __syncthreads();
  if (t < 2) part_s[t] = ((s_reds[0][t] + s_reds[1][t]) + s_reds[2][t]) + s_reds[3][t];
}

__global__ __launch_bounds__(256) void k_rf_first(const float* __restrict__ images, int H, int W, int ntx, int tiles,
                                                  const float* __restrict__ P, float* __restrict__ pre_out,
                                                  double* __restrict__ part_pre) {
  __shared__ float s_img[kWinN];
  __shared__ double s_red[4][32];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / ntx) * kT, x0 = (tile % ntx) * kT;
  const float* img = images + b * (int64_t)H * W;
  for (int i = t; i < kWinN; i += 256) {
    const int y = win_y(y0, i), x = win_x(x0, i);
    s_img[i] = inside(y, x, H, W) ? img[(int64_t)y * W + x] : 0.f;
  }
  __syncthreads();
  const int ty = t / kT, tx = t % kT;
  const int y = y0 + ty, x = x0 + tx;
  float a[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) a[c] = 0.f;
  if (y < H && x < W) {
    float v[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) v[ky * 3 + kx] = s_img[(ty + ky) * kWin + tx + kx];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      float s = P[kConvB + c];
#pragma unroll
      for (int k = 0; k < 9; ++k) s = fmaf(P[kConvW + c * 9 + k], v[k], s);
      a[c] = s;
    }
    float4* o4 = reinterpret_cast<float4*>(pre_out + pixel(b, y, x, H, W) * kC);
#pragma unroll
    for (int q = 0; q < 4; ++q) o4[q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    double r = (double)a[c], rr = r * r;  // a pixel outside the image contributes zeros
    for (int d = 32; d >= 1; d >>= 1) {
      r += __shfl_down(r, d, 64);
      rr += __shfl_down(rr, d, 64);
    }
    if ((t & 63) == 0) {
      s_red[t >> 6][c] = r;
      s_red[t >> 6][16 + c] = rr;
    }
  }
  __syncthreads();
  if (t < 32)
    part_pre[(int64_t)blockIdx.x * kPartPre + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
}

// step k = 1..9.  L: level k's parameter record, Ln: level k + 1's.  feat_in is null for k = 1, feat_out for k = 9.
__global__ __launch_bounds__(256) void k_rf_mid(const float* __restrict__ pre_in, const float* __restrict__ feat_in,
                                                int H, int W, int ntx, int tiles, const float* __restrict__ statf,
                                                const float* __restrict__ L, const float* __restrict__ Ln,
                                                float* __restrict__ feat_out, float* __restrict__ sraw,
                                                float* __restrict__ ounit, float* __restrict__ pre_out,
                                                double* __restrict__ part_pre, double* __restrict__ part_s) {
  __shared__ float s_f[kLdsFloats];
  __shared__ double s_red[4][32];
  __shared__ double s_reds[4][2];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / ntx) * kT, x0 = (tile % ntx) * kT;
  const float* st = statf + b * (kSlots * kStatFloats);
  double ssum = 0.0, ssq = 0.0;
  for (int i = t; i < kWinN; i += 256) {
    const int y = win_y(y0, i), x = win_x(x0, i);
    float f[16];
    if (inside(y, x, H, W)) {
      const int64_t p = pixel(b, y, x, H, W);
      float h[16];
      form_h(pre_in + p * kC, st, L, h);
      if (feat_in) {
        const float4* f4 = reinterpret_cast<const float4*>(feat_in + p * kC);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = f4[q];
          f[4 * q] = h[4 * q] + v.x;
          f[4 * q + 1] = h[4 * q + 1] + v.y;
          f[4 * q + 2] = h[4 * q + 2] + v.z;
          f[4 * q + 3] = h[4 * q + 3] + v.w;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 16; ++c) f[c] = h[c];
      }
      if (win_own(i)) {
        if (feat_out) {
          float4* o4 = reinterpret_cast<float4*>(feat_out + p * kC);
#pragma unroll
          for (int q = 0; q < 4; ++q) o4[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
        }
        float2 o;
        const float s = heads(h, L, o);
        sraw[p] = s;
        *reinterpret_cast<float2*>(ounit + p * 2) = o;
        ssum += (double)s;
        ssq += (double)s * (double)s;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) f[c] = 0.f;  // the next conv pads its own input with zeros
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) s_f[c * kPlane + i] = f[c];
  }
  __syncthreads();

  // pre_{k+1} = conv_{k+1}(feat_k) + bias: D[pixel m][channel n] += A[m][k] B[k][n], 36 k-steps of 4
  const int lane = t & 63, wave = t >> 6, n = lane & 15;
  float bw[36];
#pragma unroll
  for (int s = 0; s < 36; ++s) bw[s] = Ln[kConvW + s * 64 + lane];
  const float bias = Ln[kConvB + n];
  f32x4 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = f32x4{bias, bias, bias, bias};
#pragma unroll
  for (int s = 0; s < 36; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_f[lds_a_index(s, lane, wave * 4 + r)], bw[s], acc[r], 0, 0, 0);

  // lane holds channel n of pixels (row wave * 4 + r, column (lane >> 4) * 4 + j)
  double ps = 0.0, pq = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = y0 + wave * 4 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + (lane >> 4) * 4 + j;
      if (y < H && x < W) {
        const float v = acc[r][j];
        pre_out[pixel(b, y, x, H, W) * kC + n] = v;
        ps += (double)v;
        pq += (double)v * (double)v;
      }
    }
  }
  ps += __shfl_xor(ps, 16, 64);
  pq += __shfl_xor(pq, 16, 64);
  ps += __shfl_xor(ps, 32, 64);
  pq += __shfl_xor(pq, 32, 64);
  if (lane < 16) {
    s_red[wave][lane] = ps;
    s_red[wave][16 + lane] = pq;
  }
  reduce_s(ssum, ssq, s_reds, part_s + (int64_t)blockIdx.x * kPartS);  // has the __syncthreads s_red needs
  if (t < 32)
    part_pre[(int64_t)blockIdx.x * kPartPre + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
}

// step 10: level 10's heads alone
__global__ __launch_bounds__(256) void k_rf_last(const float* __restrict__ pre_in, int H, int W, int ntx, int tiles,
                                                 const float* __restrict__ statf, const float* __restrict__ L,
                                                 float* __restrict__ sraw, float* __restrict__ ounit,
                                                 double* __restrict__ part_s) {
  __shared__ double s_reds[4][2];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y = (tile / ntx) * kT + t / kT, x = (tile % ntx) * kT + t % kT;
  const float* st = statf + b * (kSlots * kStatFloats);
  double ssum = 0.0, ssq = 0.0;
  if (y < H && x < W) {
    const int64_t p = pixel(b, y, x, H, W);
    float h[16];
    form_h(pre_in + p * kC, st, L, h);
    float2 o;
    const float s = heads(h, L, o);
    sraw[p] = s;
    *reinterpret_cast<float2*>(ounit + p * 2) = o;
    ssum = (double)s;
    ssq = (double)s * (double)s;
  }
  reduce_s(ssum, ssq, s_reds, part_s + (int64_t)blockIdx.x * kPartS);
}

// One 1,024-thread workgroup per image: the partials of one step, thread (c, v) summing workgroups c, c + 32, ... of
// value v in four interleaved accumulators (four loads in flight; combined in a fixed order), then the 32 chunks in
// order; mean and 1 / sqrt(biased var + eps) in fp64.  The order depends on the tile count alone.  part_pre /
// part_s may be null.
constexpr int kStatChunks = 32;

__device__ __forceinline__ double chunk_sum(const double* __restrict__ pp, int stride, int v, int c, int tiles) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = c;
  for (; i + 3 * kStatChunks < tiles; i += 4 * kStatChunks) {
    a0 += pp[(int64_t)i * stride + v];
    a1 += pp[(int64_t)(i + kStatChunks) * stride + v];
    a2 += pp[(int64_t)(i + 2 * kStatChunks) * stride + v];
    a3 += pp[(int64_t)(i + 3 * kStatChunks) * stride + v];
  }
  for (; i < tiles; i += kStatChunks) a0 += pp[(int64_t)i * stride + v];
  return ((a0 + a1) + a2) + a3;
}

__global__ __launch_bounds__(1024) void k_rf_stats(const double* __restrict__ part_pre,
                                                   const double* __restrict__ part_s, int tiles, double n,
                                                   float in_eps, float* __restrict__ stat_slot) {
  __shared__ double s_red[kStatChunks][32];
  __shared__ double s_r2[kStatChunks][2];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  float* st = stat_slot + b * (kSlots * kStatFloats);
  if (part_pre) s_red[t >> 5][t & 31] = chunk_sum(part_pre + b * tiles * kPartPre, kPartPre, t & 31, t >> 5, tiles);
  if (part_s && t < 2 * kStatChunks)
    s_r2[t >> 1][t & 1] = chunk_sum(part_s + b * tiles * kPartS, kPartS, t & 1, t >> 1, tiles);
  __syncthreads();
  double sum = 0.0, sq = 0.0;
  int at = -1;
  if (part_pre && t < 16) {
    for (int c = 0; c < kStatChunks; ++c) {
      sum += s_red[c][t];
      sq += s_red[c][16 + t];
    }
    at = t;
  } else if (part_s && t == 16) {
    for (int c = 0; c < kStatChunks; ++c) {
      sum += s_r2[c][0];
      sq += s_r2[c][1];
    }
    at = 32;
  }
  if (at >= 0) {
    const double mean = sum / n;
    double var = sq / n - mean * mean;  // biased; fp64: the cancellation costs ~1e-16 mean^2
    if (var < 0) var = 0;
    st[at] = (float)mean;
    st[at + (at == 32 ? 1 : 16)] = (float)(1.0 / sqrt(var + (double)in_eps));
  }
}

__device__ __forceinline__ float norm_s(float raw, const float (&q)[4]) {
  return fmaf((raw - q[0]) * q[1], q[2], q[3]);
}

__global__ __launch_bounds__(256) void k_rf_tail(const float* __restrict__ sraw, const float* __restrict__ ounit,
                                                 int64_t level_stride, int H, int W, int ntx, int tiles,
                                                 const float* __restrict__ statf, const float* __restrict__ P,
                                                 float cs1, float cs2, float* __restrict__ score,
                                                 float* __restrict__ scale, float* __restrict__ ori) {
  __shared__ float s_s[kS * kSP];
  __shared__ float s_h[kS * kM];   // row maxima [kS][kM]; then row sums [kM][kT2]
  __shared__ float s_m[kM * kM];   // the 15 x 15 x 10 maximum
  __shared__ float s_e[kM * kM];   // sum over levels of e
  __shared__ float s_n[kLevels][4];  // per level: mean, 1 / sqrt(var + eps), insnorm_s weight, bias
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / ntx) * kT2, x0 = (tile % ntx) * kT2;
  const int64_t HW = (int64_t)H * W;
  if (t < kLevels) {
    const float* st = statf + (b * kSlots + t + 1) * kStatFloats;
    s_n[t][0] = st[32];
    s_n[t][1] = st[33];
    s_n[t][2] = P[t * kLevelStride + kSG];
    s_n[t][3] = P[t * kLevelStride + kSBeta];
  }
  for (int i = t; i < kM * kM; i += 256) {
    s_m[i] = -INFINITY;
    s_e[i] = 0.f;
  }
  __syncthreads();
  for (int k = 0; k < kLevels; ++k) {
    const float* r0 = sraw + k * level_stride + b * HW;
    const float q[4] = {s_n[k][0], s_n[k][1], s_n[k][2], s_n[k][3]};
    for (int i = t; i < kS * kS; i += 256) {
      const int y = y0 - kHalo2 + i / kS, x = x0 - kHalo2 + i % kS;
      // outside the image: never the maximum (max_pool2d clips its windows)
      s_s[(i / kS) * kSP + i % kS] = inside(y, x, H, W) ? norm_s(r0[(int64_t)y * W + x], q) : -INFINITY;
    }
    __syncthreads();
    for (int i = t; i < kS * kM; i += 256) {
      const int r = i / kM, c = i % kM;
      float m = s_s[r * kSP + c];
#pragma unroll
      for (int d = 1; d < 15; ++d) m = fmaxf(m, s_s[r * kSP + c + d]);
      s_h[i] = m;
    }
    __syncthreads();
    for (int i = t; i < kM * kM; i += 256) {
      const int r = i / kM, c = i % kM;
      float m = s_m[i];
#pragma unroll
      for (int d = 0; d < 15; ++d) m = fmaxf(m, s_h[(r + d) * kM + c]);
      s_m[i] = m;
    }
    // the next level's fill of s_s follows this level's last read of it (a barrier back); its row pass writes
    // s_h only after the barrier behind that fill
  }
  // e = exp(3 (x - m)) summed over the levels, zero outside the image (the box sum's zero padding)
  for (int i = t; i < kM * kM; i += 256) {
    const int y = y0 - 7 + i / kM, x = x0 - 7 + i % kM;
    if (!inside(y, x, H, W)) continue;
    const float m = s_m[i];
    float e = 0.f;
    for (int k = 0; k < kLevels; ++k) {
      const float q[4] = {s_n[k][0], s_n[k][1], s_n[k][2], s_n[k][3]};
      e += expf(3.0f * (norm_s(sraw[k * level_stride + b * HW + (int64_t)y * W + x], q) - m));
    }
    s_e[i] = e;
  }
  __syncthreads();
  for (int i = t; i < kM * kT2; i += 256) {
    const int r = i / kT2, c = i % kT2;
    float a = s_e[r * kM + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) a += s_e[r * kM + c + d];
    s_h[i] = a;
  }
  __syncthreads();
  for (int i = t; i < kT2 * kT2; i += 256) {
    const int r = i / kT2, c = i % kT2;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    float a = s_h[r * kT2 + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) a += s_h[(r + d) * kT2 + c];
    const float den = a + 1e-8f, m = s_m[(r + 7) * kM + c + 7];
    const int64_t o = b * HW + (int64_t)y * W + x;
    float p[kLevels], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kLevels; ++k) {
      const float q[4] = {s_n[k][0], s_n[k][1], s_n[k][2], s_n[k][3]};
      p[k] = expf(3.0f * (norm_s(sraw[k * level_stride + o], q) - m)) / den;
      mx = fmaxf(mx, p[k]);
    }
    // soft_max_and_argmax_1d over the ten levels
    float e1[kLevels], e2[kLevels], t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int k = 0; k < kLevels; ++k) {
      e1[k] = expf(cs1 * (p[k] - mx));
      e2[k] = expf(cs2 * (p[k] - mx));
      t1 += e1[k];
      t2 += e2[k];
    }
    t1 += 1e-8f;
    t2 += 1e-8f;
    float sc = 0.f, sl = 0.f, oc = 0.f, os = 0.f;
#pragma unroll
    for (int k = 0; k < kLevels; ++k) {
      const float w1 = e1[k] / t1, w2 = e2[k] / t2;
      const float2 ok = *reinterpret_cast<const float2*>(ounit + (k * level_stride + o) * 2);
      sc = fmaf(p[k], w1, sc);
      sl = fmaf(P[kScaleList + k], w2, sl);
      oc = fmaf(ok.x, w1, oc);
      os = fmaf(ok.y, w1, os);
    }
    score[o] = sc;
    scale[o] = sl;
    const float nrm = sqrtf(fmaf(oc, oc, os * os));
    float2 v;
    v.x = oc / nrm;
    v.y = os / nrm;
    *reinterpret_cast<float2*>(ori + o * 2) = v;
  }
}

}  // namespace

int64_t hn_rfdet_parts(int H, int W) { return hnrf::tiles(H, W); }

size_t hn_rfdet_ws_bytes(int64_t B, int H, int W) { return hnrf::plan(B, H, W).total; }

hipError_t hn_launch_rfdet(const float* params, float in_eps, float cs1, float cs2, const float* images, int64_t B,
                           int H, int W, float* score, float* scale, float* ori, void* ws, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const Plan pl = plan(B, H, W);
  char* base = static_cast<char*>(ws);
  float* statf = reinterpret_cast<float*>(base + pl.stat);
  double* part_pre = reinterpret_cast<double*>(base + pl.part_pre);
  double* part_s = reinterpret_cast<double*>(base + pl.part_s);
  float* pre[2] = {reinterpret_cast<float*>(base + pl.pre[0]), reinterpret_cast<float*>(base + pl.pre[1])};
  float* feat[2] = {reinterpret_cast<float*>(base + pl.feat[0]), reinterpret_cast<float*>(base + pl.feat[1])};
  float* sraw = reinterpret_cast<float*>(base + pl.sraw);
  float* ounit = reinterpret_cast<float*>(base + pl.ounit);
  const int ntx = tiles_x(W), nt = (int)tiles(H, W);
  const int64_t wg = B * nt, n = B * (int64_t)H * W;
  const dim3 grid((unsigned)wg), blk(256);
  const double npix = (double)H * (double)W;
  hipError_t e;
  // slot j of the partials and of the statistics: what step j produced (hn_rfdet.h)
  auto stats = [&](int j) {
    hipLaunchKernelGGL(k_rf_stats, dim3((unsigned)B), dim3(1024), 0, st,
                       j < kLevels ? part_pre + (int64_t)j * wg * kPartPre : (const double*)nullptr,
                       j >= 1 ? part_s + (int64_t)(j - 1) * wg * kPartS : (const double*)nullptr, nt, npix, in_eps,
                       statf + j * kStatFloats);
    return hipGetLastError();
  };
  hipLaunchKernelGGL(k_rf_first, grid, blk, 0, st, images, H, W, ntx, nt, params, pre[0], part_pre);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = stats(0)) != hipSuccess) return e;
  for (int k = 1; k < kLevels; ++k) {  // pre_k lives in pre[(k - 1) & 1], feat_k in feat[k & 1]
    hipLaunchKernelGGL(k_rf_mid, grid, blk, 0, st, pre[(k - 1) & 1], k >= 2 ? feat[(k - 1) & 1] : (const float*)nullptr,
                       H, W, ntx, nt, statf + (k - 1) * kStatFloats, params + (k - 1) * kLevelStride,
                       params + k * kLevelStride, k < kLevels - 1 ? feat[k & 1] : (float*)nullptr,
                       sraw + (int64_t)(k - 1) * n, ounit + (int64_t)(k - 1) * n * 2, pre[k & 1],
                       part_pre + (int64_t)k * wg * kPartPre, part_s + (int64_t)(k - 1) * wg * kPartS);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = stats(k)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_rf_last, grid, blk, 0, st, pre[(kLevels - 1) & 1], H, W, ntx, nt,
                     statf + (kLevels - 1) * kStatFloats, params + (kLevels - 1) * kLevelStride,
                     sraw + (int64_t)(kLevels - 1) * n, ounit + (int64_t)(kLevels - 1) * n * 2,
                     part_s + (int64_t)(kLevels - 1) * wg * kPartS);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = stats(kLevels)) != hipSuccess) return e;
  const int ntx2 = (W + kT2 - 1) / kT2, nt2 = (int)tiles2(H, W);
  hipLaunchKernelGGL(k_rf_tail, dim3((unsigned)(B * nt2)), blk, 0, st, sraw, ounit, n, H, W, ntx2, nt2, statf, params,
                     cs1, cs2, score, scale, ori);
  return hipGetLastError();
}
