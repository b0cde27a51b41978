// FDLNet's keypoint detector on device: eval-mode RFDet.forward of the NASNet variant
// (FDLNet-master/latency/NASNet/model/det.py:57-94) for [B,1,H,W] fp32 images, in fp32 FMA arithmetic.
//
//   features.0  conv 1 -> 16, 3x3, bias, no activation
//   features.1/2  InvertedResidual(16,16,1,benchmodel=1) (model/operations.py:449-511): channels 0..7 pass,
//               channels 8..15 through 1x1+BN+ReLU, depthwise 3x3+BN, 1x1+BN+ReLU; concat; channel_shuffle(2)
//   score head  conv 16 -> 1, 3x3, bias; InstanceNorm2d(1, affine); leaky_relu(0.01); soft_nms_3d(15, 7.0)
//   ori head    conv 16 -> 2, 3x3, bias; InstanceNorm2d(2, affine); division by the pair's L2 norm
//
// Two launches.  k_det_feat: one 256-thread workgroup per 16x16 output tile keeps the image window (halo 4), the
// 16-channel feature map (halo 3, shrinking by one per 3x3 layer) and the 8-channel branch activation in LDS,
// channel-major so that neighbouring threads read neighbouring words.  Every 3x3 layer pads its OWN input with
// zeros at the image border: every activation outside the image is stored as zero (never the folded BN bias)
// before the next stencil reads it.  The 1x1 layers run per pixel out of registers; the shuffle is the index map
// new[2j+g] = old[8g+j], done in place.  The three head convolutions write the pre-norm maps and, per workgroup,
// the fp64 sum and sum of squares of each (no float atomics: one slot per workgroup).  k_det_post: every
// workgroup (32x32 pixels) first combines its image's partials in fp64 in a fixed order (the same order whatever
// the batch, so an image's maps do not depend on its neighbours), then normalises a 60x60 score window
// (halo 14) into LDS and runs the separable 15x15 maximum (windows clipped at the image) and the separable
// 15x15 box sum of e = exp(7 (s - m)) (zero outside the image), p = e / (sum + 1e-8); the orientation pair is
// normalised and divided by its norm (IEEE division and square root, no epsilon, as the reference).
// soft_max_and_argmax_1d with the one scale of this variant is the identity on p in fp32, and the scale map is
// the constant 32: neither is materialised.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_internal.h"

namespace {

using namespace hndet;

constexpr int T = kDetTile;  // 16
constexpr int R0 = T + 8;    // image window
constexpr int R1 = T + 6;    // features.0 / block-1 branch input
constexpr int N1 = R1 * R1;

__device__ __forceinline__ bool inside(int y, int x, int H, int W) {
  return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}

// 1x1 + folded BN + ReLU on the 8 branch channels
__device__ __forceinline__ void pw8(const float* __restrict__ w, const float* __restrict__ b, const float (&x)[8],
                                    float (&y)[8]) {
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    float a = b[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) a = fmaf(w[o * 8 + i], x[i], a);
    y[o] = fmaxf(a, 0.f);
  }
}

// The tail of one InvertedResidual over the (T + 2 HALO)^2 window: depthwise 3x3 of s_t, 1x1 + ReLU, concat with
// the pass-through half and channel shuffle, in place in s_a (each thread touches only its own pixel of s_a).
template <int HALO>
__device__ __forceinline__ void block_tail(float* __restrict__ s_a, const float* __restrict__ s_t,
                                           const float* __restrict__ blk, int y0, int x0, int H, int W) {
  constexpr int R = T + 2 * HALO, OFF = 3 - HALO;
  for (int i = threadIdx.x; i < R * R; i += 256) {
    const int py = i / R + OFF, px = i % R + OFF;  // position on the R1 grid
    const int p = py * R1 + px;
    float o[8];
    if (inside(y0 - 3 + py, x0 - 3 + px, H, W)) {
      float u[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float a = blk[kBlkDwB + c];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
            a = fmaf(blk[kBlkDwW + c * 9 + ky * 3 + kx], s_t[c * N1 + p + (ky - 1) * R1 + (kx - 1)], a);
        u[c] = a;
      }
      pw8(blk + kBlkPw2W, blk + kBlkPw2B, u, o);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = 0.f;
    }
    float x1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x1[j] = s_a[j * N1 + p];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s_a[(2 * j) * N1 + p] = x1[j];
      s_a[(2 * j + 1) * N1 + p] = o[j];
    }
  }
}

// The head of one InvertedResidual: 1x1 + BN + ReLU of channels 8..15 over the same window, zero outside the image
template <int HALO>
__device__ __forceinline__ void block_head(const float* __restrict__ s_a, float* __restrict__ s_t,
                                           const float* __restrict__ blk, int y0, int x0, int H, int W) {
  constexpr int R = T + 2 * HALO, OFF = 3 - HALO;
  for (int i = threadIdx.x; i < R * R; i += 256) {
    const int py = i / R + OFF, px = i % R + OFF;
    const int p = py * R1 + px;
    float x[8], y[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = s_a[(8 + c) * N1 + p];
    pw8(blk + kBlkPw1W, blk + kBlkPw1B, x, y);
    const bool in = inside(y0 - 3 + py, x0 - 3 + px, H, W);
#pragma unroll
    for (int c = 0; c < 8; ++c) s_t[c * N1 + p] = in ? y[c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_det_feat(const float* __restrict__ images, int H, int W, int tiles_x,
                                                  int tiles, const float* __restrict__ P, float* __restrict__ raw,
                                                  double* __restrict__ part) {
  __shared__ float s_img[R0 * R0];
  __shared__ float s_a[16 * N1];
  __shared__ float s_t[8 * N1];
  __shared__ double s_red[4][6];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / tiles_x) * T, x0 = (tile % tiles_x) * T;
  const int64_t HW = (int64_t)H * W;
  const float* img = images + b * HW;

  for (int i = t; i < R0 * R0; i += 256) {
    const int y = y0 - 4 + i / R0, x = x0 - 4 + i % R0;
    s_img[i] = inside(y, x, H, W) ? img[(int64_t)y * W + x] : 0.f;
  }
  __syncthreads();
  // features.0 (halo 3) and, from registers, block 1's first 1x1
  for (int i = t; i < N1; i += 256) {
    const int py = i / R1, px = i % R1;
    float a[16], br[8];
    if (inside(y0 - 3 + py, x0 - 3 + px, H, W)) {
      float v[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) v[ky * 3 + kx] = s_img[(py + ky) * R0 + px + kx];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        float s = P[kC0B + c];
#pragma unroll
        for (int k = 0; k < 9; ++k) s = fmaf(P[kC0W + c * 9 + k], v[k], s);
        a[c] = s;
      }
      float x2[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) x2[c] = a[8 + c];
      pw8(P + kBlk + kBlkPw1W, P + kBlk + kBlkPw1B, x2, br);
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) a[c] = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) br[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) s_a[c * N1 + i] = a[c];
#pragma unroll
    for (int c = 0; c < 8; ++c) s_t[c * N1 + i] = br[c];
  }
  __syncthreads();
  block_tail<2>(s_a, s_t, P + kBlk, y0, x0, H, W);
  __syncthreads();
  block_head<2>(s_a, s_t, P + kBlk + kBlkSize, y0, x0, H, W);
  __syncthreads();
  block_tail<1>(s_a, s_t, P + kBlk + kBlkSize, y0, x0, H, W);
  __syncthreads();

  // the three head convolutions on the tile's own pixel, and this workgroup's partial statistics
  const int ty = t / T, tx = t % T;
  const int y = y0 + ty, x = x0 + tx;
  const bool in = y < H && x < W;
  float h[3] = {0.f, 0.f, 0.f};
  if (in) {
    h[0] = P[kHeadB];
    h[1] = P[kHeadB + 1];
    h[2] = P[kHeadB + 2];
    const int p = (ty + 3) * R1 + tx + 3;
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float v = s_a[c * N1 + p + (ky - 1) * R1 + (kx - 1)];
          const int k = c * 9 + ky * 3 + kx;
          h[0] = fmaf(P[kHeadW + k], v, h[0]);
          h[1] = fmaf(P[kHeadW + 144 + k], v, h[1]);
          h[2] = fmaf(P[kHeadW + 288 + k], v, h[2]);
        }
    const int64_t o = (b * 3) * HW + (int64_t)y * W + x;
    raw[o] = h[0];
    raw[o + HW] = h[1];
    raw[o + 2 * HW] = h[2];
  }
  double r[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r[k] = (double)h[k];
    r[3 + k] = (double)h[k] * (double)h[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int d = 32; d >= 1; d >>= 1) r[k] += __shfl_down(r[k], d, 64);
  if ((t & 63) == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) s_red[t >> 6][k] = r[k];
  __syncthreads();
  if (t < 6) part[((int64_t)blockIdx.x) * 6 + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
}

constexpr int T2 = kDetPostTile;  // 32
constexpr int HALO2 = 14;
constexpr int S = T2 + 2 * HALO2;  // 60: normalised score window
constexpr int SP = S + 1;
constexpr int M = T2 + 14;         // 46: maximum / exp window

__global__ __launch_bounds__(256) void k_det_post(const float* __restrict__ raw, int H, int W, int tiles_x, int tiles,
                                                  int parts, const double* __restrict__ part,
                                                  const float* __restrict__ P, float in_eps,
                                                  float* __restrict__ score, float* __restrict__ ori) {
  __shared__ double s_red[256][6];
  __shared__ float s_s[S * SP];
  __shared__ float s_h[S * M];   // row maxima [S][M]; then row sums [M][T2]
  __shared__ float s_m[M * M];   // window maxima, then e
  __shared__ float s_stat[6];    // per channel: mean, 1 / sqrt(var + eps)
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / tiles_x) * T2, x0 = (tile % tiles_x) * T2;
  const int64_t HW = (int64_t)H * W;

  // this image's statistics: partials summed in fp64, thread t takes t, t + 256, ...; then a fixed tree
  {
    double a[6] = {0, 0, 0, 0, 0, 0};
    const double* pp = part + b * parts * 6;
    for (int i = t; i < parts; i += 256)
#pragma unroll
      for (int k = 0; k < 6; ++k) a[k] += pp[(int64_t)i * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) s_red[t][k] = a[k];
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
      if (t < d)
#pragma unroll
        for (int k = 0; k < 6; ++k) s_red[t][k] += s_red[t + d][k];
      __syncthreads();
    }
    if (t < 3) {
      const double n = (double)HW;
      const double mean = s_red[0][t] / n;
      double var = s_red[0][3 + t] / n - mean * mean;  // biased; fp64: the cancellation costs ~1e-16 mean^2
      if (var < 0) var = 0;
      s_stat[t] = (float)mean;
      s_stat[3 + t] = (float)(1.0 / sqrt(var + (double)in_eps));
    }
    __syncthreads();
  }
  const float* r0 = raw + (b * 3) * HW;
  {
    const float mean = s_stat[0], rstd = s_stat[3], g = P[kInG], be = P[kInB];
    for (int i = t; i < S * S; i += 256) {
      const int y = y0 - HALO2 + i / S, x = x0 - HALO2 + i % S;
      float v = -INFINITY;  // outside the image: never the maximum (max_pool2d clips its windows)
      if (inside(y, x, H, W)) {
        v = fmaf((r0[(int64_t)y * W + x] - mean) * rstd, g, be);
        v = v > 0.f ? v : 0.01f * v;
      }
      s_s[(i / S) * SP + i % S] = v;
    }
  }
  __syncthreads();
  for (int i = t; i < S * M; i += 256) {
    const int r = i / M, c = i % M;
    float m = s_s[r * SP + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) m = fmaxf(m, s_s[r * SP + c + d]);
    s_h[i] = m;
  }
  __syncthreads();
  for (int i = t; i < M * M; i += 256) {
    const int r = i / M, c = i % M;
    float m = s_h[r * M + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) m = fmaxf(m, s_h[(r + d) * M + c]);
    const float s = s_s[(r + 7) * SP + c + 7];
    s_m[i] = s == -INFINITY ? 0.f : expf(7.0f * (s - m));  // zero padding of the box sum
  }
  __syncthreads();
  for (int i = t; i < M * T2; i += 256) {
    const int r = i / T2, c = i % T2;
    float a = s_m[r * M + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) a += s_m[r * M + c + d];
    s_h[i] = a;
  }
  __syncthreads();
  const float m1 = s_stat[1], rs1 = s_stat[4], g1 = P[kInG + 1], b1 = P[kInB + 1];
  const float m2 = s_stat[2], rs2 = s_stat[5], g2 = P[kInG + 2], b2 = P[kInB + 2];
  for (int i = t; i < T2 * T2; i += 256) {
    const int r = i / T2, c = i % T2;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    float a = s_h[r * T2 + c];
#pragma unroll
    for (int d = 1; d < 15; ++d) a += s_h[(r + d) * T2 + c];
    const int64_t o = (int64_t)y * W + x;
    score[b * HW + o] = s_m[(r + 7) * M + c + 7] / (a + 1e-8f);
    const float oc = fmaf((r0[HW + o] - m1) * rs1, g1, b1);
    const float os = fmaf((r0[2 * HW + o] - m2) * rs2, g2, b2);
    const float nrm = sqrtf(fmaf(oc, oc, os * os));
    float2 v;
    v.x = oc / nrm;
    v.y = os / nrm;
    *reinterpret_cast<float2*>(ori + (b * HW + o) * 2) = v;
  }
}

}  // namespace

int64_t hn_det_parts(int H, int W) {
  return (int64_t)((H + kDetTile - 1) / kDetTile) * ((W + kDetTile - 1) / kDetTile);
}

size_t hn_det_ws_bytes(int64_t B, int H, int W) {
  const size_t part = ((size_t)B * hn_det_parts(H, W) * 6 * sizeof(double) + 15) & ~(size_t)15;
  return part + (size_t)B * 3 * H * W * sizeof(float);
}

hipError_t hn_launch_det(const float* params, float in_eps, const float* images, int64_t B, int H, int W, float* score,
                         float* ori, void* ws, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int tx = (W + T - 1) / T, tiles = (int)hn_det_parts(H, W);
  double* part = static_cast<double*>(ws);
  const size_t part_bytes = ((size_t)B * tiles * 6 * sizeof(double) + 15) & ~(size_t)15;
  float* raw = reinterpret_cast<float*>(static_cast<char*>(ws) + part_bytes);
  hipLaunchKernelGGL(k_det_feat, dim3((unsigned)(B * tiles)), dim3(256), 0, st, images, H, W, tx, tiles, params, raw,
                     part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int tx2 = (W + T2 - 1) / T2, tiles2 = tx2 * ((H + T2 - 1) / T2);
  hipLaunchKernelGGL(k_det_post, dim3((unsigned)(B * tiles2)), dim3(256), 0, st, raw, H, W, tx2, tiles2, tiles, part,
                     params, in_eps, score, ori);
  return hipGetLastError();
}
