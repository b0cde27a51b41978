// FDLNet's keypoint detector in train(): RFDet.forward of the NASNet variant (FDLNet-master/latency/NASNet/
// model/det.py:57-94) with every BatchNorm on the batch's statistics, and its backward to every parameter
// (no image gradient), in fp32 FMA arithmetic.  DESIGN section 25 has the mathematics.
//
// One kernel per statistics barrier, one thread per pixel, activations planar ([channel][n H W]) in global memory:
// at the training shape (1 x 240 x 320) every plane lives in L2 and the step is bound by its launch count, not by
// its traffic, so the stencils read their neighbours from global memory (bounds-checked, zero / -inf padding
// decided per tap) instead of staging halos in LDS.  Every sum over pixels -- BatchNorm and InstanceNorm
// statistics, their backward sums, every weight and bias gradient -- is accumulated per thread in fp64, reduced per
// workgroup in a fixed tree into one slot of `part` ([column][workgroup]), and combined by a finalising kernel whose
// lanes walk the workgroups in a fixed order: no atomics, so outputs, running statistics and gradients are
// bit-identical call to call.
//
// Forward (19 launches): conv0 + block 1's first 1x1 | BN | depthwise | BN | 1x1 | BN | block output + block 2's
// first 1x1 | BN | depthwise | BN | 1x1 | BN | feature map | heads | IN | normalise + orientation | window maximum,
// arg-max and e | box sum and score.  `saved` keeps the pre-norm activations (95 floats per pixel) and the
// statistics.  Backward mirrors it: each norm's "apply" is fused into the next layer's "reduce".
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_internal.h"

namespace {

struct Geo {
  int H, W, bpi;   // bpi: workgroups per image (each strides over its image's pixels)
  int nblk;        // n_images * bpi: rows of `part`
  int64_t HW, NP;  // pixels per image, pixels in the call
  double N;        // NP as the BatchNorm count
};

// planes of `saved` (after the statistics) and of `scratch` (after the partial sums and coefficients)
enum { SV_F0 = 0, SV_Z = 16, SV_X2 = 64, SV_F2 = 72, SV_RAW = 88, SV_XS = 91, SV_E = 92, SV_S = 93, SV_A = 94,
       SV_PLANES = 95 };
enum { SC_T = 0, SC_U = 1, SC_DY = 2, SC_DH = 5, SC_DFA = 8, SC_DFB = 24, SC_D8A = 40, SC_D8B = 48, SC_PLANES = 56 };
constexpr int kPartCols = 432;  // widest reduction: the head convolutions' weight gradient
constexpr int kBnStats = 96;    // 6 BatchNorms x (mean[8], rstd[8])
constexpr int kCoefBn = 24;     // per BatchNorm backward: gamma * rstd [8], mean(dy) [8], mean(dy xhat) [8]

__device__ __forceinline__ bool inside(int y, int x, int H, int W) {
  return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}

// this workgroup's sums -> part[k * nblk + blockIdx.x]; every thread of the 256 calls it
template <int K>
__device__ __forceinline__ void reduce_store(double (&r)[K], double* __restrict__ part, int nblk, int col0) {
  __shared__ double s_red[4][K];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = r[k];
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
    if ((t & 63) == 0) s_red[t >> 6][k] = a;
  }
  __syncthreads();
  for (int k = t; k < K; k += 256)
    part[(int64_t)(col0 + k) * nblk + blockIdx.x] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
}

// one wave's sum of a column's rows [row0, row0 + rows): lanes stride the rows, then a fixed tree; valid in lane 0
__device__ __forceinline__ double wave_colsum(const double* __restrict__ part, int nblk, int col, int row0, int rows) {
  const int lane = threadIdx.x & 63;
  double a = 0;
  const double* p = part + (int64_t)col * nblk + row0;
  for (int r = lane; r < rows; r += 64) a += p[r];
  for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
  return a;
}

struct Bn {
  float m[8], r[8], g[8], b[8];
};
__device__ __forceinline__ void load_bn(Bn& n, const float* __restrict__ st, const float* __restrict__ gam,
                                        const float* __restrict__ bet) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    n.m[c] = st[c];
    n.r[c] = st[8 + c];
    n.g[c] = gam[c];
    n.b[c] = bet[c];
  }
}
struct Coef {
  float a[8], m1[8], m2[8];
};
__device__ __forceinline__ void load_coef(Coef& k, const float* __restrict__ c) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k.a[i] = c[i];
    k.m1[i] = c[8 + i];
    k.m2[i] = c[16 + i];
  }
}

#define PIXEL_LOOP                                                      \
  const int64_t b = blockIdx.x / g.bpi;                                 \
  const int64_t step = (int64_t)g.bpi * 256;                            \
  for (int64_t i = (int64_t)(blockIdx.x % g.bpi) * 256 + threadIdx.x; i < g.HW; i += step)

// ------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------
// features.0 (3x3, bias) -> F0; block 1's first 1x1 -> z; sums of z and z^2
__global__ __launch_bounds__(256) void k_f_conv0(Geo g, const float* __restrict__ img, const float* __restrict__ w0,
                                                 const float* __restrict__ b0, const float* __restrict__ w1,
                                                 float* __restrict__ F0, float* __restrict__ Z, double* __restrict__ part) {
  double r[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const float* im = img + b * g.HW;
    const int64_t pix = b * g.HW + i;
    float v[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        v[ky * 3 + kx] = inside(yy, xx, g.H, g.W) ? im[(int64_t)yy * g.W + xx] : 0.f;
      }
    float a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      float s = b0[c];
#pragma unroll
      for (int k = 0; k < 9; ++k) s = fmaf(w0[c * 9 + k], v[k], s);
      a[c] = s;
      F0[c * g.NP + pix] = s;
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float z = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) z = fmaf(w1[o * 8 + c], a[8 + c], z);
      Z[o * g.NP + pix] = z;
      r[o] += (double)z;
      r[8 + o] += (double)z * (double)z;
    }
  }
  reduce_store<16>(r, part, g.nblk, 0);
}

// BN + ReLU of zin at the nine taps (zero outside the image), depthwise 3x3 -> zout; its sums
__global__ __launch_bounds__(256) void k_f_dw(Geo g, const float* __restrict__ Zin, const float* __restrict__ st,
                                              const float* __restrict__ gam, const float* __restrict__ bet,
                                              const float* __restrict__ wdw, float* __restrict__ Zout,
                                              double* __restrict__ part) {
  Bn n;
  load_bn(n, st, gam, bet);
  double r[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t base = b * g.HW;
    float z[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) z[c] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        if (!inside(yy, xx, g.H, g.W)) continue;
        const int64_t p = base + (int64_t)yy * g.W + xx;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float y1 = fmaxf(fmaf((Zin[c * g.NP + p] - n.m[c]) * n.r[c], n.g[c], n.b[c]), 0.f);
          z[c] = fmaf(wdw[c * 9 + ky * 3 + kx], y1, z[c]);
        }
      }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      Zout[c * g.NP + base + i] = z[c];
      r[c] += (double)z[c];
      r[8 + c] += (double)z[c] * (double)z[c];
    }
  }
  reduce_store<16>(r, part, g.nblk, 0);
}

// BN (no activation) of zin, 1x1 -> zout; its sums
__global__ __launch_bounds__(256) void k_f_pw2(Geo g, const float* __restrict__ Zin, const float* __restrict__ st,
                                               const float* __restrict__ gam, const float* __restrict__ bet,
                                               const float* __restrict__ w, float* __restrict__ Zout,
                                               double* __restrict__ part) {
  Bn n;
  load_bn(n, st, gam, bet);
  double r[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    float y2[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) y2[c] = fmaf((Zin[c * g.NP + pix] - n.m[c]) * n.r[c], n.g[c], n.b[c]);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float z = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) z = fmaf(w[o * 8 + c], y2[c], z);
      Zout[o * g.NP + pix] = z;
      r[o] += (double)z;
      r[8 + o] += (double)z * (double)z;
    }
  }
  reduce_store<16>(r, part, g.nblk, 0);
}

// block 1's output (BN + ReLU of z3, concat, shuffle: F1[2j] = F0[j], F1[2j+1] = y3[j]); block 2's branch input
// F1[8..15] -> X2; block 2's first 1x1 -> z; its sums
__global__ __launch_bounds__(256) void k_f_next(Geo g, const float* __restrict__ F0, const float* __restrict__ Z3,
                                                const float* __restrict__ st, const float* __restrict__ gam,
                                                const float* __restrict__ bet, const float* __restrict__ w1,
                                                float* __restrict__ X2, float* __restrict__ Z, double* __restrict__ part) {
  Bn n;
  load_bn(n, st, gam, bet);
  double r[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    float x2[8];
#pragma unroll
    for (int j = 4; j < 8; ++j) {
      x2[2 * (j - 4)] = F0[j * g.NP + pix];
      x2[2 * (j - 4) + 1] = fmaxf(fmaf((Z3[j * g.NP + pix] - n.m[j]) * n.r[j], n.g[j], n.b[j]), 0.f);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) X2[c * g.NP + pix] = x2[c];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float z = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) z = fmaf(w1[o * 8 + c], x2[c], z);
      Z[o * g.NP + pix] = z;
      r[o] += (double)z;
      r[8 + o] += (double)z * (double)z;
    }
  }
  reduce_store<16>(r, part, g.nblk, 0);
}

// the 16-channel feature map the heads read: F2[2j] = F1[j], F2[2j+1] = y3 of block 2
__global__ __launch_bounds__(256) void k_f_feat(Geo g, const float* __restrict__ F0, const float* __restrict__ Z3a,
                                                const float* __restrict__ sta, const float* __restrict__ ga,
                                                const float* __restrict__ ba, const float* __restrict__ Z3b,
                                                const float* __restrict__ stb, const float* __restrict__ gb,
                                                const float* __restrict__ bb, float* __restrict__ F2) {
  Bn na, nb;
  load_bn(na, sta, ga, ba);
  load_bn(nb, stb, gb, bb);
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // F1[j]: even j is F0[j / 2], odd j is block 1's y3[j / 2]
      const int h = j >> 1;
      const float f1 = (j & 1) ? fmaxf(fmaf((Z3a[h * g.NP + pix] - na.m[h]) * na.r[h], na.g[h], na.b[h]), 0.f)
                               : F0[h * g.NP + pix];
      F2[(2 * j) * g.NP + pix] = f1;
      F2[(2 * j + 1) * g.NP + pix] =
          fmaxf(fmaf((Z3b[j * g.NP + pix] - nb.m[j]) * nb.r[j], nb.g[j], nb.b[j]), 0.f);
    }
  }
}

// the three head convolutions (score, cos, sin) -> raw; per-image sums of each and of its square
__global__ __launch_bounds__(256) void k_f_heads(Geo g, const float* __restrict__ F2, const float* __restrict__ ws,
                                                 const float* __restrict__ bs, const float* __restrict__ wo,
                                                 const float* __restrict__ bo, float* __restrict__ raw,
                                                 double* __restrict__ part) {
  double r[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t base = b * g.HW;
    // one accumulator per tap over the 16 channels, then the nine taps: 16 + 9 roundings deep instead of 144
    float h0 = bs[0], h1 = bo[0], h2 = bo[1];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        if (!inside(yy, xx, g.H, g.W)) continue;
        const int64_t p = base + (int64_t)yy * g.W + xx;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const float v = F2[c * g.NP + p];
          const int k = c * 9 + ky * 3 + kx;
          t0 = fmaf(ws[k], v, t0);
          t1 = fmaf(wo[k], v, t1);
          t2 = fmaf(wo[144 + k], v, t2);
        }
        h0 += t0;
        h1 += t1;
        h2 += t2;
      }
    raw[base + i] = h0;
    raw[g.NP + base + i] = h1;
    raw[2 * g.NP + base + i] = h2;
    r[0] += (double)h0;
    r[1] += (double)h1;
    r[2] += (double)h2;
    r[3] += (double)h0 * (double)h0;
    r[4] += (double)h1 * (double)h1;
    r[5] += (double)h2 * (double)h2;
  }
  reduce_store<6>(r, part, g.nblk, 0);
}

// BatchNorm statistics of the call (one workgroup of 16 waves, wave k sums column k): mean and 1 / sqrt(biased
// variance + eps) -> st; the running statistics move by `mom` (unbiased variance)
__global__ __launch_bounds__(1024) void k_fin_bn(Geo g, const double* __restrict__ part, float eps, float mom,
                                                 float* __restrict__ rm, float* __restrict__ rv, float* __restrict__ st) {
  __shared__ double s[16];
  const int wave = threadIdx.x >> 6;
  const double a = wave_colsum(part, g.nblk, wave, 0, g.nblk);
  if ((threadIdx.x & 63) == 0) s[wave] = a;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 8) {
    const double mean = s[t] / g.N;
    double var = s[8 + t] / g.N - mean * mean;  // fp64: the cancellation costs ~1e-16 mean^2
    if (var < 0) var = 0;
    st[t] = (float)mean;
    st[8 + t] = (float)(1.0 / sqrt(var + (double)eps));
    const double m = (double)mom;
    rm[t] = (float)((1.0 - m) * (double)rm[t] + m * mean);
    rv[t] = (float)((1.0 - m) * (double)rv[t] + m * (var * g.N / (g.N - 1.0)));
  }
}

// InstanceNorm statistics: one workgroup per image, waves 0..5 one column each over the image's own workgroups
__global__ __launch_bounds__(512) void k_fin_in(Geo g, const double* __restrict__ part, float eps,
                                                float* __restrict__ st) {
  __shared__ double s[8];
  const int wave = threadIdx.x >> 6;
  if (wave < 6) {
    const double a = wave_colsum(part, g.nblk, wave, blockIdx.x * g.bpi, g.bpi);
    if ((threadIdx.x & 63) == 0) s[wave] = a;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 3) {
    const double n = (double)g.HW;
    const double mean = s[t] / n;
    double var = s[3 + t] / n - mean * mean;
    if (var < 0) var = 0;
    st[(int64_t)blockIdx.x * 6 + t] = (float)mean;
    st[(int64_t)blockIdx.x * 6 + 3 + t] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// InstanceNorm of the heads: the score map x = leaky_relu(IN(raw0)) -> XS; the orientation pair over its norm
__global__ __launch_bounds__(256) void k_f_post1(Geo g, const float* __restrict__ raw, const float* __restrict__ ist,
                                                 const float* __restrict__ gs, const float* __restrict__ bs,
                                                 const float* __restrict__ go, const float* __restrict__ bo,
                                                 float* __restrict__ XS, float* __restrict__ ori) {
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    const float* s = ist + b * 6;
    float v = fmaf((raw[pix] - s[0]) * s[3], gs[0], bs[0]);
    XS[pix] = v > 0.f ? v : 0.01f * v;
    const float oc = fmaf((raw[g.NP + pix] - s[1]) * s[4], go[0], bo[0]);
    const float os = fmaf((raw[2 * g.NP + pix] - s[2]) * s[5], go[1], bo[1]);
    const float nrm = sqrtf(fmaf(oc, oc, os * os));
    float2 o;
    o.x = oc / nrm;
    o.y = os / nrm;
    *reinterpret_cast<float2*>(ori + pix * 2) = o;
  }
}

// 15x15 window (clipped at the image: max_pool2d's -inf padding): the maximum, its first position in raster order
// (torch's rule) and e = exp(7 (x - m))
__global__ __launch_bounds__(256) void k_f_post2(Geo g, const float* __restrict__ XS, float* __restrict__ E,
                                                 int* __restrict__ A) {
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const float* xs = XS + b * g.HW;
    const int ya = max(y - 7, 0), yb = min(y + 7, g.H - 1), xa = max(x - 7, 0), xb = min(x + 7, g.W - 1);
    float m = xs[(int64_t)ya * g.W + xa];
    int a = (int)((int64_t)ya * g.W + xa);
    for (int yy = ya; yy <= yb; ++yy)
      for (int xx = xa; xx <= xb; ++xx) {
        const float v = xs[(int64_t)yy * g.W + xx];
        if (v > m) {
          m = v;
          a = (int)((int64_t)yy * g.W + xx);
        }
      }
    E[b * g.HW + i] = expf(7.0f * (xs[i] - m));
    A[b * g.HW + i] = a;
  }
}

// 15x15 box sum of e (zero padding) -> S; score = e / (s + 1e-8)
__global__ __launch_bounds__(256) void k_f_post3(Geo g, const float* __restrict__ E, float* __restrict__ S,
                                                 float* __restrict__ score) {
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const float* e = E + b * g.HW;
    const int ya = max(y - 7, 0), yb = min(y + 7, g.H - 1), xa = max(x - 7, 0), xb = min(x + 7, g.W - 1);
    float s = 0.f;  // row sums first: the rounding error grows with 15 + 15 additions, not 225
    for (int yy = ya; yy <= yb; ++yy) {
      float row = 0.f;
      for (int xx = xa; xx <= xb; ++xx) row += e[(int64_t)yy * g.W + xx];
      s += row;
    }
    S[b * g.HW + i] = s;
    score[b * g.HW + i] = e[i] / (s + 1e-8f);
  }
}

// ------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------
// t = g p / (s + 1e-8), p = e / (s + 1e-8)
__global__ __launch_bounds__(256) void k_b_t(Geo g, const float* __restrict__ dscore, const float* __restrict__ E,
                                             const float* __restrict__ S, float* __restrict__ T) {
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    const float d = S[pix] + 1e-8f;
    T[pix] = dscore ? dscore[pix] * (E[pix] / d) / d : 0.f;
  }
}

// u = 7 e (g / (s + 1e-8) - sum of t over the window)
__global__ __launch_bounds__(256) void k_b_u(Geo g, const float* __restrict__ dscore, const float* __restrict__ E,
                                             const float* __restrict__ S, const float* __restrict__ T,
                                             float* __restrict__ U) {
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t pix = b * g.HW + i;
    const float* tt = T + b * g.HW;
    const int ya = max(y - 7, 0), yb = min(y + 7, g.H - 1), xa = max(x - 7, 0), xb = min(x + 7, g.W - 1);
    float s = 0.f;
    for (int yy = ya; yy <= yb; ++yy) {
      float row = 0.f;
      for (int xx = xa; xx <= xb; ++xx) row += tt[(int64_t)yy * g.W + xx];
      s += row;
    }
    const float gd = dscore ? dscore[pix] / (S[pix] + 1e-8f) : 0.f;
    U[pix] = 7.0f * E[pix] * (gd - s);
  }
}

// dx_k = u_k - sum of u_j over the windows j whose arg-max is k; leaky ReLU; the orientation's division; -> the
// gradient of the three InstanceNorm outputs (DY) and the per-image sums of dy and dy xhat
__global__ __launch_bounds__(256) void k_b_dy(Geo g, const float* __restrict__ U, const int* __restrict__ A,
                                              const float* __restrict__ XS, const float* __restrict__ raw,
                                              const float* __restrict__ ist, const float* __restrict__ go,
                                              const float* __restrict__ bo, const float* __restrict__ dori,
                                              float* __restrict__ DY, double* __restrict__ part) {
  double r[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t base = b * g.HW, pix = base + i;
    const float* s = ist + b * 6;
    const int ya = max(y - 7, 0), yb = min(y + 7, g.H - 1), xa = max(x - 7, 0), xb = min(x + 7, g.W - 1);
    float acc = 0.f;
    for (int yy = ya; yy <= yb; ++yy)
      for (int xx = xa; xx <= xb; ++xx) {
        const int64_t j = base + (int64_t)yy * g.W + xx;
        if (A[j] == (int)i) acc += U[j];
      }
    float dy[3], xh[3];
    dy[0] = (U[pix] - acc) * (XS[pix] > 0.f ? 1.f : 0.01f);
#pragma unroll
    for (int c = 0; c < 3; ++c) xh[c] = (raw[c * g.NP + pix] - s[c]) * s[3 + c];
    dy[1] = dy[2] = 0.f;
    if (dori) {
      const float oc = fmaf(xh[1], go[0], bo[0]), os = fmaf(xh[2], go[1], bo[1]);
      const float nrm = sqrtf(fmaf(oc, oc, os * os));
      const float ox = oc / nrm, oy = os / nrm;
      const float2 gg = *reinterpret_cast<const float2*>(dori + pix * 2);
      const float dot = fmaf(ox, gg.x, oy * gg.y);
      dy[1] = (gg.x - ox * dot) / nrm;
      dy[2] = (gg.y - oy * dot) / nrm;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      DY[c * g.NP + pix] = dy[c];
      r[c] += (double)dy[c];
      r[3 + c] += (double)dy[c] * (double)xh[c];
    }
  }
  reduce_store<6>(r, part, g.nblk, 0);
}

// InstanceNorm backward sums: per image mean(dy), mean(dy xhat) -> coef [n][6]; the affine gradients summed over
// the images in image order
__global__ __launch_bounds__(512) void k_fin_inb(Geo g, int n, const double* __restrict__ part, float* __restrict__ coef,
                                                 float* __restrict__ dgs, float* __restrict__ dbs,
                                                 float* __restrict__ dgo, float* __restrict__ dbo) {
  const int wave = threadIdx.x >> 6;
  if (wave >= 6) return;
  double tot = 0;
  for (int im = 0; im < n; ++im) {
    const double a = wave_colsum(part, g.nblk, wave, im * g.bpi, g.bpi);
    tot += a;
    if ((threadIdx.x & 63) == 0) coef[(int64_t)im * 6 + wave] = (float)(a / (double)g.HW);
  }
  if ((threadIdx.x & 63) == 0) {
    const float v = (float)tot;
    if (wave == 0) dbs[0] = v;
    else if (wave < 3) dbo[wave - 1] = v;
    else if (wave == 3) dgs[0] = v;
    else dgo[wave - 4] = v;
  }
}

// dh = (gamma rstd) (dy - mean(dy) - xhat mean(dy xhat)) -> DH; its sums are the head biases' gradients
__global__ __launch_bounds__(256) void k_b_dh(Geo g, const float* __restrict__ DY, const float* __restrict__ raw,
                                              const float* __restrict__ ist, const float* __restrict__ coef,
                                              const float* __restrict__ gs, const float* __restrict__ go,
                                              float* __restrict__ DH, double* __restrict__ part) {
  double r[3] = {0, 0, 0};
  const float gam[3] = {gs[0], go[0], go[1]};
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    const float* s = ist + b * 6;
    const float* k = coef + b * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xh = (raw[c * g.NP + pix] - s[c]) * s[3 + c];
      const float dh = gam[c] * s[3 + c] * (DY[c * g.NP + pix] - k[c] - xh * k[3 + c]);
      DH[c * g.NP + pix] = dh;
      r[c] += (double)dh;
    }
  }
  reduce_store<3>(r, part, g.nblk, 0);
}

// the head convolutions' data gradient: dF2[c](q) = sum_o sum_d w[o][c][d] dh[o](q - d)
__global__ __launch_bounds__(256) void k_b_headdx(Geo g, const float* __restrict__ DH, const float* __restrict__ ws,
                                                  const float* __restrict__ wo, float* __restrict__ DF) {
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t base = b * g.HW;
    float d[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) d[c] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y - (ky - 1), xx = x - (kx - 1);
        if (!inside(yy, xx, g.H, g.W)) continue;
        const int64_t p = base + (int64_t)yy * g.W + xx;
        const float h0 = DH[p], h1 = DH[g.NP + p], h2 = DH[2 * g.NP + p];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const int k = c * 9 + ky * 3 + kx;
          d[c] = fmaf(ws[k], h0, fmaf(wo[k], h1, fmaf(wo[144 + k], h2, d[c])));
        }
      }
#pragma unroll
    for (int c = 0; c < 16; ++c) DF[c * g.NP + base + i] = d[c];
  }
}

// the head convolutions' weight gradient, tap d = blockIdx.y: dw[o][c][d] = sum_p dh[o](p) F2[c](p + d);
// column o * 144 + c * 9 + d (conv.weight then conv_ori.weight, flat)
__global__ __launch_bounds__(256) void k_b_headw(Geo g, const float* __restrict__ DH, const float* __restrict__ F2,
                                                 double* __restrict__ part) {
  const int ky = blockIdx.y / 3, kx = blockIdx.y % 3;
  double r[48];
#pragma unroll
  for (int k = 0; k < 48; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int yy = y + ky - 1, xx = x + kx - 1;
    if (!inside(yy, xx, g.H, g.W)) continue;
    const int64_t base = b * g.HW, p = base + (int64_t)yy * g.W + xx;
    const double h0 = DH[base + i], h1 = DH[g.NP + base + i], h2 = DH[2 * g.NP + base + i];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const double v = F2[c * g.NP + p];
      r[c] += h0 * v;
      r[16 + c] += h1 * v;
      r[32 + c] += h2 * v;
    }
  }
  // columns o * 144 + c * 9 + d are not contiguous per tap: reduce in place, then scatter
  __shared__ double s_red[4][48];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 48; ++k) {
    double a = r[k];
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
    if ((t & 63) == 0) s_red[t >> 6][k] = a;
  }
  __syncthreads();
  if (t < 48) {
    const int col = (t / 16) * 144 + (t % 16) * 9 + (int)blockIdx.y;
    part[(int64_t)col * g.nblk + blockIdx.x] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
  }
}

// BN3 + ReLU backward, reduce: dyn = dFout[2j+1] (y3 > 0); sums of dyn and dyn xhat
__global__ __launch_bounds__(256) void k_b_r3(Geo g, const float* __restrict__ DFo, const float* __restrict__ Z3,
                                              const float* __restrict__ st, const float* __restrict__ gam,
                                              const float* __restrict__ bet, double* __restrict__ part) {
  Bn n;
  load_bn(n, st, gam, bet);
  double r[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (Z3[j * g.NP + pix] - n.m[j]) * n.r[j];
      const float dyn = fmaf(xh, n.g[j], n.b[j]) > 0.f ? DFo[(2 * j + 1) * g.NP + pix] : 0.f;
      r[j] += (double)dyn;
      r[8 + j] += (double)dyn * (double)xh;
    }
  }
  reduce_store<16>(r, part, g.nblk, 0);
}

// BN3 apply -> dz3; second 1x1: weight gradient (columns 16..79) and dy2 = W^T dz3 -> DY2; BN2 reduce
__global__ __launch_bounds__(256) void k_b_r2(Geo g, const float* __restrict__ DFo, const float* __restrict__ Z3,
                                              const float* __restrict__ st3, const float* __restrict__ g3,
                                              const float* __restrict__ b3, const float* __restrict__ coef3,
                                              const float* __restrict__ Z2, const float* __restrict__ st2,
                                              const float* __restrict__ g2, const float* __restrict__ b2,
                                              const float* __restrict__ w3, float* __restrict__ DY2,
                                              double* __restrict__ part) {
  Bn n3, n2;
  load_bn(n3, st3, g3, b3);
  load_bn(n2, st2, g2, b2);
  Coef k3;
  load_coef(k3, coef3);
  double r[80];
#pragma unroll
  for (int k = 0; k < 80; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    float dz[8], y2[8], xh2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (Z3[j * g.NP + pix] - n3.m[j]) * n3.r[j];
      const float dyn = fmaf(xh, n3.g[j], n3.b[j]) > 0.f ? DFo[(2 * j + 1) * g.NP + pix] : 0.f;
      dz[j] = k3.a[j] * (dyn - k3.m1[j] - xh * k3.m2[j]);
      xh2[j] = (Z2[j * g.NP + pix] - n2.m[j]) * n2.r[j];
      y2[j] = fmaf(xh2[j], n2.g[j], n2.b[j]);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o)
#pragma unroll
      for (int c = 0; c < 8; ++c) r[16 + o * 8 + c] += (double)dz[o] * (double)y2[c];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float d = 0.f;
#pragma unroll
      for (int o = 0; o < 8; ++o) d = fmaf(w3[o * 8 + c], dz[o], d);
      DY2[c * g.NP + pix] = d;
      r[c] += (double)d;
      r[8 + c] += (double)d * (double)xh2[c];
    }
  }
  reduce_store<80>(r, part, g.nblk, 0);
}

// BN2 apply at the nine taps -> dz2; depthwise 3x3: weight gradient (columns 16..87) and dy1; BN1 + ReLU reduce;
// dyn1 = dy1 (y1 > 0) -> DYN1
__global__ __launch_bounds__(256) void k_b_r1(Geo g, const float* __restrict__ DY2, const float* __restrict__ Z2,
                                              const float* __restrict__ st2, const float* __restrict__ coef2,
                                              const float* __restrict__ wdw, const float* __restrict__ Z1,
                                              const float* __restrict__ st1, const float* __restrict__ g1,
                                              const float* __restrict__ b1, float* __restrict__ DYN1,
                                              double* __restrict__ part) {
  Bn n1;
  load_bn(n1, st1, g1, b1);
  Coef k2;
  load_coef(k2, coef2);
  float m2[8], r2[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    m2[c] = st2[c];
    r2[c] = st2[8 + c];
  }
  double r[88];
#pragma unroll
  for (int k = 0; k < 88; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const int64_t base = b * g.HW, pix = base + i;
    float y1[8], xh1[8], dy1[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      xh1[c] = (Z1[c * g.NP + pix] - n1.m[c]) * n1.r[c];
      y1[c] = fmaxf(fmaf(xh1[c], n1.g[c], n1.b[c]), 0.f);
      dy1[c] = 0.f;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        // z2(p) reads y1(p + d): this pixel q = p + d feeds the output at p = q - d
        const int yy = y - (ky - 1), xx = x - (kx - 1);
        if (!inside(yy, xx, g.H, g.W)) continue;
        const int64_t p = base + (int64_t)yy * g.W + xx;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float xh = (Z2[c * g.NP + p] - m2[c]) * r2[c];
          const float dz = k2.a[c] * (DY2[c * g.NP + p] - k2.m1[c] - xh * k2.m2[c]);
          dy1[c] = fmaf(wdw[c * 9 + ky * 3 + kx], dz, dy1[c]);
          r[16 + c * 9 + ky * 3 + kx] += (double)dz * (double)y1[c];
        }
      }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float dyn = y1[c] > 0.f ? dy1[c] : 0.f;
      DYN1[c * g.NP + pix] = dyn;
      r[c] += (double)dyn;
      r[8 + c] += (double)dyn * (double)xh1[c];
    }
  }
  reduce_store<88>(r, part, g.nblk, 0);
}

// BN1 apply -> dz1; first 1x1: weight gradient (columns 0..63) and the branch input's gradient; the block input's
// gradient dFin[j] = dFout[2j] (pass-through half), dFin[8 + c] = (W^T dz1)[c]
__global__ __launch_bounds__(256) void k_b_r0(Geo g, const float* __restrict__ DYN1, const float* __restrict__ Z1,
                                              const float* __restrict__ st1, const float* __restrict__ coef1,
                                              const float* __restrict__ Xin, const float* __restrict__ w1,
                                              const float* __restrict__ DFo, float* __restrict__ DFi,
                                              double* __restrict__ part) {
  Coef k1;
  load_coef(k1, coef1);
  float m1[8], r1[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    m1[c] = st1[c];
    r1[c] = st1[8 + c];
  }
  double r[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int64_t pix = b * g.HW + i;
    float dz[8], xi[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float xh = (Z1[c * g.NP + pix] - m1[c]) * r1[c];
      dz[c] = k1.a[c] * (DYN1[c * g.NP + pix] - k1.m1[c] - xh * k1.m2[c]);
      xi[c] = Xin[c * g.NP + pix];
    }
#pragma unroll
    for (int o = 0; o < 8; ++o)
#pragma unroll
      for (int c = 0; c < 8; ++c) r[o * 8 + c] += (double)dz[o] * (double)xi[c];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float d = 0.f;
#pragma unroll
      for (int o = 0; o < 8; ++o) d = fmaf(w1[o * 8 + c], dz[o], d);
      DFi[(8 + c) * g.NP + pix] = d;
      DFi[c * g.NP + pix] = DFo[(2 * c) * g.NP + pix];
    }
  }
  reduce_store<64>(r, part, g.nblk, 0);
}

// features.0's weight and bias gradients, channels 8 blockIdx.y .. + 7: columns c * 9 + d and 144 + c
__global__ __launch_bounds__(256) void k_b_conv0w(Geo g, const float* __restrict__ DF0, const float* __restrict__ img,
                                                  double* __restrict__ part) {
  const int c0 = blockIdx.y * 8;
  double r[80];
#pragma unroll
  for (int k = 0; k < 80; ++k) r[k] = 0;
  PIXEL_LOOP {
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const float* im = img + b * g.HW;
    const int64_t pix = b * g.HW + i;
    double v[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        v[ky * 3 + kx] = inside(yy, xx, g.H, g.W) ? (double)im[(int64_t)yy * g.W + xx] : 0.0;
      }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double d = DF0[(c0 + c) * g.NP + pix];
#pragma unroll
      for (int k = 0; k < 9; ++k) r[c * 9 + k] += d * v[k];
      r[72 + c] += d;
    }
  }
  // weights: columns c0 * 9 .. + 71; biases: columns 144 + c0 .. + 7
  __shared__ double s_red[4][80];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 80; ++k) {
    double a = r[k];
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
    if ((t & 63) == 0) s_red[t >> 6][k] = a;
  }
  __syncthreads();
  if (t < 80) {
    const int col = t < 72 ? c0 * 9 + t : 144 + c0 + (t - 72);
    part[(int64_t)col * g.nblk + blockIdx.x] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
  }
}

// Workgroup 0 (has_bn): a BatchNorm's backward sums (columns 0..15) -> coef (gamma rstd, mean(dy), mean(dy xhat))
// and the gradients of gamma and beta.  Workgroups 1..: columns col0 + 16 (blockIdx.x - 1) + wave -> dst.
__global__ __launch_bounds__(1024) void k_fin_b(Geo g, const double* __restrict__ part, int has_bn,
                                                const float* __restrict__ gam, const float* __restrict__ st,
                                                float* __restrict__ coef, float* __restrict__ dgam,
                                                float* __restrict__ dbet, int col0, int ncols, float* __restrict__ dst) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (blockIdx.x == 0) {
    if (!has_bn) return;
    __shared__ double s[16];
    const double a = wave_colsum(part, g.nblk, wave, 0, g.nblk);
    if (lane == 0) s[wave] = a;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 8) {
      coef[t] = gam[t] * st[8 + t];
      coef[8 + t] = (float)(s[t] / g.N);
      coef[16 + t] = (float)(s[8 + t] / g.N);
      dbet[t] = (float)s[t];
      dgam[t] = (float)s[8 + t];
    }
    return;
  }
  const int k = (blockIdx.x - 1) * 16 + wave;
  if (k >= ncols) return;
  const double a = wave_colsum(part, g.nblk, col0 + k, 0, g.nblk);
  if (lane == 0) dst[k] = (float)a;
}

// ------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------
struct Plan {
  Geo g;
  size_t sv_planes;  // float offset of the planes in `saved`
  size_t sc_coef, sc_planes;  // byte offsets in `scratch`
  size_t saved_bytes, scratch_bytes;
};

Plan make_plan(int64_t n, int H, int W) {
  Plan p;
  Geo& g = p.g;
  g.H = H;
  g.W = W;
  g.HW = (int64_t)H * W;
  g.NP = n * g.HW;
  g.N = (double)g.NP;
  const int64_t want = (g.HW + 255) / 256, cap = n >= 1024 ? 1 : 1024 / n;
  g.bpi = (int)(want < cap ? want : cap);
  g.nblk = (int)(n * g.bpi);
  p.sv_planes = ((size_t)kBnStats + (size_t)n * 6 + 3) & ~(size_t)3;
  p.saved_bytes = (p.sv_planes + (size_t)SV_PLANES * g.NP) * sizeof(float);
  p.sc_coef = (size_t)kPartCols * g.nblk * sizeof(double);
  p.sc_planes = (p.sc_coef + ((size_t)6 * kCoefBn + (size_t)n * 6) * sizeof(float) + 15) & ~(size_t)15;
  p.scratch_bytes = p.sc_planes + (size_t)SC_PLANES * g.NP * sizeof(float);
  return p;
}

// indices into the 40-tensor table (RFDet.state_dict() order without num_batches_tracked)
enum { T_C0W = 0, T_C0B = 1, T_BLK = 2, T_HW = 32, T_HB = 33, T_ING = 34, T_INB = 35, T_OW = 36, T_OB = 37, T_OG = 38,
       T_OBE = 39 };
// within a block of 15: conv weight, then BN weight, bias, running_mean, running_var, three times
constexpr int blk(int k, int i) { return T_BLK + 15 * k + i; }
enum { B_PW1 = 0, B_G1 = 1, B_B1 = 2, B_RM1 = 3, B_RV1 = 4, B_DW = 5, B_G2 = 6, B_B2 = 7, B_RM2 = 8, B_RV2 = 9,
       B_PW2 = 10, B_G3 = 11, B_B3 = 12, B_RM3 = 13, B_RV3 = 14 };

#define LAUNCH(kern, grid, block, ...)                                      \
  do {                                                                      \
    hipLaunchKernelGGL(kern, grid, dim3(block), 0, st, __VA_ARGS__);        \
    const hipError_t e_ = hipGetLastError();                                \
    if (e_ != hipSuccess) return e_;                                        \
  } while (0)

}  // namespace

void hn_det_train_plan(int64_t n, int H, int W, size_t* saved, size_t* scratch) {
  const Plan p = make_plan(n, H, W);
  if (saved) *saved = p.saved_bytes;
  if (scratch) *scratch = p.scratch_bytes;
}

bool hn_det_train_is_param(int slot) {
  if (slot < T_BLK || slot >= T_HW) return true;
  const int i = (slot - T_BLK) % 15;
  return !(i == B_RM1 || i == B_RV1 || i == B_RM2 || i == B_RV2 || i == B_RM3 || i == B_RV3);
}

hipError_t hn_det_train_forward_impl(const float* images, int64_t n, int H, int W, float* const* T, float bn_eps,
                                     float in_eps, float momentum, float* score, float* ori, char* saved,
                                     char* scratch, hipStream_t st) {
  const Plan p = make_plan(n, H, W);
  const Geo g = p.g;
  float* sv = reinterpret_cast<float*>(saved);
  float* bnst = sv;
  float* inst = sv + kBnStats;
  float* pl = sv + p.sv_planes;
  auto P = [&](int plane) { return pl + (size_t)plane * g.NP; };
  double* part = reinterpret_cast<double*>(scratch);
  const dim3 grid((unsigned)g.nblk);

  LAUNCH(k_f_conv0, grid, 256, g, images, T[T_C0W], T[T_C0B], T[blk(0, B_PW1)], P(SV_F0), P(SV_Z), part);
  for (int k = 0; k < 2; ++k) {
    float* z1 = P(SV_Z + 24 * k);
    float* z2 = z1 + 8 * g.NP;
    float* z3 = z2 + 8 * g.NP;
    float* s1 = bnst + (3 * k) * 16;
    if (k == 1)
      LAUNCH(k_f_next, grid, 256, g, P(SV_F0), P(SV_Z + 16), bnst + 2 * 16, T[blk(0, B_G3)], T[blk(0, B_B3)],
             T[blk(1, B_PW1)], P(SV_X2), z1, part);
    LAUNCH(k_fin_bn, dim3(1), 1024, g, part, bn_eps, momentum, T[blk(k, B_RM1)], T[blk(k, B_RV1)], s1);
    LAUNCH(k_f_dw, grid, 256, g, z1, s1, T[blk(k, B_G1)], T[blk(k, B_B1)], T[blk(k, B_DW)], z2, part);
    LAUNCH(k_fin_bn, dim3(1), 1024, g, part, bn_eps, momentum, T[blk(k, B_RM2)], T[blk(k, B_RV2)], s1 + 16);
    LAUNCH(k_f_pw2, grid, 256, g, z2, s1 + 16, T[blk(k, B_G2)], T[blk(k, B_B2)], T[blk(k, B_PW2)], z3, part);
    LAUNCH(k_fin_bn, dim3(1), 1024, g, part, bn_eps, momentum, T[blk(k, B_RM3)], T[blk(k, B_RV3)], s1 + 32);
  }
  LAUNCH(k_f_feat, grid, 256, g, P(SV_F0), P(SV_Z + 16), bnst + 2 * 16, T[blk(0, B_G3)], T[blk(0, B_B3)],
         P(SV_Z + 40), bnst + 5 * 16, T[blk(1, B_G3)], T[blk(1, B_B3)], P(SV_F2));
  LAUNCH(k_f_heads, grid, 256, g, P(SV_F2), T[T_HW], T[T_HB], T[T_OW], T[T_OB], P(SV_RAW), part);
  LAUNCH(k_fin_in, dim3((unsigned)n), 512, g, part, in_eps, inst);
  LAUNCH(k_f_post1, grid, 256, g, P(SV_RAW), inst, T[T_ING], T[T_INB], T[T_OG], T[T_OBE], P(SV_XS), ori);
  LAUNCH(k_f_post2, grid, 256, g, P(SV_XS), P(SV_E), reinterpret_cast<int*>(P(SV_A)));
  LAUNCH(k_f_post3, grid, 256, g, P(SV_E), P(SV_S), score);
  return hipSuccess;
}

hipError_t hn_det_train_backward_impl(const float* dscore, const float* dori, const float* images, int64_t n, int H,
                                      int W, float* const* T, float* const* G, char* saved, char* scratch,
                                      hipStream_t st) {
  const Plan p = make_plan(n, H, W);
  const Geo g = p.g;
  float* sv = reinterpret_cast<float*>(saved);
  float* bnst = sv;
  float* inst = sv + kBnStats;
  float* pl = sv + p.sv_planes;
  auto P = [&](int plane) { return pl + (size_t)plane * g.NP; };
  double* part = reinterpret_cast<double*>(scratch);
  float* coef = reinterpret_cast<float*>(scratch + p.sc_coef);
  float* incoef = coef + 6 * kCoefBn;
  float* sp = reinterpret_cast<float*>(scratch + p.sc_planes);
  auto S = [&](int plane) { return sp + (size_t)plane * g.NP; };
  const dim3 grid((unsigned)g.nblk);
  auto fin_blocks = [](int ncols) { return dim3((unsigned)(1 + (ncols + 15) / 16)); };
  float* const nof = nullptr;

  // the score tail, the orientation's division and the InstanceNorms
  LAUNCH(k_b_t, grid, 256, g, dscore, P(SV_E), P(SV_S), S(SC_T));
  LAUNCH(k_b_u, grid, 256, g, dscore, P(SV_E), P(SV_S), S(SC_T), S(SC_U));
  LAUNCH(k_b_dy, grid, 256, g, S(SC_U), reinterpret_cast<const int*>(P(SV_A)), P(SV_XS), P(SV_RAW), inst, T[T_OG],
         T[T_OBE], dori, S(SC_DY), part);
  LAUNCH(k_fin_inb, dim3(1), 512, g, (int)n, part, incoef, G[T_ING], G[T_INB], G[T_OG], G[T_OBE]);
  LAUNCH(k_b_dh, grid, 256, g, S(SC_DY), P(SV_RAW), inst, incoef, T[T_ING], T[T_OG], S(SC_DH), part);
  LAUNCH(k_fin_b, fin_blocks(1), 1024, g, part, 0, nof, nof, nof, nof, nof, 0, 1, G[T_HB]);
  LAUNCH(k_fin_b, fin_blocks(2), 1024, g, part, 0, nof, nof, nof, nof, nof, 1, 2, G[T_OB]);
  // the head convolutions
  LAUNCH(k_b_headw, dim3((unsigned)g.nblk, 9), 256, g, S(SC_DH), P(SV_F2), part);
  LAUNCH(k_fin_b, fin_blocks(144), 1024, g, part, 0, nof, nof, nof, nof, nof, 0, 144, G[T_HW]);
  LAUNCH(k_fin_b, fin_blocks(288), 1024, g, part, 0, nof, nof, nof, nof, nof, 144, 288, G[T_OW]);
  LAUNCH(k_b_headdx, grid, 256, g, S(SC_DH), T[T_HW], T[T_OW], S(SC_DFA));
  // the blocks, last first: dFout in DFA -> block 2 -> DFB -> block 1 -> DFA
  for (int k = 1; k >= 0; --k) {
    const float* dfo = k == 1 ? S(SC_DFA) : S(SC_DFB);
    float* dfi = k == 1 ? S(SC_DFB) : S(SC_DFA);
    const float* z1 = P(SV_Z + 24 * k);
    const float* z2 = z1 + 8 * g.NP;
    const float* z3 = z2 + 8 * g.NP;
    const float* s1 = bnst + (3 * k) * 16;
    float* c1 = coef + (3 * k) * kCoefBn;
    const float* xin = k == 1 ? P(SV_X2) : P(SV_F0 + 8);
    LAUNCH(k_b_r3, grid, 256, g, dfo, z3, s1 + 32, T[blk(k, B_G3)], T[blk(k, B_B3)], part);
    LAUNCH(k_fin_b, dim3(1), 1024, g, part, 1, T[blk(k, B_G3)], s1 + 32, c1 + 2 * kCoefBn, G[blk(k, B_G3)],
           G[blk(k, B_B3)], 0, 0, nof);
    LAUNCH(k_b_r2, grid, 256, g, dfo, z3, s1 + 32, T[blk(k, B_G3)], T[blk(k, B_B3)], c1 + 2 * kCoefBn, z2, s1 + 16,
           T[blk(k, B_G2)], T[blk(k, B_B2)], T[blk(k, B_PW2)], S(SC_D8A), part);
    LAUNCH(k_fin_b, fin_blocks(64), 1024, g, part, 1, T[blk(k, B_G2)], s1 + 16, c1 + kCoefBn, G[blk(k, B_G2)],
           G[blk(k, B_B2)], 16, 64, G[blk(k, B_PW2)]);
    LAUNCH(k_b_r1, grid, 256, g, S(SC_D8A), z2, s1 + 16, c1 + kCoefBn, T[blk(k, B_DW)], z1, s1, T[blk(k, B_G1)],
           T[blk(k, B_B1)], S(SC_D8B), part);
    LAUNCH(k_fin_b, fin_blocks(72), 1024, g, part, 1, T[blk(k, B_G1)], s1, c1, G[blk(k, B_G1)], G[blk(k, B_B1)], 16,
           72, G[blk(k, B_DW)]);
    LAUNCH(k_b_r0, grid, 256, g, S(SC_D8B), z1, s1, c1, xin, T[blk(k, B_PW1)], dfo, dfi, part);
    LAUNCH(k_fin_b, fin_blocks(64), 1024, g, part, 0, nof, nof, nof, nof, nof, 0, 64, G[blk(k, B_PW1)]);
  }
  // features.0
  LAUNCH(k_b_conv0w, dim3((unsigned)g.nblk, 2), 256, g, S(SC_DFA), images, part);
  LAUNCH(k_fin_b, fin_blocks(144), 1024, g, part, 0, nof, nof, nof, nof, nof, 0, 144, G[T_C0W]);
  LAUNCH(k_fin_b, fin_blocks(16), 1024, g, part, 0, nof, nof, nof, nof, nof, 144, 16, G[T_C0B]);
  return hipSuccess;
}
