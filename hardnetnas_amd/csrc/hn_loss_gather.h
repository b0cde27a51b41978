// What the hardest-in-batch losses share (hn_loss.hip: loss_HardNet 'min'; hn_neimask.hip: FDLNet's
// neighbour-mask loss): the u64 (value bits << 32 | index) minimum keys, the 64 x 64 x 128 exact-fp32 tile
// product over k-major LDS operands, and the backward's scatter as a gather -- row i's hardest negative
// (i, r_i) feeds positive r_i, the column minimum (c_i, i) feeds anchor c_i; per-target source lists are built
// by a counting pass, a scan and an unordered fill, and one wave per target orders its list before summing
// (deterministic: O(B) work for any selection pattern but a target with > 64 sources, which scans all sources
// in order).  The two losses differ in the term a selected entry contributes (the Term argument of
// k_lmin_bwd_gather).  Everything here has internal linkage: each loss file gets its own copy.
#pragma once
#include <algorithm>
#include <cstring>

#include "hn_common.h"

namespace {

constexpr int LT_D = 128;  // descriptor length
constexpr int LT_TM = 64;  // rows (anchors) per workgroup
constexpr int LT_TN = 64;  // columns (positives) per tile

HN_DEV unsigned long long key_of(float v, int idx) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)idx;
}
HN_DEV float key_val(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }
HN_DEV int key_idx(unsigned long long k) { return (int)(unsigned)(k & 0xffffffffu); }
HN_DEV unsigned long long umin64(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

// rows [r0, r0 + 64) of src [B][128] -> a k-major LDS copy lds[128][64]; rows past B are zero
HN_DEV void lt_load_kmajor(float* __restrict__ lds, const float* __restrict__ src, int r0, int B, int tid) {
  for (int e = tid; e < LT_TM * LT_D / 4; e += 256) {
    const int row = e % LT_TM, k4 = e / LT_TM;  // consecutive threads: consecutive rows (conflict-free LDS stores)
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < B) v = reinterpret_cast<const float4*>(src + (size_t)(r0 + row) * LT_D)[k4];
    lds[(4 * k4 + 0) * LT_TM + row] = v.x;
    lds[(4 * k4 + 1) * LT_TM + row] = v.y;
    lds[(4 * k4 + 2) * LT_TM + row] = v.z;
    lds[(4 * k4 + 3) * LT_TM + row] = v.w;
  }
}

// acc[r][c] = a_{4ty+r} . p_{4tx+c}: one FMA chain per entry over k in increasing order, from 0
HN_DEV void lt_tile_dots(const float4 (*As)[LT_TM / 4], const float4 (*Ps)[LT_TN / 4], int ty, int tx,
                         float (&acc)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
#pragma unroll 4
  for (int k = 0; k < LT_D; ++k) {
    const float4 av = As[k][ty], pv = Ps[k][tx];
    const float ar[4] = {av.x, av.y, av.z, av.w}, pc[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(ar[r], pc[c], acc[r][c]);
  }
}

// the same chain for one entry (the backward's recomputation of a selected entry)
HN_DEV float dot128(const float* x, const float* y) {
  const float4* a = reinterpret_cast<const float4*>(x);
  const float4* b = reinterpret_cast<const float4*>(y);
  float s = 0.f;
  for (int k = 0; k < LT_D / 4; ++k) {
    const float4 u = a[k], v = b[k];
    s = fmaf(u.x, v.x, s);
    s = fmaf(u.y, v.y, s);
    s = fmaf(u.z, v.z, s);
    s = fmaf(u.w, v.w, s);
  }
  return s;
}

// Backward workspace shared by the two losses: per source row k the coefficients coef[3k + {0, 1, 2}] of its
// selected entries (positive (k,k), row negative (k, r_k), column negative (c_k, k)) and idx[2k + {0, 1}] =
// (r_k, c_k); cnt / off / fill / list [2B]: the per-target source lists.
// Target t < B is anchor t (sources k with a column negative c_k = t, coef slot 2; only with anchor_swap),
// t >= B positive t - B (sources with a row negative r_k = t - B, slot 1).
HN_DEV int src_target(const float* coef, const int* idx, int k, int slot, int B) {  // -1: no term
  if (coef[3 * k + 1 + slot] == 0.f) return -1;
  return slot ? idx[2 * k + 1] : B + idx[2 * k];
}
__global__ __launch_bounds__(256) void k_lmin_bwd_count(const float* __restrict__ coef, const int* __restrict__ idx,
                                                        int B, int swap, int* __restrict__ cnt) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < B; k += gridDim.x * 256)
    for (int slot = 0; slot < 1 + swap; ++slot) {
      const int tg = src_target(coef, idx, k, slot, B);
      if (tg >= 0) atomicAdd(cnt + tg, 1);
    }
}
// exclusive scan of cnt[n] -> off[n] in one workgroup (contiguous chunk per thread); fill[] := 0
__global__ __launch_bounds__(1024) void k_lmin_bwd_scan(const int* __restrict__ cnt, int n, int* __restrict__ off,
                                                        int* __restrict__ fill) {
  __shared__ int tot[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024, b0 = min(n, tid * per), b1 = min(n, b0 + per);
  int s = 0;
  for (int i = b0; i < b1; ++i) s += cnt[i];
  tot[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan of the thread totals
    const int v = tid >= o ? tot[tid - o] : 0;
    __syncthreads();
    tot[tid] += v;
    __syncthreads();
  }
  int run = tot[tid] - s;
  for (int i = b0; i < b1; ++i) {
    off[i] = run;
    run += cnt[i];
    fill[i] = 0;
  }
}
__global__ __launch_bounds__(256) void k_lmin_bwd_fill(const float* __restrict__ coef, const int* __restrict__ idx,
                                                       int B, int swap, const int* __restrict__ off,
                                                       int* __restrict__ fill, int* __restrict__ list) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < B; k += gridDim.x * 256)
    for (int slot = 0; slot < 1 + swap; ++slot) {
      const int tg = src_target(coef, idx, k, slot, B);
      if (tg >= 0) list[off[tg] + atomicAdd(fill + tg, 1)] = k;  // unordered; the gather orders it
    }
}

// one wave per target row: t < B the anchor gradient of row t, else the positive gradient of row
// t - B; each lane holds 2 of the 128 dims.  Terms: the target's own entries, then every source
// whose selected negative lies in the target's row / column, in increasing source order.
// Term::add(acc, w, self, other): acc += w * d u(self, other) / d self for the loss's own u.
template <class Term>
__global__ __launch_bounds__(256) void k_lmin_bwd_gather(const float* __restrict__ a, const float* __restrict__ p,
                                                         int B, int swap, const float* __restrict__ coef,
                                                         const int* __restrict__ idx, const int* __restrict__ cnt,
                                                         const int* __restrict__ off, const int* __restrict__ list,
                                                         float* __restrict__ ga, float* __restrict__ gp) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= 2 * B) return;
  const bool anc = t < B;
  const int i = anc ? t : t - B;
  const float2* A2 = reinterpret_cast<const float2*>(a);
  const float2* P2 = reinterpret_cast<const float2*>(p);
  // self = the target row's own vector, other(j) = the partner row on the other side
  const float2 self = anc ? A2[(size_t)i * 64 + lane] : P2[(size_t)i * 64 + lane];
  auto other = [&](int j) { return anc ? P2[(size_t)j * 64 + lane] : A2[(size_t)j * 64 + lane]; };
  float2 acc = make_float2(0.f, 0.f);
  auto add = [&](float w, const float2& o) { Term::add(acc, w, self, o); };
  const float cpos = coef[3 * i];
  if (cpos != 0.f) add(cpos, other(i));
  // anchor row i: its own row negative (i, r_i); positive row i: its own column negative (c_i, i)
  const float cown = coef[3 * i + (anc ? 1 : 2)];
  if (cown != 0.f) add(cown, other(idx[2 * i + (anc ? 0 : 1)]));
  // scattered terms: anchor i collects column negatives with c_k = i; positive j row negatives with r_k = j
  const int slot = anc ? 1 : 0;
  const int n = cnt[t];  // sources that selected an entry of this target (wave-uniform)
  if (n > 0 && n <= 64) {
    // the list in increasing source order: lane j holds source s_j, its rank = #{sources < s_j}
    const int sj = lane < n ? list[off[t] + lane] : 0x7fffffff;
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += __shfl(sj, o, 64) < sj ? 1 : 0;
    for (int r = 0; r < n; ++r) {
      const unsigned long long m = __ballot(lane < n && rank == r);
      const int kk = __shfl(sj, __ffsll((unsigned long long)m) - 1, 64);
      add(coef[3 * kk + 1 + slot], other(kk));
    }
  } else if (n > 64) {  // a heavily selected target: every source, in order
    for (int k0 = 0; k0 < B; k0 += 64) {
      const int k = k0 + lane;
      const bool hit = k < B && idx[2 * k + slot] == i && coef[3 * k + 1 + slot] != 0.f;
      unsigned long long m = __ballot(hit);
      while (m) {
        const int kk = k0 + __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        add(coef[3 * kk + 1 + slot], other(kk));
      }
    }
  }
  float2* G = reinterpret_cast<float2*>(anc ? ga : gp);
  G[(size_t)i * 64 + lane] = acc;
}

// count, scan, fill, gather over a filled coef / idx (the launches after a loss's coefficient pass)
template <class Term>
hipError_t lmin_bwd_gather_launch(const float* a, const float* p, int B, int swap, const float* coef, const int* idx,
                                  int* cnt, int* off, int* fill, int* list, float* ga, float* gp, hipStream_t st) {
  const int g = std::min((B + 255) / 256, 2048);
  if (hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int) * 2 * (size_t)B, st)) return e;
  hipLaunchKernelGGL(k_lmin_bwd_count, dim3(g), dim3(256), 0, st, coef, idx, B, swap, cnt);
  hipLaunchKernelGGL(k_lmin_bwd_scan, dim3(1), dim3(1024), 0, st, cnt, 2 * B, off, fill);
  hipLaunchKernelGGL(k_lmin_bwd_fill, dim3(g), dim3(256), 0, st, coef, idx, B, swap, off, fill, list);
  hipLaunchKernelGGL(k_lmin_bwd_gather<Term>, dim3((2 * B + 3) / 4), dim3(256), 0, st, a, p, B, swap, coef, idx, cnt,
                     off, list, ga, gp);
  return hipGetLastError();
}

}  // namespace
