// Fused nearest / second-nearest descriptor matching (FDLNet-master/latency/NASNet/utils/
// eval_utils.py:112-197 over math_utils.py:8-19) without materialising the N x M distance matrix.
//
// Both supported distances are monotone, per query row, in one key
//   key(i,j) = c_j - 2 a_i.b_j
//   HN_METRIC_UNIT  c_j = 0        d = sqrt(clamp(2 - 2 a.b, 1e-8, 4))        (math_utils.py:8-19)
//   HN_METRIC_L2    c_j = |b_j|^2  d = sqrt(|a|^2 + |b|^2 - 2 a.b + 1e-6) + 1e-8  (hardnet/Losses.py:5-13)
// so one selection kernel serves both and its epilogue has neither a sqrt nor a clamp.
//
// k_match_ring is k_pairdist_ring (hn_pairdist.hip) without the diagonal, the masks and the column
// minima: query A fragments resident in registers (bf16x3 split), the database pre-split once into bf16
// hi / lo planes (k_split_planes) and staged by LDS-DMA into the three-buffer swizzled ring, 32 x 32
// sub-tile chains with the previous sub-tile's epilogue woven into the next chain.  The epilogue keeps,
// per accumulator row and lane, the two smallest keys and the (wave-uniform) sub-tile numbers they came
// from -- the lane's column inside a sub-tile is fixed, so the column is rebuilt at the end.  After the
// sweep the 32 lanes of a row merge their pairs lexicographically on (key, column): the result does not
// depend on the order in which lanes or workgroups finish, and of equal keys the smaller column wins
// both places.  k_match_rescore then recomputes the two selected dot products in plain fp32 and writes
// the distances (swapping the pair when the exact values come out in the other order).
#include "hn_common.h"
#include "hn_internal.h"

#include <climits>
#include <cmath>
#include <type_traits>

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef int i32x16 __attribute__((ext_vector_type(16)));

template <int N>
HN_DEV void wait_vm() {  // s_waitcnt vmcnt(N), lgkmcnt / expcnt untouched
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// c_j of the MP = M rounded up to 64 columns: 0 (UNIT) or |b_j|^2 (L2) for j < M, +inf for the padding of
// the last tile, whose keys therefore reach no minimum (its rows are staged from row M - 1: a repeated
// column with a finite c_j would become a false second-nearest)
__global__ __launch_bounds__(256) void k_match_cj(const float* __restrict__ db, int M, int MP, int l2,
                                                  float* __restrict__ cj) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= MP) return;
  float s = INFINITY;
  if (j < M) {
    s = 0.f;
    if (l2) {
      const float b0 = db[(size_t)j * 128 + lane], b1 = db[(size_t)j * 128 + 64 + lane];
      s = wave_sum(b0 * b0 + b1 * b1);
    }
  }
  if (lane == 0) cj[j] = s;
}

// (x, jx) before (y, jy): smaller key, then smaller column
HN_DEV bool lex_lt(float x, int jx, float y, int jy) { return x < y || (x == y && jx < jy); }

template <int NW>
__global__ __launch_bounds__(NW * 64) void k_match_ring(const float* __restrict__ q, int N,
                                                        const uint16_t* __restrict__ ph,
                                                        const uint16_t* __restrict__ pl, int M,
                                                        const float* __restrict__ cj, int* __restrict__ idx) {
  constexpr int TN = 64, ROWB = 256, PLANE = TN * ROWB, BUF = 2 * PLANE + TN * 4;
  constexpr int G = 2 * PLANE / 1024 / NW;  // DMA instructions per wave per tile
  static_assert(G * NW * 1024 == 2 * PLANE, "tile split");
  __shared__ __attribute__((aligned(16))) char sb0[BUF], sb1[BUF], sb2[BUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * (32 * NW) + wave * 32;  // this wave's first query
  // A fragments: lane (r, h) holds query i0 + r (clamped), k = 16 ks + 8 h + j
  bf16x8 ah[8], al[8];
  {
    const int ia = min(i0 + r, N - 1);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const float4 x0 = *reinterpret_cast<const float4*>(q + (size_t)ia * 128 + ks * 16 + h * 8);
      const float4 x1 = *reinterpret_cast<const float4*>(q + (size_t)ia * 128 + ks * 16 + h * 8 + 4);
      uint4 hi, lo;
      split8(x0, x1, hi, lo);
      ah[ks] = as_bf16x8(hi);
      al[ks] = as_bf16x8(lo);
    }
  }
  // every chain starts from 0 in the row of a query, from -inf in a row past N (key = +inf)
  f32x16 areg;
#pragma unroll
  for (int i = 0; i < 16; ++i) areg[i] = i0 + (i & 3) + 8 * (i >> 2) + 4 * h < N ? 0.f : -INFINITY;
  // per accumulator row: the two smallest keys of this lane's columns and their sub-tile numbers
  f32x16 m1, m2;  // (vector elements, not arrays: the selects below would otherwise pick between addresses
  i32x16 t1, t2;  // and leave the arrays in scratch)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    m1[i] = INFINITY;
    m2[i] = INFINITY;
    t1[i] = 0;
    t2[i] = 0;
  }

  // tile j0's rows (clamped to M - 1) into a buffer, as k_pairdist_ring: wave instruction gi = wave * G + k
  // covers plane gi / 16, rows 4 (gi % 16) .. +3; lane L fills row 4 (gi % 16) + L / 16, chunk L % 16 with
  // the row's logical chunk (L % 16) ^ (row & 15); wave 0 adds c_j of the 64 columns (4 B per lane; cj
  // holds all MP of them).  k = G is wave 0's c_j piece.
  const unsigned wv = __builtin_amdgcn_readfirstlane(wave);
  auto issue_piece = [&](char* buf, int j0, int k) {
    if (k == G) {
      if (wv == 0) {
        const float* src = cj + j0 + lane;
        const unsigned dst = (unsigned)(uintptr_t)(lds_ptr_t)(buf + 2 * PLANE);
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
      }
      return;
    }
    const int gi = wave * G + k, plane = gi >> 4, r4 = (gi & 15) * 4;
    const int row = r4 + (lane >> 4), d = lane & 15;
    const int jr = min(j0 + row, M - 1);
    const uint16_t* src = (plane ? pl : ph) + (size_t)jr * 128 + ((d ^ (row & 15)) << 3);
    const int gu = (int)wv * G + k;
    const unsigned dst = (unsigned)(uintptr_t)(lds_ptr_t)(buf + (gu >> 4) * PLANE + (gu & 15) * 4 * ROWB);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
  };
  auto issue = [&](char* buf, int j0) {
#pragma unroll
    for (int k = 0; k <= G; ++k) issue_piece(buf, j0, k);
  };
  // this wave's share of the older tile's DMA retired, then every wave's (and the LDS reads of the buffer
  // about to be refilled complete: lgkmcnt(0))
  auto sync_tile = [&](bool more) {
    if (more) {
      if (wv == 0) wait_vm<G + 1>(); else wait_vm<G>();
    } else {
      wait_vm<0>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  // key v of accumulator row i, from sub-tile s (s grows along the sweep: the strict tests keep the
  // earlier, smaller column of equal keys first)
  auto top2 = [&](int i, float v, int s) {
    const float k1 = m1[i], k2 = m2[i];
    const int s1 = t1[i], s2 = t2[i];
    const bool c1 = v < k1, c2 = v < k2;
    t2[i] = c1 ? s1 : (c2 ? s : s2);
    t1[i] = c1 ? s : s1;
    m2[i] = __builtin_amdgcn_fmed3f(k1, k2, v);
    m1[i] = fminf(k1, v);
  };
  // one 32-column sub-tile's bf16x3 chain (K = 128) with the previous sub-tile's epilogue (accp, its c_j
  // and number) woven in: two accumulator entries per K-step
  auto chain_epi = [&](const char* cur, int nt, const f32x16& accp, float cp, int sp, auto hook) {
    f32x16 acc = areg;
    const int row = nt * 32 + r, sw = row & 15;
    const char* base = cur + row * ROWB;
    uint4 bh = *reinterpret_cast<const uint4*>(base + ((h ^ sw) << 4));
    uint4 bl = *reinterpret_cast<const uint4*>(base + PLANE + ((h ^ sw) << 4));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      uint4 nh, nl;
      if (ks + 1 < 8) {
        const int off = ((2 * (ks + 1) + h) ^ sw) << 4;
        nh = *reinterpret_cast<const uint4*>(base + off);
        nl = *reinterpret_cast<const uint4*>(base + PLANE + off);
      }
      acc = mfma3(ah[ks], al[ks], as_bf16x8(bh), as_bf16x8(bl), acc);
      hook(ks);
      top2(2 * ks, fmaf(-2.0f, accp[2 * ks], cp), sp);
      top2(2 * ks + 1, fmaf(-2.0f, accp[2 * ks + 1], cp), sp);
      if (ks + 1 < 8) {
        bh = nh;
        bl = nl;
      }
    }
    return acc;
  };

  const int ntile = (M + TN - 1) / TN;
  f32x16 accp{};
  float cp = INFINITY;  // (an empty epilogue before the first sub-tile: every key +inf)
  int sp = 0;
  // prologue: tiles 0 and 1 in flight, wait for tile 0
  issue(sb0, 0);
  if (ntile > 1) issue(sb1, TN);
  sync_tile(ntile > 1);
  // tile t on buffer t % 3 (compile-time within the unrolled step): tile t + 2's DMA goes into the buffer
  // tile t - 1 was read from (every wave passed the barrier after reading it), spread over the first
  // sub-tile's MFMA chain
  auto step = [&](const char* cur, char* nxt2, int t) {
    const int j0 = t * TN;
    const bool more2 = t + 2 < ntile;
    const float* cs = reinterpret_cast<const float*>(cur + 2 * PLANE);
    accp = chain_epi(cur, 0, accp, cp, sp, [&](int ks) {
#pragma unroll
      for (int k = 0; k < G; ++k)
        if (more2 && (k * 8) / G == ks) issue_piece(nxt2, j0 + 2 * TN, k);
    });
    if (more2) issue_piece(nxt2, j0 + 2 * TN, G);
    cp = cs[r];
    sp = 2 * t;
    accp = chain_epi(cur, 1, accp, cp, sp, [](int) {});
    cp = cs[32 + r];
    sp = 2 * t + 1;
    sync_tile(more2);  // retire tile t + 1's DMA, leaving tile t + 2's in flight
  };
#pragma unroll 1
  for (int t = 0; t < ntile; t += 3) {
    step(sb0, sb2, t);
    if (t + 1 < ntile) step(sb1, sb0, t + 1);
    if (t + 2 < ntile) step(sb2, sb1, t + 2);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) top2(i, fmaf(-2.0f, accp[i], cp), sp);  // the last sub-tile's epilogue

  // merge over the 32 lanes of each half-wave (the columns): a butterfly in which both partners merge
  // the same two sorted pairs, so every lane ends with the row's two smallest (key, column)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float a1 = m1[i], a2 = m2[i];
    int j1 = a1 < INFINITY ? t1[i] * 32 + r : INT_MAX, j2 = a2 < INFINITY ? t2[i] * 32 + r : INT_MAX;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float b1 = __shfl_xor(a1, o, 64), b2 = __shfl_xor(a2, o, 64);
      const int k1 = __shfl_xor(j1, o, 64), k2 = __shfl_xor(j2, o, 64);
      if (lex_lt(b1, k1, a1, j1)) {  // the partner's first wins: second = min(own first, its second)
        const bool s = lex_lt(b2, k2, a1, j1);
        a2 = s ? b2 : a1;
        j2 = s ? k2 : j1;
        a1 = b1;
        j1 = k1;
      } else {  // own first stays: second = min(own second, the partner's first)
        const bool s = lex_lt(b1, k1, a2, j2);
        a2 = s ? b1 : a2;
        j2 = s ? k1 : j2;
      }
    }
    const int row = i0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (r == 0 && row < N)
      *reinterpret_cast<int2*>(idx + (size_t)row * 2) = make_int2(a1 < INFINITY ? j1 : -1, a2 < INFINITY ? j2 : -1);
  }
}

// One wave per query: the two selected dot products again in plain fp32, the final distances, and the pair
// swapped when the exact distances come out in the other order (keys within the selection error of each
// other).  A missing place (index -1: one database row) is dist = +inf.
__global__ __launch_bounds__(256) void k_match_rescore(const float* __restrict__ q, int N,
                                                       const float* __restrict__ db, const float* __restrict__ cj,
                                                       int l2, float* __restrict__ dist, int* __restrict__ idx) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const float a0 = q[(size_t)i * 128 + lane], a1 = q[(size_t)i * 128 + 64 + lane];
  const int2 j = *reinterpret_cast<const int2*>(idx + (size_t)i * 2);
  const float asq = l2 ? wave_sum(fmaf(a0, a0, a1 * a1)) : 0.f;
  auto dist_to = [&](int jj) {
    if (jj < 0) return INFINITY;
    const float* b = db + (size_t)jj * 128;
    const float dot = wave_sum(fmaf(a0, b[lane], a1 * b[64 + lane]));
    if (l2) return sqrtf(fmaxf((asq + cj[jj]) - 2.0f * dot + 1e-6f, 0.f)) + 1e-8f;
    return sqrtf(fminf(fmaxf(2.0f - 2.0f * dot, 1e-8f), 4.0f));
  };
  const float d0 = dist_to(j.x), d1 = dist_to(j.y);
  if (lane == 0) {
    const bool sw = d1 < d0;
    *reinterpret_cast<float2*>(dist + (size_t)i * 2) = sw ? make_float2(d1, d0) : make_float2(d0, d1);
    if (sw) *reinterpret_cast<int2*>(idx + (size_t)i * 2) = make_int2(j.y, j.x);
  }
}

}  // namespace

// workspace: c_j [M rounded up to 64] | bf16 hi / lo planes of the database [M][128] each
size_t hn_match_ws_bytes(long N, long M) {
  (void)N;
  return (size_t)((M + 63) / 64 * 64) * sizeof(float) + (size_t)M * 128 * 2 * sizeof(uint16_t);
}

hipError_t hn_launch_match_nn2(const float* q, int N, const float* db, int M, int metric, float* dist, int* idx,
                               void* ws, hipStream_t st) {
  const int MP = (M + 63) / 64 * 64;
  float* cj = static_cast<float*>(ws);
  uint16_t* ph = reinterpret_cast<uint16_t*>(cj + MP);
  uint16_t* pl = ph + (size_t)M * 128;
  const int l2 = metric == HN_METRIC_L2;
  hipLaunchKernelGGL(k_match_cj, dim3(MP / 4), dim3(256), 0, st, db, M, MP, l2, cj);
  hipError_t e = hn_launch_split_planes(db, M, ph, pl, st);
  if (e != hipSuccess) return e;
  // 8-wave workgroups when they still give every CU one (N >= 65,536 queries), else 4-wave ones, as
  // hn_launch_pairdist_rows
  auto go = [&](auto nw) {
    constexpr int NW = decltype(nw)::value;
    hipLaunchKernelGGL((k_match_ring<NW>), dim3((N + 32 * NW - 1) / (32 * NW)), dim3(64 * NW), 0, st, q, N, ph, pl, M,
                       cj, idx);
  };
  if (N >= 256 * 32 * 8)
    go(std::integral_constant<int, 8>{});
  else
    go(std::integral_constant<int, 4>{});
  hipLaunchKernelGGL(k_match_rescore, dim3((N + 3) / 4), dim3(256), 0, st, q, N, db, cj, l2, dist, idx);
  return hipGetLastError();
}
