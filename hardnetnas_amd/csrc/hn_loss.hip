// Train-mode loss_HardNet with batch_reduce 'min' (hardnet/Losses.py:87-154, the default of the
// training loop, HardNet.py:408-413) and its backward (HardNet.py:421-423), without the B x B
// distance matrix: forward and backward run on these kernels end to end.
//
// Forward (k_lmin_tiles + k_lmin_finish):
//   d_ij  = sqrt((|a_i|^2 + |p_j|^2) - 2 a_i.p_j + 1e-6) + 1e-8        (Losses.py:5-13, :93)
//   dn_ij = d_ij + 10 [i = j];  dn_ij += 10 if dn_ij < 0.008            (:95-101)
//   row_i = min_j dn_ij (argmin r_i),  col_i = min_k dn_ki (argmin c_i) (:103-108)
//   mn_i  = anchor_swap ? min(row_i, col_i) : row_i,  pos_i = d_ii
//   loss  = mean_i f(pos_i, mn_i)  (triplet_margin / softmax / contrastive, :142-153)
// The products are exact fp32 FMAs (the reference's torch.bmm is fp32); minima carry their
// argmin packed below the value bits in one u64 (dn >= 0, so the float bits order like the
// floats), so a tie keeps the first index whatever order the workgroups finish in.
//
// Backward (k_lmin_bwd_src + k_lmin_bwd_gather) -- what autograd does over the reference
// formulation: the min selects one entry per row (torch.min(dim) routes the gradient to its
// argmin), torch.minimum splits a tie between the row and the column entry in halves, and
// sqrt(u) passes g / (2 sqrt(u)) to u = |a_i|^2 + |p_j|^2 - 2 a_i.p_j + 1e-6, i.e.
// 2 a_i - 2 p_j to a_i and 2 p_j - 2 a_i to p_j.  Row i's hardest negative (i, r_i) feeds p_{r_i},
// the column minimum (c_i, i) feeds a_{c_i}: the gather kernel gives each target row the terms
// of every source that selected it, in increasing source order (deterministic: the per-target source
// lists are built by a counting pass, a scan and an unordered fill, and each target's wave orders its
// list before summing -- O(B) work for any selection pattern but a target with > 64 sources, which
// scans all sources in order).
#include "hn_common.h"
#include "hn_internal.h"
#include "hn_loss_gather.h"
#include "hn_loss_terms.h"

namespace {

constexpr int D = LT_D, TM = LT_TM, TN = LT_TN;

__global__ __launch_bounds__(256) void k_lmin_init(unsigned long long* __restrict__ colbest, int B) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) colbest[i] = ~0ull;
}

// One workgroup per 64 anchors, all positives in 64-column tiles.  Thread (ty, tx) computes the
// 4 x 4 block rows 4ty..4ty+3 x columns 4tx..4tx+3 of a tile from k-major LDS copies (float4
// reads: 16 consecutive float4 across tx, broadcast across ty).
__global__ __launch_bounds__(256) void k_lmin_tiles(const float* __restrict__ a, const float* __restrict__ p,
                                                    const float* __restrict__ sq, int B, int swap,
                                                    unsigned long long* __restrict__ rowbest,
                                                    unsigned long long* __restrict__ colbest,
                                                    float* __restrict__ pos) {
  __shared__ float4 As[D][TM / 4];
  __shared__ float4 Ps[D][TN / 4];
  __shared__ unsigned long long red[16][TN];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.x * TM;
  // anchors -> As (k-major); rows past B are zero (their results are never stored)
  lt_load_kmajor(reinterpret_cast<float*>(&As[0][0]), a, r0, B, tid);
  float asq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) asq[r] = (r0 + 4 * ty + r < B) ? sq[r0 + 4 * ty + r] : 0.f;
  unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  for (int c0 = 0; c0 < B; c0 += TN) {
    __syncthreads();  // previous tile's readers are done with Ps / red
    lt_load_kmajor(reinterpret_cast<float*>(&Ps[0][0]), p, c0, B, tid);
    __syncthreads();
    float acc[4][4];
    lt_tile_dots(As, Ps, ty, tx, acc);
    unsigned long long cb[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = c0 + 4 * tx + c;
      if (j >= B) continue;
      const float psq = sq[B + j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = r0 + 4 * ty + r;
        if (i >= B) continue;
        const float x = (asq[r] + psq) - 2.0f * acc[r][c];
        const float d = sqrtf(x + 1e-6f) + 1e-8f;
        float dn = d;
        if (i == j) dn = d + 10.0f;  // (pos[i] comes from k_lmin_sq's difference form)
        if (dn < 0.008f) dn += 10.0f;
        best[r] = umin64(best[r], key_of(dn, j));
        if (swap) cb[c] = umin64(cb[c], key_of(dn, i));
      }
    }
    if (swap) {  // column minima over the workgroup's 64 rows -> one atomic per column
#pragma unroll
      for (int c = 0; c < 4; ++c) red[ty][4 * tx + c] = cb[c];
      __syncthreads();
      if (tid < TN && c0 + tid < B) {
        unsigned long long m = red[0][tid];
#pragma unroll
        for (int t = 1; t < 16; ++t) m = umin64(m, red[t][tid]);
        atomicMin(colbest + c0 + tid, m);
      }
    }
  }
  // row minima over the 16 threads (tx) sharing a row
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) red[tx][4 * ty + r] = best[r];
  __syncthreads();
  if (tid < TM && r0 + tid < B) {
    unsigned long long m = red[0][tid];
#pragma unroll
    for (int t = 1; t < 16; ++t) m = umin64(m, red[t][tid]);
    rowbest[r0 + tid] = m;
  }
}

// one workgroup: the mean in a fixed order (deterministic)
__global__ __launch_bounds__(1024) void k_lmin_finish(const unsigned long long* __restrict__ rowbest,
                                                      const unsigned long long* __restrict__ colbest,
                                                      const float* __restrict__ pos, int B, int swap, float margin,
                                                      int type, float* __restrict__ loss) {
  // the per-row losses in fp32 (as the reference computes them), their sum in fp64 in a fixed order,
  // so the mean carries no summation error of its own (the reference's fp32 torch.mean does)
  __shared__ double part[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 1024) {
    const float vr = key_val(rowbest[i]);
    const float mn = swap ? fminf(vr, key_val(colbest[i])) : vr;
    float dp, dm;
    s += (double)loss_of(type, margin, pos[i], mn, &dp, &dm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    loss[0] = (float)(t / (double)B);
  }
}

// batch_reduce 'random' (Losses.py:131-138): row i's negative is entry (i, t_i), with anchor_swap also entry
// (t_i, i) -- the 'min' computation with r_i = c_i = t_i, so the two keys go into the rowbest / colbest slots and
// the finish and the backward run unchanged.  t_i is clamped to [0, B-1] as the first thing done with it: no value
// of the index list can address memory outside a, p and sq.  One thread per row, the same FMA chain as the tiles.
__global__ __launch_bounds__(256) void k_lrand_keys(const float* __restrict__ a, const float* __restrict__ p,
                                                    const float* __restrict__ sq,
                                                    const long long* __restrict__ tidx, int B, int swap,
                                                    unsigned long long* __restrict__ rowbest,
                                                    unsigned long long* __restrict__ colbest) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const long long raw = tidx[i];
  const int t = (int)(raw < 0 ? 0ll : raw > (long long)(B - 1) ? (long long)(B - 1) : raw);
  const float x = (sq[i] + sq[B + t]) - 2.0f * dot128(a + (size_t)i * D, p + (size_t)t * D);
  rowbest[i] = key_of(masked_dn(x, t == i), t);
  if (swap) {
    const float y = (sq[t] + sq[B + i]) - 2.0f * dot128(a + (size_t)t * D, p + (size_t)i * D);
    colbest[i] = key_of(masked_dn(y, t == i), t);
  }
}

// 1 / (2 sqrt(u)) for entry (i, j): sqrt's backward factor
HN_DEV float half_rsq(const float* a, const float* p, const float* sq, int B, int i, int j) {
  const float x = (sq[i] + sq[B + j]) - 2.0f * dot128(a + (size_t)i * D, p + (size_t)j * D);
  return 0.5f / sqrtf(x + 1e-6f);
}

// per source row: the coefficients of its selected entries (pos (i,i), row negative (i, r_i),
// column negative (c_i, i)) and the indices, as g / (2 sqrt(u)) of each
__global__ __launch_bounds__(256) void k_lmin_bwd_src(const float* __restrict__ a, const float* __restrict__ p,
                                                      const float* __restrict__ sq,
                                                      const unsigned long long* __restrict__ rowbest,
                                                      const unsigned long long* __restrict__ colbest,
                                                      const float* __restrict__ pos,
                                                      const float* __restrict__ posx, int B, int swap, float margin,
                                                      int type, const float* __restrict__ dloss,
                                                      float* __restrict__ coef, int* __restrict__ idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const float g = dloss[0] / (float)B;  // mean's backward
  const float vr = key_val(rowbest[i]);
  const float vc = swap ? key_val(colbest[i]) : INFINITY;
  const float mn = swap ? fminf(vr, vc) : vr;
  float dp, dm;
  loss_of(type, margin, pos[i], mn, &dp, &dm);
  // torch.minimum(row, col): the gradient to the smaller, halves on a tie
  const float fr = !swap || vr < vc ? 1.f : vr > vc ? 0.f : 0.5f;
  const int r = key_idx(rowbest[i]);
  const int c = swap ? key_idx(colbest[i]) : 0;
  const float gp = g * dp, gn = g * dm;
  // the positive entry: sqrt's backward at the forward's own |a_i - p_i|^2 (k_lmin_sq's difference form)
  float wp = gp, w1 = gn * fr, w2 = gn * (1.f - fr);
  // a selected negative that is the row's own masked diagonal (B = 1, or every other entry beyond d_ii + 10) is
  // the positive's entry (i, i): its weight joins the positive's before sqrt's backward, as autograd accumulates
  // the two on d_ii -- the clamp losses' +g and -g then cancel to exactly zero, as there
  if (r == i) {
    wp += w1;
    w1 = 0.f;
  }
  if (swap && c == i) {
    wp += w2;
    w2 = 0.f;
  }
  coef[3 * i + 0] = wp != 0.f ? wp * (0.5f / sqrtf(posx[i] + 1e-6f)) : 0.f;
  coef[3 * i + 1] = w1 != 0.f ? w1 * half_rsq(a, p, sq, B, i, r) : 0.f;
  coef[3 * i + 2] = w2 != 0.f ? w2 * half_rsq(a, p, sq, B, c, i) : 0.f;
  idx[2 * i + 0] = r;
  idx[2 * i + 1] = c;
}

// a selected entry's term: w d u / d self with u = |self|^2 + |other|^2 - 2 self.other + 1e-6
struct L2Term {
  static HN_DEV void add(float2& acc, float w, const float2& self, const float2& o) {
    acc.x = fmaf(w, 2.0f * self.x - 2.0f * o.x, acc.x);
    acc.y = fmaf(w, 2.0f * self.y - 2.0f * o.y, acc.y);
  }
};

}  // namespace

// saved layout (hn_loss_train_saved_bytes): sq [2B] f32 | rowbest [B] u64 | colbest [B] u64 |
// pos [B] f32 | posx [B] f32 (|a_i - p_i|^2) | coef [3B] f32 | idx [2B] i32 | cnt, off, fill, list [2B] i32
// (the backward's source lists)
size_t hn_loss_train_saved_bytes(long B) {
  auto al = [](size_t n) { return (n + 255) / 256 * 256; };
  return al(2 * B * 4) + 2 * al(B * 8) + 2 * al(B * 4) + al(3 * B * 4) + 5 * al(2 * B * 4);
}

namespace {
struct LossSaved {
  float* sq;
  unsigned long long *rowbest, *colbest;
  float* pos;
  float* posx;
  float* coef;
  int* idx;
  int *cnt, *off, *fill, *list;
};
LossSaved loss_saved(void* ws, long B) {
  auto al = [](size_t n) { return (n + 255) / 256 * 256; };
  char* c = static_cast<char*>(ws);
  LossSaved s;
  s.sq = reinterpret_cast<float*>(c);
  c += al(2 * B * 4);
  s.rowbest = reinterpret_cast<unsigned long long*>(c);
  c += al(B * 8);
  s.colbest = reinterpret_cast<unsigned long long*>(c);
  c += al(B * 8);
  s.pos = reinterpret_cast<float*>(c);
  c += al(B * 4);
  s.posx = reinterpret_cast<float*>(c);
  c += al(B * 4);
  s.coef = reinterpret_cast<float*>(c);
  c += al(3 * B * 4);
  s.idx = reinterpret_cast<int*>(c);
  c += al(2 * B * 4);
  s.cnt = reinterpret_cast<int*>(c);
  c += al(2 * B * 4);
  s.off = reinterpret_cast<int*>(c);
  c += al(2 * B * 4);
  s.fill = reinterpret_cast<int*>(c);
  c += al(2 * B * 4);
  s.list = reinterpret_cast<int*>(c);
  return s;
}
}  // namespace

hipError_t hn_launch_loss_train_fwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    float* loss, void* saved, hipStream_t st) {
  const LossSaved s = loss_saved(saved, B);
  hipLaunchKernelGGL(k_lmin_sq, dim3((2 * B + 3) / 4), dim3(256), 0, st, a, p, B, s.sq, s.pos, s.posx);
  if (swap) hipLaunchKernelGGL(k_lmin_init, dim3(std::min((B + 255) / 256, 1024)), dim3(256), 0, st, s.colbest, B);
  hipLaunchKernelGGL(k_lmin_tiles, dim3((B + TM - 1) / TM), dim3(256), 0, st, a, p, s.sq, B, swap, s.rowbest,
                     s.colbest, s.pos);
  hipLaunchKernelGGL(k_lmin_finish, dim3(1), dim3(1024), 0, st, s.rowbest, s.colbest, s.pos, B, swap, margin, type,
                     loss);
  return hipGetLastError();
}

// 'random': the same saved layout; its backward is hn_launch_loss_train_bwd
hipError_t hn_launch_loss_random_fwd(const float* a, const float* p, const long long* tidx, int B, int swap,
                                     float margin, int type, float* loss, void* saved, hipStream_t st) {
  const LossSaved s = loss_saved(saved, B);
  hipLaunchKernelGGL(k_lmin_sq, dim3((2 * B + 3) / 4), dim3(256), 0, st, a, p, B, s.sq, s.pos, s.posx);
  hipLaunchKernelGGL(k_lrand_keys, dim3((B + 255) / 256), dim3(256), 0, st, a, p, s.sq, tidx, B, swap, s.rowbest,
                     s.colbest);
  hipLaunchKernelGGL(k_lmin_finish, dim3(1), dim3(1024), 0, st, s.rowbest, s.colbest, s.pos, B, swap, margin, type,
                     loss);
  return hipGetLastError();
}

hipError_t hn_launch_loss_train_bwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    const float* dloss, float* ga, float* gp, void* saved, hipStream_t st) {
  const LossSaved s = loss_saved(saved, B);
  hipLaunchKernelGGL(k_lmin_bwd_src, dim3((B + 255) / 256), dim3(256), 0, st, a, p, s.sq, s.rowbest, s.colbest,
                     s.pos, s.posx, B, swap, margin, type, dloss, s.coef, s.idx);
  return lmin_bwd_gather_launch<L2Term>(a, p, B, swap, s.coef, s.idx, s.cnt, s.off, s.fill, s.list, ga, gp, st);
}
