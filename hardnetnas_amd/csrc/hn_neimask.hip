// FDLNet's neighbour-mask descriptor loss (FDLNet-master/latency/NASNet/model/des.py:57-96 over
// utils/math_utils.py:8-40, called from model/network.py:307-309) and its backward, without the three N x N
// matrices of the reference formulation.
//
// Forward (k_nm_init + k_nm_tiles + k_nm_finish):
//   u_ij  = 2 - 2 a_i.p_j                      D_ij = sqrt(min(max(u_ij, 1e-8), 4))      pos_i = D_ii
//   m1_ij = [kd(anchor_kp_i, anchor_kp_j) < C]  m2_ij = [kd(positive_kp_i, positive_kp_j) < C]
//   dn_ij = ((D_ij + 10 [i = j]) + 10 m1_ij) + 10 m2_ij      (fp32 additions in the reference's order)
//   mn_i  = min(min_j dn_ij, min_k dn_ki)       loss = mean_i max(MARGIN + pos_i - mn_i, 0)
// kd is pairwise_distances on the (y, x) columns of the [N,4] int64 keypoint rows (b, y, x, 0):
// sqrt(max(d2, 1e-8)) with d2 the squared coordinate distance; the image index b is not used, as in the
// reference.  d2 comes from the integer differences (exactly the reference's expanded fp32 form for
// coordinates below 2,048; DESIGN.md 21 for larger ones) and `kd < C` is evaluated as d2 < T, T the smallest
// fp32 value with !(sqrtf(fmaxf(T, 1e-8f)) < C), found once per call on the host (nm_d2_threshold).
//
// u_ij has one definition: a single FMA chain over k in increasing order (hn_loss_gather.h: lt_tile_dots for
// the tiles, dot128 for the backward's recomputation of the selected entries), then fmaf(-2, dot, 2).  pos_i
// is the diagonal entry of the same tiles, so the backward's clamp test and its 1 / (2 D) see the forward's
// values.
//
// Backward (k_nm_bwd_src + the shared gather): mean passes g / N, the hinge passes at t >= 0, the minima route
// to one argmin each (lowest index on a tie; torch.min(row, col) splits an exact row / column tie in halves),
// sqrt passes 1 / (2 D), the clamp passes only for 1e-8 <= u <= 4, d u_ij / d a_i = -2 p_j, d u_ij / d p_j =
// -2 a_i; keypoints get no gradient.
#include "hn_common.h"
#include "hn_internal.h"
#include "hn_loss_gather.h"

namespace {

constexpr int D = LT_D, TM = LT_TM, TN = LT_TN;
constexpr long long KP_LIM = (1ll << 30) - 1;  // coordinates saturate here: the differences fit an int32

__global__ __launch_bounds__(256) void k_nm_init(unsigned long long* __restrict__ rowbest,
                                                 unsigned long long* __restrict__ colbest, int B) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) rowbest[i] = colbest[i] = ~0ull;
}

HN_DEV int kp_coord(const long long* __restrict__ kp, int row, int col) {
  const long long v = kp[(size_t)row * 4 + col];
  return (int)(v > KP_LIM ? KP_LIM : v < -KP_LIM ? -KP_LIM : v);
}
// [squared coordinate distance < thr]: integer differences, fp32 squares (exact below 2^12 per difference)
HN_DEV bool kp_near(int y0, int x0, int y1, int x1, float thr) {
  const float fy = (float)(y0 - y1), fx = (float)(x0 - x1);
  return fmaf(fy, fy, fx * fx) < thr;
}
HN_DEV float u_of(float dot) { return fmaf(-2.0f, dot, 2.0f); }
HN_DEV float dist_of(float u) { return sqrtf(fminf(fmaxf(u, 1e-8f), 4.0f)); }

// Workgroup (bx, by): anchors 64 bx .. 64 bx + 63 against the 64-column tiles by, by + gridDim.y, ...; thread
// (ty, tx) the 4 x 4 block rows 4ty.. x columns 4tx.. of a tile, as k_lmin_tiles (hn_loss.hip).  The masks are
// evaluated here from the (y, x) of the block's 4 rows and 4 columns in both keypoint sets; row and column
// minima leave as one u64 atomicMin per row / column per workgroup.
__global__ __launch_bounds__(256) void k_nm_tiles(const float* __restrict__ a, const float* __restrict__ p,
                                                  const long long* __restrict__ akp,
                                                  const long long* __restrict__ pkp, int B, float thr,
                                                  unsigned long long* __restrict__ rowbest,
                                                  unsigned long long* __restrict__ colbest,
                                                  float* __restrict__ pos) {
  __shared__ float4 As[D][TM / 4];
  __shared__ float4 Ps[D][TN / 4];
  __shared__ unsigned long long red[16][TN];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.x * TM;
  lt_load_kmajor(reinterpret_cast<float*>(&As[0][0]), a, r0, B, tid);
  int ray[4], rax[4], rpy[4], rpx[4];  // the rows' (y, x) in the anchor and the positive keypoints
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = r0 + 4 * ty + r;
    const bool in = i < B;
    ray[r] = in ? kp_coord(akp, i, 1) : 0;
    rax[r] = in ? kp_coord(akp, i, 2) : 0;
    rpy[r] = in ? kp_coord(pkp, i, 1) : 0;
    rpx[r] = in ? kp_coord(pkp, i, 2) : 0;
  }
  unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  for (int c0 = blockIdx.y * TN; c0 < B; c0 += gridDim.y * TN) {
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
      const int cay = kp_coord(akp, j, 1), cax = kp_coord(akp, j, 2);
      const int cpy = kp_coord(pkp, j, 1), cpx = kp_coord(pkp, j, 2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = r0 + 4 * ty + r;
        if (i >= B) continue;
        const float d = dist_of(u_of(acc[r][c]));
        float dn = d;
        if (i == j) {
          pos[i] = d;
          dn = d + 10.0f;
        }
        if (kp_near(ray[r], rax[r], cay, cax, thr)) dn += 10.0f;
        if (kp_near(rpy[r], rpx[r], cpy, cpx, thr)) dn += 10.0f;
        best[r] = umin64(best[r], key_of(dn, j));
        cb[c] = umin64(cb[c], key_of(dn, i));
      }
    }
    // column minima over the workgroup's 64 rows -> one atomic per column
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
  // row minima over the 16 threads (tx) sharing a row, then over the workgroups sharing the rows
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) red[tx][4 * ty + r] = best[r];
  __syncthreads();
  if (tid < TM && r0 + tid < B) {
    unsigned long long m = red[0][tid];
#pragma unroll
    for (int t = 1; t < 16; ++t) m = umin64(m, red[t][tid]);
    atomicMin(rowbest + r0 + tid, m);
  }
}

// the hinge max(margin + pos - mn, 0); clamp's backward passes at t >= 0 (loss_of's convention, hn_loss.hip)
HN_DEV float hinge_of(float margin, float ps, float mn, float* dpos) {
  const float t = margin + ps - mn;
  *dpos = t >= 0.f ? 1.f : 0.f;
  return fmaxf(t, 0.f);
}

// one workgroup: the per-row losses in fp32 (as the reference computes them), their sum in fp64 in a fixed
// order (deterministic); pos / min_neg copied out where asked for
__global__ __launch_bounds__(1024) void k_nm_finish(const unsigned long long* __restrict__ rowbest,
                                                    const unsigned long long* __restrict__ colbest,
                                                    const float* __restrict__ pos, int B, float margin,
                                                    float* __restrict__ loss, float* __restrict__ pos_out,
                                                    float* __restrict__ mn_out) {
  __shared__ double part[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 1024) {
    const float mn = fminf(key_val(rowbest[i]), key_val(colbest[i]));
    float dp;
    s += (double)hinge_of(margin, pos[i], mn, &dp);
    if (pos_out) pos_out[i] = pos[i];
    if (mn_out) mn_out[i] = mn;
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

// w / (2 D_ij) where the clamp passes (1e-8 <= u_ij <= 4, so D_ij = sqrt(u_ij)), else 0
HN_DEV float entry_coef(const float* a, const float* p, int i, int j, float w) {
  if (w == 0.f) return 0.f;
  const float u = u_of(dot128(a + (size_t)i * D, p + (size_t)j * D));
  return u >= 1e-8f && u <= 4.0f ? w * (0.5f / sqrtf(u)) : 0.f;
}

// per source row: the coefficients of its selected entries (pos (i,i), row negative (i, r_i), column negative
// (c_i, i)) and the indices (the layout of hn_loss_gather.h)
__global__ __launch_bounds__(256) void k_nm_bwd_src(const float* __restrict__ a, const float* __restrict__ p,
                                                    const unsigned long long* __restrict__ rowbest,
                                                    const unsigned long long* __restrict__ colbest,
                                                    const float* __restrict__ pos, int B, float margin,
                                                    const float* __restrict__ dloss, float* __restrict__ coef,
                                                    int* __restrict__ idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const float g = dloss[0] / (float)B;  // mean's backward
  const float vr = key_val(rowbest[i]), vc = key_val(colbest[i]);
  float dp;
  hinge_of(margin, pos[i], fminf(vr, vc), &dp);
  // torch.min(row, col): the gradient to the smaller, halves on a tie
  const float fr = vr < vc ? 1.f : vr > vc ? 0.f : 0.5f;
  const int r = key_idx(rowbest[i]), c = key_idx(colbest[i]);
  const float gp = g * dp, gn = -gp;
  coef[3 * i + 0] = entry_coef(a, p, i, i, gp);
  coef[3 * i + 1] = entry_coef(a, p, i, r, gn * fr);
  coef[3 * i + 2] = entry_coef(a, p, c, i, gn * (1.f - fr));
  idx[2 * i + 0] = r;
  idx[2 * i + 1] = c;
}

// a selected entry's term: w d u / d self with u = 2 - 2 self.other
struct UnitTerm {
  static HN_DEV void add(float2& acc, float w, const float2&, const float2& o) {
    acc.x = fmaf(w, -2.0f * o.x, acc.x);
    acc.y = fmaf(w, -2.0f * o.y, acc.y);
  }
};

// saved layout (hn_neimask_saved_bytes): rowbest [B] u64 | colbest [B] u64 | pos [B] f32 | coef [3B] f32 |
// idx [2B] i32 | cnt, off, fill, list [2B] i32 (the backward's source lists); each block 256-byte aligned.
// The forward writes rowbest, colbest and pos; the backward writes the rest before it reads it.
size_t al256(size_t n) { return (n + 255) / 256 * 256; }
struct NeiSaved {
  unsigned long long *rowbest, *colbest;
  float* pos;
  float* coef;
  int* idx;
  int *cnt, *off, *fill, *list;
};
NeiSaved nei_saved(void* ws, long B) {
  char* c = static_cast<char*>(ws);
  auto take = [&](size_t n) {
    char* r = c;
    c += al256(n);
    return r;
  };
  NeiSaved s;
  s.rowbest = reinterpret_cast<unsigned long long*>(take(B * 8));
  s.colbest = reinterpret_cast<unsigned long long*>(take(B * 8));
  s.pos = reinterpret_cast<float*>(take(B * 4));
  s.coef = reinterpret_cast<float*>(take(3 * B * 4));
  s.idx = reinterpret_cast<int*>(take(2 * B * 4));
  s.cnt = reinterpret_cast<int*>(take(2 * B * 4));
  s.off = reinterpret_cast<int*>(take(2 * B * 4));
  s.fill = reinterpret_cast<int*>(take(2 * B * 4));
  s.list = reinterpret_cast<int*>(take(2 * B * 4));
  return s;
}

// kd < C for the squared distance d2 >= 0: sqrtf and fmaxf are monotone, so the set is d2 < T with T the
// smallest non-negative fp32 value (in bit order: 0 .. +inf) for which the reference's comparison fails
bool nm_near(float d2, float C) { return sqrtf(fmaxf(d2, 1e-8f)) < C; }
float nm_d2_threshold(float C) {
  uint32_t lo = 0, hi = 0x7f800000u;  // nm_near(+inf, C) is false for every C
  auto val = [](uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
  };
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (nm_near(val(mid), C)) lo = mid + 1; else hi = mid;
  }
  return val(lo);
}

}  // namespace

size_t hn_neimask_saved_bytes(long B) {
  return 2 * al256(B * 8) + al256(B * 4) + al256(3 * B * 4) + 5 * al256(2 * B * 4);
}

hipError_t hn_launch_neimask_fwd(const float* a, const float* p, const long long* akp, const long long* pkp, int B,
                                 float margin, float coo_thresh, float* loss, float* pos_out, float* mn_out,
                                 void* saved, hipStream_t st) {
  const NeiSaved s = nei_saved(saved, B);
  const int rows = (B + TM - 1) / TM, tiles = (B + TN - 1) / TN;
  // column tiles spread over grid.y until about two workgroups per CU are in flight (a small batch has few rows)
  const int split = std::max(1, std::min(tiles, 512 / rows));
  hipLaunchKernelGGL(k_nm_init, dim3(std::min((B + 255) / 256, 1024)), dim3(256), 0, st, s.rowbest, s.colbest, B);
  hipLaunchKernelGGL(k_nm_tiles, dim3(rows, split), dim3(256), 0, st, a, p, akp, pkp, B, nm_d2_threshold(coo_thresh),
                     s.rowbest, s.colbest, s.pos);
  hipLaunchKernelGGL(k_nm_finish, dim3(1), dim3(1024), 0, st, s.rowbest, s.colbest, s.pos, B, margin, loss, pos_out,
                     mn_out);
  return hipGetLastError();
}

hipError_t hn_launch_neimask_bwd(const float* a, const float* p, int B, float margin, const float* dloss, float* ga,
                                 float* gp, void* saved, hipStream_t st) {
  const NeiSaved s = nei_saved(saved, B);
  hipLaunchKernelGGL(k_nm_bwd_src, dim3((B + 255) / 256), dim3(256), 0, st, a, p, s.rowbest, s.colbest, s.pos, B,
                     margin, dloss, s.coef, s.idx);
  return lmin_bwd_gather_launch<UnitTerm>(a, p, B, 1, s.coef, s.idx, s.cnt, s.off, s.fill, s.list, ga, gp, st);
}
