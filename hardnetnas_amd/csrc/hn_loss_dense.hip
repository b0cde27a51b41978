// Train-mode loss_HardNet with batch_reduce 'average' (hardnet/Losses.py:124-130) and its backward, without
// the B x B matrix: every one of the B^2 masked entries is a negative, paired -- as the reference's
// pos1.repeat(B) pairs it -- with the positive distance of its COLUMN.
//
//   u_ij  = (|a_i|^2 + |p_j|^2) - 2 a_i.p_j,  d_ij = sqrt(u_ij + 1e-6) + 1e-8
//   dn_ij = d_ij + 10 [i = j];  dn_ij += 10 if dn_ij < 0.008
//   m_ij  = anchor_swap ? min(dn_ij, dn_ji) : dn_ij
//   loss  = (1 / B^2) sum_ij f(pos_j, m_ij)        (f, its partials: loss_of; pos_j from the difference form)
//
// Backward, as autograd differentiates that, with g = dloss / B^2 and G_ij = g df/dmn at entry (i, j):
//   c_ij  = G_ij, with swap s_ij (G_ij + G_ji): s_ij = 1 if dn_ij < dn_ji, 0 if greater, 1/2 on an exact tie
//           (torch.minimum's backward; 1 - s_ji = s_ij)
//   W_ij  = c_ij / (2 sqrt(u_ij + 1e-6)) for i != j;  the diagonal's c_ii = G_ii joins the positive's weight
//   wpos_i   = (g sum_k df/dpos(k, i) + c_ii) / (2 sqrt(|a_i - p_i|^2 + 1e-6))
//   grad_a_i = 2 (sum_j W_ij) a_i - 2 sum_j W_ij p_j + 2 wpos_i (a_i - p_i)
//   grad_p_j = 2 (sum_i W_ij) p_j - 2 sum_i W_ij a_i + 2 wpos_j (p_j - a_j)
//
// One kernel shape does all of it (k_ldense).  A workgroup of four waves OWNS 64 rows of one side and walks the
// other side in 64-row tiles; both operands of a tile lie k-major in LDS and the 64 x 64 x 128 product runs on
// the f32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit the k-ordered fmaf chain of lt_tile_dots, one 32 x 32
// block per wave).  With anchor_swap the transposed tile (the other matrix's rows at the same indices) is a
// second product beside it.  The forward owns positives (columns: the per-column sums of f and df/dpos are row
// sums of the owner); the backward runs twice in one launch, once owning anchors (-> grad_a) and once owning
// positives (-> grad_p): the weight tile W goes through LDS into a second MFMA product W . other[64][128] whose
// result stays in registers across the walk.  Both passes form u_ij by the same operations on the same values
// (products commute, the k order is the same), so they take the same s_ij decisions; no float atomics anywhere.
// The walk is split over several workgroups per row block so that a small batch fills the machine; the partial
// sums of the splits are combined in split order by k_ldense_finish / k_ldense_combine: results are bit-identical
// call to call.  Nothing B^2-sized is written: the saved state is O(B) plus the split partials.
#include <algorithm>

#include "hn_common.h"
#include "hn_internal.h"
#include "hn_loss_terms.h"

namespace {

constexpr int D = 128;        // descriptor length
constexpr int T = 64;         // rows per owner block and per walked tile
constexpr int LDK = T + 1;    // k-major operand [D][LDK]: the padding keeps both products' reads off one bank
constexpr int OPER = D * LDK;  // floats per operand (33,280 bytes)

// the walk's split: `per` tiles per workgroup, ns workgroups per row block -- a function of B alone
struct DenseSplit {
  int nrb, per, ns;
};
DenseSplit dense_split(int B) {
  DenseSplit s;
  s.nrb = (B + T - 1) / T;
  const int want = std::min(std::max(256 / s.nrb, 2), s.nrb);
  s.per = (s.nrb + want - 1) / want;
  s.ns = (s.nrb + s.per - 1) / s.per;
  return s;
}

// rows [r0, r0 + 64) of src [B][128] -> lds[128][LDK] (k-major); rows past B are zero
HN_DEV void load_kmajor(float* __restrict__ lds, const float* __restrict__ src, int r0, int B, int tid) {
  for (int e = tid; e < T * D / 4; e += 256) {
    const int row = e % T, k4 = e / T;  // consecutive threads: consecutive rows (conflict-free LDS stores)
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < B) v = reinterpret_cast<const float4*>(src + (size_t)(r0 + row) * D)[k4];
    lds[(4 * k4 + 0) * LDK + row] = v.x;
    lds[(4 * k4 + 1) * LDK + row] = v.y;
    lds[(4 * k4 + 2) * LDK + row] = v.z;
    lds[(4 * k4 + 3) * LDK + row] = v.w;
  }
}

// one 32 x 32 block of own[64][128] . other[64][128]^T: rows 32 rb.., columns 32 cb.. (lane: A[row l & 31][k = l >> 5],
// B[k = l >> 5][column l & 31]; result register q: row (q & 3) + 8 (q >> 2) + 4 (l >> 5), column l & 31)
HN_DEV f32x16 block_dots(const float* __restrict__ own, const float* __restrict__ oth, int rb, int cb, int lane) {
  const int l32 = lane & 31, half = lane >> 5;
  const float* ao = own + half * LDK + rb * 32 + l32;
  const float* bo = oth + half * LDK + cb * 32 + l32;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int s = 0; s < D / 2; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[2 * s * LDK], bo[2 * s * LDK], acc, 0, 0, 0);
  return acc;
}

// Saved layout: sq [2B] f32 | pos [B] | posx [B] | cdiag [B] (df/dmn at the diagonal entry) | dpos [B] (the
// column sums of df/dpos) | lossp [ns][B] f64, dposp [ns][B] f32 (the forward's split partials) |
// wsum [2][ns][B] f32, gpart [2][ns][B][128] f32 (the backward's: side 0 anchors, 1 positives)
struct DenseSaved {
  float *sq, *pos, *posx, *cdiag, *dpos;
  double* lossp;
  float *dposp, *wsum, *gpart;
  size_t bytes;
};
DenseSaved dense_saved(void* ws, long B) {
  auto al = [](size_t n) { return (n + 255) / 256 * 256; };
  const size_t nsB = (size_t)dense_split((int)B).ns * (size_t)B;
  char* c = static_cast<char*>(ws);
  char* const c0 = c;
  DenseSaved s;
  auto take = [&](size_t n) {
    char* r = c;
    c += al(n);
    return r;
  };
  s.sq = reinterpret_cast<float*>(take(2 * B * 4));
  s.pos = reinterpret_cast<float*>(take(B * 4));
  s.posx = reinterpret_cast<float*>(take(B * 4));
  s.cdiag = reinterpret_cast<float*>(take(B * 4));
  s.dpos = reinterpret_cast<float*>(take(B * 4));
  s.lossp = reinterpret_cast<double*>(take(nsB * 8));
  s.dposp = reinterpret_cast<float*>(take(nsB * 4));
  s.wsum = reinterpret_cast<float*>(take(2 * nsB * 4));
  s.gpart = reinterpret_cast<float*>(take(2 * nsB * D * 4));
  s.bytes = (size_t)(c - c0);
  return s;
}

size_t dense_lds_bytes(bool bwd, int swap) {
  return sizeof(float) * ((size_t)(swap ? 4 : 2) * OPER + (bwd ? T * LDK : 0));
}

// BWD = false: the forward (owns positives).  BWD = true: blockIdx.z = 0 owns anchors, 1 positives.
// grid (row blocks, splits, BWD ? 2 : 1); dynamic LDS: Xs, Ys [, Zs, Vs with swap] [, Ws in the backward].
template <bool BWD>
__global__ __launch_bounds__(256) void k_ldense(const float* __restrict__ a, const float* __restrict__ p,
                                                const float* __restrict__ sq, const float* __restrict__ pos, int B,
                                                int swap, float margin, int type, int per,
                                                const float* __restrict__ dloss, double* __restrict__ lossp,
                                                float* __restrict__ dposp, float* __restrict__ cdiag,
                                                float* __restrict__ wsum, float* __restrict__ gpart) {
  extern __shared__ float4 dense_lds[];
  float* const Xs = reinterpret_cast<float*>(dense_lds);  // own rows of the own side
  float* const Ys = Xs + OPER;                            // walked rows of the other side
  float* const Zs = Ys + OPER;                            // swap: own rows of the other side
  float* const Vs = Zs + OPER;                            // swap: walked rows of the own side
  float* const Ws = Xs + (swap ? 4 : 2) * OPER;           // backward: the weight tile [own 64][LDK]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, half = lane >> 5;
  const int rb = wave >> 1, cb = wave & 1;
  const bool own_a = BWD && blockIdx.z == 0;
  const float* const X = own_a ? a : p;  // the own side's matrix; Z the other's
  const float* const Z = own_a ? p : a;
  const float* const sqX = own_a ? sq : sq + B;
  const float* const sqZ = own_a ? sq + B : sq;
  const int r0 = blockIdx.x * T, nrb = (B + T - 1) / T;
  const int t0 = blockIdx.y * per, t1 = min(t0 + per, nrb);
  const size_t part = ((size_t)(BWD ? blockIdx.z : 0) * gridDim.y + blockIdx.y) * (size_t)B;  // this split's rows

  load_kmajor(Xs, X, r0, B, tid);
  if (swap) load_kmajor(Zs, Z, r0, B, tid);
  // this lane's 16 own rows: |x|^2 on both sides and the positive distance
  float sx[16], sz[16], pown[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int oi = r0 + rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
    const bool in = oi < B;
    sx[q] = in ? sqX[oi] : 0.f;
    sz[q] = in ? sqZ[oi] : 0.f;
    pown[q] = in ? pos[oi] : 0.f;
  }
  const float g = BWD ? dloss[0] / ((float)B * (float)B) : 0.f;  // the mean's backward
  double lsum[16];
  float fsum[16];  // forward: df/dpos; backward: the weights
#pragma unroll
  for (int q = 0; q < 16; ++q) lsum[q] = 0.0, fsum[q] = 0.f;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 g0 = zero16, g1 = zero16;  // backward: rows 32 rb.., dims 64 cb.. and 64 cb + 32..

  for (int t = t0; t < t1; ++t) {
    const int c0 = t * T;
    __syncthreads();  // the previous tile's readers are done with Ys / Vs / Ws
    load_kmajor(Ys, Z, c0, B, tid);
    if (swap) load_kmajor(Vs, X, c0, B, tid);
    __syncthreads();
    const f32x16 s1 = block_dots(Xs, Ys, rb, cb, lane);
    const f32x16 s2 = swap ? block_dots(Zs, Vs, rb, cb, lane) : zero16;
    const int oth = c0 + cb * 32 + l32;
    const bool oin = oth < B;
    const float sy = oin ? sqZ[oth] : 0.f, sv = oin ? sqX[oth] : 0.f, poth = oin ? pos[oth] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * half, oi = r0 + row;
      const bool valid = oin && oi < B, diag = oi == oth;
      // the entry whose weight the owner needs, and with swap its transpose (i and j exchanged)
      const float u1 = (sx[q] + sy) - 2.0f * s1[q];
      const float dn1 = masked_dn(u1, diag);
      float dn2 = dn1, m = dn1;
      if (swap) {
        dn2 = masked_dn((sz[q] + sv) - 2.0f * s2[q], diag);
        m = fminf(dn1, dn2);
      }
      float dp, dm;
      if (!BWD) {  // own = the column: f(pos_own, m)
        const float f = loss_of(type, margin, pown[q], m, &dp, &dm);
        if (valid) {
          lsum[q] += (double)f;
          fsum[q] += dp;
          if (diag) cdiag[oi] = dm;  // (one writer: the diagonal lies in one tile of one split)
        }
      } else {
        // entry 1 pairs with the positive of its column: the walked row when anchors own, else the own row
        loss_of(type, margin, own_a ? poth : pown[q], m, &dp, &dm);
        float c = dm;
        if (swap) {
          float dm2;
          loss_of(type, margin, own_a ? pown[q] : poth, m, &dp, &dm2);
          const float s = dn1 < dn2 ? 1.f : dn1 > dn2 ? 0.f : 0.5f;
          c = s * (dm + dm2);
        }
        const float w = valid && !diag ? (g * c) * (0.5f / sqrtf(u1 + 1e-6f)) : 0.f;
        fsum[q] += w;
        Ws[row * LDK + cb * 32 + l32] = w;
      }
    }
    if (BWD) {
      __syncthreads();  // the weight tile is complete
      // G[own 64][128] += W[own 64][walked 64] . Y[walked 64][128]: Y[k][d] = Ys[d * LDK + k]
      const float* wo = Ws + (rb * 32 + l32) * LDK + half;
      const float* y0 = Ys + (cb * 64 + l32) * LDK + half;
      const float* y1 = y0 + 32 * LDK;
#pragma unroll 8
      for (int s = 0; s < T / 2; ++s) {
        const float wv = wo[2 * s];
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, y0[2 * s], g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, y1[2 * s], g1, 0, 0, 0);
      }
    }
  }

  // row sums: over the 32 lanes of a half-wave, then over the two waves (cb) of a row block, in that order
  __syncthreads();  // Ys is free: it holds the two waves' sums
  double(*redd)[T] = reinterpret_cast<double(*)[T]>(Ys);
  float(*redf)[T] = reinterpret_cast<float(*)[T]>(Ys + 4 * T);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
    float f = fsum[q];
    double l = lsum[q];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      f += __shfl_xor(f, o, 64);
      if (!BWD) l += __shfl_xor(l, o, 64);
    }
    if (l32 == 0) {
      redf[cb][row] = f;
      if (!BWD) redd[cb][row] = l;
    }
  }
  __syncthreads();
  if (tid < T && r0 + tid < B) {
    const float f = redf[0][tid] + redf[1][tid];
    if (!BWD) {
      lossp[part + r0 + tid] = redd[0][tid] + redd[1][tid];
      dposp[part + r0 + tid] = f;
    } else {
      wsum[part + r0 + tid] = f;
    }
  }
  if (BWD) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int oi = r0 + rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
      if (oi < B) {
        float* dst = gpart + (part + oi) * D + cb * 64 + l32;
        dst[0] = g0[q];
        dst[32] = g1[q];
      }
    }
  }
}

// one workgroup: the column sums of df/dpos over the splits and the mean, both in a fixed order
__global__ __launch_bounds__(1024) void k_ldense_finish(const double* __restrict__ lossp,
                                                        const float* __restrict__ dposp, int B, int ns,
                                                        float* __restrict__ dpos, float* __restrict__ loss) {
  __shared__ double part[16];
  double s = 0.0;
  for (int j = threadIdx.x; j < B; j += 1024) {
    float d = 0.f;
    for (int k = 0; k < ns; ++k) {
      s += lossp[(size_t)k * B + j];
      d += dposp[(size_t)k * B + j];
    }
    dpos[j] = d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    loss[0] = (float)(t / ((double)B * (double)B));
  }
}

// one wave per target row (t < B: anchor t, else positive t - B), two dims per lane: the splits' partial sums in
// split order, then the row's own terms
__global__ __launch_bounds__(256) void k_ldense_combine(const float* __restrict__ a, const float* __restrict__ p,
                                                        const float* __restrict__ posx,
                                                        const float* __restrict__ dpos,
                                                        const float* __restrict__ cdiag,
                                                        const float* __restrict__ wsum,
                                                        const float* __restrict__ gpart, int B, int ns,
                                                        const float* __restrict__ dloss, float* __restrict__ ga,
                                                        float* __restrict__ gp) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= 2 * B) return;
  const int side = t < B ? 0 : 1, i = t - side * B;
  float ws = 0.f;
  float2 acc = make_float2(0.f, 0.f);
  for (int k = 0; k < ns; ++k) {
    const size_t r = ((size_t)side * ns + k) * (size_t)B + i;
    ws += wsum[r];
    const float2 v = reinterpret_cast<const float2*>(gpart + r * D)[lane];
    acc.x += v.x;
    acc.y += v.y;
  }
  const float g = dloss[0] / ((float)B * (float)B);
  const float wpos = (g * dpos[i] + g * cdiag[i]) * (0.5f / sqrtf(posx[i] + 1e-6f));
  const float2 av = reinterpret_cast<const float2*>(a + (size_t)i * D)[lane];
  const float2 pv = reinterpret_cast<const float2*>(p + (size_t)i * D)[lane];
  const float2 self = side ? pv : av, other = side ? av : pv;
  float2 out;
  out.x = 2.0f * ws * self.x - 2.0f * acc.x + 2.0f * wpos * (self.x - other.x);
  out.y = 2.0f * ws * self.y - 2.0f * acc.y + 2.0f * wpos * (self.y - other.y);
  reinterpret_cast<float2*>((side ? gp : ga) + (size_t)i * D)[lane] = out;
}

template <bool BWD>
hipError_t dense_lds_attr(int swap) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ldense<BWD>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)dense_lds_bytes(BWD, swap));
}

}  // namespace

size_t hn_loss_dense_saved_bytes(long B) { return dense_saved(nullptr, B).bytes; }

hipError_t hn_launch_loss_dense_fwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    float* loss, void* saved, hipStream_t st) {
  const DenseSaved s = dense_saved(saved, B);
  const DenseSplit sp = dense_split(B);
  if (hipError_t e = dense_lds_attr<false>(1)) return e;
  hipLaunchKernelGGL(k_lmin_sq, dim3((2 * B + 3) / 4), dim3(256), 0, st, a, p, B, s.sq, s.pos, s.posx);
  hipLaunchKernelGGL(k_ldense<false>, dim3(sp.nrb, sp.ns, 1), dim3(256), dense_lds_bytes(false, swap), st, a, p, s.sq,
                     s.pos, B, swap, margin, type, sp.per, nullptr, s.lossp, s.dposp, s.cdiag, nullptr, nullptr);
  hipLaunchKernelGGL(k_ldense_finish, dim3(1), dim3(1024), 0, st, s.lossp, s.dposp, B, sp.ns, s.dpos, loss);
  return hipGetLastError();
}

hipError_t hn_launch_loss_dense_bwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    const float* dloss, float* ga, float* gp, void* saved, hipStream_t st) {
  const DenseSaved s = dense_saved(saved, B);
  const DenseSplit sp = dense_split(B);
  if (hipError_t e = dense_lds_attr<true>(1)) return e;
  hipLaunchKernelGGL(k_ldense<true>, dim3(sp.nrb, sp.ns, 2), dim3(256), dense_lds_bytes(true, swap), st, a, p, s.sq,
                     s.pos, B, swap, margin, type, sp.per, dloss, nullptr, nullptr, nullptr, s.wsum, s.gpart);
  hipLaunchKernelGGL(k_ldense_combine, dim3((2 * B + 3) / 4), dim3(256), 0, st, a, p, s.posx, s.dpos, s.cdiag, s.wsum,
                     s.gpart, B, sp.ns, dloss, ga, gp);
  return hipGetLastError();
}
