// Keypoint selection on device: RFDet.process followed by Network.inference's second topk_map, nonzero() and
// gathers (FDLNet-master/latency/NASNet/model/det.py:96-133, model/network.py:155-183,
// utils/image_utils.py:197-274) for any [B,H,W] score map.  Built without fast-math: every comparison is IEEE.
//
// Four launches, no float atomics, no host round trip (the output count is exactly B K):
//   k_sel_nms   v = f keep: f the score inside the border (NaN counts as 0), t = f < thresh ? 0 : f, keep where
//               t >= the maximum of t over the ksize x ksize window with 0 outside the image.
//   k_sel_topk  (dense form) one 1,024-thread workgroup per image: an 8-bit radix SELECT over the order-preserving
//               integer keys of v finds the K-th largest key and how many of its ties belong to the K.  The first
//               histogram pass reads the image (16 elements per thread in flight, LDS integer atomics, lanes that
//               share a digit add once); if the chosen bin holds at most 8,192 keys they are gathered into LDS and the
//               other three passes run there, else they read the image again.  Then one ordered pass over the image
//               (wave scans + a running carry, one barrier per 16,384 elements) takes the ties in flat-index order
//               and writes g = v mask (and the mask).
//   k_sel_blur  q = clamp(conv(g, psf), 0, 1) per 16 x 16 tile from LDS: up to 225 taps in row-major order, table
//               computed on the host; a tile whose window holds no nonzero pixel is written as zeros at once.
//   k_sel_topk  (keypoint form) the same select on q; the ordered pass is a compaction that emits the K pixels in
//               raster order straight to their rows: position = (greater keys before) + min(ties before, ties taken).
// Both top-K steps order pixels by (value descending, flat index ascending) whatever order workgroups finish in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hardnet_mi355x.h"
#include "hn_internal.h"

namespace {

constexpr int kSelThreads = 1024;
constexpr int kPer = 16;                       // elements per thread and iteration
constexpr int kChunk = kSelThreads * kPer;
constexpr int kGroups = kPer / 4;               // the ordered pass's groups of 4 consecutive elements per thread

__device__ __forceinline__ float clean(float v) { return v != v ? 0.f : v; }

// order-preserving key of a float that is not NaN; -0 and +0 share a key
__device__ __forceinline__ uint32_t to_key(float v) {
  const uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_sel_nms(const float* __restrict__ s, int64_t total, int H, int W, int border,
                                                 float thresh, int ksize, float* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t HW = (int64_t)H * W;
  const int64_t b = i / HW;
  const int rem = (int)(i - b * HW);
  const int y = rem / W, x = rem % W;
  const float* img = s + b * HW;
  const int pad = ksize / 2;
  auto tval = [&](int yy, int xx) -> float {
    if (yy < border || yy >= H - border || xx < border || xx >= W - border) return 0.f;
    const float f = clean(img[(int64_t)yy * W + xx]);
    return f < thresh ? 0.f : f;
  };
  float out = 0.f;
  if (y >= border && y < H - border && x >= border && x < W - border) {
    const float f = clean(img[rem]);
    if (f != 0.f) {
      const float c = f < thresh ? 0.f : f;
      const int ya = max(y - pad, 0), yb = min(y + pad, H - 1), xa = max(x - pad, 0), xb = min(x + pad, W - 1);
      const bool clipped = y - pad < 0 || y + pad > H - 1 || x - pad < 0 || x + pad > W - 1;
      float m = clipped ? 0.f : -INFINITY;
      for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx) m = fmaxf(m, tval(yy, xx));
      if (c >= m) out = f;
    }
  }
  v[i] = out;
}

struct Taps {
  float w[225];
};

constexpr int kBlurTile = 16;
constexpr int kBlurSpan = kBlurTile + 14;  // a tile's window at the widest kernel

// One 16 x 16 tile of q per workgroup: the tile's (16 + 2 pad)^2 window of g goes to LDS (zero outside the image:
// a zero product leaves the accumulator as it is, so the sum equals the in-image taps in row-major order); a
// window without a nonzero pixel -- nearly all of them, g has at most K per image -- is written as zeros at once.
__global__ __launch_bounds__(256) void k_sel_blur(const float* __restrict__ g, int H, int W, int tiles_x, int tiles,
                                                  int ksize, Taps taps, float* __restrict__ q,
                                                  float* __restrict__ q_out) {
  __shared__ float s_g[kBlurSpan * kBlurSpan];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int y0 = (tile / tiles_x) * kBlurTile, x0 = (tile % tiles_x) * kBlurTile;
  const int pad = ksize / 2, span = kBlurTile + 2 * pad;
  const float* img = g + b * (int64_t)H * W;
  int any = 0;
  for (int i = t; i < span * span; i += 256) {
    const int y = y0 - pad + i / span, x = x0 - pad + i % span;
    const float v = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? img[(int64_t)y * W + x] : 0.f;
    s_g[i] = v;
    any |= v != 0.f;
  }
  any = __syncthreads_or(any);
  const int ty = t / kBlurTile, tx = t % kBlurTile;
  const int y = y0 + ty, x = x0 + tx;
  if (y >= H || x >= W) return;
  float a = 0.f;
  if (any) {
    for (int ky = 0; ky < ksize; ++ky)
      for (int kx = 0; kx < ksize; ++kx) a = fmaf(s_g[(ty + ky) * span + tx + kx], taps.w[ky * ksize + kx], a);
    a = fminf(fmaxf(a, 0.f), 1.f);
  }
  const int64_t o = b * (int64_t)H * W + (int64_t)y * W + x;
  q[o] = a;
  if (q_out) q_out[o] = a;
}

struct SelOut {
  // dense form
  float* g;
  uint8_t* mask;
  // keypoint form
  const float* score;
  const float* scale_map;
  float scale_value;
  const float* ori_map;
  int64_t* kpts;
  float* kscore;
  float* kscale;
  float* kori;
};

constexpr int kCand = 8192;  // keys of the first pass's chosen bin kept in LDS for the other three passes

// one count into a wave's LDS histogram (uniform control flow required): the lanes sharing the first active
// lane's digit add once, twice over -- that takes the zeros that fill these maps whichever lane comes first --
// and what is left (distinct digits, mostly) adds lane by lane
__device__ __forceinline__ void hist_add(uint32_t* s_hist, bool act, uint32_t d, int lane) {
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long remn = __ballot(act);
    if (!remn) return;
    const int leader = __ffsll((long long)remn) - 1;
    const uint32_t ld = __shfl(d, leader, 64);
    const unsigned long long peers = __ballot(act && d == ld);
    if (lane == leader) atomicAdd(&s_hist[ld], (uint32_t)__popcll(peers));
    act = act && d != ld;
  }
  if (act) atomicAdd(&s_hist[d], 1u);
}

// wave 0: the highest digit d with (count of higher digits) < need <= (that + hist[d]); s_sel = {d, what is still
// needed inside d, hist[d]}.  Lane l owns digits 4l .. 4l+3; a suffix scan over the lanes finds the owner.
__device__ __forceinline__ void pick_digit(const uint32_t* s_hist, uint32_t need, uint32_t* s_sel, int lane) {
  uint32_t h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = s_hist[4 * lane + k];
  const uint32_t tot = h[0] + h[1] + h[2] + h[3];
  uint32_t suf = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t dn = __shfl_down(suf, d, 64);
    if (lane + d < 64) suf += dn;
  }
  const uint32_t above = suf - tot;
  if (above < need && need <= above + tot) {
    need -= above;
    int d = 3;
    for (; d > 0; --d) {
      if (h[d] >= need) break;
      need -= h[d];
    }
    s_sel[0] = (uint32_t)(4 * lane + d);
    s_sel[1] = need;
    s_sel[2] = h[d];
  }
}

template <bool KEYPOINTS>
__global__ __launch_bounds__(kSelThreads) void k_sel_topk(const float* __restrict__ src, int H, int W, int K,
                                                          SelOut o) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_sel[3];        // chosen digit, ties still to take, keys in the chosen bin
  __shared__ uint32_t s_tot[2][kGroups][16];  // the ordered pass's wave totals, double buffered
  __shared__ uint32_t s_cand[kCand];
  __shared__ uint32_t s_ncand;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t b = blockIdx.x;
  const int N = H * W;
  const float* in = src + b * (int64_t)N;

  uint32_t prefix = 0, mask = 0, kr = (uint32_t)K;
  bool in_lds = false;
  uint32_t ncand = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (t < 256) s_hist[t] = 0;
    if (t == 0) s_ncand = 0;
    __syncthreads();
    if (in_lds) {
      for (uint32_t i = t; i < ncand; i += kSelThreads) {
        const uint32_t key = s_cand[i];
        if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
    } else {
      for (int base = 0; base < N; base += kChunk) {
        float v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const int i = base + j * kSelThreads + t;
          v[j] = i < N ? in[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const uint32_t key = to_key(v[j]);
          const bool act = base + j * kSelThreads + t < N && (key & mask) == prefix;
          hist_add(s_hist, act, (key >> shift) & 255u, lane);
        }
      }
    }
    __syncthreads();
    if (wave == 0) pick_digit(s_hist, kr, s_sel, lane);
    __syncthreads();
    prefix |= s_sel[0] << shift;
    mask |= 255u << shift;
    kr = s_sel[1];
    const uint32_t in_bin = s_sel[2];
    if (shift == 24 && in_bin <= (uint32_t)kCand) {
      // the chosen bin's keys into LDS (slot order is arbitrary: only the K-th key is read off them)
      for (int base = 0; base < N; base += kChunk) {
        float v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const int i = base + j * kSelThreads + t;
          v[j] = i < N ? in[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const uint32_t key = to_key(v[j]);
          if (base + j * kSelThreads + t < N && (key & mask) == prefix) s_cand[atomicAdd(&s_ncand, 1u)] = key;
        }
      }
      in_lds = true;
      ncand = in_bin;
    }
    __syncthreads();
  }
  // prefix: the K-th largest key; kr >= 1 of its ties (lowest flat index first) belong to the K.  The ordered pass:
  // a chunk is kGroups groups of 4,096 elements, thread t owning 4 consecutive ones of each (order: group, thread,
  // element); one barrier per chunk.
  uint32_t carry_gt = 0, carry_ti = 0;
  int buf = 0;
  for (int base = 0; base < N; base += kChunk, buf ^= 1) {
    float val[kGroups][4];
    uint32_t packed[kGroups], incl[kGroups];  // greater keys << 16 | ties
#pragma unroll
    for (int g = 0; g < kGroups; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = base + g * (kSelThreads * 4) + t * 4 + j;
        val[g][j] = i < N ? in[i] : 0.f;
      }
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      packed[g] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t key = to_key(val[g][j]);
        if (base + g * (kSelThreads * 4) + t * 4 + j < N)
          packed[g] += key > prefix ? 0x10000u : (key == prefix ? 1u : 0u);
      }
      incl[g] = packed[g];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        const uint32_t up = __shfl_up(incl[g], d, 64);
        if (lane >= d) incl[g] += up;
      }
    if (lane == 63)
#pragma unroll
      for (int g = 0; g < kGroups; ++g) s_tot[buf][g][wave] = incl[g];
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      uint32_t before = incl[g] - packed[g], all = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        const uint32_t tw = s_tot[buf][g][w];
        if (w < wave) before += tw;
        all += tw;
      }
      uint32_t gt = carry_gt + (before >> 16), ti = carry_ti + (before & 0xffffu);
      carry_gt += all >> 16;
      carry_ti += all & 0xffffu;
      if (KEYPOINTS && packed[g] == 0) continue;  // nothing of this thread's group is selected
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = base + g * (kSelThreads * 4) + t * 4 + j;
        if (i >= N) break;
        const uint32_t key = to_key(val[g][j]);
        const float vj = val[g][j];
        bool sel = false;
        uint32_t pos = 0;
        if (key > prefix) {
          sel = true;
          pos = gt + min(ti, kr);
          ++gt;
        } else if (key == prefix) {
          sel = ti < kr;
          pos = gt + ti;
          ++ti;
        }
        if constexpr (!KEYPOINTS) {
          o.g[b * (int64_t)N + i] = sel ? vj : 0.f;
          if (o.mask) o.mask[b * (int64_t)N + i] = sel ? 1 : 0;
        } else if (sel) {
          const int64_t row = b * (int64_t)K + pos, px = b * (int64_t)N + i;
          o.kpts[row * 4 + 0] = b;
          o.kpts[row * 4 + 1] = i / W;
          o.kpts[row * 4 + 2] = i % W;
          o.kpts[row * 4 + 3] = 0;
          o.kscore[row] = o.score[px];
          o.kscale[row] = o.scale_map ? o.scale_map[px] : o.scale_value;
          if (o.kori) {
            o.kori[row * 2] = o.ori_map[px * 2];
            o.kori[row * 2 + 1] = o.ori_map[px * 2 + 1];
          }
        }
      }
    }
  }
}

}  // namespace

size_t hn_select_ws_bytes(int64_t B, int H, int W) {
  return 3 * (((size_t)B * H * W * sizeof(float) + 15) & ~(size_t)15);  // v, g, q
}

hipError_t hn_launch_select(const HnSelectArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const int64_t total = a.B * (int64_t)a.H * a.W;
  const size_t plane = ((size_t)total * sizeof(float) + 15) & ~(size_t)15;
  float* v = static_cast<float*>(a.ws);
  float* g = reinterpret_cast<float*>(static_cast<char*>(a.ws) + plane);
  float* q = reinterpret_cast<float*>(static_cast<char*>(a.ws) + 2 * plane);
  const dim3 pix((unsigned)((total + 255) / 256)), blk(256);
  hipLaunchKernelGGL(k_sel_nms, pix, blk, 0, st, a.score, total, a.H, a.W, a.border, a.nms_thresh, a.nms_ksize, v);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  SelOut o{};
  o.g = g;
  o.mask = a.topk_mask;
  hipLaunchKernelGGL(k_sel_topk<false>, dim3((unsigned)a.B), dim3(kSelThreads), 0, st, v, a.H, a.W, a.topk, o);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  Taps taps;
  for (int i = 0; i < 225; ++i) taps.w[i] = i < a.gauss_ksize * a.gauss_ksize ? a.taps[i] : 0.f;
  const int btx = (a.W + kBlurTile - 1) / kBlurTile, btiles = btx * ((a.H + kBlurTile - 1) / kBlurTile);
  hipLaunchKernelGGL(k_sel_blur, dim3((unsigned)(a.B * btiles)), blk, 0, st, g, a.H, a.W, btx, btiles, a.gauss_ksize,
                     taps, q, a.score_proc);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  SelOut k{};
  k.score = a.score;
  k.scale_map = a.scale_map;
  k.scale_value = a.scale_value;
  k.ori_map = a.ori_map;
  k.kpts = a.kpts;
  k.kscore = a.kscore;
  k.kscale = a.kscale;
  k.kori = a.kori;
  hipLaunchKernelGGL(k_sel_topk<true>, dim3((unsigned)a.B), dim3(kSelThreads), 0, st, q, a.H, a.W, a.topk, k);
  return hipGetLastError();
}
