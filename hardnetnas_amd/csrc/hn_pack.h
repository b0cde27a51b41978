// Host-side weight preparation of hn_create (hn_api.hip): eval-mode BatchNorm folded into the conv before it, and
// the folded weights packed into the device layouts the kernels read.  Plain C++ with nothing of HIP in it, so that
// hn_pack_host_check.cpp can run every packer under the sanitizers (make pack_check).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

uint16_t f2bf(float x) {  // round-to-nearest-even, as v_cvt_pk_bf16_f32
  uint32_t u;
  std::memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// eval BatchNorm folded into the preceding bias-free conv:
//   y = (conv(x) - mean) * gamma / sqrt(var + eps) + beta
struct Folded {
  std::vector<float> w, b;
};
Folded fold(const float* w, size_t per_out, int cout, const float* gamma, const float* beta,
            const float* mean, const float* var, float eps) {
  Folded f;
  f.w.resize((size_t)cout * per_out);
  f.b.resize(cout);
  for (int n = 0; n < cout; ++n) {
    const double sc = (gamma ? (double)gamma[n] : 1.0) / std::sqrt((double)var[n] + (double)eps);
    for (size_t j = 0; j < per_out; ++j)
      f.w[(size_t)n * per_out + j] = (float)((double)w[(size_t)n * per_out + j] * sc);
    f.b[n] = (float)((beta ? (double)beta[n] : 0.0) - (double)mean[n] * sc);
  }
  return f;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------------------
// conv1..5 of HardNet as bf16x3 MFMA fragments: [cc][tap][ks][nt][plane][lane][8]
static std::vector<uint16_t> pack_conv3x3(const std::vector<float>& w, int cin, int cout) {
  const int ncc = cin / 32, ntot = cout / 32;
  std::vector<uint16_t> out((size_t)ncc * 9 * 2 * ntot * 2 * 64 * 8);
  size_t o = 0;
  for (int cc = 0; cc < ncc; ++cc)
    for (int tap = 0; tap < 9; ++tap)
      for (int ks = 0; ks < 2; ++ks)
        for (int nt = 0; nt < ntot; ++nt) {
          uint16_t* hi = &out[o];
          uint16_t* lo = &out[o + 64 * 8];
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
              const int n = nt * 32 + (lane & 31);
              const int c = cc * 32 + ks * 16 + (lane >> 5) * 8 + j;
              const float v = w[((size_t)n * cin + c) * 9 + tap];
              const uint16_t h = f2bf(v);
              hi[lane * 8 + j] = h;
              lo[lane * 8 + j] = f2bf(v - bf2f(h));
            }
          o += 2 * 64 * 8;
        }
  return out;
}

// head conv (kernel kk x kk over an NHWC map): GEMM k = (y*kk + x)*cin + c,
// fragments [ks][nt][plane][lane][8]
// folded weights whose fp16 hi half is not finite (|w| >= 65520 or NaN): counted while a model is
// packed (per calling thread), hn_create then fails instead of packing an infinite fragment
static thread_local long tl_f16_out_of_range = 0;
static void put_f16_split(float v, uint16_t* hi, uint16_t* lo) {  // hn_common.h split8_f16
  const _Float16 hv = (_Float16)v;
  if (!std::isfinite((float)hv)) ++tl_f16_out_of_range;
  const _Float16 lv = (_Float16)(v - (float)hv);
  std::memcpy(hi, &hv, 2);
  std::memcpy(lo, &lv, 2);
}

static std::vector<uint16_t> pack_head(const std::vector<float>& w, int cin, int kk, bool f16 = false) {
  const int K = cin * kk * kk;
  std::vector<uint16_t> out((size_t)(K / 16) * 4 * 2 * 64 * 8);
  size_t o = 0;
  for (int ks = 0; ks < K / 16; ++ks)
    for (int nt = 0; nt < 4; ++nt) {
      uint16_t* hi = &out[o];
      uint16_t* lo = &out[o + 64 * 8];
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int n = nt * 32 + (lane & 31);
          const int k = ks * 16 + (lane >> 5) * 8 + j;
          const int c = k % cin, yx = k / cin;
          const float v = w[((size_t)n * cin + c) * kk * kk + yx];
          if (f16) {
            put_f16_split(v, &hi[lane * 8 + j], &lo[lane * 8 + j]);
          } else {
            const uint16_t h = f2bf(v);
            hi[lane * 8 + j] = h;
            lo[lane * 8 + j] = f2bf(v - bf2f(h));
          }
        }
      o += 2 * 64 * 8;
    }
  return out;
}

// [cout][kg] -> [kg][cout]
static std::vector<float> transpose_pw(const std::vector<float>& w, int cout, int kg) {
  std::vector<float> t((size_t)kg * cout);
  for (int n = 0; n < cout; ++n)
    for (int k = 0; k < kg; ++k) t[(size_t)k * cout + n] = w[(size_t)n * kg + k];
  return t;
}


// Fused-front stem weights as the MFMA A operand: [plane hi/lo][lane][8] fp16, lane
// (r = l & 31 = output channel, h = l >> 5) holding taps 8h..8h+7 (taps >= 9 are zero).
// The fused front's stem as 32x32x16 A operands [op][plane hi/lo][lane][8] fp16, lane (channel
// r = l & 31, K slots 8 (l >> 5) ..): op 0 = the 9 taps in K slots 0..8 (one image row per MFMA);
// op 1 = the same taps shifted to K slots 3..11, so that one B operand holding the 4 x 3 input
// window of two adjacent rows (slot 3 dy + dx, dy = 0..3) feeds row y (op 0) and row y + 1 (op 1).
static std::vector<uint16_t> pack_front_stem(const Folded& f) {
  std::vector<uint16_t> a(2 * 2 * 64 * 8, 0);
  for (int op = 0; op < 2; ++op)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int r = lane & 31, tap = 8 * (lane >> 5) + j - 3 * op;
        uint16_t* d = &a[(size_t)op * 2 * 64 * 8];
        put_f16_split(tap >= 0 && tap < 9 ? f.w[(size_t)r * 9 + tap] : 0.f, &d[lane * 8 + j], &d[64 * 8 + lane * 8 + j]);
      }
  return a;
}

// Fused-front pw weights (fp16 hi/lo) as the MFMA A operand (rows = output channels in dw
// order, i.e. after ChannelShuffle(g); grouped conv densified with zeros):
// [MID/32][kstep][plane hi/lo][lane][8] fp16, lane (r = l & 31, h = l >> 5), element j
// multiplying stem channel kappa(16*kstep + 8h + j) -- the order in which the stem MFMA
// leaves its outputs in the lanes (C row (i & 3) + 8 (i >> 2) + 4h for i = 8*kstep + j).
static void pack_front(const Folded& f, int mid, int g, std::vector<uint16_t>* a,
                       std::vector<float>* bias) {
  const int cin = 32, kg = cin / g, cg = mid / g;
  auto src = [&](int d) { return g > 1 ? (d % g) * cg + d / g : d; };  // fbnet_builder.py:332-349
  a->assign((size_t)mid / 32 * 2 * 2 * 64 * 8, 0);
  bias->resize(mid);
  for (int d = 0; d < mid; ++d) (*bias)[d] = f.b[src(d)];
  for (int mc = 0; mc < mid / 32; ++mc)
    for (int ks = 0; ks < 2; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int d = 32 * mc + (lane & 31), h = lane >> 5;
          const int k = (j & 3) + 8 * (2 * ks + (j >> 2)) + 4 * h;  // stem channel
          const int c = src(d), grp = c / (mid / g);
          const float v = (k >= grp * kg && k < (grp + 1) * kg) ? f.w[(size_t)c * kg + (k - grp * kg)] : 0.f;
          const size_t o = ((((size_t)mc * 2 + ks) * 2) * 64 + lane) * 8 + j;
          put_f16_split(v, &(*a)[o], &(*a)[o + 64 * 8]);
        }
}

// 1x1 conv [cout][cin/g] (groups densified with zeros, output rows permuted by row_src) as
// the fp16x3 MFMA A operand: [cout/32][cin/16][plane][lane][8], lane (r = l & 31, h = l >> 5)
// holding W[row_src(32t + r)][16s + 8h + j].
template <class RowSrc>
static std::vector<uint16_t> pack_1x1_a(const std::vector<float>& w, int cout, int cin, int g,
                                        RowSrc row_src) {
  const int kg = cin / g;
  std::vector<uint16_t> a((size_t)cout / 32 * (cin / 16) * 2 * 64 * 8, 0);
  for (int tt = 0; tt < cout / 32; ++tt)
    for (int ks = 0; ks < cin / 16; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int c = row_src(32 * tt + (lane & 31)), k = 16 * ks + 8 * (lane >> 5) + j;
          const int grp = c / (cout / g);
          const float v = (k >= grp * kg && k < (grp + 1) * kg) ? w[(size_t)c * kg + (k - grp * kg)] : 0.f;
          const size_t o = ((((size_t)tt * (cin / 16) + ks) * 2) * 64 + lane) * 8 + j;
          put_f16_split(v, &a[o], &a[o + 64 * 8]);
        }
  return a;
}

// 1x1 conv (cout = 32, groups densified) as 16x16x32 fp16 hi/lo A operands: [cin/32][out tile 2][plane]
// [lane 64][8], lane (row = l & 15 -> output channel 16 tile + row, k-group l >> 4 -> input
// channels 32 chunk + 8 (l >> 4) + j) -- the NAS front's pwl (hn_front.hip, no-fold form)
static std::vector<uint16_t> pack_1x1_a16(const std::vector<float>& w, int cout, int cin, int g) {
  const int kg = cin / g;
  std::vector<uint16_t> a((size_t)cin / 32 * (cout / 16) * 2 * 64 * 8, 0);
  for (int ch = 0; ch < cin / 32; ++ch)
    for (int tt = 0; tt < cout / 16; ++tt)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int c = 16 * tt + (lane & 15), k = 32 * ch + 8 * (lane >> 4) + j;
          const int grp = c / (cout / g);
          const float v = (k >= grp * kg && k < (grp + 1) * kg) ? w[(size_t)c * kg + (k - grp * kg)] : 0.f;
          const size_t o = ((((size_t)ch * (cout / 16) + tt) * 2) * 64 + lane) * 8 + j;
          put_f16_split(v, &a[o], &a[o + 64 * 8]);
        }
  return a;
}

// 3x3 conv (cin = 32, BN folded) as 16x16x32 bf16 hi/lo A operands for k_c12:
// [tap 9][group of 16 output channels][plane][lane 64][8], lane (row = l & 15 -> output
// channel 16 g + row, k-group l >> 4 -> input channels 8 (l >> 4) + j).
static std::vector<uint16_t> pack_c12(const std::vector<float>& w, int cout) {
  const int cin = 32, ng = cout / 16;
  std::vector<uint16_t> a((size_t)9 * ng * 2 * 64 * 8);
  for (int tap = 0; tap < 9; ++tap)
    for (int g = 0; g < ng; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int oc = 16 * g + (lane & 15), ic = 8 * (lane >> 4) + j;
          const float v = w[((size_t)oc * cin + ic) * 9 + tap];
          const uint16_t hv = f2bf(v);
          const size_t o = (((size_t)tap * ng + g) * 2 * 64 + lane) * 8 + j;
          a[o] = hv;
          a[o + 64 * 8] = f2bf(v - bf2f(hv));
        }
  return a;
}

// conv1 (cin = cout = 32, BN folded) as 1-D Winograd F(4,3) along x for k_c12w (hn_c12w.hip):
// Toom-Cook points 0, 1, -1, 1/2, -1/2, inf; U_xi[ky] = sum_kx G[xi][kx] W[ky][kx] in fp64, bf16
// hi / lo 16x16x32 A fragments [xi 6][ky 3][group 2][plane][lane 64][8], lane (row = l & 15 ->
// output channel 16 g + row, k-group l >> 4 -> input channels 8 (l >> 4) + j)
static std::vector<uint16_t> pack_c12w(const std::vector<float>& w) {
  static const double G[6][3] = {{4, 0, 0},           {2.0 / 3, 2.0 / 3, 2.0 / 3},   {2.0 / 3, -2.0 / 3, 2.0 / 3},
                                 {-8.0 / 3, -4.0 / 3, -2.0 / 3}, {-8.0 / 3, 4.0 / 3, -2.0 / 3}, {0, 0, 1}};
  std::vector<uint16_t> a((size_t)6 * 3 * 2 * 2 * 64 * 8);
  for (int xi = 0; xi < 6; ++xi)
    for (int ky = 0; ky < 3; ++ky)
      for (int g = 0; g < 2; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int oc = 16 * g + (lane & 15), ic = 8 * (lane >> 4) + j;
            double u = 0;
            for (int kx = 0; kx < 3; ++kx) u += G[xi][kx] * (double)w[((size_t)oc * 32 + ic) * 9 + ky * 3 + kx];
            const float v = (float)u;
            const uint16_t hv = f2bf(v);
            const size_t o = ((((size_t)(xi * 3 + ky) * 2 + g) * 2) * 64 + lane) * 8 + j;
            a[o] = hv;
            a[o + 64 * 8] = f2bf(v - bf2f(hv));
          }
  return a;
}

// stride-1 3x3 conv (BN folded) as 1-D Winograd F(2,3) along x (hn_wino1.hip): U_xi[ky] =
// sum_kx G[xi][kx] W[ky][kx] in fp64 (U3 negated: it accumulates into the odd output column with a
// minus sign), bf16 hi / lo A fragments [cin/32][xi][ky][ks][cout/32][plane][lane][8] in the
// kernel's K-step order kx = 6 xi + 2 ky + ks
static std::vector<uint16_t> pack_wino1(const std::vector<float>& w, int cin, int cout) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  const int ncc = cin / 32, ntot = cout / 32;
  std::vector<uint16_t> out((size_t)ncc * 24 * ntot * 2 * 64 * 8);
  size_t o = 0;
  for (int cc = 0; cc < ncc; ++cc)
    for (int kx = 0; kx < 24; ++kx)
      for (int nt = 0; nt < ntot; ++nt) {
        const int xi = kx / 6, ky = (kx % 6) / 2, ks = kx % 2;
        uint16_t* hi = &out[o];
        uint16_t* lo = &out[o + 64 * 8];
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int n = nt * 32 + (lane & 31);
            const int c = cc * 32 + ks * 16 + (lane >> 5) * 8 + j;
            double u = 0;
            for (int t = 0; t < 3; ++t) u += G[xi][t] * (double)w[((size_t)n * cin + c) * 9 + ky * 3 + t];
            const float v = (float)(xi == 3 ? -u : u);
            const uint16_t hv = f2bf(v);
            hi[lane * 8 + j] = hv;
            lo[lane * 8 + j] = f2bf(v - bf2f(hv));
          }
        o += 2 * 64 * 8;
      }
  return out;
}

// stride-1 3x3 conv (BN folded) as 1-D Winograd F(4,3) along x (hn_wino1.hip k_conv_w4): U_xi[ky] =
// sum_kx G[xi][kx] W[ky][kx] in fp64, bf16 hi / lo A fragments of the 16x16x32 MFMA
// [cin/32][kx 18][cout/16][plane][lane][8] in the kernel's K-step order kx = 3 xo + ky, xi = w4_xi(xo)
// (lane: output channel 16 nt + (lane & 15), input channels 32 cc + 8 (lane >> 4) + j)
static std::vector<uint16_t> pack_wino4(const std::vector<float>& w, int cin, int cout) {
  static const double G[6][3] = {{4, 0, 0},
                                 {2.0 / 3, 2.0 / 3, 2.0 / 3},
                                 {2.0 / 3, -2.0 / 3, 2.0 / 3},
                                 {-8.0 / 3, -4.0 / 3, -2.0 / 3},
                                 {-8.0 / 3, 4.0 / 3, -2.0 / 3},
                                 {0, 0, 1}};
  static const int XO[6] = {0, 5, 1, 2, 3, 4};
  const int ncc = cin / 32, ntot = cout / 16;
  std::vector<uint16_t> out((size_t)ncc * 18 * ntot * 2 * 64 * 8);
  size_t o = 0;
  for (int cc = 0; cc < ncc; ++cc)
    for (int kx = 0; kx < 18; ++kx)
      for (int nt = 0; nt < ntot; ++nt) {
        const int xi = XO[kx / 3], ky = kx % 3;
        uint16_t* hi = &out[o];
        uint16_t* lo = &out[o + 64 * 8];
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int n = nt * 16 + (lane & 15);
            const int c = cc * 32 + (lane >> 4) * 8 + j;
            double u = 0;
            for (int t = 0; t < 3; ++t) u += G[xi][t] * (double)w[((size_t)n * cin + c) * 9 + ky * 3 + t];
            const float v = (float)u;
            const uint16_t hv = f2bf(v);
            hi[lane * 8 + j] = hv;
            lo[lane * 8 + j] = f2bf(v - bf2f(hv));
          }
        o += 2 * 64 * 8;
      }
  return out;
}

#ifdef HN_EXPERIMENTS
// stride-1 3x3 conv (BN folded) as Winograd F(2x2,3x3) U = G g G^T (fp64, then bf16 hi/lo),
// packed as the B operand of hn_wino.hip's 32x32x16 MFMAs: [cout/32][cin/16][xi 16][plane][lane
// 64][8], lane (column l & 31 -> output channel, k-group l >> 5 -> input channels 8 (l >> 5) + j)
static std::vector<uint16_t> pack_wino(const std::vector<float>& w, int cin, int cout) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  const int ncb = cout / 32, nks = cin / 16;
  std::vector<uint16_t> a((size_t)ncb * nks * 16 * 2 * 64 * 8);
  for (int cb = 0; cb < ncb; ++cb)
    for (int ks = 0; ks < nks; ++ks)
      for (int xi = 0; xi < 16; ++xi)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int co = 32 * cb + (lane & 31), ci = 16 * ks + 8 * (lane >> 5) + j;
            const float* g = &w[((size_t)co * cin + ci) * 9];
            const int i0 = xi >> 2, j0 = xi & 3;
            double u = 0;
            for (int r = 0; r < 3; ++r)
              for (int c = 0; c < 3; ++c) u += G[i0][r] * (double)g[r * 3 + c] * G[j0][c];
            const float v = (float)u;
            const uint16_t hv = f2bf(v);
            const size_t o = ((((size_t)(cb * nks + ks) * 16 + xi) * 2) * 64 + lane) * 8 + j;
            a[o] = hv;
            a[o + 64 * 8] = f2bf(v - bf2f(hv));
          }
  return a;
}
#endif

// stem [32][9] -> [tap][32] for the VALU stem / front kernels
static std::vector<float> stem_taps(const std::vector<float>& w) {
  std::vector<float> sw(9 * 32);
  for (int n = 0; n < 32; ++n)
    for (int t = 0; t < 9; ++t) sw[t * 32 + n] = w[n * 9 + t];
  return sw;
}
