// Host-only sweep of hn_rfdet.h's window, halo and tile address arithmetic: every index the kernels of hn_rfdet.hip
// form -- image and workspace reads and writes, LDS windows, MFMA operand reads, partial-statistics slots -- is
// applied to a real array of the size the plan gives it, for every image of H, W in 1 .. 50 with H * W >= 2 and
// for 61 x 83, 97 x 131 and 240 x 320, under the address and undefined-behaviour sanitizers.  Also checked: every
// workspace word a step reads was written by an earlier step of the same call, and the weight packing is a
// bijection onto the 2304 words of a level.  Built by `make rfdet_check`; links nothing of the library.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hn_rfdet.h"

using namespace hnrf;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static long g_indices = 0;

// a buffer that remembers which words were written
struct Buf {
  std::vector<unsigned char> w;
  explicit Buf(size_t n) : w(n, 0) {}
  void write(int64_t i) { CHECK(i >= 0); w.at((size_t)i) = 1; ++g_indices; }
  void read(int64_t i) { CHECK(i >= 0); CHECK(w.at((size_t)i) == 1); ++g_indices; }
};

static void check_shape(int64_t B, int H, int W) {
  const Plan pl = plan(B, H, W);
  const int64_t n = B * H * W, nt = tiles(H, W), wg = B * nt;
  CHECK(pl.total % 16 == 0 && pl.stat == 0);
  CHECK(pl.part_pre >= pl.stat + (size_t)B * kSlots * kStatFloats * 4);
  CHECK(pl.part_s >= pl.part_pre + (size_t)wg * kLevels * kPartPre * 8);
  CHECK(pl.pre[0] >= pl.part_s + (size_t)wg * kLevels * kPartS * 8);
  CHECK(pl.pre[1] >= pl.pre[0] + (size_t)n * kC * 4 && pl.feat[0] >= pl.pre[1] + (size_t)n * kC * 4);
  CHECK(pl.feat[1] >= pl.feat[0] + (size_t)n * kC * 4 && pl.sraw >= pl.feat[1] + (size_t)n * kC * 4);
  CHECK(pl.ounit >= pl.sraw + (size_t)n * kLevels * 4 && pl.total >= pl.ounit + (size_t)n * kLevels * 8);

  Buf image((size_t)n), stat((size_t)B * kSlots * kStatFloats), part_pre((size_t)wg * kLevels * kPartPre),
      part_s((size_t)wg * kLevels * kPartS), sraw((size_t)n * kLevels), ounit((size_t)n * kLevels * 2),
      out((size_t)n);
  Buf pre[2] = {Buf((size_t)n * kC), Buf((size_t)n * kC)}, feat[2] = {Buf((size_t)n * kC), Buf((size_t)n * kC)};
  for (int64_t i = 0; i < n; ++i) image.write(i);
  const int ntx = tiles_x(W);
  std::vector<float> lds(kLdsFloats);
  std::vector<unsigned char> lds_set(kLdsFloats);

  auto stats = [&](int j) {  // k_rf_stats of slot j
    for (int64_t b = 0; b < B; ++b) {
      for (int64_t i = 0; i < nt; ++i) {
        if (j < kLevels)
          for (int v = 0; v < kPartPre; ++v) part_pre.read(((int64_t)j * wg + b * nt + i) * kPartPre + v);
        if (j >= 1)
          for (int v = 0; v < kPartS; ++v) part_s.read(((int64_t)(j - 1) * wg + b * nt + i) * kPartS + v);
      }
      if (j < kLevels)
        for (int v = 0; v < 32; ++v) stat.write((b * kSlots + j) * kStatFloats + v);
      if (j >= 1)
        for (int v = 32; v < 34; ++v) stat.write((b * kSlots + j) * kStatFloats + v);
    }
  };

  // k_rf_first
  for (int64_t g = 0; g < wg; ++g) {
    const int64_t b = g / nt;
    const int tile = (int)(g % nt), y0 = (tile / ntx) * kT, x0 = (tile % ntx) * kT;
    for (int i = 0; i < kWinN; ++i) {
      const int y = win_y(y0, i), x = win_x(x0, i);
      if (inside(y, x, H, W)) image.read(b * H * W + (int64_t)y * W + x);
    }
    for (int t = 0; t < 256; ++t) {
      const int ty = t / kT, tx = t % kT, y = y0 + ty, x = x0 + tx;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) CHECK((ty + ky) * kWin + tx + kx < kWinN);
      if (y < H && x < W)
        for (int c = 0; c < kC; ++c) pre[0].write(pixel(b, y, x, H, W) * kC + c);
    }
    for (int v = 0; v < kPartPre; ++v) part_pre.write(g * kPartPre + v);
  }
  stats(0);
  // k_rf_mid, steps 1 .. 9
  for (int k = 1; k < kLevels; ++k) {
    Buf& pin = pre[(k - 1) & 1];
    Buf& pout = pre[k & 1];
    for (int64_t g = 0; g < wg; ++g) {
      const int64_t b = g / nt;
      const int tile = (int)(g % nt), y0 = (tile / ntx) * kT, x0 = (tile % ntx) * kT;
      for (int v = 0; v < 32; ++v) stat.read((b * kSlots + (k - 1)) * kStatFloats + v);
      std::fill(lds_set.begin(), lds_set.end(), 0);
      int own = 0;
      for (int i = 0; i < kWinN; ++i) {
        const int y = win_y(y0, i), x = win_x(x0, i);
        if (inside(y, x, H, W)) {
          const int64_t p = pixel(b, y, x, H, W);
          for (int c = 0; c < kC; ++c) pin.read(p * kC + c);
          if (k >= 2)
            for (int c = 0; c < kC; ++c) feat[(k - 1) & 1].read(p * kC + c);
          if (win_own(i)) {
            ++own;
            CHECK(y >= y0 && y < y0 + kT && x >= x0 && x < x0 + kT);
            if (k < kLevels - 1)
              for (int c = 0; c < kC; ++c) feat[k & 1].write(p * kC + c);
            sraw.write((int64_t)(k - 1) * n + p);
            ounit.write(((int64_t)(k - 1) * n + p) * 2);
            ounit.write(((int64_t)(k - 1) * n + p) * 2 + 1);
          }
        }
        for (int c = 0; c < kC; ++c) {
          lds.at((size_t)(c * kPlane + i)) = 0.f;
          lds_set.at((size_t)(c * kPlane + i)) = 1;
        }
      }
      int want = 0;
      for (int ty = 0; ty < kT; ++ty)
        for (int tx = 0; tx < kT; ++tx) want += (y0 + ty < H && x0 + tx < W);
      CHECK(own == want);  // every pixel of the tile inside the image is some window position's own pixel
      for (int s = 0; s < 36; ++s)
        for (int lane = 0; lane < 64; ++lane)
          for (int row = 0; row < kT; ++row) {
            const int a = lds_a_index(s, lane, row);
            CHECK(a >= 0 && lds_set.at((size_t)a) == 1);
            ++g_indices;
          }
      for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 4; ++r)
            for (int j = 0; j < 4; ++j) {
              const int y = y0 + wave * 4 + r, x = x0 + (lane >> 4) * 4 + j;
              if (y < H && x < W) pout.write(pixel(b, y, x, H, W) * kC + (lane & 15));
            }
      for (int v = 0; v < kPartPre; ++v) part_pre.write(((int64_t)k * wg + g) * kPartPre + v);
      for (int v = 0; v < kPartS; ++v) part_s.write(((int64_t)(k - 1) * wg + g) * kPartS + v);
    }
    stats(k);
  }
  // k_rf_last
  for (int64_t g = 0; g < wg; ++g) {
    const int64_t b = g / nt;
    const int tile = (int)(g % nt);
    for (int v = 0; v < 32; ++v) stat.read((b * kSlots + kLevels - 1) * kStatFloats + v);
    for (int t = 0; t < 256; ++t) {
      const int y = (tile / ntx) * kT + t / kT, x = (tile % ntx) * kT + t % kT;
      if (y < H && x < W) {
        const int64_t p = pixel(b, y, x, H, W);
        for (int c = 0; c < kC; ++c) pre[(kLevels - 1) & 1].read(p * kC + c);
        sraw.write((int64_t)(kLevels - 1) * n + p);
        ounit.write(((int64_t)(kLevels - 1) * n + p) * 2);
        ounit.write(((int64_t)(kLevels - 1) * n + p) * 2 + 1);
      }
    }
    for (int v = 0; v < kPartS; ++v) part_s.write(((int64_t)(kLevels - 1) * wg + g) * kPartS + v);
  }
  stats(kLevels);
  // k_rf_tail
  const int ntx2 = (W + kT2 - 1) / kT2;
  const int64_t nt2 = tiles2(H, W);
  std::vector<float> s_s(kS * kSP), s_h(kS * kM), s_m(kM * kM), s_e(kM * kM);
  for (int64_t g = 0; g < B * nt2; ++g) {
    const int64_t b = g / nt2;
    const int tile = (int)(g % nt2), y0 = (tile / ntx2) * kT2, x0 = (tile % ntx2) * kT2;
    for (int k = 0; k < kLevels; ++k) {
      stat.read((b * kSlots + k + 1) * kStatFloats + 32);
      stat.read((b * kSlots + k + 1) * kStatFloats + 33);
      for (int i = 0; i < kS * kS; ++i) {
        const int y = y0 - kHalo2 + i / kS, x = x0 - kHalo2 + i % kS;
        if (inside(y, x, H, W)) sraw.read((int64_t)k * n + b * H * W + (int64_t)y * W + x);
        s_s.at((size_t)((i / kS) * kSP + i % kS)) = 0.f;
      }
      if (k > 0) continue;  // the LDS passes are the same at every level
      for (int i = 0; i < kS * kM; ++i)
        for (int d = 0; d < 15; ++d) s_h.at((size_t)i) = s_s.at((size_t)((i / kM) * kSP + i % kM + d));
      for (int i = 0; i < kM * kM; ++i)
        for (int d = 0; d < 15; ++d) s_m.at((size_t)i) = s_h.at((size_t)((i / kM + d) * kM + i % kM));
    }
    for (int i = 0; i < kM * kM; ++i) {
      const int y = y0 - 7 + i / kM, x = x0 - 7 + i % kM;
      if (inside(y, x, H, W))
        for (int k = 0; k < kLevels; ++k) sraw.read((int64_t)k * n + b * H * W + (int64_t)y * W + x);
      s_e.at((size_t)i) = 0.f;
    }
    for (int i = 0; i < kM * kT2; ++i)
      for (int d = 0; d < 15; ++d) s_h.at((size_t)i) = s_e.at((size_t)((i / kT2) * kM + i % kT2 + d));
    for (int i = 0; i < kT2 * kT2; ++i) {
      const int r = i / kT2, c = i % kT2, y = y0 + r, x = x0 + c;
      if (y >= H || x >= W) continue;
      float a = 0.f;
      for (int d = 0; d < 15; ++d) a += s_h.at((size_t)((r + d) * kT2 + c));
      a += s_m.at((size_t)((r + 7) * kM + c + 7));
      const int64_t o = b * H * W + (int64_t)y * W + x;
      for (int k = 0; k < kLevels; ++k) {
        sraw.read((int64_t)k * n + o);
        ounit.read(((int64_t)k * n + o) * 2);
        ounit.read(((int64_t)k * n + o) * 2 + 1);
      }
      out.write(o);
      (void)a;
    }
  }
  for (int64_t i = 0; i < n; ++i) out.read(i);  // every output pixel written
}

int main() {
  // the weight packing: a bijection onto a level's 2304 words
  std::vector<int> seen(2304, 0);
  for (int co = 0; co < 16; ++co)
    for (int ci = 0; ci < 16; ++ci)
      for (int tap = 0; tap < 9; ++tap) {
        const int i = mfma_weight_index(co, ci, tap);
        CHECK(i >= 0 && i < 2304);
        ++seen.at((size_t)i);
        // the lane and step that read it use the same (cout, cin, tap)
        const int s = i / 64, lane = i % 64;
        CHECK((lane & 15) == co && (s & 3) * 4 + (lane >> 4) == ci && (s >> 2) == tap);
      }
  for (int v : seen) CHECK(v == 1);
  CHECK(kConvB == 2304 && kOB + 2 <= kLevelStride && kLevelStride % 4 == 0 && kPlane >= kWinN);
  CHECK(160 + 9 * 2320 + 10 * 32 + 10 * 17 + 10 * 2 + 10 * 34 == kStateFloats);

  int shapes = 0;
  for (int H = 1; H <= 50; ++H)
    for (int W = 1; W <= 50; ++W)
      if (H * W >= 2) {
        check_shape(H * W <= 64 ? 2 : 1, H, W);
        ++shapes;
      }
  check_shape(3, 61, 83);
  check_shape(2, 97, 131);
  check_shape(1, 240, 320);
  shapes += 3;
  std::printf("hn_rfdet_host_check: %d shapes, %ld indices, all inside their arrays\n", shapes, g_indices);
  return 0;
}
