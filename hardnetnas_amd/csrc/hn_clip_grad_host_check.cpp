// Host check of the keypoint patch extraction's backward (hn_clip.h: sample_grad / accumulate_grad /
// keypoint_grad, the very functions k_clip_patch_backward calls).  Built by `make clip_grad_check` with the address
// and undefined-behaviour sanitizers (float-cast-overflow included).  Stand-alone: links nothing of the library and
// needs no GPU.  Two sweeps:
//   1. the adversarial keypoints of hn_clip_host_check.cpp through all 1,024 samples of the patch: every flat index
//      in [0, B * H * W) of exactly sized heap buffers, no undefined conversion, whatever the keypoint data;
//   2. a grid of ordinary keypoints, whose (a, b) -- the fp32 shares summed over the patch -- must equal the closed
//      form evaluated in double at the same corner cells.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hn_clip.h"

namespace {

struct AB {
  double a, b;      // the fp32 shares of hn_clip.h, summed in double
  double ra, rb;    // the closed form in double at the same cells
  double mag;       // the scale of the fp32 rounding error, see patch()
  bool in_bounds;
};

// all 1,024 samples of one keypoint; upstream gradient d(row, col) from a small integer hash
AB patch(const hnclip::Keypoint& k, const std::vector<float>& images, int64_t total, int32_t H, int32_t W) {
  AB r{0, 0, 0, 0, 0, true};
  for (int row = 0; row < hnclip::kPatch; ++row)
    for (int col = 0; col < hnclip::kPatch; ++col) {
      const hnclip::SampleGrad g = hnclip::sample_grad(k, row, col, H, W);
      for (int64_t idx : {g.s.p0, g.s.p0 + 1, g.s.p1, g.s.p1 + 1})
        if (idx < 0 || idx >= total) {
          r.in_bounds = false;
          return r;
        }
      const hnclip::PixelPair top = *reinterpret_cast<const hnclip::PixelPair*>(&images[(size_t)g.s.p0]);
      const hnclip::PixelPair bot = *reinterpret_cast<const hnclip::PixelPair*>(&images[(size_t)g.s.p1]);
      const float d = (float)((row * 37 + col * 11) % 17 - 8) * 0.125f;
      float a = 0.0f, b = 0.0f;
      hnclip::accumulate_grad(g, top, bot, d, &a, &b);
      r.a += a;
      r.b += b;
      // closed form in double: the same cells (the fp32 corners), coordinates from the fp32 affine in double
      const double gx = hnclip::grid_value(col), gy = hnclip::grid_value(row);
      const double xs = (double)k.sc * gx + (double)k.nss * gy + k.kx, ys = (double)k.ss * gx + (double)k.sc * gy + k.ky;
      int32_t x0, x1, y0, y1;
      hnclip::floor_pair(k.sc * (float)gx + k.nss * (float)gy + k.kx, W - 1, &x0, &x1);
      hnclip::floor_pair(k.ss * (float)gx + k.sc * (float)gy + k.ky, H - 1, &y0, &y1);
      auto px = [&](int32_t y, int32_t x) { return (double)images[(size_t)(k.base + (int64_t)y * W + x)]; };
      const double Ia = px(y0, x0), Ib = px(y1, x0), Ic = px(y0, x1), Id = px(y1, x1);
      const double gX = (y1 - ys) * (Ic - Ia) + (ys - y0) * (Id - Ib), gY = (x1 - xs) * (Ib - Ia) + (xs - x0) * (Id - Ic);
      r.ra += d * (gX * gx + gY * gy);
      r.rb += d * (gY * gx - gX * gy);
      // the fp32 coordinate is off by roundings of its terms (|s cos|, |s sin|, |kx|, |ky|), and that error meets
      // the pixel differences; the products and sums after it round relative to the same quantities
      const double coord = 1.0 + std::fabs((double)k.kx) + std::fabs((double)k.ky) +
                           2.0 * (std::fabs((double)k.sc) + std::fabs((double)k.ss));
      r.mag += std::fabs((double)d) * coord *
               (std::fabs(Ic - Ia) + std::fabs(Id - Ib) + std::fabs(Ib - Ia) + std::fabs(Id - Ic));
    }
  return r;
}

}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float denorm = std::numeric_limits<float>::denorm_min();
  long long n_keypoints = 0, n_compared = 0;
  double sink = 0.0, worst = 0.0;

  // ---- 1. adversarial keypoints: bounds and conversions ----
  {
    const std::vector<float> scales = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, denorm, 4.0f, 40.0f, 1e9f};
    const std::vector<float> oris = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, 1.0f, -0.70710678f};
    const std::vector<float> ratios = {0.0f, -0.0f, denorm, 1e-40f, nan, inf, -1.0f, 1.0f, 0.5f, 1.0f / 3.0f};
    const int64_t big = (int64_t)1 << 62;
    const std::vector<int64_t> coords = {big, -big, std::numeric_limits<int64_t>::max(),
                                         std::numeric_limits<int64_t>::min(), -1, 0, 1, 30, 60, 61, 1000};
    const std::vector<int32_t> dims = {2, 3, 61};
    for (int64_t B : {(int64_t)1, (int64_t)3}) {
      const std::vector<int64_t> batches = {-1, (int64_t)1 << 40, 0, B - 1, B, std::numeric_limits<int64_t>::min()};
      for (int32_t H : dims)
        for (int32_t W : dims) {
          const int64_t total = B * H * W;
          std::vector<float> images((size_t)total);  // exactly sized: one element past either end is a report
          for (size_t i = 0; i < images.size(); ++i) images[i] = 0.25f + (float)(i % 7);
          std::vector<float> ratio((size_t)B);
          size_t round = 0;
          for (float r : ratios) {
            for (int64_t i = 0; i < B; ++i) ratio[(size_t)i] = r;
            for (int64_t b : batches)
              for (size_t ci = 0; ci < coords.size(); ++ci) {
                std::vector<int64_t> kp = {b, coords[(ci * 5 + 3) % coords.size()], coords[ci], 0};
                // every scale with one orientation, every orientation with one scale (the full product is the
                // forward's sweep; here each keypoint runs all 1,024 samples)
                for (size_t v = 0; v < scales.size() + oris.size() + 1; ++v, ++round) {
                  const float sc = v < scales.size() ? scales[v] : scales[round % scales.size()];
                  const size_t oi = v < scales.size() ? round % (oris.size() + 1) : v - scales.size();
                  std::vector<float> ori = {oi < oris.size() ? oris[oi] : 1.0f,
                                            oi < oris.size() ? oris[(oi * 3 + 1) % oris.size()] : 0.0f};
                  const float* op = oi < oris.size() ? ori.data() : nullptr;  // the last: no rotation
                  const hnclip::Keypoint k = hnclip::keypoint(kp.data(), sc, op, ratio.data(), B, H, W);
                  const AB g = patch(k, images, total, H, W);
                  if (!g.in_bounds) {
                    std::fprintf(stderr, "index outside [0, %lld): B %lld H %d W %d b %lld y %lld x %lld scale %g "
                                 "ori (%g, %g) ratio %g\n", (long long)total, (long long)B, H, W, (long long)b,
                                 (long long)kp[1], (long long)kp[2], sc, ori[0], ori[1], r);
                    return 1;
                  }
                  float ds = 0.0f, dor[2] = {0.0f, 0.0f};
                  hnclip::keypoint_grad(kp.data(), sc, op, ratio.data(), B, (float)g.a, (float)g.b, &ds, op ? dor : nullptr);
                  sink += (ds == 0.0f) + (dor[0] == 0.0f) + (dor[1] == 0.0f);
                  ++n_keypoints;
                }
              }
          }
        }
    }
  }

  // ---- 2. ordinary keypoints: (a, b) against the closed form in double ----
  {
    const int64_t B = 3;
    const std::vector<float> ratio = {1.0f, 0.5f, 1.0f / 3.0f};
    for (auto hw : {std::pair<int32_t, int32_t>{2, 2}, {3, 5}, {61, 83}, {240, 320}}) {
      const int32_t H = hw.first, W = hw.second;
      const int64_t total = B * H * W;
      std::vector<float> images((size_t)total);
      uint32_t lcg = 12345u + (uint32_t)H;
      for (float& v : images) {
        lcg = lcg * 1664525u + 1013904223u;
        v = (float)(lcg >> 8) / 16777216.0f;
      }
      for (int64_t b = 0; b < B; ++b)
        for (int yi = 0; yi < 5; ++yi)
          for (int xi = 0; xi < 5; ++xi)
            for (float sc : {2.0f, 7.3f, 19.0f, 40.0f})
              for (int ai = 0; ai <= 8; ++ai) {  // the last: no rotation
                const float r = ratio[(size_t)b];
                std::vector<int64_t> kp = {b, (int64_t)((H - 1) * r * yi / 4.0f), (int64_t)((W - 1) * r * xi / 4.0f), 0};
                const float ang = 0.785398f * (float)ai + 0.1f;
                const float ori[2] = {std::cos(ang), std::sin(ang)};
                const float scale = sc * r;
                const hnclip::Keypoint k = hnclip::keypoint(kp.data(), scale, ai < 8 ? ori : nullptr, ratio.data(), B, H, W);
                const AB g = patch(k, images, total, H, W);
                if (!g.in_bounds) return 1;
                // a handful of fp32 roundings per term: 8 eps of the terms' magnitude (AB::mag)
                const double tol = 8.0 * 1.1920929e-7 * g.mag + 1e-30;
                const double err = std::fmax(std::fabs(g.a - g.ra), std::fabs(g.b - g.rb));
                worst = std::fmax(worst, err / tol);
                if (!(err <= tol)) {
                  std::fprintf(stderr, "gradient off: H %d W %d b %lld y %lld x %lld scale %g angle %d: a %.9g (%.9g) "
                               "b %.9g (%.9g) tol %.3g\n", H, W, (long long)b, (long long)kp[1], (long long)kp[2],
                               scale, ai, g.a, g.ra, g.b, g.rb, tol);
                  return 3;
                }
                ++n_keypoints;
                ++n_compared;
              }
    }
  }
  std::printf("clip_grad_check: %lld keypoints, every index in bounds, %lld gradients equal the closed form "
              "(worst error / tolerance %.3f, checksum %g)\n", n_keypoints, n_compared, worst, sink);
  return 0;
}
