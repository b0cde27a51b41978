// Host check of the keypoint patch extraction's bounds guarantee (hn_clip.h): sweeps adversarial keypoints
// through the very functions the kernel calls and requires every flat index to lie in [0, B * H * W).  Built
// by `make clip_check` with the address and undefined-behaviour sanitizers (float-cast-overflow included), so
// an out-of-range float -> integer conversion or a read outside the exactly-sized heap buffers ends the run
// with a report.  Stand-alone: links nothing of the library and needs no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hn_clip.h"

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float denorm = std::numeric_limits<float>::denorm_min();
  const std::vector<float> scales = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, denorm, 4.0f, 40.0f, 1e9f};
  const std::vector<float> oris = {nan, inf, -inf, 1e30f, -1e30f, 0.0f, 1.0f, -0.70710678f};
  const std::vector<float> ratios = {0.0f, -0.0f, denorm, 1e-40f, nan, inf, -1.0f, 1.0f, 0.5f, 1.0f / 3.0f};
  const int64_t big = (int64_t)1 << 62;
  const std::vector<int64_t> coords = {big, -big, std::numeric_limits<int64_t>::max(),
                                       std::numeric_limits<int64_t>::min(), -1, 0, 1, 30, 60, 61, 1000};
  const std::vector<int32_t> dims = {2, 3, 61};
  const std::vector<int> taps = {0, 1, 15, 16, 30, 31};  // grid rows / columns: both ends and the middle

  long long n_samples = 0, n_keypoints = 0;
  double sink = 0.0;
  for (int64_t B : {(int64_t)1, (int64_t)3}) {
    const std::vector<int64_t> batches = {-1, (int64_t)1 << 40, 0, B - 1, B, std::numeric_limits<int64_t>::min()};
    for (int32_t H : dims)
      for (int32_t W : dims) {
        const int64_t total = B * H * W;
        // exactly sized heap buffers: one element past either end is a sanitizer report
        std::vector<float> images((size_t)total);
        for (size_t i = 0; i < images.size(); ++i) images[i] = 0.25f + (float)(i % 7);
        std::vector<float> ratio((size_t)B);
        for (float r : ratios) {
          for (int64_t i = 0; i < B; ++i) ratio[(size_t)i] = r;
          for (int64_t b : batches)
            for (size_t ci = 0; ci < coords.size(); ++ci) {
              // y runs through the list with x, offset so that huge and small values meet
              std::vector<int64_t> kp = {b, coords[(ci * 5 + 3) % coords.size()], coords[ci], 0};
              for (float sc : scales)
                for (size_t oi = 0; oi <= oris.size(); ++oi) {
                  std::vector<float> ori = {oi < oris.size() ? oris[oi] : 1.0f,
                                            oi < oris.size() ? oris[(oi * 3 + 1) % oris.size()] : 0.0f};
                  const float* op = oi < oris.size() ? ori.data() : nullptr;  // the last round: no rotation
                  const hnclip::Keypoint k = hnclip::keypoint(kp.data(), sc, op, ratio.data(), B, H, W);
                  ++n_keypoints;
                  for (int row : taps)
                    for (int col : taps) {
                      const hnclip::Sample s = hnclip::sample(k, row, col, H, W);
                      for (int64_t idx : {s.p0, s.p0 + 1, s.p1, s.p1 + 1}) {
                        if (idx < 0 || idx >= total) {
                          std::fprintf(stderr,
                                       "index %lld outside [0, %lld): B %lld H %d W %d b %lld y %lld x %lld scale %g "
                                       "ori (%g, %g) ratio %g row %d col %d\n",
                                       (long long)idx, (long long)total, (long long)B, H, W, (long long)b,
                                       (long long)kp[1], (long long)kp[2], sc, ori[0], ori[1], r, row, col);
                          return 1;
                        }
                        sink += images[(size_t)idx];
                      }
                      const hnclip::PixelPair top = *reinterpret_cast<const hnclip::PixelPair*>(&images[(size_t)s.p0]);
                      const hnclip::PixelPair bot = *reinterpret_cast<const hnclip::PixelPair*>(&images[(size_t)s.p1]);
                      sink += hnclip::blend(s, top, bot) == 0.0f ? 1.0 : 0.0;
                      ++n_samples;
                    }
                }
            }
        }
      }
  }
  // every grid value inside [-1, 1], the ends exact
  for (int i = 0; i < hnclip::kPatch; ++i)
    if (!(hnclip::grid_value(i) >= -1.0f && hnclip::grid_value(i) <= 1.0f)) return 2;
  if (hnclip::grid_value(0) != -1.0f || hnclip::grid_value(31) != 1.0f) return 2;
  std::printf("clip_check: %lld keypoints, %lld samples, every index in bounds (checksum %g)\n", n_keypoints,
              n_samples, sink);
  return 0;
}
