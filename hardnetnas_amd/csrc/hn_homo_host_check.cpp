// Host check of the homography ground-truth stage's bounds guarantee (hn_homo.h): sweeps adversarial homographies,
// keypoints, scales, orientations and masks through the very functions the kernels call and requires every index to
// lie inside its array.  Built by `make homo_check` with the address and undefined-behaviour sanitizers
// (float-cast-overflow included), so an out-of-range float -> integer conversion, a signed overflow or a read outside
// the exactly-sized heap buffers ends the run with a report.  Stand-alone: links nothing of the library, needs no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hn_homo.h"

namespace {

using Mat = std::vector<float>;

std::vector<Mat> homographies(int32_t H, int32_t W) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float fw = (float)W, fh = (float)H;
  std::vector<Mat> m = {
      {1, 0, 0, 0, 1, 0, 0, 0, 1},                                  // identity
      {1.05f, -0.2f, 3.3f, 0.2f, 1.05f, -2.6f, 4e-4f, -3e-4f, 1},   // a well-conditioned one
      {1, 0, 2 * fw, 0, 1, 0, 0, 0, 1},                             // out of view
      {1, 0, 0, 0, 1, 0, 1, 0, -fw / 2},                            // horizon line x = W / 2: w crosses 0 in the image
      {1, 0, 0, 0, 1, 0, 0, 1, -fh / 2},                            // horizon line y = H / 2
      {1, 0, 0, 0, 1, 0, 1, 1, -(fw + fh) / 4},                     // a diagonal horizon
      {1, 0, 0, 0, 1, 0, 0, 0, 0},                                  // w == 0 everywhere: division by 1e-8
      {1, 0, 0, 0, 1, 0, 0, 0, -1e-8f},                             // w + 1e-8 == 0: 0 / 0 and x / 0
      {0, 0, 0, 0, 0, 0, 0, 0, 0},                                  // all zero
      {1, 2, 3, 2, 4, 6, 0, 0, 1},                                  // singular
      {1, 1, 1, 1, 1, 1, 1, 1, 1},                                  // rank one
      {nan, 0, 0, 0, 1, 0, 0, 0, 1},
      {1, 0, 0, 0, 1, 0, 0, 0, nan},
      {inf, 0, 0, 0, -inf, 0, 0, 0, 1},
      {1, 0, inf, 0, 1, -inf, 0, 0, 1},
      {1, 0, 0, 0, 1, 0, inf, 0, 1},
      {1e38f, 1e38f, 1e38f, -1e38f, -1e38f, -1e38f, 1, 0, 1},       // overflows to +-Inf in the sums
      {1e38f, 0, 0, 0, 1e38f, 0, 0, 0, 1e-38f},
      {1e9f, 0, 0.5f, 0, -1e9f, 0.5f, 0, 0, 1},                     // beyond the int32 range
      {1, 0, 2147483648.0f, 0, 1, -2147483648.0f, 0, 0, 1},
      {1, 0, 0.5f, 0, 1, 1.5f, 0, 0, 1},                            // half-integer ties
  };
  return m;
}

int fail(const char* what, long long idx, long long total, int32_t H, int32_t W, size_t mi) {
  std::fprintf(stderr, "%s: index %lld outside [0, %lld): H %d W %d homography %zu\n", what, idx, total, H, W, mi);
  return 1;
}

}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> scales = {nan, inf, -inf, 1e38f, -1e38f, 0.0f, 1.0f, 8.0f, 32.0f, 47.9f, 1e9f, 4e9f};
  const std::vector<float> oris = {nan, inf, -inf, 1e38f, 0.0f, 1.0f, -0.70710678f};
  const std::vector<std::pair<int32_t, int32_t>> dims = {{2, 2}, {2, 3}, {3, 2}, {17, 19}, {61, 83}};
  long long n_pixels = 0, n_keypoints = 0, n_masks = 0;
  double sink = 0.0;

  // the conversions alone: every value is defined and inside its documented range
  for (float v : {nan, inf, -inf, 1e38f, -1e38f, 2147483648.0f, -2147483648.0f, 2147483520.0f, 1073741824.0f,
                  -1073741824.0f, 0.5f, 1.5f, 2.5f, -0.5f, -1.5f, 0.0f, -0.0f, 1e-40f}) {
    const int32_t t = hnhomo::trunc_i32(v), r = hnhomo::round_i32(v);
    if (t > 1073741760 || t < -1073741760 || r > 2147483520 || r < -2147483520) return 2;
    int32_t i = -1;
    if (hnhomo::inside(v, 1 << 30, &i) && (i < 0 || i >= (1 << 30))) return 2;
    sink += (double)t + (double)r;
  }
  if (hnhomo::round_i32(0.5f) != 0 || hnhomo::round_i32(1.5f) != 2 || hnhomo::round_i32(2.5f) != 2 ||
      hnhomo::round_i32(-0.5f) != 0 || hnhomo::round_i32(-1.5f) != -2)
    return 3;  // half to even
  if (hnhomo::trunc_i32(-1.9f) != -1 || hnhomo::trunc_i32(1.9f) != 1 || hnhomo::trunc_i32(nan) != 0) return 3;
  // the largest squared distance fits
  sink += hnhomo::msd(1073741760, 1073741760, -1073741760, -1073741760);

  for (auto [H, W] : dims) {
    const int32_t hw = H * W;
    const auto homos = homographies(H, W);
    for (int64_t B : {(int64_t)1, (int64_t)3}) {
      const int64_t total = B * hw;
      // exactly sized heap buffers: one element past either end is a sanitizer report
      std::vector<float> score((size_t)total), scale((size_t)total), ori((size_t)total * 2);
      for (size_t i = 0; i < score.size(); ++i) score[i] = 0.25f + (float)(i % 7);
      for (size_t mi = 0; mi < homos.size(); ++mi) {
        const float* h = homos[mi].data();
        const float* h2 = homos[(mi * 7 + 3) % homos.size()].data();
        for (size_t si = 0; si < scales.size(); ++si) {
          for (size_t i = 0; i < scale.size(); ++i) scale[i] = scales[(si + i) % scales.size()];
          for (size_t i = 0; i < ori.size(); ++i) ori[i] = oris[(si * 3 + i) % oris.size()];
          for (int64_t b = 0; b < B; ++b)
            for (int32_t y = 0; y < H; ++y)
              for (int32_t x = 0; x < W; ++x) {
                // hn_warp_score: both settings, every border
                if (si < 2)
                  for (int align = 0; align < 2; ++align) {
                    const hnhomo::Bilinear s = hnhomo::bilinear(h, x, y, H, W, align);
                    for (int k = 0; k < 4; ++k)
                      if (s.ok[k]) {
                        if (s.idx[k] < 0 || s.idx[k] >= hw) return fail("warp", s.idx[k], hw, H, W, mi);
                        const int32_t border = (int32_t)si * ((H < W ? H : W) - 1) / 2;
                        sink += hnhomo::in_border(s.idx[k], H, W, border) ? 0.0f : score[(size_t)(b * hw + s.idx[k])];
                      }
                  }
                // hn_gt_scale_orin
                int32_t qx, qy;
                const int32_t q = hnhomo::gt_source(h, x, y, H, W, &qx, &qy);
                if (q < 0 || q >= hw || qx < 0 || qx >= W || qy < 0 || qy >= H) return fail("gt", q, hw, H, W, mi);
                const size_t at = (size_t)(b * hw + q);
                hnhomo::Point centre;
                const float gs = hnhomo::gt_scale_at(h2, qx, qy, scale[at], &centre);
                const hnhomo::Point go = hnhomo::gt_ori_at(h2, qx, qy, scale[at], ori[at * 2], ori[at * 2 + 1], centre);
                sink += (gs == gs ? 1.0 : 0.0) + (go.x == go.x ? 1.0 : 0.0);
                ++n_pixels;
              }
        }
        // hn_project_keypoints: keypoints and batch indices far outside, both clamp settings
        const int64_t big = (int64_t)1 << 62;
        const std::vector<int64_t> coords = {big, -big, std::numeric_limits<int64_t>::max(),
                                             std::numeric_limits<int64_t>::min(), -1, 0, 1, W - 1, W, 1000};
        const std::vector<int64_t> batches = {-1, (int64_t)1 << 40, 0, B - 1, B, std::numeric_limits<int64_t>::min(),
                                              std::numeric_limits<int64_t>::max()};
        std::vector<float> all_h((size_t)B * 9);
        for (int64_t b = 0; b < B; ++b)
          for (int k = 0; k < 9; ++k) all_h[(size_t)b * 9 + k] = homos[(mi + (size_t)b) % homos.size()][k];
        for (int64_t bi : batches)
          for (size_t ci = 0; ci < coords.size(); ++ci)
            for (int clamp = 0; clamp < 2; ++clamp) {
              const int64_t kp[4] = {bi, coords[(ci * 3 + 1) % coords.size()], coords[ci], 0};
              const int64_t hb = hnhomo::homography_of(kp, B);
              if (hb < 0 || hb >= B) return fail("homography", hb, B, H, W, mi);
              const hnhomo::Projected r = hnhomo::project_keypoint(kp, &all_h[(size_t)hb * 9], B, H, W, clamp);
              if (r.gather < 0 || r.gather >= total) return fail("gather", r.gather, total, H, W, mi);
              if (clamp && (r.x < 0 || r.x >= W || r.y < 0 || r.y >= H)) return fail("clamp", r.x, W, H, W, mi);
              sink += scale[(size_t)r.gather] == 0.0f ? 1.0 : 0.0;
              sink += ori[(size_t)r.gather * 2 + 1] == 0.0f ? 1.0 : 0.0;
              ++n_keypoints;
            }
      }
      // hn_mask_keypoints: masks with 0, 1, every other and H W set pixels; the rows of every pixel
      for (int kind = 0; kind < 4; ++kind) {
        std::vector<uint8_t> mask((size_t)total);
        for (size_t i = 0; i < mask.size(); ++i)
          mask[i] = kind == 0 ? 0 : kind == 1 ? (i % (size_t)hw == (size_t)hw - 1) : kind == 2 ? (i & 1) * 255 : 1;
        for (int32_t K : {1, hw / 2 > 0 ? hw / 2 : 1, hw}) {
          std::vector<int64_t> rows((size_t)B * K * 4, -7);
          for (int64_t b = 0; b < B; ++b) {
            int32_t rank = 0;
            for (int32_t idx = 0; idx < hw; ++idx)
              if (mask[(size_t)(b * hw + idx)] && rank < K) hnhomo::keypoint_row(&rows[(size_t)((b * K + rank++) * 4)], b, idx, W);
            for (; rank < K; ++rank) hnhomo::keypoint_row(&rows[(size_t)((b * K + rank) * 4)], b, 0, W);
          }
          for (size_t r = 0; r < rows.size(); r += 4) {
            if (rows[r] < 0 || rows[r] >= B || rows[r + 1] < 0 || rows[r + 1] >= H || rows[r + 2] < 0 ||
                rows[r + 2] >= W || rows[r + 3] != 0)
              return fail("mask row", rows[r + 1] * W + rows[r + 2], hw, H, W, 0);
            sink += score[(size_t)(rows[r] * hw + rows[r + 1] * W + rows[r + 2])];
          }
          ++n_masks;
        }
      }
    }
  }
  std::printf("homo_check: %lld pixels, %lld keypoints, %lld masks, every index in bounds (checksum %g)\n", n_pixels,
              n_keypoints, n_masks, sink);
  return 0;
}
