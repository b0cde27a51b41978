// Projection, float -> integer conversions and address computations of the homography ground-truth stage
// (hn_gt.hip), restating in fp32 FDLNet-master/latency/NASNet utils/image_utils.py:161-213 (warp, filter_border),
// utils/common_utils.py:45-75 (imgBatchXYZ, transXYZ_2_to_1), utils/math_utils.py:43-125 (ptCltoCr, L2Norm, MSD),
// utils/net_utils.py:27-37 (pair's nonzero / masked_select) and model/network.py:200-264 (gt_scale_orin).
// __host__ __device__ and free of HIP types: the kernels and the host program that sweeps adversarial homographies,
// keypoints and masks under the sanitizers (hn_homo_host_check.cpp) compile the same text.
//
// Bounds guarantee: for n_images >= 1, height, width >= 2, height * width < 2^31 and n_images * height * width
// < 2^62, every index returned here lies inside its array whatever the homography, keypoint, scale, orientation or
// mask data holds (NaN, Inf, values beyond the integer range, any batch index), and no float -> integer conversion
// is undefined.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HN_HOMO_HD __host__ __device__ inline
#else
#define HN_HOMO_HD inline
#endif

namespace hnhomo {

struct Point {
  float x, y;
};

// (u / (w + 1e-8), v / (w + 1e-8)) of h (row-major 3x3) applied to (x, y, 1): transXYZ_2_to_1's matmul row by
// row, products summed left to right, IEEE divisions.
HN_HOMO_HD Point project(const float* h, float x, float y) {
#pragma clang fp contract(off)
  const float u = h[0] * x + h[1] * y + h[2];
  const float v = h[3] * x + h[4] * y + h[5];
  const float w = h[6] * x + h[7] * y + h[8];
  const float d = w + 1e-8f;
  Point p;
  p.x = u / d;
  p.y = v / d;
  return p;
}

// .long(): truncation toward zero.  A NaN gives 0 and the value saturates at +-(2^30 - 64), the largest float
// below 2^30, so that the difference of two results and the sum of two squared differences fit an int64.  Every
// image has fewer than 2^31 pixels, so a saturated coordinate lies outside it either way.
HN_HOMO_HD int32_t trunc_i32(float v) {
  const float lim = 1073741760.0f;
  float c = v >= -lim ? v : -lim;  // NaN -> -lim ...
  c = c > lim ? lim : c;
  c = v != v ? 0.0f : c;  // ... -> 0
  return (int32_t)c;
}

// .round().long(): half to even.  A NaN gives 0; saturates at +-(2^31 - 128), the largest float below 2^31.
HN_HOMO_HD int32_t round_i32(float v) {
  const float lim = 2147483520.0f;
  const float r = rintf(v);
  float c = r >= -lim ? r : -lim;
  c = c > lim ? lim : c;
  c = r != r ? 0.0f : c;
  return (int32_t)c;
}

HN_HOMO_HD int32_t clamp_i32(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
HN_HOMO_HD int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// MSD of two truncated points (math_utils.py:114-125): 2 sqrt(float(dx^2 + dy^2) + 1e-8), the sum in integers
HN_HOMO_HD float msd(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
#pragma clang fp contract(off)
  const int64_t dx = (int64_t)ax - (int64_t)bx, dy = (int64_t)ay - (int64_t)by;  // |.| < 2^31
  const float sm = (float)(dx * dx + dy * dy);                                   // < 2^63
  return sqrtf(sm + 1e-8f) * 2.0f;
}

// ---- hn_warp_score ----------------------------------------------------------------------------------------
// grid_sample's bilinear sample with zeros padding at the projection of output pixel (x, y): the four corners
// floor and floor + 1 (unclamped) with the weights computed from them; ok[k] says whether corner k lies inside the
// image, and only then is idx[k] (flat within the image, in [0, H W)) defined.  Order: nw, ne, sw, se.
struct Bilinear {
  float w[4];
  int32_t idx[4];
  bool ok[4];
};

// whether the float (an integer value, +-Inf or NaN) is an index of [0, n); then *i is it.  The comparison with n is
// made on integers: (float)(n - 1) rounds up for n above 2^24.
HN_HOMO_HD bool inside(float f, int32_t n, int32_t* i) {
  if (!(f >= 0.0f && f < 2147483648.0f)) return false;  // NaN, Inf: outside; below 2^31 the conversion is defined
  const int32_t v = (int32_t)f;
  if (v >= n) return false;
  *i = v;
  return true;
}

HN_HOMO_HD Bilinear bilinear(const float* h, int32_t x, int32_t y, int32_t H, int32_t W, int align_corners) {
#pragma clang fp contract(off)
  const Point p = project(h, (float)x, (float)y);
  const float xn = p.x / (float)(W - 1) * 2.0f - 1.0f, yn = p.y / (float)(H - 1) * 2.0f - 1.0f;
  float ix, iy;
  if (align_corners) {
    ix = (xn + 1.0f) / 2.0f * (float)(W - 1);
    iy = (yn + 1.0f) / 2.0f * (float)(H - 1);
  } else {
    ix = ((xn + 1.0f) * (float)W - 1.0f) / 2.0f;
    iy = ((yn + 1.0f) * (float)H - 1.0f) / 2.0f;
  }
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  Bilinear s;
  s.w[0] = (x1 - ix) * (y1 - iy);
  s.w[1] = (ix - x0) * (y1 - iy);
  s.w[2] = (x1 - ix) * (iy - y0);
  s.w[3] = (ix - x0) * (iy - y0);
  int32_t xi0 = 0, xi1 = 0, yi0 = 0, yi1 = 0;
  const bool bx0 = inside(x0, W, &xi0), bx1 = inside(x1, W, &xi1);
  const bool by0 = inside(y0, H, &yi0), by1 = inside(y1, H, &yi1);
  s.ok[0] = bx0 && by0;
  s.ok[1] = bx1 && by0;
  s.ok[2] = bx0 && by1;
  s.ok[3] = bx1 && by1;
  s.idx[0] = s.ok[0] ? yi0 * W + xi0 : 0;
  s.idx[1] = s.ok[1] ? yi0 * W + xi1 : 0;
  s.idx[2] = s.ok[2] ? yi1 * W + xi0 : 0;
  s.idx[3] = s.ok[3] ? yi1 * W + xi1 : 0;
  return s;
}

// filter_border: whether pixel idx of an H x W image lies within `border` of an edge (its value reads as 0)
HN_HOMO_HD bool in_border(int32_t idx, int32_t H, int32_t W, int32_t border) {
  const int32_t y = idx / W, x = idx - y * W;
  return x < border || x >= W - border || y < border || y >= H - border;
}

// ---- hn_gt_scale_orin -------------------------------------------------------------------------------------
// q = clamp(round(proj(homo12, p))) of output pixel p = (x, y), flat within the image: in [0, H W)
HN_HOMO_HD int32_t gt_source(const float* h12, int32_t x, int32_t y, int32_t H, int32_t W, int32_t* qx, int32_t* qy) {
  const Point p = project(h12, (float)x, (float)y);
  *qx = clamp_i32(round_i32(p.x), 0, W - 1);
  *qy = clamp_i32(round_i32(p.y), 0, H - 1);
  return *qy * W + *qx;
}

// centScale at q (network.py:210-229): s the scale there
HN_HOMO_HD float gt_scale_at(const float* h21, int32_t qx, int32_t qy, float s, Point* centre) {
#pragma clang fp contract(off)
  const float fx = (float)qx, fy = (float)qy;
  const float hs = floorf(s / 2.0f);  // the reference's float //
  const Point c = project(h21, fx, fy);
  const Point u = project(h21, fx, fy - hs), b = project(h21, fx, fy + hs);
  const Point r = project(h21, fx + hs, fy), l = project(h21, fx - hs, fy);
  const int32_t cx = trunc_i32(c.x), cy = trunc_i32(c.y);
  const float up = msd(trunc_i32(u.x), trunc_i32(u.y), cx, cy);
  const float right = msd(trunc_i32(r.x), trunc_i32(r.y), cx, cy);
  const float bottom = msd(trunc_i32(b.x), trunc_i32(b.y), cx, cy);
  const float left = msd(trunc_i32(l.x), trunc_i32(l.y), cx, cy);
  *centre = c;
  return (up + right + bottom + left) / 4.0f;
}

// (cos_w, sin_w) at q divided by the pair's L2 norm (network.py:232-240, 261-262): (c, sn) the orientation there
HN_HOMO_HD Point gt_ori_at(const float* h21, int32_t qx, int32_t qy, float s, float c, float sn, const Point& centre) {
#pragma clang fp contract(off)
  const Point o = project(h21, (float)qx + s * c, (float)qy + s * sn);
  const float ww = o.x - centre.x, hw = o.y - centre.y;
  const float r = sqrtf(ww * ww + hw * hw + 1e-8f);
  const float cw = ww / (r + 1e-8f), sw = hw / (r + 1e-8f);
  const float n = sqrtf(cw * cw + sw * sw);
  Point out;
  out.x = cw / n;
  out.y = sw / n;
  return out;
}

// ---- hn_mask_keypoints ------------------------------------------------------------------------------------
// the row (b, y, x, 0) of pixel idx of image b
HN_HOMO_HD void keypoint_row(int64_t* row, int64_t b, int32_t idx, int32_t W) {
  const int32_t y = idx / W;
  row[0] = b;
  row[1] = y;
  row[2] = idx - y * W;
  row[3] = 0;
}

// ---- hn_project_keypoints ---------------------------------------------------------------------------------
// ptCltoCr for one keypoint row (b, y, x, .): the image index that selects the homography (column 0 clamped to
// [0, B - 1]), the projected and rounded (x', y'), clamped to the image if `clamp`, and the gather index
// b H W + y' W + x' clamped to [0, B H W - 1] (math_utils.py:85-90).
struct Projected {
  int64_t b;       // in [0, B - 1]
  int32_t x, y;
  int64_t gather;  // in [0, B H W)
};

HN_HOMO_HD int64_t homography_of(const int64_t* kp, int64_t B) { return clamp_i64(kp[0], 0, B - 1); }

HN_HOMO_HD Projected project_keypoint(const int64_t* kp, const float* h, int64_t B, int32_t H, int32_t W, int clamp) {
  Projected r;
  r.b = homography_of(kp, B);
  const Point p = project(h, (float)kp[2], (float)kp[1]);  // leftC_homo.float()
  r.x = round_i32(p.x);
  r.y = round_i32(p.y);
  if (clamp) {
    r.x = clamp_i32(r.x, 0, W - 1);
    r.y = clamp_i32(r.y, 0, H - 1);
  }
  const int64_t hw = (int64_t)H * (int64_t)W;
  // |y' W| < 2^31 2^30 and b H W < 2^62: no overflow
  r.gather = clamp_i64(r.b * hw + (int64_t)r.y * (int64_t)W + (int64_t)r.x, 0, B * hw - 1);
  return r;
}

}  // namespace hnhomo
