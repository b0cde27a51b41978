// Per-sample address and weight computation of the keypoint patch extraction (hn_clip.hip), restating
// FDLNet-master/latency/NASNet/utils/image_utils.py:11-158 (clip_patch) in fp32 in its operation order.
// __host__ __device__ and free of HIP types, so that the same text runs in the kernel and in the host
// programs that sweep adversarial keypoints under the sanitizers (hn_clip_host_check.cpp, and
// hn_clip_grad_host_check.cpp for the backward's functions at the end of this file).
//
// Bounds guarantee: whatever the keypoint data (NaN, Inf, values beyond the integer range, any batch index),
// every pixel pair returned (p and p + 1) lies in [0, B * H * W), for B >= 1 and H, W >= 2 with B * H * W < 2^63.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HN_CLIP_HD __host__ __device__ inline
#else
#define HN_CLIP_HD inline
#endif

namespace hnclip {

constexpr int kPatch = 32;  // PSIZE of the native path

// What a patch's 1,024 samples share: the 2x2 affine (scale and rotation), the keypoint in raw-image
// pixels and the flat offset of its image.
struct Keypoint {
  float sc, nss, ss;  // s cos, -(s sin), s sin with s = (scale / ratio) / 2
  float kx, ky;
  int64_t base;       // b * H * W, b clamped to [0, B - 1]
};

// One output pixel: its four neighbours a = (y0, x0), b = (y1, x0), c = (y0, x1), d = (y1, x1) and their
// bilinear weights (image_utils.py:125-152).  x0 and x1 are neighbours or, clamped at a border, the same
// column, so each image row is read as ONE pair of adjacent pixels, images[p] and images[p + 1] with
// p = p0 (row y0) or p1 (row y1) at column min(x0, W - 2): hi0 / hi1 say whether x0 / x1 is the pair's second.
struct Sample {
  int64_t p0, p1;
  bool hi0, hi1;
  float wa, wb, wc, wd;
};

// A pair of adjacent pixels, read as one 8-byte access at 4-byte alignment.
struct __attribute__((packed, aligned(4))) PixelPair {
  float lo, hi;
};

// torch.linspace(-1, 1, 32, dtype=float)[i]: step = 2 / 31, counted from the nearer end.
HN_CLIP_HD float grid_value(int i) {
#pragma clang fp contract(off)
  const float step = 2.0f / 31.0f;
  return i < kPatch / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(kPatch - 1 - i);
}

// kp: the keypoint's row (b, y, x, .); ori: its (cos, sin) or null for no rotation; ratio: [B] (im_info[:,0]).
// The batch index addresses both the image and the ratio, clamped to [0, B - 1].
HN_CLIP_HD Keypoint keypoint(const int64_t* kp, float scale, const float* ori, const float* ratio, int64_t B,
                             int32_t H, int32_t W) {
#pragma clang fp contract(off)
  int64_t b = kp[0];
  b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
  const float r = ratio[b];
  const float s = (scale / r) / 2.0f;
  const float c = ori ? ori[0] : 1.0f, sn = ori ? ori[1] : 0.0f;
  Keypoint k;
  k.sc = s * c;
  k.ss = s * sn;
  k.nss = -k.ss;
  k.kx = (float)kp[2] / r;
  k.ky = (float)kp[1] / r;
  k.base = b * ((int64_t)H * (int64_t)W);
  return k;
}

// floor(v) as an integer clamped to [0, hi] together with floor(v) + 1 clamped likewise (image_utils.py:99-107).
// 32-bit throughout (the 64-bit conversions and clamps cost the kernel half its VALU time): the float is
// limited to [-1, 2^31 - 128], the largest float below 2^31, before the conversion, and a value of 2^31 or
// more becomes 2^31 - 2, so the clamp maps everything as it would the unlimited value (hi <= 2^31 - 2) and
// a + 1 cannot overflow; a NaN takes the lower limit.  No conversion here is undefined for any v.
HN_CLIP_HD void floor_pair(float v, int32_t hi, int32_t* i0, int32_t* i1) {
  const float f = floorf(v);
  float fc = f >= -1.0f ? f : -1.0f;  // NaN -> -1
  fc = fc > 2147483520.0f ? 2147483520.0f : fc;
  int32_t a = (int32_t)fc;
  a = f >= 2147483648.0f ? INT32_MAX - 1 : a;
  const int32_t b = a + 1;
  *i0 = a < 0 ? 0 : (a > hi ? hi : a);
  *i1 = b < 0 ? 0 : (b > hi ? hi : b);
}

HN_CLIP_HD Sample sample(const Keypoint& k, int row, int col, int32_t H, int32_t W) {
#pragma clang fp contract(off)
  const float gx = grid_value(col), gy = grid_value(row);
  const float xs = k.sc * gx + k.nss * gy + k.kx;
  const float ys = k.ss * gx + k.sc * gy + k.ky;
  int32_t x0, x1, y0, y1;
  floor_pair(xs, W - 1, &x0, &x1);
  floor_pair(ys, H - 1, &y0, &y1);
  const int64_t r0 = k.base + (int64_t)y0 * W, r1 = k.base + (int64_t)y1 * W;
  // the weights come from the clamped corners: a sample outside the image gets (nearly) zero
  const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
  const int32_t xl = x0 < W - 1 ? x0 : W - 2;  // in [0, W - 2]: both xl and xl + 1 are columns of the image
  Sample s;
  s.p0 = r0 + xl;
  s.p1 = r1 + xl;
  s.hi0 = x0 != xl;
  s.hi1 = x1 != xl;
  s.wa = (x1f - xs) * (y1f - ys);
  s.wb = (x1f - xs) * (ys - y0f);
  s.wc = (xs - x0f) * (y1f - ys);
  s.wd = (xs - x0f) * (ys - y0f);
  return s;
}

// wa Ia + wb Ib + wc Ic + wd Id, summed left to right without contraction (image_utils.py:154-156), from the
// two pixel pairs top = images[p0], images[p0 + 1] and bottom = images[p1], images[p1 + 1]
HN_CLIP_HD float blend(const Sample& s, const PixelPair& top, const PixelPair& bottom) {
#pragma clang fp contract(off)
  const float Ia = s.hi0 ? top.hi : top.lo, Ic = s.hi1 ? top.hi : top.lo;
  const float Ib = s.hi0 ? bottom.hi : bottom.lo, Id = s.hi1 ? bottom.hi : bottom.lo;
  return s.wa * Ia + s.wb * Ib + s.wc * Ic + s.wd * Id;
}

// ---- backward (hn_clip_patch_backward): gradients to the keypoint's scale and orientation ----
// The corners are detached (the reference's .floor().long()), so a sample's value is bilinear in (xs, ys) inside
// its cell and its derivative is a difference of pixels weighted by the distance to the opposite edge.

// One output pixel for the backward: the forward's addresses (so its bounds guarantee carries over) and the four
// edge distances ux = x1 - xs, vx = xs - x0, uy = y1 - ys, vy = ys - y0, computed as the forward computes them.
struct SampleGrad {
  Sample s;
  float ux, vx, uy, vy;
  float gx, gy;  // the sample's grid values (col, row)
};

HN_CLIP_HD SampleGrad sample_grad(const Keypoint& k, int row, int col, int32_t H, int32_t W) {
#pragma clang fp contract(off)
  SampleGrad g;
  g.s = sample(k, row, col, H, W);
  g.gx = grid_value(col);
  g.gy = grid_value(row);
  const float xs = k.sc * g.gx + k.nss * g.gy + k.kx;
  const float ys = k.ss * g.gx + k.sc * g.gy + k.ky;
  int32_t x0, x1, y0, y1;
  floor_pair(xs, W - 1, &x0, &x1);
  floor_pair(ys, H - 1, &y0, &y1);
  g.ux = (float)x1 - xs;
  g.vx = xs - (float)x0;
  g.uy = (float)y1 - ys;
  g.vy = ys - (float)y0;
  return g;
}

// Adds one sample's share of a = d out / d (s cos) and b = d out / d (s sin), d being the upstream gradient of
// the pixel:  gX = d value / d xs = uy (Ic - Ia) + vy (Id - Ib),  gY = d value / d ys = ux (Ib - Ia) + vx (Id - Ic)
// (pixel differences first: where clamping makes two corners one pixel the term is exactly 0), and
// xs = (s cos) gx - (s sin) gy + kx,  ys = (s sin) gx + (s cos) gy + ky.
HN_CLIP_HD void accumulate_grad(const SampleGrad& g, const PixelPair& top, const PixelPair& bottom, float d, float* a,
                                float* b) {
#pragma clang fp contract(off)
  const float Ia = g.s.hi0 ? top.hi : top.lo, Ic = g.s.hi1 ? top.hi : top.lo;
  const float Ib = g.s.hi0 ? bottom.hi : bottom.lo, Id = g.s.hi1 ? bottom.hi : bottom.lo;
  const float gX = g.uy * (Ic - Ia) + g.vy * (Id - Ib);
  const float gY = g.ux * (Ib - Ia) + g.vx * (Id - Ic);
  *a += d * (gX * g.gx + gY * g.gy);
  *b += d * (gY * g.gx - gX * g.gy);
}

// The chain rule from (a, b), summed over the patch, to the keypoint's scale and orientation: with
// s = (scale / r) / 2, s cos and s sin give  d scale = (a cos + b sin) / r / 2,  d ori = (a s, b s).
// ori null: cos = 1, sin = 0.  dscale / dori (two floats) may each be null.
HN_CLIP_HD void keypoint_grad(const int64_t* kp, float scale, const float* ori, const float* ratio, int64_t B,
                              float a, float b, float* dscale, float* dori) {
#pragma clang fp contract(off)
  int64_t bi = kp[0];
  bi = bi < 0 ? 0 : (bi > B - 1 ? B - 1 : bi);
  const float r = ratio[bi];
  const float c = ori ? ori[0] : 1.0f, sn = ori ? ori[1] : 0.0f;
  if (dscale) *dscale = ((a * c + b * sn) / r) / 2.0f;
  if (dori) {
    const float s = (scale / r) / 2.0f;
    dori[0] = a * s;
    dori[1] = b * s;
  }
}

}  // namespace hnclip
