// What every reduction of the train-mode loss_HardNet shares (hn_loss.hip: 'min' and 'random'; hn_loss_dense.hip:
// 'average'): the per-row pass (|v|^2 of every row and the positive distance from the difference form) and the
// per-entry loss f(pos, mn) with its two partials.  Internal linkage: each loss file gets its own copy.
#pragma once
#include "hn_common.h"

namespace {

// |v|^2 of every row (a then p), one wave per row; for w < B also the positive distance d_ii from
// |a_i - p_i|^2 directly: the expanded |a|^2 + |p|^2 - 2 a.p of the distance matrix cancels for the
// close pairs of a training batch (the reference's fp32 loss carries that error: 2e-6 on a mean of
// distances), the difference form keeps d_ii at fp32 accuracy
HN_DEV float diff_sq(const float* a, const float* p, int lane) {
  const float2 u = reinterpret_cast<const float2*>(a)[lane], v = reinterpret_cast<const float2*>(p)[lane];
  const float dx = u.x - v.x, dy = u.y - v.y;
  return wave_sum(fmaf(dx, dx, dy * dy));
}
__global__ __launch_bounds__(256) void k_lmin_sq(const float* __restrict__ a, const float* __restrict__ p, int B,
                                                 float* __restrict__ sq, float* __restrict__ pos,
                                                 float* __restrict__ posx) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= 2 * B) return;
  const float* r = (w < B ? a + (size_t)w * 128 : p + (size_t)(w - B) * 128);
  const float2 v = reinterpret_cast<const float2*>(r)[lane];
  const float s = wave_sum(v.x * v.x + v.y * v.y);
  if (lane == 0) sq[w] = s;
  if (w < B) {
    const float x = diff_sq(a + (size_t)w * 128, p + (size_t)w * 128, lane);
    if (lane == 0) {
      pos[w] = sqrtf(x + 1e-6f) + 1e-8f;
      posx[w] = x;  // (kept for the backward's sqrt derivative)
    }
  }
}

// per-row loss f(pos, mn) and its partials d f / d pos, d f / d mn (autograd's forms)
HN_DEV float loss_of(int type, float margin, float ps, float mn, float* dpos, float* dmn) {
  if (type == 0) {  // clamp(margin + pos - mn, min=0); clamp's backward passes at t >= 0
    const float t = margin + ps - mn;
    *dpos = t >= 0.f ? 1.f : 0.f;
    *dmn = -*dpos;
    return fmaxf(t, 0.f);
  }
  if (type == 1) {  // -log(exp_pos / (exp_pos + exp(2 - mn) + eps))
    const float ep = expf(2.0f - ps), en = expf(2.0f - mn);
    const float den = ep + en + 1e-8f;
    *dpos = (en + 1e-8f) / den;
    *dmn = -en / den;
    return -logf(ep / den);
  }
  const float t = margin - mn;  // clamp(margin - mn, min=0) + pos
  *dpos = 1.f;
  *dmn = t >= 0.f ? -1.f : 0.f;
  return fmaxf(t, 0.f) + ps;
}

// the masked distance dn of entry (i, j) from u = (|a_i|^2 + |p_j|^2) - 2 a_i.p_j (Losses.py:5-13, :93-101)
HN_DEV float masked_dn(float u, bool diag) {
  const float d = sqrtf(u + 1e-6f) + 1e-8f;
  float dn = diag ? d + 10.0f : d;
  if (dn < 0.008f) dn += 10.0f;
  return dn;
}

}  // namespace
