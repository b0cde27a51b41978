// RF-Net's ten-scale detector (hn_rfdet.hip): the parameter layout, the workspace plan and the window, halo and
// tile address arithmetic of its kernels.  Plain C++ with no HIP type, so that a host program
// (hn_rfdet_host_check.cpp) can include it and walk every index the kernels form.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HNRF_HD __host__ __device__ __forceinline__
#else
#define HNRF_HD inline
#endif

namespace hnrf {

constexpr int kLevels = 10;
constexpr int kC = 16;              // channels of every level
constexpr int kStateFloats = 21890; // RFDetSO.state_dict(): 160 + 9 * 2320 + 10 * 32 + 10 * 17 + 10 * 2 + 10 * 34

// ---- device parameter block: kLevels records of kLevelStride floats, then scale_list[10] -------------------------
// conv weights: level 1 as [cout][tap] (144 floats); levels 2..10 in the MFMA B-operand order
// [step s = 0..35][lane l = 0..63] = w[cout = l & 15][cin = (s & 3) * 4 + (l >> 4)][tap = s >> 2]
constexpr int kConvW = 0;
constexpr int kConvB = 2304;   // [16]
constexpr int kInG = 2320;     // insnorm_k.weight [16]
constexpr int kInB = 2336;     // insnorm_k.bias [16]
constexpr int kSW = 2352;      // conv_s.weight [16]
constexpr int kSB = 2368;      // conv_s.bias
constexpr int kSG = 2369;      // insnorm_s.weight
constexpr int kSBeta = 2370;   // insnorm_s.bias
constexpr int kOW = 2371;      // conv_o.weight [2][16]
constexpr int kOB = 2403;      // conv_o.bias [2]
constexpr int kLevelStride = 2408;
constexpr int kScaleList = kLevels * kLevelStride;
constexpr int kDeviceFloats = kScaleList + kLevels;

HNRF_HD int mfma_weight_index(int cout, int cin, int tap) {  // where w[cout][cin][tap] sits in a level's kConvW block
  const int s = tap * 4 + (cin >> 2), lane = ((cin & 3) << 4) | cout;
  return s * 64 + lane;
}

// ---- layer kernels: one 256-thread workgroup per 16 x 16 tile, input window with halo 1 ---------------------------
constexpr int kT = 16;
constexpr int kWin = kT + 2;          // 18
constexpr int kWinN = kWin * kWin;    // 324
constexpr int kPlane = 336;           // LDS floats per channel plane (>= kWinN, = 16 mod 64: the four k-lanes of an
                                      // MFMA A read fall on different banks)
constexpr int kLdsFloats = kC * kPlane;

HNRF_HD bool inside(int y, int x, int H, int W) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; }
HNRF_HD int tiles_x(int W) { return (W + kT - 1) / kT; }
HNRF_HD int64_t tiles(int H, int W) { return (int64_t)((H + kT - 1) / kT) * tiles_x(W); }
// window position i (0 .. kWinN - 1) of the tile at (y0, x0): image coordinates
HNRF_HD int win_y(int y0, int i) { return y0 - 1 + i / kWin; }
HNRF_HD int win_x(int x0, int i) { return x0 - 1 + i % kWin; }
// is window position i one of the tile's own 16 x 16 pixels
HNRF_HD bool win_own(int i) {
  const int r = i / kWin, c = i % kWin;
  return r >= 1 && r <= kT && c >= 1 && c <= kT;
}
HNRF_HD int64_t pixel(int64_t b, int y, int x, int H, int W) { return (b * H + y) * (int64_t)W + x; }
// the LDS word an MFMA lane reads as A[m][k] of step s for output row `row` (0..15) of the tile
HNRF_HD int lds_a_index(int s, int lane, int row) {
  const int tap = s >> 2, cin = (s & 3) * 4 + (lane >> 4), m = lane & 15;
  return cin * kPlane + (row + tap / 3) * kWin + m + tap % 3;
}

// ---- tail kernel: 32 x 32 tile, score window with halo 14 ---------------------------------------------------------
constexpr int kT2 = 32;
constexpr int kHalo2 = 14;
constexpr int kS = kT2 + 2 * kHalo2;  // 60: normalised score window
constexpr int kSP = kS + 1;           // its padded row
constexpr int kM = kT2 + 14;          // 46: maximum / exp window (halo 7)
HNRF_HD int64_t tiles2(int H, int W) { return (int64_t)((H + kT2 - 1) / kT2) * ((W + kT2 - 1) / kT2); }

// ---- statistics --------------------------------------------------------------------------------------------------
// slot j (0..10) holds what step j produced: [0..15] mean, [16..31] 1/sqrt(var + eps) of pre_{j+1} (j <= 9),
// [32] mean, [33] 1/sqrt(var + eps) of the raw score s_j (j >= 1)
constexpr int kSlots = kLevels + 1;
constexpr int kStatFloats = 36;
constexpr int kPartPre = 32;  // doubles per workgroup: sum[16], sum of squares[16]
constexpr int kPartS = 2;

// ---- workspace plan (bytes from the start, every block 16-byte aligned) -------------------------------------------
struct Plan {
  size_t stat, part_pre, part_s, pre[2], feat[2], sraw, ounit, total;
};
HNRF_HD size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
HNRF_HD Plan plan(int64_t B, int H, int W) {
  Plan p;
  const size_t n = (size_t)B * (size_t)H * (size_t)W, wg = (size_t)B * (size_t)tiles(H, W);
  size_t o = 0;
  p.stat = o;      o += align16((size_t)B * kSlots * kStatFloats * sizeof(float));
  p.part_pre = o;  o += align16(wg * kLevels * kPartPre * sizeof(double));
  p.part_s = o;    o += align16(wg * kLevels * kPartS * sizeof(double));
  for (int i = 0; i < 2; ++i) { p.pre[i] = o;  o += align16(n * kC * sizeof(float)); }
  for (int i = 0; i < 2; ++i) { p.feat[i] = o; o += align16(n * kC * sizeof(float)); }
  p.sraw = o;      o += align16(n * kLevels * sizeof(float));
  p.ounit = o;     o += align16(n * kLevels * 2 * sizeof(float));
  p.total = o;
  return p;
}

}  // namespace hnrf
