// Internal host-side interface between the C ABI (hn_api*.hip; their own helpers: hn_api_util.h) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "hardnet_mi355x.h"

// A/B switches of the launchers.  Read from the environment once per model in hn_create (and
// once per process for the model-less entry points); hn_forward makes the calling model's
// set current for the duration of the call (thread-local), so launchers never call getenv.
// Every switch selects a parity-tested alternative kernel; the ablation switches (c12_abl,
// head_abl, w4_abl, pairdist_abl, dbg: timing-only builds with wrong results) exist only in the
// HN_EXPERIMENTS library.
struct HnKnobs {
  int c12_cfg = 15;            // HN_C12_CFG: k_c12 configuration (0..15, all within the parity bar; 15 = k_c12s)
  int head = 4;                // HN_HEAD: head GEMM form (1 k_head, 2 k_head2, 3 k_head3 LDS-DMA rings, 4 k_head4 256-patch rings)
  bool head_pf = true;         // HN_HEAD_PF: k_head4 reads chunk c + 1 from LDS while chunk c runs (0: off)
  bool fdl_valu = false;       // HN_FDL_VALU: FDLNet front as fp32 VALU
  bool naive_pw = false;       // HN_NAIVE_PW: untiled 1x1 conv kernel
  bool naive_dw = false;       // HN_NAIVE_DW: untiled depthwise kernel
  bool no_skipfuse = false;    // HN_NO_SKIPFUSE: maxpool + pw instead of k_skip_s2 (and no k_irf_skip)
  bool no_irfskip = false;     // HN_NO_IRFSKIP: k_irf + k_skip_s2 instead of k_irf_skip
  bool pairdist_valu = false;  // HN_PAIRDIST_VALU: fp32 VALU pair-distance kernel
  bool pairdist_reg = false;   // HN_PAIRDIST_REG: register-staged positives instead of the LDS-DMA ring
  bool pairdist_spread = true;  // HN_PAIRDIST_SPREAD: the ring's DMA issued inside the MFMA chain (0: before it)
  bool front_fold = false;     // HN_FRONT_FOLD: the NAS front's pwl with the LDS partial-sum fold
  bool u8_apart = false;       // HN_U8_APART: uint8 input preprocessed into the workspace first (A/B)
  bool front_xch3 = false;     // HN_FRONT_XCH3: the k3 front's dw per channel group (SGPR weights, s_x; two
                               // workgroups per CU instead of three: wang2 front 5.05 -> 5.57 ms, not the default)
  bool no_mpfront = false;     // HN_NO_MPFRONT: k_front (max-pool) + k_irf instead of k_mpfront_irf
  bool pipeline = false;       // HN_PIPELINE=1: HardNet batches of several chunks overlap chunk k + 1's k_c12s (second
                               // stream) with chunk k's conv3 .. head (opt-in: measured within noise)
  bool irf3 = false;           // HN_IRF3 (HN_EXPERIMENTS only): k_irf3 for layers 3 -> 4 -> 5 (measured slower)
  int dyn_tiles = 3;           // HN_DYN_TILES: the persistent kernels that claim their work tiles (hn_tiles.h;
                               // bits kTilesConv3 / kTilesConv5); HN_STATIC_TILES=1: none -- the static
                               // assignment rb + k nwg, bit-identical results (the A/B arm and the oracle)
  int train_splitk = 1024;     // HN_TRAIN_SPLITK: K per split-K slice of the train GEMMs
  int train_f32 = 17;          // HN_TRAIN_F32: bit 0 train forward convs, bit 1 stride-1 dgrads as f32-MFMA
                               // GEMMs (else the bf16x3 conv kernels); 1 = every product f32; default 17 =
                               // f32 forwards, the stride-1 dgrads on the bf16x3 conv kernels;
                               // bit 2: stride-1 weight gradients as the generic GEMM (else k_wgrad3);
                               // bit 3: stride-1 f32 forwards as the generic GEMM (else k_fwd3);
                               // bit 4: stride-1 dgrads not as k_fwd3 over dY (then bit 1 decides);
                               // bit 5: stride-2 layers as the generic GEMM + col2im (else k_fwd2 /
                               // k_wgrad2 / k_dgrad2); bit 6: conv0 as the generic GEMM (else
                               // k_fwd0 / k_wgrad0); bit 7: swaps the one-ring-per-wave and the
                               // shared-ring-per-patch forms (default shared: conv3 / conv5 k_fwd3s,
                               // conv4 k_dgrad2; per wave: conv2 / conv4 k_fwd2)
  int c12w_pd = 11;            // HN_C12W_PD: k_c12w's P2 / P3 B-fragment prefetch distances (tens / units)
  int c12_abl = 0;             // HN_C12_ABL (HN_EXPERIMENTS only)
  int head_abl = 0;            // HN_HEAD_ABL, HN_W4_ABL, HN_PAIRDIST_ABL (HN_EXPERIMENTS only): timing-only builds of
  int w4_abl = 0;              // k_head4, k_conv_w4 (HN_VARIANT digit w) and the pair-distance ring
  int pairdist_abl = 0;
  int dbg = 0;                 // HN_DEBUG (HN_EXPERIMENTS only)
};
void hn_read_knobs(HnKnobs* k);
const HnKnobs& hn_knobs();

// Dynamic tile claiming (hn_tiles.h).  A forward call of a HardNet model takes one block of the model's counter
// ring (hardnet_mi355x.h: HN_TILE_RING) and makes it current on the calling thread; each launch of a claiming kernel
// inside the call gets the block's next (ticket, checked-out) counter pair, kTileLaunches pairs per block in
// rotation -- launches that far apart are in stream order.  The counters are zero between launches (the kernels
// reset them), so no call adds a stream operation.  Null -- no model in scope, HN_STATIC_TILES, `kernel` not in
// HN_DYN_TILES, or the counters' allocation failed -- selects the static kernel.
constexpr int kTilesConv3 = 1, kTilesConv5 = 2;  // HN_DYN_TILES bits
constexpr int kTileLaunches = 32;
unsigned* hn_tile_counters(int kernel);

// Resident workgroups of `fn` on the current device at `nthreads` threads and `lds` bytes of
// dynamic LDS (also raises the function's dynamic-LDS limit to `lds` on that device).  Cached
// per (function, device) under a mutex.
hipError_t hn_resident_blocks(const void* fn, int nthreads, int lds, int* resident);

// Device-resident, BN-folded, packed HardNet parameters.
struct HardnetDev {
  float* stem_w = nullptr;   // [9][32]   conv0 folded
  float* stem_b = nullptr;   // [32]
  void* wpack[7] = {};       // conv1..5: bf16 hi/lo MFMA fragments; [6] = head
  float* bias[7] = {};       // folded BN bias per conv
  void* c12_w1 = nullptr;    // conv1 / conv2 as 16x16x32 A operands for the fused k_c12
  void* c12_w2 = nullptr;
  void* c12_w1w = nullptr;   // conv1 as 1-D Winograd F(4,3) U fragments for k_c12w
  void* wino[7] = {};        // conv3 / conv5: Winograd F(2x2,3x3) U fragments (hn_wino.hip)
  void* wino1[7] = {};       // conv3 / conv5: 1-D Winograd F(2,3) U fragments (hn_wino1.hip)
  void* wino4[7] = {};       // conv3: 1-D Winograd F(4,3) U fragments (hn_wino1.hip k_conv_w4)
};
// uint8 patches for the fused preprocessing load (hn_forward_u8)
struct HnU8In {
  const uint8_t* in;  // this chunk's patches
  int resize;         // enum hn_resize
  int normalize;
  float mean, stdv;
};
// fused input_norm + conv0 + conv1 + conv2 (hn_c12.hip): [P,1,32,32] -> a2 [P,16,16,64]; with
// u8 the patches are uint8 and preprocessed in the load (production configuration only)
hipError_t hn_launch_c12(const float* in, float* out, const HardnetDev& d, int P, float eps,
                         hipStream_t st, const HnU8In* u8 = nullptr);

hipError_t hn_launch_stem(const float* in, float* out, const float* w, const float* b, int P,
                          bool norm, float eps, hipStream_t st);
// One build of a HardNet conv layer's kernel: `layer` is the HN_VARIANT position (0 = stem + conv1 from the raw
// patches, 1 = conv1 alone, 2..5 = conv2..conv5), `variant` its digit (0-9, a-z = 10..35).  Each kernel file owns
// constexpr rows for the kernels it defines (hn_hardnet.hip, hn_wino1.hip; hn_wino.hip in the experiments
// library) and a static_assert that they are unique; a new kernel build is one more row.  hn_create resolves a
// model's six rows once: what it accepts is what the forward launches.
using HnConvLaunch = hipError_t (*)(const HardnetDev& d, const float* in, float* out, int P, float eps,
                                    hipStream_t st);
struct HnConvRow {
  int layer, variant;
  HnConvLaunch launch;
};
template <int N>
constexpr const HnConvRow* hn_find_row(const HnConvRow (&rows)[N], int layer, int variant) {
  for (const HnConvRow& r : rows)
    if (r.layer == layer && r.variant == variant) return &r;
  return nullptr;
}
template <int N>
constexpr bool hn_rows_unique(const HnConvRow (&rows)[N]) {
  for (int i = 0; i < N; ++i)
    if (hn_find_row(rows, rows[i].layer, rows[i].variant) != &rows[i]) return false;
  return true;
}
const HnConvRow* hn_hardnet_conv_row(int layer, int variant);  // across the files; null: no such build here
const HnConvRow* hn_wino1_conv_row(int layer, int variant);    // hn_wino1.hip's rows
const HnConvRow* hn_wino_conv_row(int layer, int variant);     // hn_wino.hip's (experiments library only)
bool hn_hardnet_variant_ok(int layer, int variant);  // hn_hardnet_conv_row found one

// A persistent kernel's launch: grid = min(tiles, resident workgroups) (occupancy query, cached), NTHR threads,
// SMEM bytes of dynamic LDS
template <auto Kernel, int NTHR, int SMEM, class... Args>
hipError_t hn_launch_persistent(int tiles, hipStream_t st, Args... args) {
  int resident = 0;
  const hipError_t e = hn_resident_blocks(reinterpret_cast<const void*>(Kernel), NTHR, SMEM, &resident);
  if (e != hipSuccess) return e;
  const int grid = std::min(tiles, resident);
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(NTHR), SMEM, st, args...);
  return hipGetLastError();
}

// The builds of the fused stem + conv1 + conv2 kernels, keyed by what selects them: HN_C12_CFG (0..13 k_c12 /
// k_c12h in hn_c12.hip; 14 = k_c12w, 15 = k_c12s in hn_c12w.hip), HN_C12_ABL and HN_C12W_PD (the last two are
// 0 / 11 in the product library).  hn_c12_cfg_ok and hn_launch_c12 both read the files' tables.
using HnC12Launch = hipError_t (*)(const float* in, float* out, const HardnetDev& d, int P, float eps,
                                   hipStream_t st, const HnU8In* u8);
constexpr int kAnyPd = -1;  // a row's pd: HN_C12W_PD selects nothing for this (cfg, abl)
struct HnC12Row {
  int cfg, abl, pd;
  HnC12Launch launch;
};
constexpr int kC12Wino = 14;   // k_c12w: conv1 as a 1-D Winograd F(4,3)
constexpr int kC12Split = 15;  // k_c12s: k_c12w's arithmetic with conv1 / conv2+stem waves per SIMD
template <int N>  // the first matching row: a (cfg, abl)'s exact-pd rows stand before its kAnyPd row
constexpr const HnC12Row* hn_find_row(const HnC12Row (&rows)[N], int cfg, int abl, int pd) {
  for (const HnC12Row& r : rows)
    if (r.cfg == cfg && r.abl == abl && (r.pd == pd || r.pd == kAnyPd)) return &r;
  return nullptr;
}
template <int N>
constexpr bool hn_rows_unique(const HnC12Row (&rows)[N]) {
  for (int i = 0; i < N; ++i)
    if (hn_find_row(rows, rows[i].cfg, rows[i].abl, rows[i].pd) != &rows[i]) return false;
  return true;
}
const HnC12Row* hn_c12_row(int cfg, int abl, int pd);   // across both files; null: no such build here
const HnC12Row* hn_c12w_row(int cfg, int abl, int pd);  // hn_c12w.hip's rows
bool hn_c12_cfg_ok(int cfg, int abl, int pd);            // hn_c12_row found one
// One launch of a fused kernel (the four share their argument list): w1 = conv1's weights in the kernel's layout,
// grid = min(P, resident workgroups of Base) -- Base is the configuration's fp32, ABL = 0 build
template <auto Kernel, auto Base, int NTHR>
hipError_t hn_c12_launch(const void* w1, const float* in, float* out, const HardnetDev& d, int P, float eps,
                         hipStream_t st, const HnU8In* u8) {
  int resident = 0;
  const hipError_t e = hn_resident_blocks(reinterpret_cast<const void*>(Base), NTHR, 0, &resident);
  if (e != hipSuccess) return e;
  const int grid = (int)std::min<long>((long)P, resident);
  const void* src = u8 ? u8->in : static_cast<const void*>(in);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(NTHR), 0, st, src, out, d.stem_w, d.stem_b, static_cast<const uint4*>(w1),
                     d.bias[1], static_cast<const uint4*>(d.c12_w2), d.bias[2], P, eps, u8 ? u8->mean : 0.f,
                     u8 ? u8->stdv : 1.f, u8 ? u8->normalize : 0);
  return hipGetLastError();
}
// The fp32 / uint8 choice of the fused kernels' U8 template argument: calls f(std::integral_constant<int, U8>)
// with U8 = -1 for fp32 input (u8 null), else the uint8 patches' enum hn_resize
template <class F>
hipError_t hn_with_u8(const HnU8In* u8, F&& f) {
  if (!u8) return f(std::integral_constant<int, -1>{});
  switch (u8->resize) {
    case HN_RESIZE_NONE: return f(std::integral_constant<int, HN_RESIZE_NONE>{});
    case HN_RESIZE_CV2_LINEAR: return f(std::integral_constant<int, HN_RESIZE_CV2_LINEAR>{});
    case HN_RESIZE_PIL_BILINEAR: return f(std::integral_constant<int, HN_RESIZE_PIL_BILINEAR>{});
  }
  return hipErrorInvalidValue;
}
// part: scratch for the split-K partials of small batches (P <= kHeadSplitMaxP: head_split(K) x P x 128
// floats), or null for the unsplit forms
constexpr int kHeadSplitMaxP = 16384;
constexpr int head_split(int K) { return K / 128; }  // 64 (HardNet, K = 8,192) / 16 (NAS, K = 2,048): 4 K-chunks each
hipError_t hn_launch_head(const float* a, float* out, const void* wp, const float* bias, int P,
                          int K, float l2eps, hipStream_t st, bool f16 = false, float* part = nullptr);
int hn_conv_lds_bytes(int layer);
// train mode: conv layer 1..5 as a plain NHWC convolution (no bias, no ReLU), bf16x3 fragments
// in the pack_conv3x3 layout
hipError_t hn_launch_conv_raw(int layer, const void* wp, const float* zero_bias, const float* in, float* out,
                              int P, hipStream_t st);
int hn_wino1_lds_bytes(int layer);

hipError_t hn_launch_pw(const float* in, float* out, const float* wt, const float* bias,
                        const float* res, long npix, int cin, int cout, int groups, bool relu,
                        int shuffle_g, hipStream_t st);
hipError_t hn_launch_dw(const float* in, float* out, const float* wd, const float* bias, int P,
                        int hin, int c, int k, int s, hipStream_t st);
hipError_t hn_launch_maxpool(const float* in, float* out, int P, int hin, int c, hipStream_t st);
// fused MaxPool2d(3, 2, 1) + ConvBNRelu 1x1 of the channel-changing "skip" op (hn_nas.hip)
bool hn_skip_s2_supported(int hin, int cin, int cout);
hipError_t hn_launch_skip_s2(const float* in, float* out, const float* wt, const float* bias, int P, int hin,
                             int cin, int cout, hipStream_t st);
hipError_t hn_launch_se(float* y, const float* w1, const float* b1, const float* w2,
                        const float* b2, int P, int hw, int c, int mid, hipStream_t st);
hipError_t hn_launch_nas_head(const float* a, float* out, const float* wt, const float* bias,
                              int P, int K, float l2eps, hipStream_t st);

hipError_t hn_launch_pairdist(const float* a, const float* p, int B, int D, int swap,
                              float* pos, float* minneg, void* ws, hipStream_t st);
// rows [row0, row0 + NA) of the B x B matrix (a = those NA anchors, p = all B positives);
// colmin (float bits, atomicMin; may be NULL) gets the column minima over these rows
size_t hn_pairdist_rows_ws_bytes(long NA, long B);
hipError_t hn_launch_pairdist_rows(const float* a, int NA, int row0, const float* p, int B, float* pos,
                                   float* rowmin, float* colmin, void* ws, hipStream_t st);
hipError_t hn_launch_split_planes(const float* p, int B, uint16_t* ph, uint16_t* pl, hipStream_t st);
// nearest / second-nearest database row of every query (hn_match.hip): idx [N,2] (-1: no such row), dist [N,2]
size_t hn_match_ws_bytes(long N, long M);
hipError_t hn_launch_match_nn2(const float* q, int N, const float* db, int M, int metric, float* dist, int* idx,
                               void* ws, hipStream_t st);
// rotated, scaled 32x32 windows around keypoints (b, y, x, .) of images [B,1,H,W] (hn_clip.hip): out [n,1,32,32];
// ori null: no rotation.  Reads nothing outside images whatever the keypoint data (B >= 1, H, W >= 2)
hipError_t hn_launch_clip(const float* images, int64_t B, int H, int W, const int64_t* kpts, const float* scale,
                          const float* ori, const float* ratio, int64_t n, float* out, hipStream_t st);
// its backward to the keypoints: dscale [n] and dori [n,2] (either may be null) from dout [n,1,32,32]; same reads
hipError_t hn_launch_clip_backward(const float* dout, const float* images, int64_t B, int H, int W,
                                   const int64_t* kpts, const float* scale, const float* ori, const float* ratio,
                                   int64_t n, float* dscale, float* dori, hipStream_t st);
// FDLNet's NASNet detector (hn_det.hip): layout of the BN-folded device parameters (floats) and the launch
namespace hndet {
constexpr int kDetTile = 16;      // k_det_feat's output tile (one partial-statistics slot per tile)
constexpr int kDetPostTile = 32;  // k_det_post's
constexpr int kC0W = 0;           // features.0.weight [16][9]
constexpr int kC0B = 144;         // features.0.bias [16]
constexpr int kBlk = 160;         // two InvertedResidual blocks of kBlkSize floats, BN folded:
constexpr int kBlkPw1W = 0;       //   1x1 [8 out][8 in]
constexpr int kBlkPw1B = 64;
constexpr int kBlkDwW = 72;       //   depthwise [8][9]
constexpr int kBlkDwB = 144;
constexpr int kBlkPw2W = 152;     //   1x1 [8 out][8 in]
constexpr int kBlkPw2B = 216;
constexpr int kBlkSize = 224;
constexpr int kHeadW = kBlk + 2 * kBlkSize;  // conv.weight, conv_ori.weight: [3][16][9] (score, cos, sin)
constexpr int kHeadB = kHeadW + 432;         // [3]
constexpr int kInG = kHeadB + 3;             // insnorm.weight, insnorm_ori.weight [3]
constexpr int kInB = kInG + 3;               // insnorm.bias, insnorm_ori.bias [3]
constexpr int kFolded = kInB + 3;
constexpr int kStateFloats = 160 + 2 * (64 + 32 + 72 + 32 + 64 + 32) + 145 + 2 + 290 + 4;  // RFDet.state_dict()
}  // namespace hndet
int64_t hn_det_parts(int H, int W);  // partial-statistics slots (k_det_feat workgroups) per image
size_t hn_det_ws_bytes(int64_t B, int H, int W);
hipError_t hn_launch_det(const float* params, float in_eps, const float* images, int64_t B, int H, int W, float* score,
                         float* ori, void* ws, hipStream_t st);
// RF-Net's ten-scale detector (hn_rfdet.hip; the parameter layout and the workspace plan are hn_rfdet.h's)
int64_t hn_rfdet_parts(int H, int W);  // layer-kernel workgroups per image
size_t hn_rfdet_ws_bytes(int64_t B, int H, int W);
hipError_t hn_launch_rfdet(const float* params, float in_eps, float score_com_strength, float scale_com_strength,
                           const float* images, int64_t B, int H, int W, float* score, float* scale, float* ori,
                           void* ws, hipStream_t st);
// the detector in train() (hn_det_train.hip): T / G are host arrays of 40 device pointers, RFDet.state_dict() order
void hn_det_train_plan(int64_t n, int H, int W, size_t* saved, size_t* scratch);
bool hn_det_train_is_param(int slot);  // false for the running statistics' slots
hipError_t hn_det_train_forward_impl(const float* images, int64_t n, int H, int W, float* const* T, float bn_eps,
                                     float in_eps, float momentum, float* score, float* ori, char* saved,
                                     char* scratch, hipStream_t st);
hipError_t hn_det_train_backward_impl(const float* dscore, const float* dori, const float* images, int64_t n, int H,
                                      int W, float* const* T, float* const* G, char* saved, char* scratch,
                                      hipStream_t st);
// keypoint selection (hn_select.hip); taps: the gauss_ksize^2 blur weights, row-major (host memory)
struct HnSelectArgs {
  const float* score;
  int64_t B;
  int H, W, border;
  float nms_thresh;
  int nms_ksize, topk, gauss_ksize;
  const float* taps;
  const float* scale_map;
  float scale_value;
  const float* ori_map;
  int64_t* kpts;
  float *kscore, *kscale, *kori, *score_proc;
  uint8_t* topk_mask;
  void* ws;
};
size_t hn_select_ws_bytes(int64_t B, int H, int W);
hipError_t hn_launch_select(const HnSelectArgs& a, hipStream_t st);
// homography ground-truth stage (hn_gt.hip): warp + visibility, gt_scale_orin, mask -> keypoints, ptCltoCr
hipError_t hn_launch_warp_score(const float* score, const float* homo, int64_t B, int H, int W, int border,
                                int align_corners, float* warped, float* visible, hipStream_t st);
hipError_t hn_launch_gt_scale_orin(const float* scale, float scale_value, const float* ori, const float* homo12,
                                   const float* homo21, int64_t B, int H, int W, float* gt_scale, float* gt_ori,
                                   hipStream_t st);
hipError_t hn_launch_mask_keypoints(const uint8_t* mask, int64_t B, int H, int W, int K, const float* scale_map,
                                    float scale_value, const float* ori_map, int64_t* kpts, float* kscale, float* kori,
                                    int32_t* counts, hipStream_t st);
hipError_t hn_launch_project_kpts(const int64_t* kpts, int64_t n, const float* homo, int64_t B, int H, int W,
                                  const float* scale_map, float scale_value, const float* ori_map, int clamp,
                                  int64_t* kpts_r, float* scale_r, float* ori_r, hipStream_t st);
hipError_t hn_launch_loss(const float* pos, const float* rmin, const float* cmin, int n, float margin,
                          int type, float scale, float* min_neg, float* loss, hipStream_t st);

hipError_t hn_fpr95_ws_bytes(int64_t n, size_t* bytes);
// fused NAS front (stem + layer 0), hn_front.hip
struct HnFrontArgs {
  const float* in;
  float* out;
  const uint4* spack;   // stem A operand, [plane 2][lane 64] x 8 fp16 (taps 8h..8h+7)
  const float* stem_b;
  const uint4* apack;   // pw A operand, [MID/32][kstep 2][plane 2][lane 64] x 8 fp16
  const float* pw_b;    // [MID], dw channel order
  const float* dw_w;    // [K*K][MID]
  const float* dw_b;
  const uint4* pwl_a;   // pwl A operand, [1][MID/16][plane 2][lane 64] x 8 fp16
  const float* pwl_b;   // [32]
  const uint4* pwl_a16; // pwl A operand for 16x16x32: [MID/32][out tile 2][plane 2][lane 64] x 8 fp16
};
bool hn_front_supported(int k, int mid);
// u8: uint8 patches preprocessed in the front's patch load (the production forms without
// input_norm, HN_FRONT_FOLD off; hn_api.hip u8_fused)
hipError_t hn_launch_front(const HnFrontArgs& a, int P, int k, int mid, bool maxpool, bool norm,
                           float eps, hipStream_t st, const HnU8In* u8 = nullptr);
// FDLNet HardNetNeiMask front (32x32 patch -> 8x8x64), hn_fdl.hip; mode 0 = NASNet, 1 = NASNet_0.1
struct HnFdlFrontArgs {
  const float* in;
  float* out;
  const float *stem_w, *stem_b;  // [9][32], [32]
  const float *w1, *b1;          // [32][32], [32] (mode 0)
  const float *w2, *b2;          // [32][64], [64]
};
// u8: uint8 patches preprocessed in the patch load (hn_forward_u8), else a.in (fp32)
hipError_t hn_launch_fdl_front(const HnFdlFrontArgs& a, int P, int mode, float eps, hipStream_t st,
                               const HnU8In* u8 = nullptr);
// fused IRF block (pw -> dw -> pwl [+ residual]) for layers 1..5, hn_irf.hip
struct HnIrfArgs {
  const float* x;
  float* y;
  const uint4* pw_a;   // [MID/32][CIN/16][plane 2][lane 64] x 8 fp16, rows in dw order
  const float* pw_b;   // [MID] dw order
  const float* dw_w;   // [K*K][MID]
  const float* dw_b;
  const uint4* pwl_a;  // [COUT/32][MID/16][plane 2][lane 64] x 8 fp16
  const float* pwl_b;  // [COUT]
};
bool hn_irf_supported(int cin, int cout, int hin, int s, int k, int mid);
// two consecutive blocks in one kernel (hn_irf.hip k_irf2): A (ca -> ca, stride 1) then B (ca -> cb, stride 2)
bool hn_irf2_supported(int ca, int hi, int ka, int ma, int cb, int kb, int mb);
hipError_t hn_launch_irf2(const HnIrfArgs& a, const HnIrfArgs& b, int P, int ca, int hi, int ka, int ma, int cb,
                          int kb, int mb, hipStream_t st);
hipError_t hn_launch_irf(const HnIrfArgs& a, int P, int cin, int cout, int hin, int s, int k, int mid,
                         hipStream_t st);
// a 16x16 stride-2 32 -> 64 block and the 8x8 64 -> 128 stride-2 skip that follows it (after identity
// skips) in one kernel (hn_irf.hip k_irf_skip); a.y receives the skip's [P,4,4,128] output
bool hn_irf_skip_supported(int cin, int cout, int hin, int s, int k, int mid);
// k_irf2's 8x8 pair (64 -> 64 s1, 64 -> 128 s2, mid 64) and the 4x4 128 -> 128 e1 block in one kernel (k_irf3,
// experiments library only)
bool hn_irf3_supported(int ka, int ma, int kb, int mb, int kc, int mc);
hipError_t hn_launch_irf3(const HnIrfArgs& a, const HnIrfArgs& b, const HnIrfArgs& c, int P, int ka, int kb, int kc,
                          hipStream_t st);
// the max-pool front + the first (16x16 stride-2 32 -> 64) IRF block in one kernel (hn_irf.hip k_mpfront_irf)
bool hn_mpfront_irf_supported(int cin, int cout, int hin, int s, int k, int mid);
hipError_t hn_launch_mpfront_irf(const float* in, const uint4* spack, const float* stem_b, const HnIrfArgs& a, int P,
                                 int k, int mid, bool norm, float eps, hipStream_t st);
hipError_t hn_launch_irf_skip(const HnIrfArgs& a, const uint4* skip_a, const float* skip_b, int P, int k, int mid,
                              hipStream_t st);
hipError_t hn_launch_preprocess(const uint8_t* in, int64_t n, int resize, int norm, float mean,
                                float stdv, float* out, hipStream_t st);
hipError_t hn_launch_fpr95(const float* a, const float* p, const int* labels, int64_t n, int dim,
                           float* dists, double* fpr, void* ws, size_t ws_bytes, hipStream_t st);

// train-mode stock HardNet (hn_train.hip): conv shapes and workspace layout
struct HnTrainLayer {
  int cin, cout, hin, ks, s, pad;
};
extern const HnTrainLayer kHardnetTrainLayers[7];
// CANDIDATE_BLOCKS (lookup_table_builder.py:18-20) as (skip, expansion, kernel, pw groups, SE);
// the ChannelShuffle runs iff groups > 1 (fbnet_builder.py:36-191); defined in hn_api.hip
struct HnOpSpec {
  const char* name;
  int skip, e, k, g, se;
};
extern const HnOpSpec kHnOps[17];

struct HnTrainWs {  // byte offsets into the train workspace's saved region (xn .. rstd) / scratch region
  size_t xn, inv_sd, z[7], rstd[7], saved_total;
  size_t g0, g1, col, part, bnpart, bnmean, wt, nhwc0, nhwc1, wpack, zero, scratch_total;
};
HnTrainWs hn_train_layout(long B, int tf = -1, int ns = 0);  // tf < 0: the process's HN_TRAIN_F32 bits
// one layer operation of the step on caller-owned buffers (hn_hardnet_train_layer_op): the form of a convolution
// operation under the HN_TRAIN_F32 bits `tf` (-1: not a convolution operation), and the call itself
enum HnConvForm {
  kHnFormDirect0,     // conv0: k_fwd0 / k_wgrad0
  kHnFormBf16x3,      // the inference bf16x3 conv kernels over NHWC
  kHnFormRing,        // one LDS ring per wave: k_fwd3 / k_fwd2 / k_dgrad2 / k_wgrad3 / k_wgrad2 (row segments)
  kHnFormRingShared,  // one LDS ring per patch: k_fwd3s / k_fwd2 / k_dgrad2 with NWP > 1 (row segments)
  kHnFormGemm,        // the generic implicit GEMM
  kHnFormCol          // the column GEMM + col2im / conv6's transpose (patch chunks)
};
int hn_train_conv_form(int op, int layer, int tf);
struct HnTrainOpArgs {
  int op, layer, tf, ns;
  long chunk, B;
  const float* x;
  const float* w;
  float* y;
  float *aux0, *aux1, *aux2;
  float mom, drop_p, bn_eps, in_eps, l2_eps;
  unsigned long long seed;
};
hipError_t hn_train_layer_op(const HnTrainOpArgs& o, char* scratch, hipStream_t st);
// train-mode hardnetNAS (hn_nas_train.hip): tensors consumed, saved / scratch workspace bytes
int hn_nas_train_plan(const hn_arch_desc& d, long B, size_t* n_tensors, size_t* saved, size_t* scratch);
int hn_nas_train_null_grad_slot(const hn_arch_desc& d, float* const* grads);
hipError_t hn_nas_train_forward_impl(const hn_arch_desc& d, const float* in, long B, float* const* tensors,
                                     float momentum, const float* soft, float* out, char* saved, char* scratch,
                                     hipStream_t st);
hipError_t hn_nas_train_backward_impl(const hn_arch_desc& d, const float* dout, long B, const float* in,
                                      float* const* tensors, const float* soft, float* const* grads, float* dsoft,
                                      float* din, char* saved, char* scratch, hipStream_t st);
hipError_t hn_train_forward(const float* in, long B, const float* const* W, float* const* rmean, float* const* rvar,
                            float mom, float bn_eps, float in_eps, float l2_eps, float drop_p,
                            unsigned long long seed, float* out, char* saved, char* scratch, hipStream_t st);
hipError_t hn_train_backward(const float* dout, long B, const float* const* W, float* const* dW, float* din,
                             float l2_eps, float drop_p, unsigned long long seed, char* saved, char* scratch,
                             hipStream_t st);

// train-mode loss_HardNet 'min' reduce and its backward (hn_loss.hip)
size_t hn_loss_train_saved_bytes(long B);
hipError_t hn_launch_loss_train_fwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    float* loss, void* saved, hipStream_t st);
hipError_t hn_launch_loss_train_bwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    const float* dloss, float* ga, float* gp, void* saved, hipStream_t st);

// batch_reduce 'random' (hn_loss.hip): tidx [B] int64, each value clamped to [0, B-1] on load; the saved layout and
// the backward are 'min''s (hn_loss_train_saved_bytes, hn_launch_loss_train_bwd)
hipError_t hn_launch_loss_random_fwd(const float* a, const float* p, const long long* tidx, int B, int swap,
                                     float margin, int type, float* loss, void* saved, hipStream_t st);

// batch_reduce 'average' and its backward on the f32-input MFMA (hn_loss_dense.hip)
size_t hn_loss_dense_saved_bytes(long B);
hipError_t hn_launch_loss_dense_fwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    float* loss, void* saved, hipStream_t st);
hipError_t hn_launch_loss_dense_bwd(const float* a, const float* p, int B, int swap, float margin, int type,
                                    const float* dloss, float* ga, float* gp, void* saved, hipStream_t st);

// FDLNet's neighbour-mask loss and its backward (hn_neimask.hip); akp / pkp: [B,4] int64 rows (b, y, x, 0)
size_t hn_neimask_saved_bytes(long B);
hipError_t hn_launch_neimask_fwd(const float* a, const float* p, const long long* akp, const long long* pkp, int B,
                                 float margin, float coo_thresh, float* loss, float* pos_out, float* mn_out,
                                 void* saved, hipStream_t st);
hipError_t hn_launch_neimask_bwd(const float* a, const float* p, int B, float margin, const float* dloss, float* ga,
                                 float* gp, void* saved, hipStream_t st);
