/* RF-Net's ten-scale keypoint detector (RFDetSO) on the MI355X: an extension of the C ABI of hardnet_mi355x.h
 * (which includes this file; include either).  Same conventions: device pointers, int status (HN_OK or an
 * HN_ERR_* code, the message through hn_last_error), every argument check before the GPU is touched. */
#ifndef HARDNET_MI355X_RFDET_H
#define HARDNET_MI355X_RFDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Eval-mode RFDetSO.forward (FDLNet-master/latency/rfnet/model/rf_det_so.py) with ksize 3, padding 1, dilation 1:
 * ten receptive-field levels 3 .. 21 (3x3 conv, affine InstanceNorm, leaky ReLU, residual), a 1x1 score head and a
 * 1x1 orientation head per level read before the residual is added, soft_nms_3d(15, 3.0) over (y, x, level) and the
 * three-output soft_max_and_argmax_1d.  An addition to the ABI of hardnet_mi355x.h: HN_ABI_VERSION stays 2.
 *   hn_rfdet_create: host_params holds the float tensors of RFDetSO.state_dict() in its own order, 100 tensors and
 *       21,890 floats (hn_rfdet_param_count): per level conv_k.{weight,bias}, insnorm_k.{weight,bias},
 *       conv_s*.{weight,bias}, insnorm_s*.{weight,bias}; then conv_o3 .. conv_o21 .{weight,bias}.  scale_list: 10
 *       host floats, one per level.  in_eps (> 0) is every InstanceNorm's eps; the two strengths are
 *       soft_max_and_argmax_1d's com_strength1 (score and orientation) and com_strength2 (scale).  Every value
 *       must be finite.
 *   hn_rfdet_forward: d_images fp32 [n_images,1,height,width] -> d_score [n,H,W], d_scale [n,H,W] and d_ori
 *       [n,H,W,2] (cos, sin; divided by its norm with no epsilon, as the reference).  d_ori 8-byte and d_workspace
 *       16-byte aligned; d_workspace of hn_rfdet_workspace_bytes(n_images, height, width) bytes is transient: no
 *       byte of it is read before the same call writes it, and a short one is HN_ERR_WORKSPACE.  The InstanceNorm
 *       statistics are per-workgroup fp64 partial sums combined in fp64 in a fixed order that depends on the image
 *       alone; there are no float atomics: an image's three maps are bit-identical call to call, alone or inside any
 *       batch.  The 16 -> 16 convolutions run on the f32-input MFMA, which is an fmaf chain: fp32 arithmetic
 *       throughout, IEEE divisions and square roots.  Caller's stream, no allocation or synchronisation inside:
 *       capturable in a graph.
 * Every argument check runs before the GPU is touched: n_images >= 0 (0 returns HN_OK), height, width >= 1 with
 * height * width in 2 .. 2^31 - 1, n_images * tiles below 2^31 (16 x 16 tiles); else HN_ERR_ARG. */
typedef struct hn_rfdet hn_rfdet;
int hn_rfdet_param_count(size_t* n_out);
int hn_rfdet_create(const float* host_params, size_t n_params, const float* scale_list, float in_eps,
                    float score_com_strength, float scale_com_strength, hn_rfdet** out);
int hn_rfdet_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* bytes_out);
int hn_rfdet_forward(hn_rfdet* d, const float* d_images, int64_t n_images, int32_t height, int32_t width,
                     float* d_score, float* d_scale, float* d_ori, void* d_workspace, size_t workspace_bytes,
                     void* hip_stream);
void hn_rfdet_destroy(hn_rfdet* d);

#ifdef __cplusplus
}
#endif

#endif /* HARDNET_MI355X_RFDET_H */
