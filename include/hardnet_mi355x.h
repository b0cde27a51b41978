/*
 * hardnet_mi355x.h -- C ABI of the MI355X-native HardNet / hardnetNAS descriptor forward.
 *
 * This is the drop-in boundary for the reference hot path
 *   hardnet/HardNet.py:312-315          HardNet.forward(input [B,1,32,32]) -> [B,128]
 *   hardnet/HardNet.py:306-310          HardNet.input_norm (fused into hn_forward)
 *   hardnet/Utils.py:15-22              L2Norm (fused into hn_forward)
 *   hardnetNAS/supernet_functions/model_supernet.py:70-85
 *                                       sampled-supernet forward (argmax op per layer)
 *   hardnet/Losses.py:5-13,87-154       distance_matrix_vector + loss_HardNet 'min' reduce
 *                                       (hn_pairdist_hardneg)
 * The reference is pure PyTorch and has no FFI of its own; the Python host package
 * (hardnetnas_amd/_native.py) binds these entry points with ctypes -- see
 * INTEGRATION.md for the binding a maintainer adds to the reference.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Device pointers are HIP device memory owned by the
 *    caller; nothing is copied host<->device inside hn_forward.
 *  - Every call is ordered on the caller's HIP stream (hipStream_t passed as void*;
 *    NULL = the legacy default stream).  No allocation or synchronisation happens inside
 *    hn_forward / hn_pairdist_hardneg, so they can be captured in a hipGraph.
 *  - Return value 0 = success; nonzero = error, message in hn_last_error() (thread-local).
 *    The library never exits the process.
 */
#ifndef HARDNET_MI355X_H
#define HARDNET_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HN_ABI_VERSION 2

enum hn_status {
  HN_OK = 0,
  HN_ERR_ARG = 1,      /* invalid argument / shape / size mismatch */
  HN_ERR_HIP = 2,      /* HIP runtime error (message has the HIP error string) */
  HN_ERR_NOMEM = 3,    /* device allocation failed */
  HN_ERR_WORKSPACE = 4 /* workspace too small for the requested batch */
};

enum hn_kind {
  HN_KIND_HARDNET = 0,      /* stock HardNet, hardnet/HardNet.py:275-304 */
  HN_KIND_NAS = 1,          /* sampled hardnetNAS net, model_supernet.py:53-85 */
  HN_KIND_FDL_NASNET = 2,   /* FDLNet HardNetNeiMask, FDLNet-master/latency/NASNet/model/des.py:8-55 */
  HN_KIND_FDL_NASNET01 = 3, /* FDLNet HardNetNeiMask, FDLNet-master/latency/NASNet_0.1/model/des.py:10-55 */
  HN_KIND_NAS_SUPERNET = 4  /* train mode only: FBNet_Stochastic_SuperNet, model_supernet.py:53-85 (every layer
                               a MixedOperation over all 17 CANDIDATE_BLOCKS, :10-36) */
};

#define HN_MAX_LAYERS 8

/* Architecture description.
 *  HardNet: only kind, input_norm_eps, l2_eps, bn_eps are read.
 *  NAS:     op[i] = index into CANDIDATE_BLOCKS (lookup_table_builder.py:18-20);
 *           c_in/c_out/stride from SEARCH_SPACE2 (lookup_table_builder.py:22-45).
 *  FDL:     a fixed front (des.py) to 8x8x64, then op/c_in/c_out/stride of its IRFBlocks in the
 *           same CANDIDATE_BLOCKS vocabulary (NASNet: ir_k5_e1 64->64, ir_k3_e3 64->128 s2,
 *           ir_k5_s2 128->128), then the 4x4 head; input_norm_eps 1e-8, l2_eps 0.
 *  input_norm_eps < 0 disables input_norm (the NAS nets have none);
 *  l2_eps: HardNet 1e-10 inside the sqrt (Utils.py:18); NAS 0 (torch.norm, model_supernet.py:84). */
typedef struct hn_arch_desc {
  int32_t kind;
  int32_t n_layers;
  int32_t op[HN_MAX_LAYERS];
  int32_t c_in[HN_MAX_LAYERS];
  int32_t c_out[HN_MAX_LAYERS];
  int32_t stride[HN_MAX_LAYERS];
  float input_norm_eps;
  float l2_eps;
  float bn_eps;
} hn_arch_desc;

typedef struct hn_model hn_model;

/* Number of floats hn_create expects in host_params for this architecture. */
int hn_param_count(const hn_arch_desc* desc, size_t* n_out);

/* Build a device model on the current HIP device from host fp32 parameters.
 * host_params is the concatenation, in state_dict order, of every conv weight and
 * BatchNorm tensor of the module (HardNet: for each of the 7 convs
 *   features.{c}.weight, features.{b}.running_mean, features.{b}.running_var;
 * NAS / FDL: see hardnetnas_amd/_native.py::state_dict_blob, which documents the order).
 * BatchNorm (eval) is folded into the conv weights/bias here, once. */
int hn_create(const hn_arch_desc* desc, const float* host_params, size_t n_params,
              hn_model** out);

/* Bytes of device workspace hn_forward needs for a batch of B patches.  The forward walks the batch in
 * chunks of min(B, 65,536) patches and sizes the workspace for one chunk; for the stock HardNet at the
 * defaults that is 160 KiB per patch: 10 GiB from 65,536 patches up, 80 MiB at the reference eval loop's
 * 512.  Two environment knobs, read by hn_create, bound it for the stock HardNet (both default 65,536; any
 * values give bit-identical descriptors): HN_C12_GROUP (patches per fused stem+conv1+conv2 launch) and
 * HN_SUBCHUNK (patches per conv3..conv5 launch); the footprint is max(HN_SUBCHUNK x 64 KiB, min(chunk,
 * 16,384) x 32 KiB) + HN_C12_GROUP x 64 KiB + chunk x 32 KiB, e.g. 4 GiB per 65,536-patch chunk at 16,384 /
 * 16,384 (about 4 % slower end to end).  (The first term's second operand is the scratch of the head's
 * split-K form, which every chunk of up to 16,384 patches runs whatever the knobs; it exceeds the first
 * only for an HN_SUBCHUNK below half such a chunk.)
 * HN_PIPELINE=1 (opt-in) overlaps a multi-chunk HardNet batch's chunks over a second, internally created
 * stream (forked from and joined back into hip_stream, so graph capture holds) and adds one more
 * chunk x 64 KiB buffer for batches of more than one chunk.
 * NAS / FDL descriptors need four buffers of their largest per-patch activation.
 *
 * Work-tile counters (stock HardNet).  The persistent conv3 / conv5 kernels claim their work tiles from
 * counters in a small allocation the model owns (made and zeroed by hn_create, freed by hn_destroy; no part
 * of the workspace, and no stream operation per call: the kernels leave the counters at zero).  Each forward
 * call takes the next of HN_TILE_RING counter blocks in rotation, so what the ring bounds is: at most
 * HN_TILE_RING forward calls of ONE model may be in flight on DIFFERENT streams at a time -- calls on one
 * stream run in order and may share a block, however many are queued.  A call made while its stream is being
 * captured takes one of HN_TILE_CAPTURES further blocks for good (a graph may be replayed at any later time,
 * beside eager calls); the model's captures past that number, and every call if the allocation failed, use
 * the static tile assignment.  HN_STATIC_TILES=1 (read by hn_create) selects the static assignment
 * everywhere: the same descriptors, bit for bit. */
#define HN_TILE_RING 64
#define HN_TILE_CAPTURES 64
int hn_workspace_bytes(const hn_model* m, int64_t batch, size_t* bytes_out);

/* d_in: [B,1,32,32] fp32 contiguous (device); d_out: [B,128] fp32 (device).
 * Eval-mode forward of the whole descriptor network (HardNet: input_norm, 7 conv+BN
 * stages, ReLU, L2Norm; NAS: stem, 6 searched blocks, 4x4 head, BN, L2).
 * Non-finite input: the descriptor of a patch that holds a NaN or an Inf is unspecified (the reference
 * returns NaN for it; the kernels are built without NaN semantics and may return anything, finite or not).
 * Such a patch never changes the descriptor of another patch of the batch, and nothing it leaves in the
 * workspace changes a later call: the forward reads no workspace byte it has not written in the same call,
 * and writes none outside hn_workspace_bytes nor any output row but its B. */
int hn_forward(hn_model* m, const float* d_in, int64_t batch, float* d_out,
               void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Fused distance_matrix_vector + hardest-in-batch negative (loss_HardNet 'min' reduce,
 * hardnet/Losses.py:87-154) without materialising the B x B matrix.
 * d_anchor, d_positive: [B,D] fp32.  Outputs (device, [B] fp32 each):
 *   d_pos[i]     = dist(a_i, p_i) + 1e-8              (pos1)
 *   d_min_neg[i] = min_j masked dist(a_i, p_j)        (row min, or min(row,col) if anchor_swap)
 * d_workspace needs hn_pairdist_workspace_bytes(B). */
int hn_pairdist_workspace_bytes(int64_t batch, size_t* bytes_out);
int hn_pairdist_hardneg(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim,
                        int32_t anchor_swap, float* d_pos, float* d_min_neg,
                        void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Row block of the same computation, for a batch sharded over ranks: rows
 * [row0, row0 + n_rows) of the batch x batch distance matrix between this rank's anchors
 * d_anchor_rows [n_rows, dim] and ALL positives d_positive [batch, dim] (all-gathered).
 * Outputs for the local rows: d_pos[i] = dist(a_i, p_{row0+i}) + 1e-8, d_row_min[i] = masked
 * row minimum; if d_col_min is not NULL it receives, for every column j of the batch, the
 * masked minimum over these rows (reduce it across ranks with an all-reduce(MIN), then
 * min_neg = min(row_min, col_min[row0 + i]) for anchor_swap; hn_hardnet_loss does that).
 * The single-GPU hn_pairdist_hardneg is this call with row0 = 0, n_rows = batch. */
int hn_pairdist_rows_workspace_bytes(int64_t n_rows, int64_t batch, size_t* bytes_out);
int hn_pairdist_rows(const float* d_anchor_rows, int64_t n_rows, int64_t row0, const float* d_positive,
                     int64_t batch, int32_t dim, float* d_pos, float* d_row_min, float* d_col_min,
                     void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* loss_HardNet's margin loss over the 'min' reduce (hardnet/Losses.py:142-153) for n rows:
 * min_neg = d_col_min ? min(d_row_min, d_col_min) : d_row_min (written to d_min_neg if not
 * NULL); *d_loss = scale * sum_i loss_i (scale = 1/B for torch.mean; with a sharded batch
 * every rank passes 1/B_total and the partial sums are all-reduced).  One workgroup, fixed
 * summation order (deterministic). */
enum hn_loss_type { HN_LOSS_TRIPLET_MARGIN = 0, HN_LOSS_SOFTMAX = 1, HN_LOSS_CONTRASTIVE = 2 };
int hn_hardnet_loss(const float* d_pos, const float* d_row_min, const float* d_col_min, int64_t n,
                    float margin, int32_t loss_type, float scale, float* d_min_neg, float* d_loss,
                    void* hip_stream);

/* Train-mode loss_HardNet, batch_reduce 'min' (hardnet/Losses.py:87-154 as the training loop calls
 * it, HardNet.py:408-413) and its backward (HardNet.py:421-423), without a B x B matrix.
 *   forward : *d_loss = mean_i loss(pos_i, min_neg_i) over d_anchor / d_positive [B,128] fp32
 *             (exact fp32 dot products; the hardest negatives and their argmins -- the first index
 *             on a tie -- are kept in d_saved);
 *   backward: d_dloss (one float on the device: d L / d loss) -> d_grad_anchor, d_grad_positive
 *             [B,128] (overwritten), as autograd differentiates the reference formulation: the
 *             gradient reaches each row's positive entry and its selected negative (the row
 *             minimum's argmin, the column minimum's for anchor_swap; halves on a row / column
 *             tie, as torch.minimum's backward).  Deterministic: no atomics in the backward.
 * d_saved (hn_hardnet_loss_train_workspace_bytes) is written by the forward and read by the
 * backward with the same anchors, positives and arguments; 1 <= batch <= 2^22. */
int hn_hardnet_loss_train_workspace_bytes(int64_t batch, size_t* bytes_out);
int hn_hardnet_loss_train_forward(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim,
                                  int32_t anchor_swap, float margin, int32_t loss_type, float* d_loss,
                                  void* d_saved, size_t saved_bytes, void* hip_stream);
int hn_hardnet_loss_backward(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim,
                             int32_t anchor_swap, float margin, int32_t loss_type, const float* d_dloss,
                             float* d_grad_anchor, float* d_grad_positive, void* d_saved, size_t saved_bytes,
                             void* hip_stream);

/* Train-mode loss_HardNet's other two reductions, 'average' and 'random' (hn_hardnet_loss_reduce_*): declared in
 * hardnet_mi355x_loss_reduce.h, which this header includes at its end. */

/* FDLNet's neighbour-mask descriptor loss (FDLNet-master/latency/NASNet/model/des.py:57-96, the hard loss of
 * model/network.py:307-309) and its backward, without an N x N matrix:
 *   D_ij  = sqrt(min(max(2 - 2 a_i.p_j, 1e-8), 4))  (exact fp32 dot products; rows need not be unit vectors)
 *   dn_ij = ((D_ij + 10 [i = j]) + 10 [kd(anchor_kp_i, anchor_kp_j) < C]) + 10 [kd(positive_kp_i, positive_kp_j) < C]
 *   loss  = mean_i max(margin + D_ii - min(min_j dn_ij, min_k dn_ki), 0)
 * kd = sqrt(max(squared distance of the (y, x) columns, 1e-8)); d_anchor_kp / d_positive_kp: [batch,4] int64
 * rows (b, y, x, 0), b not used (as in the reference).  The squared distance is taken from the integer
 * differences: the reference's value for coordinates below 2,048; coordinates saturate at +-(2^30 - 1).  Any
 * keypoint value is safe: keypoints never index memory.
 *   forward : *d_loss; d_pos / d_min_neg ([batch], each may be NULL) receive D_ii and the selected minimum;
 *             the minima and their argmins (the lowest index on a tie) are kept in d_saved;
 *   backward: d_dloss (one float on the device) -> d_grad_anchor, d_grad_positive [batch,128] (overwritten),
 *             as autograd differentiates the reference formulation: one argmin per minimum, halves on an exact
 *             row / column tie, nothing through an active clamp.  Deterministic, bit-identical run to run.
 * d_saved (hn_neimask_loss_workspace_bytes) is written by the forward and read by the backward with the same
 * descriptors and margin; 1 <= batch <= 2^22; dim must be 128.  Non-finite descriptors give an unspecified
 * loss and no out-of-bounds access. */
int hn_neimask_loss_workspace_bytes(int64_t batch, size_t* bytes_out);
int hn_neimask_loss_forward(const float* d_anchor, const float* d_positive, const int64_t* d_anchor_kp,
                            const int64_t* d_positive_kp, int64_t batch, int32_t dim, float margin, float coo_thresh,
                            float* d_loss, float* d_pos, float* d_min_neg, void* d_saved, size_t saved_bytes,
                            void* hip_stream);
int hn_neimask_loss_backward(const float* d_anchor, const float* d_positive, int64_t batch, int32_t dim, float margin,
                             const float* d_dloss, float* d_grad_anchor, float* d_grad_positive, void* d_saved,
                             size_t saved_bytes, void* hip_stream);

/* FPR at 95 % recall of an evaluation batch of descriptor pairs (hardnet/HardNet.py:450-472
 * + hardnet/EvalMetrics.py:6-19): per-pair L2 distance, scores -> distances transform, sort,
 * first index reaching 95 % recall, FP / (FP + TN).
 * d_anchor, d_positive: [n,dim] fp32; d_labels: [n] int32 (1 = match).  Outputs: d_dists
 * ([n] fp32 pair distances, may be NULL) and d_fpr (one double; NaN if there are no
 * negatives; 0 if there are no matches).  Ties are ordered stably (numpy's quicksort order is
 * unspecified).  Labels: any nonzero value counts as one match, 0 as a non-match; the reference's
 * cumsum adds the labels raw, so it agrees only for labels in {0, 1}. */
int hn_fpr95_workspace_bytes(int64_t n, size_t* bytes_out);
int hn_fpr95(const float* d_anchor, const float* d_positive, const int32_t* d_labels, int64_t n,
             int32_t dim, float* d_dists, double* d_fpr, void* d_workspace, size_t workspace_bytes,
             void* hip_stream);

/* Nearest and second-nearest database descriptor of every query, the matching step of FDLNet's evaluation
 * (FDLNet-master/latency/NASNet/utils/eval_utils.py:112-197 over math_utils.py:8-19), without materialising
 * the n_query x n_db distance matrix.
 *   HN_METRIC_UNIT  d(a,b) = sqrt(clamp(2 - 2 a.b, 1e-8, 4))           FDLNet's distance_matrix_vector (unit rows)
 *   HN_METRIC_L2    d(a,b) = sqrt(|a|^2 + |b|^2 - 2 a.b + 1e-6) + 1e-8  hardnet/Losses.py:5-13
 * d_query [n_query,128], d_db [n_db,128] fp32 (16-byte aligned).  Outputs (8-byte aligned): d_dist [n_query,2]
 * fp32 and d_idx [n_query,2] int32, column 0 the nearest database row and column 1 the second-nearest, with
 * d_dist[i][0] <= d_dist[i][1] and d_idx[i][0] != d_idx[i][1].  With n_db == 1 the second place is
 * dist = +inf, idx = -1.  1 <= n_query, n_db <= 2^22.
 * Precision: the two rows are SELECTED on the key c_j - 2 a_i.b_j (c_j = 0 / |b_j|^2: both distances are
 * monotone in it) with the dot product on the bf16 MFMA in bf16x3 split precision, about 5e-6 absolute on
 * unit descriptors: a selected row's key exceeds the true minimum (second minimum) by at most twice that
 * error.  The reported distances are then recomputed for the two selected rows in plain fp32; should they
 * come out in the other order (keys within the selection error), the pair is swapped.
 * Ties: rows are ordered lexicographically on (key, index): of equal keys the smaller database index comes
 * first, for both places, whatever the order the GPU finishes its work in; the call is deterministic and a
 * query's result does not depend on which other queries share the call.
 * One deliberate difference from the reference: where several database rows fall inside the clamp
 * (2 - 2 a.b < 1e-8) the reference's min sees equal distances and returns whichever index torch picks; this
 * call orders such rows by the unclamped key.
 * No allocation or synchronisation inside; every argument check runs before the GPU is touched. */
enum hn_metric { HN_METRIC_UNIT = 0, HN_METRIC_L2 = 1 };
int hn_match_workspace_bytes(int64_t n_query, int64_t n_db, size_t* bytes_out);
int hn_match_nn2(const float* d_query, int64_t n_query, const float* d_db, int64_t n_db, int32_t dim,
                 int32_t metric, float* d_dist, int32_t* d_idx, void* d_workspace, size_t workspace_bytes,
                 void* hip_stream);

/* Patch preprocessing: uint8 patches -> fp32 [n,1,32,32] network input,
 * bit-exact with the reference loaders.
 *   HN_RESIZE_CV2_LINEAR   hardnet/HardNet.py:345-349 'transform' + Utils.py:10-11 cv2_scale:
 *                          64x64 -> 32x32 cv2 INTER_LINEAR (= OpenCV's 2x area-fast path)
 *   HN_RESIZE_PIL_BILINEAR hardnet/HardNet.py:333-337 'transform_test': PIL Resize(32), bilinear
 *   HN_RESIZE_NONE         input already 32x32 (cv2.resize to the same size is a copy)
 * then ToTensor (/255) and, if normalize != 0, Normalize((mean,), (std,)) in fp32.
 * d_in: [n, in_hw, in_hw] uint8 (in_hw 64 for the resizing modes, 32 for NONE). */
enum hn_resize { HN_RESIZE_NONE = 0, HN_RESIZE_CV2_LINEAR = 1, HN_RESIZE_PIL_BILINEAR = 2 };
int hn_preprocess(const uint8_t* d_in, int64_t n, int32_t in_hw, int32_t resize, int32_t normalize,
                  float mean, float std, float* d_out, void* hip_stream);

/* Descriptor forward from uint8 patches (the loader transforms of
 * hardnet/HardNet.py:333-337 / 345-349 + Utils.py:10-11 fused into the network's patch load):
 * d_in [B, in_hw, in_hw] uint8; resize / normalize / mean / std as hn_preprocess.  Equals
 * hn_preprocess followed by hn_forward bit for bit.  For the stock HardNet, FDLNet and the
 * hardnetNAS descriptors (every resize mode) the preprocessing runs inside the first fused kernel
 * (k_c12 / the FDLNet and NAS fronts: 4 / 1 KiB of input HBM per patch and no fp32 copy); the k5
 * NAS front in PIL mode (measured faster apart) and the A/B configurations (HN_NO_FRONT,
 * HN_FRONT_FOLD, HN_FDL_VALU, HN_U8_APART) preprocess each chunk into the workspace tail first.
 * Workspace: hn_workspace_bytes_u8. */
int hn_workspace_bytes_u8(const hn_model* m, int64_t batch, size_t* bytes_out);
int hn_forward_u8(hn_model* m, const uint8_t* d_in, int64_t batch, int32_t in_hw, int32_t resize,
                  int32_t normalize, float mean, float std, float* d_out, void* d_workspace,
                  size_t workspace_bytes, void* hip_stream);

/* Keypoint patch extraction, the step between FDLNet's detector and its descriptor (clip_patch,
 * FDLNet-master/latency/NASNet/utils/image_utils.py:11-158, as model/network.py:163-176 calls it): a rotated,
 * scaled 32x32 window around every keypoint, sampled from its image by bilinear interpolation.
 *   d_images [n_images,1,height,width] fp32 contiguous; d_kpts [n,4] int64 rows (b, y, x, .) as nonzero()
 *   gives them; d_scale [n] fp32; d_ori [n,2] fp32 (cos, sin), or NULL for no rotation; d_ratio [n_images]
 *   fp32 (im_info[:,0]); d_patches [n,1,32,32] fp32 (16-byte aligned).
 * Arithmetic: the reference's, in fp32 and in its operation order, with IEEE division and no fused multiply-add:
 *   r = ratio[b]; s = (scale / r) / 2; kx = float(x) / r; ky = float(y) / r;
 *   g[i] = torch.linspace(-1, 1, 32)[i] (step 2/31: -1 + step i for i < 16, else 1 - step (31 - i));
 *   xs = (s cos) g[col] + (-(s sin)) g[row] + kx;  ys = (s sin) g[col] + (s cos) g[row] + ky;
 *   x0 = floor(xs), x1 = x0 + 1, both clamped to [0, width - 1]; y0, y1 likewise with height - 1;
 *   the four weights (x1 - xs)(y1 - ys), (x1 - xs)(ys - y0), (xs - x0)(y1 - ys), (xs - x0)(ys - y0) use the
 *   CLAMPED corners converted back to float, which is what makes a sample outside the image come out (nearly)
 *   zero; out = wa Ia + wb Ib + wc Ic + wd Id, summed left to right.
 * Bounds guarantee: the call reads no byte outside d_images whatever the keypoint data.  The batch index is
 * clamped to [0, n_images - 1] for addressing (image and ratio); NaN, +-Inf and coordinates beyond the integer
 * range are made safe before the float -> integer conversion.  The patch of such a keypoint is unspecified; every
 * other keypoint's patch is unaffected, and a keypoint's patch never depends on which others share the call.
 * One deliberate difference from the reference: the reference maps keypoint i to ratio row i / (n / n_images)
 * (a .view(B, -1)) but to its image through the keypoint's own column 0, which agree only when every image
 * has the same number of keypoints, in batch order.  Here column 0 selects both, so unequal counts per image and
 * any keypoint order work; where the reference is consistent the results are the same.
 * No allocation or synchronisation inside; every argument check runs before the GPU is touched: n, n_images
 * >= 0 (n == 0 returns HN_OK; n > 0 needs n_images >= 1), height, width >= 2, n_images * height * width < 2^63. */
int hn_clip_patch(const float* d_images, int64_t n_images, int32_t height, int32_t width, const int64_t* d_kpts,
                  const float* d_scale, const float* d_ori, const float* d_ratio, int64_t n, float* d_patches,
                  void* hip_stream);

/* Backward of hn_clip_patch to the keypoints' scale and orientation: d_dscale [n] and d_dori [n,2] from the
 * patches' gradient d_dpatches [n,1,32,32] (16-byte aligned); every other argument as in the forward call.  Not
 * differentiated: the images, the ratio and the integer keypoint rows.  Either output may be NULL (not computed);
 * d_dori != NULL without d_ori is HN_ERR_ARG.
 * Mathematics: the corners are detached (the reference's .floor().long()), so inside its cell a sample is bilinear
 * in (xs, ys).  With d the sample's upstream gradient, g[col], g[row] its grid values and the clamped corners of
 * the forward:
 *   gX = (y1 - ys)(Ic - Ia) + (ys - y0)(Id - Ib);   gY = (x1 - xs)(Ib - Ia) + (xs - x0)(Id - Ic)
 *   (pixel differences first: where clamping makes two corners one pixel the term is exactly 0);
 *   a = sum d (gX g[col] + gY g[row]) = d/d(s cos);   b = sum d (gY g[col] - gX g[row]) = d/d(s sin);
 *   d_dscale = (a cos + b sin) / r / 2;   d_dori = (a s, b s),  s = (scale / r) / 2;   no rotation: cos 1, sin 0.
 * fp32 without fused multiply-add; the 1,024 terms of a keypoint are summed in a fixed order by one workgroup (no
 * atomics), so a keypoint's gradient is bit-identical call to call, alone or inside any batch.
 * Bounds guarantee: the forward's -- the sample addresses are computed by the same code, and the call reads no
 * byte outside d_images whatever the keypoint data.  The gradient of a keypoint with non-finite data is
 * unspecified; every other keypoint's gradient is unaffected.
 * Caller's stream, no allocation or synchronisation inside, capturable; the argument checks are hn_clip_patch's
 * and run before the GPU is touched (n == 0 returns HN_OK). */
int hn_clip_patch_backward(const float* d_dpatches, const float* d_images, int64_t n_images, int32_t height,
                           int32_t width, const int64_t* d_kpts, const float* d_scale, const float* d_ori,
                           const float* d_ratio, int64_t n, float* d_dscale, float* d_dori, void* hip_stream);

/* Descriptors of keypoints: hn_clip_patch into the workspace tail, a chunk of min(n, chunk) keypoints at a
 * time, then the model's forward on the chunk.  Equals hn_clip_patch followed by hn_forward bit for bit, for
 * every model kind; d_out [n,128] fp32.  Workspace: hn_workspace_bytes_kp = hn_workspace_bytes + min(n, chunk)
 * x 4 KiB; a short one is HN_ERR_WORKSPACE.  d_out and d_workspace 16-byte aligned.  Capturable like hn_forward.
 * (The sampling is not fused into the first kernel's patch load the way the uint8 path is.) */
int hn_workspace_bytes_kp(const hn_model* m, int64_t n, size_t* bytes_out);
int hn_forward_kp(hn_model* m, const float* d_images, int64_t n_images, int32_t height, int32_t width,
                  const int64_t* d_kpts, const float* d_scale, const float* d_ori, const float* d_ratio, int64_t n,
                  float* d_out, void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* FDLNet's keypoint detector, the first step of Network.inference (model/network.py:148-183): eval-mode
 * RFDet.forward of the NASNet variant (FDLNet-master/latency/NASNet/model/det.py:57-94; single scale, pairs with
 * HN_KIND_FDL_NASNET) for fp32 images, in fp32 FMA arithmetic, two kernel launches.
 *   features.0 conv 1->16 3x3 (bias, no activation); two InvertedResidual(16,16,1,benchmodel=1) blocks
 *   (model/operations.py:449-511: channels 0..7 pass, 8..15 through 1x1+BN+ReLU, depthwise 3x3+BN, 1x1+BN+ReLU,
 *   concat, channel_shuffle(2): new channel 2j+g = old channel 8g+j); every 3x3 layer pads its own input with
 *   zeros.  Score head: conv 16->1 3x3, InstanceNorm2d(1, affine) with THIS image's statistics (biased variance,
 *   in_eps), leaky_relu(0.01), then soft_nms_3d(ksize 15, strength 7) (utils/image_utils.py:298-329):
 *   m = 15x15 maximum (windows clipped at the image), e = exp(7 (s - m)), p = e / (15x15 box sum of e with zero
 *   padding + 1e-8).  Orientation head: conv 16->2 3x3, InstanceNorm2d(2, affine), division by the pair's L2
 *   norm (no epsilon, as the reference).  soft_max_and_argmax_1d over the one scale is the identity on p in fp32
 *   and the scale map is the constant scale_list[0] = 32: neither is computed.
 * host_params: every float tensor of RFDet.state_dict() in its order, num_batches_tracked left out --
 *   features.0.{weight,bias}; for features.1 and features.2: banch2.0.weight, banch2.1.{weight,bias,running_mean,
 *   running_var}, banch2.3.weight, banch2.4.{...}, banch2.5.weight, banch2.6.{...}; conv.{weight,bias};
 *   insnorm.{weight,bias}; conv_ori.{weight,bias}; insnorm_ori.{weight,bias}: 40 tensors, hn_det_param_count
 *   floats (1,193).  BatchNorm (eval mode, bn_eps) is folded into the weights at create time, in double.
 * d_images [n_images,1,height,width] fp32 contiguous -> d_score [n_images,height,width] (the reference's
 * im_rawsc), d_ori [n_images,height,width,2] (cos, sin; 8-byte aligned).  Workspace (16-byte aligned):
 * hn_det_workspace_bytes = the three pre-norm maps plus 48 bytes per 16x16 tile; a short one is
 * HN_ERR_WORKSPACE.  The InstanceNorm statistics are per-workgroup fp64 partial sums combined in fp64 in a fixed
 * order (no float atomics): an image's maps are bit-identical call to call, alone or inside any batch.
 * Caller's stream, no allocation or synchronisation inside (capturable); every argument check runs before the GPU
 * is touched: n_images >= 0 (0 returns HN_OK), height, width >= 1 with height * width in 2 .. 2^31 - 1,
 * n_images * ceil(height / 16) * ceil(width / 16) < 2^31. */
typedef struct hn_detector hn_detector;
int hn_det_param_count(size_t* n_out);
int hn_det_create(const float* host_params, size_t n_params, float bn_eps, float in_eps, hn_detector** out);
int hn_det_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* bytes_out);
int hn_det_forward(hn_detector* d, const float* d_images, int64_t n_images, int32_t height, int32_t width,
                   float* d_score, float* d_ori, void* d_workspace, size_t workspace_bytes, void* hip_stream);
void hn_det_destroy(hn_detector* d);

/* The same detector in train() and its backward: what autograd does over RFDet in FDLNet's training step
 * (train.py:310-336 calls det(im1), det(im2) with model.train()).  Shaped like hn_nas_train_*: no handle and no
 * host blob -- the weights change every step and are read where the optimiser left them.
 * d_tensors: host array of HN_DET_TRAIN_TENSORS device pointers, the float tensors of RFDet.state_dict() in its
 *   order (the order hn_det_create documents; num_batches_tracked left out, the caller increments it).
 * forward: as hn_det_forward, but every BatchNorm normalises with the statistics of all n_images * height * width
 *   pixels of the call (biased variance) and moves its running statistics in place:
 *   running <- (1 - momentum) running + momentum batch, with the unbiased variance for running_var.
 *   d_score [n,H,W], d_ori [n,H,W,2]; d_saved keeps the pre-norm activations, the statistics, and the soft NMS's
 *   e, s and window arg-max (the first maximum in raster order, torch's max_pool2d rule) for the backward.
 * backward: d_dscore [n,H,W], d_dori [n,H,W,2] (either may be NULL: zero) -> d_grads, a host array parallel to
 *   d_tensors: every parameter slot needs a buffer (frozen parameters included; overwritten), the running
 *   statistics' slots are ignored (may be NULL).  No image gradient.  The window maximum is not detached: its
 *   gradient is routed to the arg-max, as autograd routes it through max_pool2d.
 * Every sum over pixels (BatchNorm / InstanceNorm statistics, their backward sums, every weight and bias gradient)
 * is a per-workgroup fp64 partial combined in a fixed order, no float atomics: outputs, running statistics and
 * gradients are bit-identical call to call.
 * Workspaces from hn_det_train_workspace_bytes; d_saved is written by the forward and read by its backward,
 * d_scratch is transient; a short one is HN_ERR_WORKSPACE.  Caller's stream, no allocation or synchronisation
 * inside; every argument check runs before the GPU is touched: n_images in 1 .. 2^24, height, width >= 1,
 * height * width < 2^31, n_images * height * width >= 2 (the unbiased variance), bn_eps, in_eps > 0, momentum in
 * 0 .. 1, no NULL pointer but d_dscore / d_dori, and d_images, d_score, d_ori, d_dscore, d_dori, d_saved and
 * d_scratch 16-byte aligned. */
#define HN_DET_TRAIN_TENSORS 40
int hn_det_train_workspace_bytes(int64_t n_images, int32_t height, int32_t width, size_t* saved_bytes_out,
                                 size_t* scratch_bytes_out);
int hn_det_train_forward(const float* d_images, int64_t n_images, int32_t height, int32_t width,
                         float* const* d_tensors, float bn_eps, float in_eps, float momentum, float* d_score,
                         float* d_ori, void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                         void* hip_stream);
int hn_det_train_backward(const float* d_dscore, const float* d_dori, const float* d_images, int64_t n_images,
                          int32_t height, int32_t width, float* const* d_tensors, float* const* d_grads,
                          void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* Keypoint selection, the step between the detector's score map and hn_clip_patch: RFDet.process followed by
 * Network.inference's second topk_map, nonzero() and gathers (model/det.py:96-133, model/network.py:155-183,
 * utils/image_utils.py:197-274) for any score map d_score [n_images,height,width] fp32, K = topk:
 *   1. f = s inside the border, 0 within `border` pixels of an edge (filter_border; the reference's radius is 8);
 *      a NaN score counts as 0.
 *   2. t = f < nms_thresh ? 0 : f; keep where t >= the maximum of t over the nms_ksize x nms_ksize window, with 0
 *      outside the image; v = f keep.
 *   3. per image the K largest v form the mask; g = v mask.
 *   4. q = clamp(conv(g, psf, zero padding gauss_ksize / 2), 0, 1), psf[y][x] = exp(-((x-c)^2 / (2 sigma^2) +
 *      (y-c)^2 / (2 sigma^2))) in fp32, NOT normalised; sigma == 0 is a delta; taps summed in row-major order.
 *   5. per image the K largest q are the keypoints (yes: the second top-K runs on the blurred map).
 *   6. the keypoints leave in raster order per image, images in order, as nonzero() lists them:
 *      d_kpts [n_images K, 4] int64 rows (b, y, x, 0); d_kscore [n_images K] = s at the keypoint (the raw score);
 *      d_kscale [n_images K] from d_scale_map [n_images,height,width], or scale_value where the map is NULL;
 *      d_kori [n_images K, 2] from d_ori_map [n_images,height,width,2] (both given or both NULL).
 *      Optional dense outputs (process's own return values; NULL to skip): d_score_proc [n_images,height,width]
 *      = q, d_topk_mask [n_images,height,width] uint8 = the mask of step 3.
 * The one deliberate difference from the reference (next to hn_match_nn2's): both top-K steps order pixels by
 * (value descending, flat index ascending), where the reference leaves ties to torch.sort.  So fewer than K
 * positive pixels are filled up with the zeros of lowest index, and the result does not depend on the order in
 * which workgroups finish.  The output count is exactly n_images K: nothing is read back, no allocation or
 * synchronisation inside (capturable), no float atomics.  Workspace (16-byte aligned): hn_select_workspace_bytes
 * = three fp32 maps; every byte of it is written before it is read.
 * Every argument check runs before the GPU is touched: n_images >= 0 (0 returns HN_OK), 1 <= topk <= height *
 * width < 2^31, border >= 0 with height, width > 2 border, nms_ksize and gauss_ksize odd in 1 .. 15,
 * gauss_sigma finite and >= 0, nms_thresh not NaN, d_kori and d_ori_map both or neither; else HN_ERR_ARG. */
int hn_select_workspace_bytes(int64_t n_images, int32_t height, int32_t width, int32_t topk, size_t* bytes_out);
int hn_select_keypoints(const float* d_score, int64_t n_images, int32_t height, int32_t width, int32_t border,
                        float nms_thresh, int32_t nms_ksize, int32_t topk, int32_t gauss_ksize, float gauss_sigma,
                        const float* d_scale_map, float scale_value, const float* d_ori_map, int64_t* d_kpts,
                        float* d_kscore, float* d_kscale, float* d_kori, float* d_score_proc, uint8_t* d_topk_mask,
                        void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* The homography ground-truth stage of Network.forward (model/network.py:23-142, 185-264): what lies between the
 * detector's maps of an image pair and its patch pairs.  Homographies are device arrays [n_images, 9] fp32, row-major
 * 3x3, as the batch holds them; maps are dense [n_images,height,width(,2)] fp32.  One projection is used everywhere:
 *   u = h00 x + h01 y + h02, v = h10 x + h11 y + h12, w = h20 x + h21 y + h22 -> (u / (w + 1e-8), v / (w + 1e-8)),
 * products summed left to right without contraction, IEEE divisions.  .long() truncates toward zero and .round()
 * rounds half to even; before either conversion a NaN becomes 0 and the value saturates (truncation at +-(2^30 - 64),
 * rounding at +-(2^31 - 128): every image has fewer than 2^31 pixels, so such a coordinate is outside it either way).
 * All four calls: caller's stream, one kernel launch, no allocation, workspace or synchronisation inside
 * (capturable), no float atomics; an image's result is bit-identical call to call and independent of what else is
 * in the batch.  Bounds guarantee: no byte outside the inputs is read whatever the homography, keypoint, map or mask
 * data holds (the address computations are hn_homo.h's, swept on the host by `make homo_check`).  Every argument
 * check runs before the GPU is touched: n_images >= 0 (0 returns HN_OK), height, width >= 2, height * width < 2^31,
 * n_images * height * width < 2^62; else HN_ERR_ARG.
 *
 * hn_warp_score -- gtscore's two warp calls with filter_border fused into the read (utils/image_utils.py:161-213).
 *   Output pixel (x, y) is projected by d_homo to (px, py); xn = px / (W - 1) * 2 - 1, yn likewise with H; then
 *   grid_sample's bilinear sampling with zeros padding: ix = ((xn + 1) W - 1) / 2 (align_corners 0) or
 *   (xn + 1) / 2 (W - 1) (align_corners 1), corners floor(ix) and floor(ix) + 1, unclamped, the four weights from the
 *   unclamped corners, a corner outside the image contributing 0.  The source value reads as 0 within `border`
 *   pixels of an edge (8 in the reference; 0 = no filter).  d_warped = the sample of d_score, d_visible = the same
 *   sample of a map of ones (the sum of the in-bounds weights, no border); either may be NULL.
 *   Deliberate note on align_corners: the reference calls grid_sample without the argument, which in today's torch
 *   means False, so 0 is "what the reference's code does" (and under 0 the identity homography is not an identity
 *   warp); 1 is the behaviour its (W - 1) normalisation was written for.  Both are supported.
 *   Also needs border >= 0 with height, width > 2 border and align_corners in {0, 1}.
 *
 * hn_gt_scale_orin -- Network.gt_scale_orin (model/network.py:200-264) with no intermediate map.  The reference
 *   computes centScale, cos_w, sin_w at every pixel of image 2 and gathers them at q = clamp(round(proj(homo12, p)));
 *   here output pixel p computes q first and evaluates the formulas at q only.  With s = d_scale[q] (or scale_value
 *   where d_scale is NULL) and h = floor(s / 2): the centre q and (qx, qy -+ h), (qx +- h, qy) are projected by homo21
 *   and truncated; each distance is 2 sqrt(float(dx^2 + dy^2) + 1e-8); d_gt_scale = (up + right + bottom + left) / 4
 *   in that order.  Orientation: (qx + s cos, qy + s sin) and the centre projected, untruncated; ww, hw their
 *   differences; r = sqrt(ww^2 + hw^2 + 1e-8); (ww / (r + 1e-8), hw / (r + 1e-8)) divided by that pair's L2 norm (no
 *   epsilon).  d_ori and d_gt_ori [n_images,height,width,2] (cos, sin), 8-byte aligned.
 *
 * hn_mask_keypoints -- pair's left_imtopk.nonzero() and masked_selects (utils/net_utils.py:27-37) for a top-K mask
 *   d_mask [n_images,height,width] uint8 (hn_select_keypoints' d_topk_mask: pair uses the FIRST top-K mask, not the
 *   keypoints of the second): d_kpts [n_images topk, 4] int64 rows (b, y, x, 0), the first topk set pixels of every
 *   image in raster order, images in order; d_kscale / d_kori gathered from the maps (or scale_value; d_kori and
 *   d_ori_map both or neither).  An image with fewer set pixels gets rows (b, 0, 0, 0) for the rest (scale and
 *   orientation of its pixel (0, 0)); the count is never read back.  d_counts [n_images] int32 (or NULL) receives the
 *   true number of set pixels.  The compaction is a scan, not an atomic append.  1 <= topk <= height * width.
 *
 * hn_project_keypoints -- ptCltoCr (utils/math_utils.py:43-106): d_kpts [n,4] rows (b, y, x, .) -> d_kpts_r [n,4]
 *   rows (b, y', x', 0) with (x', y') = round(proj(d_homo[b], (x, y))), clamped to [0, W - 1] x [0, H - 1] if `clamp`;
 *   d_scale_r [n] and d_ori_r [n,2] gathered from the right image's maps (or scale_value; d_ori_r and d_ori_map both
 *   or neither) at index b H W + y' W + x' clamped to [0, n_images H W - 1], exactly as the reference does: with
 *   clamp = 0 (eval_model's use) a keypoint projected outside keeps its outside coordinates and gathers whatever that
 *   clamped index names.  One deliberate difference, hn_clip_patch's: the keypoint's own column 0, clamped to
 *   [0, n_images - 1], selects the homography (the reference's .view(B, -1) agrees with it only for equal counts in
 *   batch order).  n >= 0 (0 returns HN_OK; n > 0 needs n_images >= 1), clamp in {0, 1}. */
int hn_warp_score(const float* d_score, const float* d_homo, int64_t n_images, int32_t height, int32_t width,
                  int32_t border, int32_t align_corners, float* d_warped, float* d_visible, void* hip_stream);
int hn_gt_scale_orin(const float* d_scale, float scale_value, const float* d_ori, const float* d_homo12,
                     const float* d_homo21, int64_t n_images, int32_t height, int32_t width, float* d_gt_scale,
                     float* d_gt_ori, void* hip_stream);
int hn_mask_keypoints(const uint8_t* d_mask, int64_t n_images, int32_t height, int32_t width, int32_t topk,
                      const float* d_scale_map, float scale_value, const float* d_ori_map, int64_t* d_kpts,
                      float* d_kscale, float* d_kori, int32_t* d_counts, void* hip_stream);
int hn_project_keypoints(const int64_t* d_kpts, int64_t n, const float* d_homo, int64_t n_images, int32_t height,
                         int32_t width, const float* d_scale_map, float scale_value, const float* d_ori_map,
                         int32_t clamp, int64_t* d_kpts_r, float* d_scale_r, float* d_ori_r, void* hip_stream);

/* Train-mode stock HardNet (the module of hardnet/HardNet.py:275-315 in
 * model.train() as the training loop :379-441 runs it through autograd).
 *  forward : input_norm (mean / std detached), 7 x [conv -> BatchNorm2d(affine=False) with the
 *            batch's statistics (running_mean / running_var updated in place with `momentum`,
 *            unbiased variance) -> ReLU], Dropout(dropout_p) before conv6, L2Norm.
 *  backward: d_dout [B,128] -> d_dweights[l] (each [Cout,Cin,k,k] like the module's weights,
 *            overwritten), and d_din [B,1,32,32] if not NULL.
 * d_weights / d_running_* / d_dweights are host arrays of 7 device pointers (features.{0,3,6,9,
 * 12,15,19}.weight and the matching BN buffers, fp32 contiguous).  The workspace has two parts:
 *   d_saved   -- written by the forward, read by its backward: keep it unchanged between a
 *                forward and its backward (the training loop's two forwards, anchors and
 *                positives, HardNet.py:392-393, each need their own);
 *   d_scratch -- transient: any buffer of the size asked for, reusable by every call.
 * The backward must get the forward's batch, dropout_p and seed (the dropout mask is a counter
 * hash of (seed, element), recomputed).  It only reads d_saved, so it may run more than once.
 * Batch >= 2 (train-mode BatchNorm of the 1x1 conv6 output needs more than one value). */
int hn_hardnet_train_workspace_bytes(int64_t batch, size_t* saved_bytes_out, size_t* scratch_bytes_out);
int hn_hardnet_train_forward(const float* d_in, int64_t batch, const float* const* d_weights,
                             float* const* d_running_mean, float* const* d_running_var, float momentum,
                             float dropout_p, uint64_t seed, float* d_out, void* d_saved, size_t saved_bytes,
                             void* d_scratch, size_t scratch_bytes, void* hip_stream);
int hn_hardnet_train_backward(const float* d_dout, int64_t batch, const float* const* d_weights,
                              float* const* d_dweights, float* d_din, float dropout_p, uint64_t seed,
                              void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                              void* hip_stream);

/* Test and diagnostic entry, NO STABILITY PROMISE (an addition: HN_ABI_VERSION stays 2, but the argument list may
 * change with any release): one layer operation of the train step above, alone, on caller-owned buffers.  The step
 * functions are loops over the same code, so what this entry runs is what they run.
 *   layer          0..6 (read by the CONV_* and BN_* operations only, but always checked).
 *   train_f32_bits the HN_TRAIN_F32 bits (0..255) that choose a convolution's kernel form; -1: the process's.
 *   row_segments   0: by batch, as the step; 1, 2 or 4: the row segments per patch of the ring kernels (clamped to
 *                  what the kernel's geometry allows).  Non-zero only where the chosen form has row segments.
 *   dgrad_chunk    0: as the step; n: patches per column chunk (1..batch) of the column-GEMM data gradient.
 *                  Non-zero only for CONV_DGRAD where the chosen form is the column GEMM.
 * Activations are CNHW ([C][batch][H][W], fp32), all device pointers 16-byte aligned:
 *   op              d_x                     d_w              d_y                    d_aux0 / 1 / 2
 *   INPUT_NORM      in [B][1024]            -                xn [B][1024]           1/(std+eps) [B] / - / -
 *   CONV_FWD        input of layer l (*)    W[l]             conv output            -
 *   BN_FWD          -                       -                conv output, in place  rstd [Cout] out / running_mean /
 *                                                                                   running_var (both or neither)
 *   L2_FWD          z6 [128][B]             -                out [B][128]           -
 *   L2_BWD          z6 [128][B]             dout [B][128]    dz6 [128][B]           -
 *   BN_BWD          z_l (BN output)         rstd [Cout]      gradient, in place     -
 *   CONV_WGRAD      input of layer l (*)    dY               dW[l]                  -
 *   CONV_DGRAD      dY                      W[l]             d input activation     -
 *   INPUT_NORM_BWD  1/(std+eps) [B]         -                d xn, scaled in place  d_in [B][1024] (a copy) / - / -
 * (*) layer 0: the normalised patch; else the previous layer's BN output z, pre-activation: the kernel applies the
 * ReLU (and, for layer 6, the dropout of dropout_p / seed) as the step does.  BN_BWD masks with ReLU for layers 0..5
 * and with the dropout for layer 5.  d_scratch: hn_hardnet_train_layer_op_workspace_bytes of the same batch, bits and
 * row_segments. */
enum hn_train_op {
  HN_TRAIN_OP_INPUT_NORM = 0,
  HN_TRAIN_OP_CONV_FWD = 1,
  HN_TRAIN_OP_BN_FWD = 2,
  HN_TRAIN_OP_L2_FWD = 3,
  HN_TRAIN_OP_L2_BWD = 4,
  HN_TRAIN_OP_BN_BWD = 5,
  HN_TRAIN_OP_CONV_WGRAD = 6,
  HN_TRAIN_OP_CONV_DGRAD = 7,
  HN_TRAIN_OP_INPUT_NORM_BWD = 8
};
int hn_hardnet_train_layer_op_workspace_bytes(int32_t train_f32_bits, int32_t row_segments, int64_t batch,
                                              size_t* scratch_bytes_out);
int hn_hardnet_train_layer_op(int32_t op, int32_t layer, int32_t train_f32_bits, int32_t row_segments,
                              int64_t dgrad_chunk, int64_t batch, const float* d_x, const float* d_w, float* d_y,
                              float* d_aux0, float* d_aux1, float* d_aux2, float momentum, float dropout_p,
                              uint64_t seed, void* d_scratch, size_t scratch_bytes, void* hip_stream);

/* Train-mode hardnetNAS (second half; hardnetNAS/supernet_functions/
 * training_functions_supernet.py:88-103 runs the module in train() through autograd):
 *   desc->kind HN_KIND_NAS           the sampled descriptor (op[i] per layer), model_supernet.py:53-85
 *                                    with each MixedOperation replaced by its arch op;
 *   desc->kind HN_KIND_NAS_SUPERNET  the supernet: layer i outputs sum_j m[i][j] op_j(x) over all 17
 *                                    CANDIDATE_BLOCKS (MixedOperation.forward, model_supernet.py:23-36);
 *                                    d_soft = the soft weights m [n_layers][17] (the caller's
 *                                    Gumbel-softmax draw, :24), d_dsoft receives d loss / d m.
 *   desc->kind HN_KIND_FDL_NASNET / _FDL_NASNET01  FDLNet HardNetNeiMask (des.py:8-55 / NASNet_0.1
 *                                    des.py:10-55): input_norm (desc->input_norm_eps), conv0 3x3 + bias,
 *                                    then BN(affine=False) -> 1x1 s2 BN ReLU -> 1x1 s2 BN ReLU (NASNet) or
 *                                    MaxPool(3,2,1) -> 1x1 s2 BN ReLU (NASNet_0.1), then the layers at 8x8.
 * forward : front -> the layers -> 4x4 head conv -> BatchNorm2d(affine=False) -> y / ||y||,
 *           every BatchNorm with the batch's statistics (running stats updated with `momentum`,
 *           unbiased variance).  d_in [B,1,32,32] fp32 (NAS: no input_norm, the NAS loaders normalise;
 *           FDL: input_norm in the forward).
 * backward: d_dout [B,128] -> d_grads (every conv weight, BN weight / bias and SE weight / bias,
 *           overwritten).  hn_nas_train_backward forms no input gradient; hn_nas_train_backward_dx is the same
 *           call with d_din [B,1,32,32] (16-byte aligned; NULL: none, then the two calls are identical), which
 *           receives d loss / d d_in for every kind: conv0's data gradient (zero padding, fp32 FMA) times, for
 *           the FDL kinds, the saved 1 / (std + eps) of input_norm, whose mean and std are detached (des.py:40-49).
 *           Every other result is bit-identical with or without d_din; the workspace sizes are the same.
 * d_tensors: host array of hn_nas_train_tensor_count() device pointers, one per float tensor of the
 * module's state_dict in order (num_batches_tracked and the supernet's `thetas` left out): conv
 * weights, BN weight, bias, running_mean, running_var (updated in place), SE weights / biases.
 * d_grads: the same length; entries for running buffers are ignored (may be NULL); every weight
 * slot (conv / SE weights and biases) needs a buffer, frozen parameters included (HN_ERR_ARG if NULL).
 * Workspace: d_saved is written by the forward and read by its backward (one per forward call);
 * d_scratch is transient. */
int hn_nas_train_tensor_count(const hn_arch_desc* desc, size_t* n_out);
int hn_nas_train_workspace_bytes(const hn_arch_desc* desc, int64_t batch, size_t* saved_bytes_out,
                                 size_t* scratch_bytes_out);
int hn_nas_train_forward(const hn_arch_desc* desc, const float* d_in, int64_t batch, float* const* d_tensors,
                         float momentum, const float* d_soft, float* d_out, void* d_saved, size_t saved_bytes,
                         void* d_scratch, size_t scratch_bytes, void* hip_stream);
int hn_nas_train_backward(const hn_arch_desc* desc, const float* d_dout, const float* d_in, int64_t batch,
                          float* const* d_tensors, const float* d_soft, float* const* d_grads, float* d_dsoft,
                          void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                          void* hip_stream);
int hn_nas_train_backward_dx(const hn_arch_desc* desc, const float* d_dout, const float* d_in, int64_t batch,
                             float* const* d_tensors, const float* d_soft, float* const* d_grads, float* d_dsoft,
                             float* d_din, void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes,
                             void* hip_stream);

/* Per-stage timing (profiling aid used by bench.py): when enabled, hn_forward records a
 * hipEvent pair around every kernel launch on the caller's stream.  hn_stage_times
 * waits for the recorded events, accumulates their durations per stage name and returns
 * the number of stages (<= max_stages); it then clears the accumulators.
 * names_out[i] points to storage owned by the model. */
int hn_set_profiling(hn_model* m, int enable);
int hn_stage_times(hn_model* m, int max_stages, const char** names_out, double* total_ms_out,
                   int64_t* launches_out);

void hn_destroy(hn_model* m);

/* Message of the last failing call on this thread ("" if none). */
const char* hn_last_error(void);

/* HN_ABI_VERSION of the loaded library. */
int hn_abi_version(void);

#ifdef __cplusplus
}
#endif

#include "hardnet_mi355x_loss_reduce.h"
#include "hardnet_mi355x_rfdet.h"

#endif /* HARDNET_MI355X_H */
