/*
 * mvs_abi.h -- C ABI of the MI355X-native MVSNet depth-inference path (libmvs_hip.so).
 *
 * Drop-in boundary: these are the entry points the reference's Python side
 * binds (ctypes) to replace, for inference, the torch ops dispatched by
 *   models/mvsnet.py:145-218  (cost volume -> CostRegNet -> soft-argmin / confidence)
 *   models/module.py:96-147   (homo_warping, depth_regression)
 * of /root/reference.  FeatureNet (models/mvsnet.py:10-30) is part of the library as well (mvs_feature_net,
 * mvs_forward_images: csrc/featnet.hip); a caller that keeps its own FeatureNet hands its NCHW fp32 output to
 * mvs_warp_variance / mvs_depth_infer instead.
 *
 * Conventions
 *  - extern "C", plain pointers and ints; no torch / C++ types.
 *  - Every `dev` pointer is device memory owned by the caller (torch's allocator); the library
 *    borrows it for the duration of the enqueue and allocates nothing on the device.
 *  - Work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream).  No entry point synchronises the device.
 *  - Return value: MVS_OK or an error code; mvs_last_error_string() (thread-local) explains it.
 *    The library never aborts the process.
 *  - Re-entrant: no mutable global state besides the thread-local error string.
 *  - Volumes between stages use a PRIVATE "C8-planar" layout: a C-channel volume is C/8 planes,
 *    each a channels-last volume of 8 channels, [C/8][D][h][w][8].  Only the documented
 *    inputs/outputs below have reference layouts.
 *  - Shape domain: every device entry point states the admitted range of each integer argument and which pointers may
 *    be NULL.  Outside it the call returns MVS_ERR_NULL (a required pointer is NULL), MVS_ERR_BAD_SHAPE,
 *    MVS_ERR_BAD_DTYPE or MVS_ERR_WORKSPACE, decided on the host from the arguments alone: nothing is enqueued on a
 *    refusal and no HIP call is made.  The upper ends come from the index types of the kernel forms an entry point can
 *    select, whichever MVS_* switch is set; they are derived, and beyond the largest shapes the tests run
 *    (D*h*w*32 < 2^32 volumes at 512 x 640) not measured: a HIP runtime that declines a grid of that many blocks
 *    returns MVS_ERR_HIP for such a shape, it is never served wrongly.  "The volume domain" below is the one
 *    mvs_query_workspace checks: N in [1,64], C = 32, D, h, w positive multiples of 8, D*h*w*32 < 2^32, dtype an
 *    mvs_dtype.
 *  - Alignment.  Read from the gfx950 code of the kernels each entry point can select.  Where a public tensor is read or
 *    written wider than an element (float4 / f32x4 / dwordx4 loads and stores, 16-byte LDS-staged epilogues), or read
 *    as consecutive wave-uniform values (rt, depth_values, proj: scalar loads the compiler merges into multi-dword
 *    ones), the pointer must be 16-byte aligned, else MVS_ERR_BAD_SHAPE; the blobs are read with uniform and 16-byte
 *    loads and must be 16-byte aligned, else MVS_ERR_WORKSPACE; a workspace 256 bytes, else MVS_ERR_WORKSPACE.  Decided
 *    on the host before anything is enqueued; a NULL that is allowed passes.  Whether the hardware would serve such an
 *    access at a 4-byte aligned address is not measured and no test tries.  A pointer stated "per element" below is
 *    touched by single-dword vector accesses only and needs a float's alignment: tests/test_gpu_wrapper_contract.py runs
 *    each of them one element into a larger allocation.  torch's allocations are 256-byte aligned; a row of a batch is
 *    16-byte aligned when a row is a multiple of 4 floats.  The entry points with a rule of their own state it:
 *    mvs_conv3d_train_* (min(C, 4) floats), mvs_bn3d_train_*, mvs_volume_relayout (16 bytes), mvs_depth_metrics
 *    (element-aligned tensors are served by a scalar or shifted path; workspace 8 bytes).  mvs_filter_depth states none
 *    and is outside this rule.
 */
#ifndef MVS_ABI_H
#define MVS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): + mvs_feature_net_fmt / mvs_forward_images_fmt (uint8 images); mvs_warp_conv0 removed (it left in round
 * 3 without a bump); the packed weight blob grew (split-operand conv0 panel) and lost the round-2 conv0 panels.
 * A packed blob (mvs_pack_weights / mvs_pack_feature_weights) is valid ONLY for the library version that produced it:
 * never cache one across builds -- re-pack from the state_dict (4 MB, milliseconds).
 * Added within version 2, without a bump (additive; packed blobs unchanged): mvs_depth_infer_views,
 * mvs_query_metrics_workspace, mvs_depth_metrics, mvs_warp_variance_backward, mvs_softargmin_backward,
 * mvs_query_conv3d_train_workspace, mvs_conv3d_train_forward, mvs_conv3d_train_backward_data,
 * mvs_conv3d_train_backward_weight, mvs_feature_conv01_fmt, mvs_query_bn3d_train_workspace, mvs_bn3d_train_forward,
 * mvs_bn3d_train_backward, mvs_volume_relayout; and, declared in a header of their own, include/mvs_fuse_abi.h:
 * mvs_query_fuse_workspace, mvs_fuse_points.
 * Likewise include/mvs_cloud_abi.h: mvs_query_cloud_workspace, mvs_cloud_downsample.
 * Likewise include/mvs_normals_abi.h: point normals of a cloud, and the downsample that carries them.
 * Likewise include/mvs_outliers_abi.h: statistical outlier removal among the points of a cloud inside a box.
 * Likewise include/mvs_distance_abi.h: the distance from every point of one cloud to the nearest point of another.
 * Likewise include/mvs_reduce_abi.h: DTU's point reduction, observability mask and ground-plane filter of a cloud.
 * Likewise include/mvs_cluster_abi.h: the density-connected components (DBSCAN) of a cloud and the mask of the large ones.
 * Likewise include/ext/mvs_register_abi.h: the rigid registration of one cloud onto another (ICP). */
#define MVS_ABI_VERSION 2

typedef enum mvs_status {
    MVS_OK = 0,
    MVS_ERR_BAD_SHAPE = 1,   /* dims not supported (C != 32, D/h/w not multiples of 8, N < 1 ...);
                                the reference raises a torch shape error here (mvsnet.py:69-71) */
    MVS_ERR_BAD_DTYPE = 2,   /* storage dtype not implemented */
    MVS_ERR_WORKSPACE = 3,   /* workspace / blob too small or misaligned (workspace: 256 bytes; blob: 16 bytes) */
    MVS_ERR_HIP = 4,         /* a HIP runtime call failed (launch error ...) */
    MVS_ERR_NULL = 5         /* required pointer is NULL */
} mvs_status;

/* pixel format of the images handed to mvs_feature_net_fmt / mvs_forward_images_fmt.  The uint8 forms are the decoded
 * image as the reference's loader holds it BEFORE `np.array(img, dtype=np.float32) / 255.` (datasets/data_io.py:143);
 * the library performs that IEEE division itself (bit-equal), so a caller copies a quarter of the bytes to the device. */
typedef enum mvs_image_format {
    MVS_IMG_F32_CHW = 0,     /* float32 [N][3][H][W] in [0,1]: the tensor MVSNet.forward receives (models/mvsnet.py:103) */
    MVS_IMG_U8_CHW = 1,      /* uint8 [N][3][H][W] */
    MVS_IMG_U8_HWC = 2       /* uint8 [N][H][W][3], as PIL / np.array(img) yields it (datasets/data_io.py:143) */
} mvs_image_format;

/* storage dtype of the private volumes (accumulation is always fp32; a stored value is the round-to-nearest-even cast of
 * the fp32 one, ties to even, fp16 subnormals kept on both sides, +inf from 65520 on) */
typedef enum mvs_dtype { MVS_F32 = 0, MVS_F16 = 1, MVS_BF16 = 2 } mvs_dtype;

/* Number of conv layers in CostRegNet (models/mvsnet.py:35-62):
 *   0..6 conv0..conv6, 7 conv7 (deconv), 8 conv9 (deconv), 9 conv11 (deconv), 10 prob */
#define MVS_NUM_LAYERS 11

int mvs_abi_version(void);

/* Thread-local description of the last non-OK status returned on this thread. */
const char* mvs_last_error_string(void);

/* Bytes of device workspace needed by mvs_depth_infer / mvs_warp_variance / mvs_costreg_forward
 * for a [N views, C, D, h, w] problem.  Replaces nothing in the reference (torch allocates its
 * intermediates implicitly at models/mvsnet.py:145-180).
 * Domain: the volume domain (N in [1,64], C = 32, D,h,w positive multiples of 8, D*h*w*32 < 2^32; dtype 0..2 else
 * MVS_ERR_BAD_DTYPE); bytes must not be NULL.  Host only: no device work. */
int mvs_query_workspace(int N, int C, int D, int h, int w, int dtype, size_t* bytes);

/* Bytes of the packed weight blob produced by mvs_pack_weights. */
int mvs_query_weights_blob(size_t* bytes);

/* HOST function.  Folds eval-mode BatchNorm3d (eps as given; torch default 1e-5) into the conv
 * weights and re-lays them out for the kernels.  Replaces the per-forward BN arithmetic of
 * models/module.py:29-33 and models/mvsnet.py:47-60.
 *   conv_weights[l]  host fp32, reference layout: Conv3d [Cout][Cin][3][3][3] for l in 0..6,10;
 *                    ConvTranspose3d [Cin][Cout][3][3][3] for l in 7..9
 *   bn_params[4*l+{0,1,2,3}] = gamma, beta, running_mean, running_var of layer l (l in 0..9)
 *   prob_bias        host fp32 [1]          (cost_regularization.prob.bias)
 *   blob_out         host buffer of mvs_query_weights_blob() bytes; copy it to the device
 *                    and pass that device pointer as `weights_blob` below.
 * Domain: no pointer may be NULL, nor any of conv_weights[0..10] and bn_params[0..39] (MVS_ERR_NULL); blob_bytes >=
 * mvs_query_weights_blob (MVS_ERR_WORKSPACE).  Host only. */
int mvs_pack_weights(const float* const* conv_weights, const float* const* bn_params,
                     const float* prob_bias, float eps, void* blob_out, size_t blob_bytes);

/* rt_out[(v-1)*12 .. +12] = rows 0..2 of proj[v] @ inverse(proj[0]) as rot (9, row-major) then
 * trans (3), for v = 1..N-1.   Replaces torch.inverse/matmul at models/module.py:107-109.
 *   proj   dev fp32 [N][4][4]      rt_out dev fp32 [(N-1)][12]
 * Domain: N in [1,64]; neither pointer may be NULL.  N = 1 enqueues nothing and leaves rt_out untouched.
 * Alignment: proj and rt_out 16-byte aligned, else MVS_ERR_BAD_SHAPE (the kernel reads proj with dwordx4 and 16-dword
 *   uniform loads and writes rt_out with dwordx4 stores). */
int mvs_relative_proj(const float* proj, float* rt_out, int N, void* stream);

/* Fused homography warp + variance cost volume.
 * Replaces models/module.py:96-139 (per source view) and models/mvsnet.py:145-177.
 *   feats         dev fp32 [N][C][h][w]   (FeatureNet outputs, view 0 = reference view)
 *   rt            dev fp32 [(N-1)][12]    (from mvs_relative_proj)
 *   depth_values  dev fp32 [D]
 *   var_out       dev, C8-planar [4][D][h][w][8] in `dtype`; must not alias the workspace
 *   workspace     dev, >= mvs_query_workspace bytes (uses the feature-transpose region only)
 * Domain: the volume domain.  rt may be NULL when N = 1; no other pointer may.  A workspace smaller than the
 * feature-transpose region or not 256-byte aligned is MVS_ERR_WORKSPACE.  Nothing is enqueued on a refusal.
 * Alignment: feats per element (the transpose reads single floats).  var_out (f32x4 / 16-byte stores), rt and
 *   depth_values (consecutive uniform reads) 16-byte aligned, else MVS_ERR_BAD_SHAPE. */
int mvs_warp_variance(const float* feats, const float* rt, const float* depth_values,
                      void* var_out, void* workspace, size_t workspace_bytes, int N, int C, int D,
                      int h, int w, int dtype, void* stream);

/* 3D U-Net cost regularisation.  Replaces CostRegNet.forward, models/mvsnet.py:64-73.
 *   var           dev C8-planar [4][D][h][w][8] in `dtype` (from mvs_warp_variance)
 *   weights_blob  dev copy of the mvs_pack_weights blob
 *   cost_out      dev fp32 [D][h][w]  (== cost_reg.squeeze(1) of models/mvsnet.py:192)
 * Non-finite voxels (the warp writes NaN for non-finite sampling coordinates) are ordinary data: every layer keeps
 *   them as F.relu and conv3d do.  A logit is non-finite wherever the reference's is (NaN where it is NaN; NaN or the
 *   infinity where it is +-inf: the split-operand and zero-padded forms turn inf into inf - inf or inf * 0); every finite
 *   logit keeps its bound; non-finite logits outside the reference's set stay within the kernel forms' tile geometry
 *   (Winograd along z: the rest of the 4- or 2-plane output tile; Toeplitz-pair and transposed forms: one voxel in x).
 * Domain: the volume domain with N = 1, C = 32; no pointer may be NULL; workspace >= mvs_query_workspace(1, 32, D, h, w,
 * dtype) bytes and 256-byte aligned, else MVS_ERR_WORKSPACE.  Nothing is enqueued on a refusal.
 * Alignment: every data pointer 16-byte aligned, else MVS_ERR_BAD_SHAPE (the conv kernels load and store activations and
 *   logits 16 bytes at a time); weights_blob 16-byte aligned, else MVS_ERR_WORKSPACE. */
int mvs_costreg_forward(const void* var, const void* weights_blob, float* cost_out,
                        void* workspace, size_t workspace_bytes, int D, int h, int w, int dtype,
                        void* stream);

/* One CostRegNet layer (0..10, table above) on C8-planar tensors: the building block of
 * mvs_costreg_forward, exported for per-layer parity tests and per-kernel timing in bench.py.
 * Replaces one ConvBnReLU3D / ConvTranspose3d+BN+ReLU(+skip) / prob conv of
 * models/mvsnet.py:36-62.
 *   x     dev [Cin/8][Di][Hi][Wi][8]    skip  dev [Cout/8][Do][Ho][Wo][8] or NULL (layers 7..9
 *   y     dev [Cout/8][Do][Ho][Wo][8]   need it)              (layer 10: y is fp32 [D][h][w])
 * NaN and infinity in x or skip: as stated at mvs_costreg_forward, per layer (the ReLU keeps NaN; a 16-bit store keeps
 *   NaN and infinity).
 * Domain: layer in [0,10]; dtype 0..2 (MVS_FORCE_DIRECT=1: MVS_F32 only), else MVS_ERR_BAD_DTYPE; Di, Hi, Wi >= 1, all
 * three even at the stride-2 layers 1, 3, 5, and Di*Hi*Wi < 2^28 (every kernel form addresses one 8-channel plane of
 * its input with 31-bit element offsets; planes and outputs are 64-bit), at layer 10 also (5 Hi + 9) Wi + 33 < 2^28
 * (the prob kernel holds a piece's offset from its tile's halo origin, up to 5 planes and 9 rows on, in 31 bits: it
 * bites only below D = 5 or within a row of the first bound), else MVS_ERR_BAD_SHAPE.  Any such volume is served, down
 * to 1 x 1 x 1: the tile forms pad.  skip may be NULL at layers 0..6 and 10 (it is not read); x, y,
 * weights_blob and, at layers 7..9, skip may not.  Nothing is enqueued on a refusal.
 * Alignment: every data pointer 16-byte aligned, else MVS_ERR_BAD_SHAPE (the conv kernels load and store activations and
 *   logits 16 bytes at a time); weights_blob 16-byte aligned, else MVS_ERR_WORKSPACE. */
int mvs_conv_layer(int layer, const void* x, const void* skip, void* y, const void* weights_blob,
                   int Di, int Hi, int Wi, int dtype, void* stream);

/* The last two layers in one kernel (what mvs_costreg_forward runs): conv11 + BN + ReLU, the conv0 skip add
 * and the prob convolution, without the full-resolution 8-channel tensor in between.
 * Replaces models/mvsnet.py:71-72 (`x = conv0 + self.conv11(x); x = self.prob(x)`).  Exported like
 * mvs_conv_layer, for parity tests and per-kernel timing.  x and skip in `dtype` (16-bit storage: the transposed
 * convolution runs on the 16-bit MFMA, the sum that feeds prob stays fp32); the logits are always fp32.
 *   x     dev [2][Di][Hi][Wi][8]  (output of layer 8)     skip  dev [1][2Di][2Hi][2Wi][8]  (output of layer 0)
 *   cost_out  dev fp32 [2Di][2Hi][2Wi]
 * NaN and infinity in x or skip: as stated at mvs_costreg_forward (a non-finite skip voxel reaches its 27 logits, a
 *   non-finite x voxel the logits of its transposed footprint and one more voxel in x).
 * Domain: Di, Hi, Wi >= 1 and Di*Hi*Wi*64 < 2^31 (31-bit element offsets into the full-resolution skip plane), else
 * MVS_ERR_BAD_SHAPE; dtype 0..2; no pointer may be NULL.  Nothing is enqueued on a refusal.
 * Alignment: every data pointer 16-byte aligned, else MVS_ERR_BAD_SHAPE (the conv kernels load and store activations and
 *   logits 16 bytes at a time); weights_blob 16-byte aligned, else MVS_ERR_WORKSPACE. */
int mvs_conv11_prob(const void* x, const void* skip, float* cost_out, const void* weights_blob,
                    int Di, int Hi, int Wi, int dtype, void* stream);

/* softmax over D, depth expectation and photometric confidence in one pass.
 * Replaces models/mvsnet.py:192-193,204,214-218 and models/module.py:144-147.
 *   cost dev fp32 [D][h][w]; depth_out, conf_out dev fp32 [h][w]
 * A pixel's depth and confidence are NaN exactly where softmax-then-sum is: a NaN or +inf logit, or -inf logits only
 *   (the reference's trunc of the NaN expectation picks some window of an all-NaN row: NaN whichever).  A -inf logit
 *   among finite ones is a term of exactly 0; other pixels of the block are untouched.
 * Domain: D in [1, 2^24] (the expected depth index is an fp32 sum of p_d * d: exact integers end there), h, w >= 1 and
 * h*w <= 2^31 - 256 (the pixel index of the last, partly filled block is an int), else MVS_ERR_BAD_SHAPE; no pointer
 * may be NULL.  D = 1 yields depth = depth_values[0] and confidence 1.  Nothing is enqueued on a refusal.
 * Alignment: cost, depth_out and conf_out per element.  depth_values is read uniformly (the unrolled forms may merge
 *   its loads); nothing is asked of it: tests/test_gpu_softargmin_ref.py has always run rows of a batch that are only
 *   4-byte aligned. */
int mvs_softargmin_conf(const float* cost, const float* depth_values, float* depth_out,
                        float* conf_out, int D, int h, int w, void* stream);

/* mvs_relative_proj -> mvs_warp_variance -> mvs_costreg_forward -> mvs_softargmin_conf for one
 * batch item.  Replaces models/mvsnet.py:145-218 after FeatureNet.
 *   proj dev fp32 [N][4][4]; other arguments as above.
 * Domain: the volume domain; no pointer may be NULL; workspace >= mvs_query_workspace(N, C, D, h, w, dtype) bytes and
 * 256-byte aligned, else MVS_ERR_WORKSPACE.  Nothing is enqueued on a refusal.
 * Alignment: feats, depth_out and conf_out per element (the transpose reads, the soft-argmin kernel writes, single
 *   floats).  proj (mvs_relative_proj's dwordx4 reads) and depth_values (consecutive uniform reads) 16-byte aligned,
 *   else MVS_ERR_BAD_SHAPE; weights_blob 16-byte aligned, else MVS_ERR_WORKSPACE. */
int mvs_depth_infer(const float* feats, const float* proj, const float* depth_values,
                    const void* weights_blob, float* depth_out, float* conf_out, void* workspace,
                    size_t workspace_bytes, int N, int C, int D, int h, int w, int dtype,
                    void* stream);

/* mvs_depth_infer with the N views taken from a bank of V NCHW feature maps, so that FeatureNet runs
 * once per image of a scan instead of once per map that reads it (reference models/mvsnet.py:125 runs
 * it on every view of every sample).  Results are bit-identical to mvs_depth_infer on the gathered
 * features feats[view_idx[0]], ..., feats[view_idx[N-1]].
 *   feats     dev fp32 [V][C][h][w]  (any V >= 1; e.g. FeatureNet outputs of every view of a scan)
 *   view_idx  HOST int32 [N]: view_idx[0] = reference view, 1..N-1 = source views; each in [0, V);
 *             repeats allowed.  Copied into the launch; not read after the call returns.
 *   proj      dev fp32 [N][4][4] in view_idx order; other arguments as mvs_depth_infer
 *             (workspace of mvs_query_workspace(N, ...) bytes).
 * An index outside [0, V) or V < 1 returns MVS_ERR_BAD_SHAPE, a NULL view_idx MVS_ERR_NULL; nothing
 * is enqueued then.  Otherwise the domain, pointers, workspace and alignment of mvs_depth_infer (view_idx is a host
 * array: any alignment of an int). */
int mvs_depth_infer_views(const float* feats, int V, const int* view_idx, const float* proj,
                          const float* depth_values, const void* weights_blob, float* depth_out,
                          float* conf_out, void* workspace, size_t workspace_bytes, int N, int C,
                          int D, int h, int w, int dtype, void* stream);

/* Stand-alone ops with reference layouts (API parity with models/module.py).
 * mvs_homo_warp: src_fea dev fp32 [C][h][w], rt dev fp32 [12] -> out dev fp32 [C][D][h][w]
 *   (models/module.py:96-139 for one batch item).
 * mvs_depth_regression: p dev fp32 [D][h][w] -> depth dev fp32 [h][w] = sum_d p*depth_values
 *   (models/module.py:144-147).
 * Domain, mvs_homo_warp: C, D >= 1; h, w >= 2 (the reference's grid normalisation divides by h - 1 and w - 1);
 *   h*w < 2^31 (int texel offsets), D*h*w <= (2^31 - 2) * 256 (one thread per output voxel of a channel, fewer than
 *   2^31 blocks of 256) and C*D*h*w <= 2^61 (64-bit byte offsets), else MVS_ERR_BAD_SHAPE.
 * Domain, mvs_depth_regression: D, h, w >= 1 and h*w <= 2^31 - 256 (int pixel index), else MVS_ERR_BAD_SHAPE.
 * Neither takes a NULL pointer; nothing is enqueued on a refusal.
 * Alignment, mvs_homo_warp: src_fea, depth_values and out per element (one thread, one float, gathered or stored singly);
 *   rt 16-byte aligned, else MVS_ERR_BAD_SHAPE (12 consecutive uniform reads).  mvs_depth_regression: p and depth_out
 *   per element; depth_values is read uniformly and nothing is asked of it. */
int mvs_homo_warp(const float* src_fea, const float* rt, const float* depth_values, float* out,
                  int C, int D, int h, int w, void* stream);
int mvs_depth_regression(const float* p, const float* depth_values, float* depth_out, int D,
                         int h, int w, void* stream);

/* ---- depth-map filter / fusion (reference eval.py:508-585, 620-705, 253-275) ----
 * Replaces the numpy + cv2.remap loops of reproject_with_depth / check_geometric_consistency /
 * the per-reference-view body of filter_depth, for all reference views of a scan in one launch.
 *
 * mvs_filter_compose (HOST pointers only, no GPU work): forms the float32 camera products the
 *   reference forms with np.linalg.inv / np.matmul on float32 inputs.
 *     intrinsics [V][9], extrinsics [V][16] row-major (read_camera_parameters, eval.py:89-104)
 *     ref_idx [R]; src_idx [R][S] with -1 for "no view" (pair.txt rows may be ragged)
 *     ref_mats  [R][30]   = inv(K_ref)[9] | K_ref[9] | inv(E_ref[:3,:3])[9] | E_ref[:3,3][3]
 *     pair_mats [R][S][42] = (E_src inv(E_ref))[:3][12] | K_src[9] | inv(K_src)[9] | (E_ref inv(E_src))[:3][12]
 * mvs_filter_depth (DEVICE pointers): depth, conf fp32 [V][h][w]; ref_mats / pair_mats / ref_idx /
 *   src_idx as above but in device memory.  Thresholds = eval.py:46-49 (--photomask, --geomask,
 *   --condmask_pixel, --condmask_depth).  Outputs, per reference view r:
 *     geo_sum   int32  [R][h][w]     number of source views that agree           (eval.py:694)
 *     depth_avg double [R][h][w]     (sum of agreeing reprojected depths + d_ref)/(geo_sum+1) (699)
 *     masks     uint8  [R][3][h][w]  photo, geo, final as 0/1                    (660, 702, 706)
 *     xyz_world double [R][h*w][3]   depth2pts_np(depth_avg, K_ref, E_ref)       (752, 253-265)
 *   Selecting xyz_world[final] and the colours (eval.py:753-759) stays with the caller (or with mvs_fuse_points,
 *   include/mvs_fuse_abi.h).
 *   Index contract: mvs_filter_compose rejects a ref_idx outside [0,V) and a src_idx >= V with
 *   MVS_ERR_BAD_SHAPE, and ref_idx / src_idx handed to mvs_filter_depth must be the arrays it
 *   accepted.  mvs_filter_depth cannot read device memory on the host and does not validate them:
 *   for a ref_idx[r] outside [0,V) the kernel returns without writing ANY output of row r (the
 *   caller's buffers keep whatever they held), and a src_idx outside [0,V) is skipped like -1. */
#define MVS_FILTER_REF_FLOATS 30
#define MVS_FILTER_PAIR_FLOATS 42
int mvs_filter_compose(const float* intrinsics, const float* extrinsics, const int* ref_idx,
                       const int* src_idx, int V, int R, int S, float* ref_mats, float* pair_mats);
int mvs_filter_depth(const float* depth, const float* conf, const float* ref_mats,
                     const float* pair_mats, const int* ref_idx, const int* src_idx, int V, int R,
                     int S, int h, int w, double photomask, int geomask, double condmask_pixel,
                     double condmask_depth, int* geo_sum, double* depth_avg, unsigned char* masks,
                     double* xyz_world, void* stream);

/* ---- FeatureNet (reference models/mvsnet.py:10-30, block models/module.py:6-13)
 * and the whole MVSNet.forward of one batch item from images (models/mvsnet.py:103-239, eval).
 *
 * mvs_pack_feature_weights (HOST pointers): conv_weights[8] = feature.conv0..conv6.conv.weight and
 *   feature.feature.weight, each [Cout][Cin][k][k]; bn_params[7*4] = per ConvBnReLU block
 *   (bn.weight, bn.bias, bn.running_mean, bn.running_var); feature_bias [32].  Folds eval BatchNorm
 *   into the weights and lays them out as MFMA panels; blob_out is host memory of
 *   mvs_query_feature_blob() bytes that the caller then copies to the device.
 * mvs_feature_net: imgs dev fp32 [N][3][H][W] -> feats_out dev fp32 [N][32][H/4][W/4] (NCHW, as
 *   FeatureNet.forward returns them); workspace of mvs_query_feature_workspace(N,H,W) bytes.
 * mvs_feature_layer: one layer (0..6 = conv0..conv6, 7 = feature) for per-layer parity tests;
 *   x = NCHW image [N][3][Hi][Wi] for layer 0, else C8-planar [Cin/8][N][Hi][Wi][8]; y C8-planar.
 * mvs_feature_conv01_fmt: conv0 + conv1 as the ONE fused kernel that mvs_feature_net / mvs_forward_images run first
 *   (mvs_feature_layer 0 and 1 are the two separate kernels of MVS_FEAT_SPLIT01=1), for parity tests and per-kernel
 *   timing; imgs in any mvs_image_format -> y C8-planar [1][N][H][W][8].  Same refusals as mvs_feature_net_fmt
 *   (NULL, format, N*H*W*8 >= 2^31, H or W < 4); nothing is enqueued on a refusal.
 * NaN and infinity (mvs_feature_layer, mvs_feature_conv01_fmt, mvs_feature_net[_fmt], mvs_forward_images[_fmt]): a
 *   non-finite pixel, activation, weight or BatchNorm parameter is ordinary data and is never hidden.  Every ReLU keeps
 *   a NaN, as F.relu does.  An output is non-finite wherever the reference's is: NaN where it is NaN; NaN or the
 *   infinity where it is +-inf (the layers' padded last tap multiplies the pixel under the last real tap by a packed
 *   weight of exactly 0, and inf * 0 is NaN; that pixel belongs to the same output, so nothing spreads).  Outside the
 *   reference's own footprint of the damaged pixels -- k x k per layer, every output channel; 5 x 5 for the fused
 *   conv0 + conv1 kernel, which computes conv0 on conv1's halo and selects 0 outside the image; 41 x 41 image pixels
 *   per feature pixel for the whole net -- the output bytes are those of the same call on the same input with the
 *   damaged values replaced by finite ones, other views included.  A NaN in a weight or a BatchNorm parameter is
 *   folded into the blob by mvs_pack_feature_weights and makes that channel, hence every feature, depth and
 *   confidence, NaN.  mvs_feature_net's last step moves layer 7's bits to NCHW; the 16-bit copy of the features
 *   (MVS_FEAT16=1) keeps NaN and +-inf and turns a finite value beyond the format's range into the infinity of its
 *   sign.
 * mvs_forward_images: FeatureNet + mvs_depth_infer with the features handed over in the private
 *   C8-planar layout (no NCHW round trip); H, W multiples of 32; workspace of
 *   mvs_query_forward_workspace(N,H,W,D,dtype) bytes.
 * Domain of the image calls (mvs_query_feature_workspace, mvs_feature_layer, mvs_feature_conv01_fmt, mvs_feature_net,
 *   mvs_feature_net_fmt): N in [1,65535] (the image index is a grid dimension), H, W >= 4 (Hi, Wi of mvs_feature_layer
 *   likewise: the dims of that layer's INPUT), N*H*W*8 < 2^31 (31-bit offsets into the 8-channel full-resolution
 *   activation), else MVS_ERR_BAD_SHAPE; feature layer in [0,7]; image_format 0..2 else MVS_ERR_BAD_DTYPE; odd H, W are
 *   served (the stride-2 layers yield (H - 1) / 2 + 1).  mvs_query_forward_workspace, mvs_forward_images and
 *   mvs_forward_images_fmt: both that domain and the volume domain at h = H / 4, w = W / 4, so H, W are positive
 *   multiples of 32.  No pointer of any of them may be NULL (the packers: nor conv_weights[0..7], bn_params[0..27]);
 *   a workspace (blob) smaller than its query or not 256-byte aligned is MVS_ERR_WORKSPACE.  Nothing is enqueued on a
 *   refusal.
 * Alignment, mvs_feature_layer, mvs_feature_conv01_fmt, mvs_feature_net[_fmt], mvs_forward_images[_fmt] alike: imgs (the
 *   uint8 forms too), x, y and feats_out 16-byte aligned, else MVS_ERR_BAD_SHAPE (csrc/featnet.hip stages and stores
 *   activations 16 bytes at a time; its image reads and the NCHW store were not settled and stay with them);
 *   feature_blob and weights_blob 16-byte aligned, else MVS_ERR_WORKSPACE.  mvs_forward_images[_fmt]: proj and
 *   depth_values as mvs_depth_infer; depth_out and conf_out per element. */
#define MVS_FEATURE_LAYERS 8
int mvs_query_feature_blob(size_t* bytes);
int mvs_pack_feature_weights(const float* const* conv_weights, const float* const* bn_params,
                             const float* feature_bias, float eps, void* blob_out, size_t blob_bytes);
int mvs_query_feature_workspace(int N, int H, int W, size_t* bytes);
int mvs_feature_layer(int layer, const float* x, float* y, const void* feature_blob, int N, int Hi, int Wi,
                      void* stream);
int mvs_feature_conv01_fmt(const void* imgs, int image_format, float* y, const void* feature_blob, int N, int H, int W,
                           void* stream);
int mvs_feature_net(const float* imgs, const void* feature_blob, float* feats_out, void* workspace,
                    size_t workspace_bytes, int N, int H, int W, void* stream);
int mvs_query_forward_workspace(int N, int H, int W, int D, int dtype, size_t* bytes);
int mvs_forward_images(const float* imgs, const float* proj, const float* depth_values,
                       const void* feature_blob, const void* weights_blob, float* depth_out,
                       float* conf_out, void* workspace, size_t workspace_bytes, int N, int H, int W,
                       int D, int dtype, void* stream);
/* The same two entry points with the images in any mvs_image_format (ABI 2).  Replaces, for uint8 input, the host-side
 * float conversion of datasets/data_io.py:143 + the 4x larger host-to-device copy (eval.py:358 `tocuda`). */
int mvs_feature_net_fmt(const void* imgs, int image_format, const void* feature_blob, float* feats_out,
                        void* workspace, size_t workspace_bytes, int N, int H, int W, void* stream);
int mvs_forward_images_fmt(const void* imgs, int image_format, const float* proj, const float* depth_values,
                           const void* feature_blob, const void* weights_blob, float* depth_out,
                           float* conf_out, void* workspace, size_t workspace_bytes, int N, int H, int W,
                           int D, int dtype, void* stream);

/* ---- Depth error against ground truth (reference train.py:302-358 test mode: mvsnet_loss models/mvsnet.py:242-244,
 * AbsDepthError_metrics / Thres_metrics utils.py:128-158, errormap train.py:315).
 *
 * mvs_depth_metrics: depth_est, depth_gt, mask dev fp32 [B][h][w] (mask as the loaders produce it, PNG / 255);
 *   thresholds HOST fp32 [n_thres] (0 <= n_thres <= 8).  A pixel is valid where mask > 0.5; e = est - gt in fp32.
 *   sums_out dev fp64 [B][3 + n_thres], one row per image:
 *     [n_valid, sum |e|, sum smooth_l1(e) (beta 1, fp32 per pixel), count(|e| > t_k) for each k]
 *   accumulated in fp64 (counts exact); |e| > t is an fp32 comparison, so a NaN error enters the sums and no count.
 *   errmap_out (dev fp32 [B][h][w], or NULL) = |e| * mask for every pixel, as torch computes it (inf * 0 = NaN).
 *   Per-block partials go to the workspace (mvs_query_metrics_workspace(B,h,w) bytes, 8-byte aligned) and a
 *   second kernel adds them per image in a fixed order: no atomics, bit-identical across runs and streams.
 *   Any h, w >= 1; B >= 1; B*h*w < 2^31; else MVS_ERR_BAD_SHAPE.  Nothing is enqueued on an error. */
int mvs_query_metrics_workspace(int B, int h, int w, size_t* bytes);
int mvs_depth_metrics(const float* depth_est, const float* depth_gt, const float* mask, int B, int h, int w,
                      const float* thresholds, int n_thres, double* sums_out, float* errmap_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- Training: adjoints of the cost volume and of the soft-argmin (csrc/train_backward.hip).
 * Replace the autograd backward of models/module.py:96-139 (grid_sample), models/mvsnet.py:145-177 (the training
 * branch's out-of-place sums and squares, 167-169, and the variance), models/mvsnet.py:192-193 (softmax) and
 * models/module.py:144-147 (depth_regression).  The projections and depth values carry no gradient (the reference
 * builds the sampling grid under no_grad, module.py:106-133), nor does the photometric confidence (mvsnet.py:213).
 *
 * mvs_warp_variance_backward: the exact adjoint of mvs_warp_variance in fp32 (same bilinear taps and weights,
 *   including zero weights outside the image and NaN weights for non-finite sampling coordinates).
 *     feats       dev fp32 [N][C][h][w]     the forward's input (view 0 = reference view)
 *     rt          dev fp32 [(N-1)][12]      from mvs_relative_proj (may be NULL for N = 1)
 *     grad_var    dev fp32 [C][D][h][w]     gradient w.r.t. the variance volume, NCDHW as conv3d's backward hands it
 *     grad_feats  dev fp32 [N][C][h][w]     written (zero-filled inside the call, on `stream`); must not alias inputs
 *   Any shape mvs_warp_variance accepts (N in [1,64], C = 32, D,h,w positive multiples of 8, D*h*w*C < 2^32), else
 *   MVS_ERR_BAD_SHAPE and nothing is enqueued.  Float atomics reorder the sums: not bit-reproducible run to run.
 * mvs_softargmin_backward: grad_cost[d][p] = grad_depth[p] * p_d * (depth_values[d] - depth[p]), with the softmax
 *   p and the depth recomputed from the logits in mvs_softargmin_conf's max-subtracted form.
 *     cost dev fp32 [D][h][w]; grad_depth dev fp32 [h][w]; grad_cost dev fp32 [D][h][w] (written, no atomics)
 *   mvs_softargmin_conf's domain: D in [1, 2^24], h, w >= 1 and h*w <= 2^31 - 256, else MVS_ERR_BAD_SHAPE (narrowed from
 *   "any D, h*w < 2^31": the launcher's rounded-up int grid wrapped in the last 127 pixels of that range, and the
 *   backward accepts what its forward does).
 *   NaN and infinity: a thread owns a pixel.  A NaN or +inf logit at pixel p, logits that are all -inf at p, or a
 *   non-finite grad_depth[p] make grad_cost[:, p] non-finite (NaN, or the infinity the formula gives for an infinite
 *   grad_depth); a single -inf logit among finite ones is a term of exactly 0 with gradient 0, and the other depths
 *   of that pixel keep their bound.  The bytes of every other pixel are those of the call on finite input.
 * Alignment: mvs_warp_variance_backward holds every pointer to 16 bytes, else MVS_ERR_BAD_SHAPE (rt and depth_values are
 *   consecutive uniform reads; feats, grad_var and grad_feats were not read from the compiled code and stay with them).
 *   mvs_softargmin_backward asks for none: its kernel is compiled with 8-byte (dwordx2) accesses, and
 *   tests/test_gpu_train_autograd.py has always run it on rows of a batch that are only 4-byte aligned; no test of
 *   the alignment rule adds to that.
 * Neither allocates, needs a workspace or synchronises. */
int mvs_warp_variance_backward(const float* feats, const float* rt, const float* depth_values, const float* grad_var,
                               float* grad_feats, int N, int C, int D, int h, int w, void* stream);
int mvs_softargmin_backward(const float* cost, const float* depth_values, const float* grad_depth,
                            float* grad_cost, int D, int h, int w, void* stream);

/* ---- Training: CostRegNet's 3x3x3 convolutions in their raw form (no BatchNorm folded in, no ReLU), fp32 in and fp32
 * accumulate on the exact-fp32 matrix instruction (csrc/train_conv3d.hip).  Replace the nn.Conv3d of
 * models/module.py:26-33 (ConvBnReLU3D.conv) and the nn.Conv3d / nn.ConvTranspose3d of models/mvsnet.py:36-62 (conv0 ..
 * conv6, conv7 / conv9 / conv11 [0], prob), and their autograd backward; BatchNorm3d and ReLU stay with the caller.
 *
 * Volumes are CHANNELS-LAST per batch item, [D][H][W][C] fp32 (torch's channels_last_3d of a [1,C,D,H,W] tensor; a
 * 1-channel volume is a plain [D][H][W]) and aligned to min(C, 4) floats.  Weights are the reference tensors as they
 * live on the device, [Cout][Cin][3][3][3]; nothing is packed or cached, so a weight update needs no call.
 * Cin, Cout, D, H, W, stride always describe the CONVOLUTION: x is [D][H][W][Cin], y is [D/stride][H/stride][W/stride][Cout].
 * (Cin, Cout, stride) must be a CostRegNet layer: stride 1 (32,8) (16,16) (32,32) (64,64) (8,1); stride 2 (8,16)
 * (16,32) (32,64).  D, H, W >= 1, even for stride 2, and D*H*W*max(Cin,Cout) < 2^31; anything else is
 * MVS_ERR_BAD_SHAPE and nothing is enqueued.
 *
 * ConvTranspose3d(k=3, s=2, p=1, output_padding=1) with weight [Cin_T][Cout_T][3][3][3] is the adjoint of the stride-2
 * conv with Cin = Cout_T, Cout = Cin_T and THE SAME weight tensor: its forward is mvs_conv3d_train_backward_data
 * (gy = its input), its data gradient mvs_conv3d_train_forward (x = the gradient of its output), its weight gradient
 * mvs_conv3d_train_backward_weight (x = the gradient of its output, gy = its input).
 *
 * mvs_conv3d_train_forward: y[co][o] = bias[co] + sum_{ci,tap} w[co][ci][tap] x[ci][stride*o + tap - 1], zero padding.
 *     bias may be NULL.  flip_transpose = 1 (stride 1 only): w is [Cin][Cout][27] and is read with the taps reversed
 *     and the channels transposed -- the data gradient of the stride-1 conv (Cout -> Cin) that owns w.
 * mvs_conv3d_train_backward_data: gx [D][H][W][Cin] from gy [D/s][H/s][W/s][Cout]; every voxel of gx is written.
 * mvs_conv3d_train_backward_weight: gw[co][ci][tap] = sum_o gy[co][o] x[ci][stride*o + tap - 1] in the layout of w, and,
 *     when gbias != NULL, gbias[co] = sum_o gy[co][o].  Split-K into per-block partial sums in `workspace`
 *     (>= mvs_query_conv3d_train_workspace bytes, 256-byte aligned, else MVS_ERR_WORKSPACE) and a second kernel that
 *     adds them in a fixed order: no float atomics, bit-identical from run to run and stream to stream.
 * NaN and infinity in x or gy are ordinary data and never hidden; they reach exactly what the formulas above say and
 *   the bytes of every other output are those of the call on finite input.  Forward and data gradient: the 3 x 3 x 3
 *   (adjoint) footprint of the damaged voxel, every output channel (lanes, rows and taps outside the volume are selected
 *   to 0 or skipped, never multiplied).  Weight gradient: a non-finite x[ci] at voxel v reaches gw[:, ci, tap] for the
 *   taps through which an in-range output reads v; a non-finite gy[co] reaches gbias[co] and all of gw[co, :, :], also
 *   the taps that are out of range at that output (NaN * 0 is NaN; fp64 conv3d autograd gives the same set).  A
 *   non-finite weight is never hidden either; how far it reaches is not stated.
 * None allocates or synchronises. */
int mvs_query_conv3d_train_workspace(int Cin, int Cout, int D, int H, int W, int stride, size_t* bytes);
int mvs_conv3d_train_forward(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int D,
                             int H, int W, int stride, int flip_transpose, void* stream);
int mvs_conv3d_train_backward_data(const float* gy, const float* w, float* gx, int Cin, int Cout, int D, int H, int W,
                                   int stride, void* stream);
int mvs_conv3d_train_backward_weight(const float* x, const float* gy, float* gw, float* gbias, void* workspace,
                                     size_t workspace_bytes, int Cin, int Cout, int D, int H, int W, int stride,
                                     void* stream);

/* ---- Training: BatchNorm3d with batch statistics, fused with the ReLU and the skip addition that follow it in
 * CostRegNet, and its backward (csrc/train_bn3d.hip).  Replace, in training mode, the nn.BatchNorm3d + F.relu of
 * models/module.py:26-33 and models/mvsnet.py:47-60, the additions of models/mvsnet.py:66-70, and their autograd
 * backward.  With them and the convolutions above, nothing between mvs_warp_variance and mvs_softargmin_conf is left
 * to the caller's framework during a training step.
 *
 * Data is channels-last [M][C] fp32: M = B*D*H*W voxels of a contiguous [B][D][H][W][C] tensor (the statistics are
 * pooled over the batch, as nn.BatchNorm3d pools them), 16-byte aligned.  C in {8, 16, 32, 64}, M >= 2 (torch refuses
 * one value per channel in training mode as well) and M*C < 2^31; anything else is MVS_ERR_BAD_SHAPE and nothing is
 * enqueued.  gamma, beta, save_mean, save_invstd, grad_gamma, grad_beta, running_* are dev fp32 [C], 16-byte aligned.
 *
 * mvs_bn3d_train_forward:
 *     mean_c = sum y / M;  var_c = sum (y - mean_c)^2 / M (biased);  invstd = 1 / sqrt(var + eps)   (IEEE sqrt, divide)
 *     r = ((y - mean) * invstd) * gamma + beta, each operation rounded once;  relu != 0: r = max(r, 0)
 *     out = r + skip when skip != NULL: the skip is added AFTER the ReLU (conv4 + conv7(x), models/mvsnet.py:66-70)
 *     save_mean, save_invstd are written for the backward.  running_mean / running_var (both or neither):
 *     running <- (1 - momentum) running + momentum stat, the variance in its unbiased form var M / (M - 1);
 *     num_batches_tracked stays with the caller.
 *   The variance is a merge of per-thread and per-block (count, mean, M2) triples: one statistics read of y, and no
 *   mean^2 / var term in its error (tests/bn3d_ref.py derives the bound).
 * mvs_bn3d_train_backward: with g = 0 where r <= 0, else grad_out (relu != 0; r recomputed from y, save_mean,
 *   save_invstd, gamma, beta by the forward's instruction sequence, so the mask is the sign of the forward's output bit
 *   for bit; a NaN r passes grad_out, as the forward's ReLU passes the NaN and as torch's threshold_backward does),
 *   and xhat = (y - mean) * invstd:
 *     grad_beta = sum g;  grad_gamma = sum g xhat;  grad_y = gamma invstd (g - grad_beta / M - xhat grad_gamma / M)
 *   The skip's gradient is grad_out itself: no kernel.
 * NaN and infinity: a channel is the unit.  A non-finite y[:, c] makes all of out[:, c], save_mean[c], save_invstd[c],
 *   running_mean[c] and running_var[c] non-finite (the merge of the (count, mean, M2) triples turns an infinite mean
 *   into inf - inf: NaN where the reference holds an infinity, or 0 for the invstd of an infinite variance); a
 *   non-finite skip element reaches its own output element only.  Backward: a non-finite grad_out[:, c] (where the ReLU
 *   is open) or y[:, c] reaches grad_y[:, c], grad_gamma[c] and grad_beta[c]; in a channel whose statistics are NaN
 *   every element passes the ReLU, so grad_beta[c] is the plain sum of grad_out[:, c].  The bytes of every other
 *   channel, through the block tree and the second kernel, are those of the call on finite input.
 * Both: per-block partial results in `workspace` (>= mvs_query_bn3d_train_workspace bytes, 256-byte aligned, else
 * MVS_ERR_WORKSPACE) combined by a second kernel in a fixed order: no float atomics, bit-identical from run to run and
 * stream to stream.  Forward reads y twice and skip once and writes out once; backward reads y and grad_out twice each
 * and writes grad_y once; nothing else of size M*C is touched.  Neither allocates or synchronises.
 *
 * mvs_volume_relayout: a pure copy through LDS between the layouts at the cost volume's boundary, C channels (8, 16, 32
 * or 64) by V voxels (V a positive multiple of 4, V*C < 2^31), both 16-byte aligned:
 *     MVS_RELAYOUT_C8_TO_CHANNELS_LAST      C8-planar [C/8][V][8] (mvs_warp_variance's output) -> channels-last [V][C]
 *     MVS_RELAYOUT_CHANNELS_LAST_TO_PLANAR  channels-last [V][C] -> planar [C][V], the NCDHW gradient that
 *                                           mvs_warp_variance_backward reads
 *   Every 32-bit pattern is moved as it is, NaN payloads and signed zeros included. */
#define MVS_RELAYOUT_C8_TO_CHANNELS_LAST 0
#define MVS_RELAYOUT_CHANNELS_LAST_TO_PLANAR 1
int mvs_query_bn3d_train_workspace(int C, long long M, size_t* bytes);
int mvs_bn3d_train_forward(const float* y, const float* gamma, const float* beta, const float* skip, float* out,
                           float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                           float momentum, float eps, int relu, int C, long long M, void* workspace,
                           size_t workspace_bytes, void* stream);
int mvs_bn3d_train_backward(const float* y, const float* grad_out, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, float* grad_y, float* grad_gamma,
                            float* grad_beta, int relu, int C, long long M, void* workspace, size_t workspace_bytes,
                            void* stream);
int mvs_volume_relayout(const float* src, float* dst, int C, long long V, int direction, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVS_ABI_H */
