/*
 * dodt_hip.h -- C ABI of libdodt_hip.so, the MI355X (gfx950) hot path of DODT/AVOD.
 *
 * The reference has no FFI on this path: its seams are ordinary Python call
 * signatures.  Each entry point below names the reference
 * call it stands behind (paths relative to the reference root).  The ABI follows
 * the one C precedent in the reference, wavedata's integralImage3D
 * (wavedata/wavedata/tools/core/lib/src/integral_images_3d.cpp:66-77, bound in
 * wavedata/wavedata/tools/core/integral_image.py:22-23,96-122): extern "C",
 * caller-allocated outputs, plain pointers and sizes, no ownership transfer --
 * except that every call returns an int status (0 = ok) and the message is
 * available from dodt_last_error() instead of failing silently.
 *
 * Conventions
 *   - One dodt_ctx per GPU per process; it owns one HIP stream and the scratch
 *     memory.  Calls on a ctx are serialised by the caller (the reference is
 *     single threaded, one sess.run at a time).
 *   - Every pointer argument whose name starts with d_ is DEVICE memory
 *     (dodt_malloc, or any hipMalloc'ed / torch-allocated buffer); all other
 *     pointers are host memory, read before the call returns.
 *   - Compute calls are asynchronous on the ctx stream; dodt_ctx_sync() or a
 *     dodt_memcpy_d2h() makes results visible to the host.
 *   - Image-like tensors are NHWC float32 with the batch dimension dropped,
 *     exactly the layout of the reference's TF placeholders.
 *   - No call retains a caller pointer past its return (weights are copied).
 */
#ifndef DODT_HIP_H
#define DODT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DODT_OK 0
#define DODT_ERR_INVALID 1   /* bad argument (the reference raises ValueError) */
#define DODT_ERR_HIP 2       /* a HIP runtime call failed                       */
#define DODT_ERR_UNSUPPORTED 3

typedef struct dodt_ctx dodt_ctx;

/* ---- context, memory --------------------------------------------------- */
int dodt_version(void);
const char* dodt_last_error(void);            /* thread-local, never NULL */
int dodt_ctx_create(int device_id, dodt_ctx** out);
/* Own stream at the device's greatest priority: for short latency-critical chains
 * (per-frame NMS / heads) that share the GPU with long persistent conv launches. */
int dodt_ctx_create_high_priority(int device_id, dodt_ctx** out);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int dodt_ctx_create_on_stream(int device_id, void* hip_stream, dodt_ctx** out);
int dodt_ctx_destroy(dodt_ctx* ctx);
/* The CU count that extractors created on ctx AFTER this call plan their layers with and size their grids by (by
 * default the device's).  Lets a small input walk the code a full-size one walks: several work items per persistent
 * workgroup, tail launches, the wide tiles.  n: a multiple of 8 from 8 to the device's count, anything else is
 * DODT_ERR_INVALID (the grouped work queues hand block b the queue b & 7: a grid of fewer than 8 blocks with more
 * than 8 items would leave queues without a block).  It never raises the count: grids only shrink. */
int dodt_ctx_set_plan_cus(dodt_ctx* ctx, int n);
int dodt_ctx_sync(dodt_ctx* ctx);
/* Timing marks (256 per context) for stream-level timelines: record one on ctx's stream;
 * elapsed GPU time between two marks, possibly of different contexts (waits for `to`). */
int dodt_mark(dodt_ctx* ctx, int slot);
/* Later work on ctx waits for mark `slot` of `other` as last recorded (dodt_ctx_wait_for with the point of
 * `other`'s stream chosen earlier than the call). */
int dodt_ctx_wait_mark(dodt_ctx* ctx, dodt_ctx* other, int slot);
int dodt_mark_elapsed(dodt_ctx* from, int from_slot, dodt_ctx* to, int to_slot, float* ms);
/* Stream-level join: work enqueued on ctx AFTER this call starts only when
 * everything enqueued on `other` BEFORE this call has finished (hipEventRecord on
 * other's stream + hipStreamWaitEvent on ctx's stream; the host does not block).
 * Lets independent frames run on their own contexts/streams and meet again. */
int dodt_ctx_wait_for(dodt_ctx* ctx, dodt_ctx* other);
int dodt_malloc(dodt_ctx* ctx, size_t bytes, void** d_out);
int dodt_free(dodt_ctx* ctx, void* d_ptr);
int dodt_memcpy_h2d(dodt_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int dodt_memcpy_d2h(dodt_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int dodt_memset(dodt_ctx* ctx, void* d_dst, int value, size_t bytes);
/* Page-locked host memory and copies from it that do not block the host: the way raw frames
 * (velodyne .bin contents, camera images -- what KittiUtils hands to create_feed_dict,
 * avod/core/models/dt_rpn_model.py:865-1042) reach the device under the previous step's
 * kernels.  The source must stay untouched until the stream has passed the copy. */
int dodt_pinned_alloc(dodt_ctx* ctx, size_t bytes, void** out);
int dodt_pinned_free(dodt_ctx* ctx, void* ptr);
int dodt_memcpy_h2d_async(dodt_ctx* ctx, void* d_dst, const void* pinned_src, size_t bytes);

/* Small device->host reads that do not stall the stream: begin enqueues a copy of
 * n <= 16 int32 into pinned slot `slot` (0..31) and records an event; end waits for
 * that event only (kernels enqueued after begin keep running) and returns the
 * values.  Used to learn the kept-anchor count while the conv stacks run. */
int dodt_fetch_i32_begin(dodt_ctx* ctx, const int32_t* d_src, int n, int slot);
int dodt_fetch_i32_end(dodt_ctx* ctx, int slot, int32_t* dst, int n);

/* HIP-event stopwatch on the ctx stream: start; ...launches...; stop -> ms
 * (stop waits for the stream). */
int dodt_timer_start(dodt_ctx* ctx);
int dodt_timer_stop(dodt_ctx* ctx, float* ms_out);

/* ---- a0-a3: BEV voxel/slice generator --------------------------------------
 * Stands behind BevSlices.generate_bev (avod/core/bev_generators/bev_slices.py:
 * 33-150) and, with DODT_PTS_VELO_XYZI, also the point path in front of it:
 * lidar_to_cam_frame + z>0 + image-frustum filter
 * (wavedata/.../core/calib_utils.py:484-523, obj_detection/tracking_utils.py:
 * 117-150).  All geometry is evaluated in float64 like the reference. */
#define DODT_PTS_VELO_XYZI 0 /* d_points = (N,4) float32 x,y,z,intensity, velodyne frame */
#define DODT_PTS_CAM_3XN 1   /* d_points = (3,N) float64 rectified camera frame          */

typedef struct dodt_bev_params {
    int32_t point_format;     /* DODT_PTS_*                                         */
    int32_t num_slices;       /* height slices (5); output depth = num_slices + 1   */
    double velo_to_cam[12];   /* (3,4) row major = (R0_rect . Tr_velo_to_cam)[0:3]  */
    double p2[12];            /* (3,4) camera matrix                                 */
    double im_w, im_h;        /* frustum: 0 < u < im_w, 0 < v < im_h (strict)       */
    double plane[4];          /* ground plane a,b,c,d                               */
    double extents[6];        /* x0,x1,y0,y1,z0,z1 (strict on both sides)           */
    double voxel_size;        /* float32-rounded 0.1 as python sees it (F7)         */
    double height_lo, height_hi;
    double occ_lo, occ_hi;    /* slice of the anchor-filter occupancy grid (0.2,2.0) */
    /* Ego-motion registration of the second frame of a pair into the first frame's
     * coordinates, KittiTrackingDataset.point_cloud_transform
     * (avod/datasets/kitti/kitti_tracking_dataset.py:303-335, call site :489):
     * p' = float32((p + pre_translate) @ pre_rotate) in the VELODYNE frame (float64 arithmetic,
     * one rounding into the float32 cloud, as the reference stores it), applied in front of
     * velo_to_cam when has_pre_transform != 0 (DODT_PTS_VELO_XYZI only).  pre_rotate is (3,3)
     * row major = Rz . Rx . Ry of Oxts.get_rotate_matrix (kitti_tracking_utils.py:147-215).
     * The BEV maps come from the warped cloud; the occupancy bits for the anchor filter from
     * the UN-warped one, because the reference re-reads the raw file for that grid
     * (kitti_tracking_utils.py:98-126) -- reproduced, not fixed. */
    int32_t has_pre_transform;
    int32_t reserved_;
    double pre_translate[3];
    double pre_rotate[9];
} dodt_bev_params;

/* d_bev_out: (Z, X, num_slices+1) float32, Z = 700 rows, X = 800 cols for the
 *            KITTI extents; out[r, c, s] = map_s[c, Z-1-r] like the reference.
 * d_occ_bits_out (may be NULL): occupancy of the [occ_lo, occ_hi) slice as a
 *            bit grid, Z rows of ceil(X/32) uint32 words, bit (x & 31) of word
 *            [z * ceil(X/32) + (x >> 5)]; feeds dodt_anchor_filter.
 * Returns DODT_ERR_INVALID when X*Z cells or the y-bin range do not fit the
 * packed 32-bit key (n_points >= 2^25 or more than 127 y-bins). */
int dodt_bev_slices(dodt_ctx* ctx, const void* d_points, int n_points,
                    const dodt_bev_params* params, float* d_bev_out,
                    uint32_t* d_occ_bits_out);
/* Waits for the stream and reports whether the last dodt_bev_slices on this ctx
 * met a point whose cell lies outside the grid (*flags & 1) -- the case in which
 * the reference raises ValueError("Extents are smaller than ...")
 * (voxel_grid_2d.py:130-138) -- or overflowed its work list (*flags & 2). */
int dodt_bev_status(dodt_ctx* ctx, int* flags);
/* Host only (no device work): the BEV cells dodt_bev_slices can ever write for DODT_PTS_VELO_XYZI points under
 * `params`, as a (pad_top + Z, X) byte map in a pyramid extractor's padded input layout (row pad_top + Z-1-z, the
 * pad_top rows 0): 1 = possibly written, 0 = zero in every frame.  A point survives only if its image column
 * u = (P2 p)_0 / (P2 p)_2 lies in (0, im_w); a cell counts as possibly written if u, evaluated in float64 at the
 * 8 corners of its (x, y, z) box over the y extents, reaches (0, im_w), or if w = (P2 p)_2 <= 0 at a corner.
 * Then the substitute-point cell of the slice quirk (x = z = 0) is added and the map dilated by one cell.  The
 * frustum test follows the ego-motion warp, so the map holds for has_pre_transform frames too.
 * DODT_PTS_CAM_3XN skips the frustum test: DODT_ERR_INVALID. */
int dodt_bev_support_mask(const dodt_bev_params* params, int pad_top, uint8_t* mask_out, int rows, int cols);

/* ---- a4: empty-anchor filter -------------------------------------------------
 * Stands behind get_empty_anchor_filter_2d (avod/core/anchor_filter.py:64-119)
 * + IntegralImage2D.query (wavedata/.../core/integral_image_2d.py:39-87).
 * d_anchor_cells: (n_anchors,4) int32 [x1,z1,x2,z2] grid indices produced on the
 *   host once per configuration exactly as the reference does (float32 corners,
 *   float32 division, int32 truncation, clip to [0,X] / [0,Z]).
 * d_keep_idx_out: (n_anchors) int32, first *count entries = kept anchor indices in
 *   ascending (generator) order.  d_count_out: (1) int32. */
int dodt_anchor_filter(dodt_ctx* ctx, const uint32_t* d_occ_bits, int nx, int nz,
                       const int32_t* d_anchor_cells, int n_anchors,
                       int density_threshold, int32_t* d_keep_idx_out,
                       int32_t* d_count_out);

/* ---- a5/a6: anchor projection --------------------------------------------------
 * project_to_bev (avod/core/anchor_projector.py:13-69), project_to_image_space
 * (:72-156, numpy branch, float64 in / float32 out) and the [y1,x1,y2,x2] reorder
 * (:254-273; models/dt_rpn_model.py:983-985).
 * d_anchors: (n_total,6) float64 table; d_idx (may be NULL = identity): (n) int32
 * rows to project; *d_n (may be NULL): device count overriding n (<= n).
 * Outputs (n,4) float32 normalised boxes in TF order [y1,x1,y2,x2]. */
int dodt_project_anchors_f64(dodt_ctx* ctx, const double* d_anchors,
                             const int32_t* d_idx, int n, const int32_t* d_n,
                             const double bev_extents[4], const double p2[12],
                             double im_w, double im_h, float* d_bev_norm_out,
                             float* d_img_norm_out, float* d_anchors_f32_out);

/* TF-branch twins, float32 throughout (models/dt_avod_model.py:170-206):
 * project_to_bev + tf_project_to_image_space (anchor_projector.py:159-251).
 * d_bev_out (n,4) metres [x1,z1,x2,z2] (may be NULL), d_bev_norm_tf_out and
 * d_img_norm_tf_out (n,4) in TF order. */
int dodt_project_anchors_f32(dodt_ctx* ctx, const float* d_anchors, int n,
                             const int32_t* d_n, const float bev_extents[4],
                             const float p2[12], float im_w, float im_h,
                             float* d_bev_out, float* d_bev_norm_tf_out,
                             float* d_img_norm_tf_out);

/* ---- a7: image preprocessing ---------------------------------------------------
 * ImgFeatureExtractor.preprocess_input (avod/core/feature_extractors/
 * img_feature_extractor.py:16-35): legacy bilinear resize + per-channel mean
 * subtraction.  d_img_u8: (in_h,in_w,3) uint8 RGB.  d_out: (out_h,out_w,out_c)
 * float32 with out_c >= 3; channels >= 3 are written as 0 (the conv kernels
 * want an even channel count). */
int dodt_img_preprocess(dodt_ctx* ctx, const uint8_t* d_img_u8, int in_h, int in_w,
                        int out_h, int out_w, int out_c, const float mean_rgb[3],
                        float* d_out);

/* ---- a8-a10: feature extractors ---------------------------------------------------
 * Stands behind feature_extractor_builder.get_extractor(cfg).build(...)
 * (avod/core/feature_extractors/bev_vgg_pyramid.py:30-178, img_vgg_pyramid.py:
 * 30-177) plus the 1x1 bottleneck (models/dt_rpn_model.py:298-322). */
typedef struct dodt_extractor dodt_extractor;
#define DODT_EXTRACTOR_VGG_PYR 0
/* The plain-VGG extractors of the AVOD cars_example configuration (BASELINE.json configs[0]):
 * BevVgg / ImgVgg.build (avod/core/feature_extractors/bev_vgg.py:34-118, img_vgg.py:33-120):
 * the same encoder (conv1_1 .. conv4_3, three VALID 2x2 pools that floor odd sizes), then
 * tf.image.resize_bilinear of conv4_3 to (in_h / 8 * 4, in_w / 8 * 4) -- 256 channels -- and the
 * 256 -> 1 bottleneck of avod/core/models/rpn_model.py:251-267.  fp32 only, pad_top = 0. */
#define DODT_EXTRACTOR_VGG 1
/* OR into `kind`: the extractor shares the GPU with other streams (the frame-pair pipeline
 * runs both nets side by side).  Layers are then single launches: the tail launches that
 * even out a layer's last round when it has the GPU to itself only add work when another
 * stream fills the idle CUs anyway. */
#define DODT_EXTRACTOR_SHARED_GPU 0x100
/* OR into `kind`: conv path on the bf16 MFMA (BASELINE.json configs[2]: "bf16 conv path").
 * Inputs and weights of every conv are rounded to bf16 (nearest even), products accumulate
 * in fp32, batch-norm + ReLU run in fp32, activations between layers are stored as bf16;
 * the first layer's arithmetic, the network output and the bottleneck stay fp32.  The
 * reference computes in fp32: with this flag conv outputs agree with an fp32
 * run to ~1e-2 of their scale, not 1e-4 (tests/test_gpu_conv_bf16.py states the bars). */
#define DODT_EXTRACTOR_BF16 0x200
/* OR into `kind`: fp32-grade convs on the bf16 MFMA ("split" mode).  Every stored activation
 * and every weight is a pair hi + lo of bf16 values (16 mantissa bits), a product is
 * w_hi x_hi + w_hi x_lo + w_lo x_hi in three bf16 MFMAs with fp32 accumulation: relative
 * error ~2^-16 per product instead of bf16's 2^-8, within the 1e-4 bar of the fp32 tests
 * (tests/test_gpu_conv_split.py runs them at the fp32 tolerances). */
#define DODT_EXTRACTOR_SPLIT 0x400
/* Form of the fp32 3x3 stride-1 layers (everything else has one kernel): 4 = Winograd F(4x4,3x3),
 * 2 = Winograd F(2x2,3x3), 0 = direct implicit GEMM.  All are
 * fp32 throughout and within the 1e-4 layer bar; they differ in speed and in how far the rounding
 * noise of a whole stack lies from the exact sums (DESIGN.md 2 / 5.0 give both, and the rule that
 * chose the default).  DODT_CONV_WINO in the environment overrides the default, once per process;
 * any other value is the default. */
#define DODT_CONV_MODE_DEFAULT 2
int dodt_conv_mode(void);
/* in_c: channels of the input tensor as stored (6 for BEV; 4 for the padded
 * image); pad_top: zero rows added on top (4 for BEV 700->704, 0 for images);
 * batch: frames processed per forward call (2 = both frames of a pair). */
int dodt_extractor_create(dodt_ctx* ctx, int kind, int in_h, int in_w, int in_c,
                          int pad_top, int batch, dodt_extractor** out);
int dodt_extractor_destroy(dodt_extractor* ex);
/* One conv layer: name as in the TF variable scope ("conv1_1" ... "conv4_3",
 * "upconv3", "pyramid_fusion3", ..., "bottleneck" -- (1,1,32,1), or (1,1,256,1) for
 * DODT_EXTRACTOR_VGG).  w: HWIO (kh,kw,cin,cout)
 * for conv2d, (kh,kw,cout,cin) for conv2d_transpose, as TF stores them.
 * beta/mean/var: slim.batch_norm variables (no gamma, eps = 1e-3).  Host memory. */
int dodt_extractor_set_layer(dodt_extractor* ex, const char* name, const float* w,
                             int kh, int kw, int c_a, int c_b, const float* beta,
                             const float* mean, const float* var);
/* Zero-copy input: *d_ptr = where frame 0 of the (batch, in_h, in_w, in_c) input
 * lives inside the extractor (frame f at + f * *frame_stride_floats).  A producer
 * that writes there (e.g. dodt_bev_slices) can pass d_in = NULL to forward. */
int dodt_extractor_input(dodt_extractor* ex, float** d_ptr, long long* frame_stride_floats);
/* d_in: (batch, in_h, in_w, in_c) or NULL (see above); d_feat_out: (batch, in_h, in_w, 32);
 * d_bottleneck_out (may be NULL): (batch, in_h, in_w, 1).  DODT_EXTRACTOR_VGG: the outputs are
 * (batch, out_h, out_w, 256) and (batch, out_h, out_w, 1), sizes from
 * dodt_extractor_output_shape. */
int dodt_extractor_forward(dodt_extractor* ex, const float* d_in, float* d_feat_out,
                           float* d_bottleneck_out);
/* The same forward on an input the caller keeps in the extractor's own input layout: (batch, pad_top + in_h, in_w,
 * in_c) float32 whose first pad_top rows of every frame are zero (bev_vgg_pyramid.py:58 pads the BEV map by four rows)
 * -- read in place by the first layer, no copy into the extractor's buffer (a pipeline that double-buffers its
 * inputs writes them straight into two such buffers). */
int dodt_extractor_forward_padded(dodt_extractor* ex, const float* d_x0, float* d_feat_out,
                                  float* d_bottleneck_out);
/* Until further notice (d_x0 = NULL: back to its own buffer) forwards without an input argument read d_x0, laid out
 * as above, as the extractor's input buffer; d_x0 must outlive that use (tools: stand-alone timing on a pipeline's inputs). */
int dodt_extractor_set_input(dodt_extractor* ex, const float* d_x0);
/* Input support of an fp32 pyramid extractor: mask (rows = pad_top + in_h, cols = in_w bytes, host memory, e.g.
 * dodt_bev_support_mask) is nonzero wherever some input frame may be nonzero; every input it marks 0 is zero in
 * every frame.  The mask is propagated through the net (3x3 convs dilate by 1, pools OR their 2x2 windows,
 * transposed convs dilate by 2 at the output resolution, concat ORs), and each layer's work items whose outputs all
 * lie where no input reaches are dropped from its launches (table order kept).  Skipped outputs are not rewritten:
 * they keep the input-independent values of a full forward.  So the first forward after this call or after any
 * dodt_extractor_set_layer runs full tables, and pyramid_fusion1 runs full tables for every (d_feat_out,
 * d_bottleneck_out) pair it has not written since then (pairs are told apart by address: a caller that frees
 * and reallocates its output buffers calls this again); the caller must not write those buffers itself.  mask NULL:
 * full tables again.  The bf16 / split conv paths and DODT_EXTRACTOR_VGG keep full tables (the call only checks the
 * sizes).  *skipped_items (may be NULL): work items dropped per forward in steady state. */
int dodt_extractor_set_input_support(dodt_extractor* ex, const uint8_t* mask, int rows, int cols,
                                     long long* skipped_items);
/* Per-frame tables for an extractor with an input support set (on = 0: the static skip tables again).  Every forward
 * then builds its tables on the device, ahead of the layers on the extractor's stream and without a host round trip:
 * the non-zero cells of the input map (any channel) as a bit mask per frame, propagated by the same geometry at cell
 * resolution, keep the items of each skip table this input reaches, in the table's order; the kernels read the item
 * count from device memory.  A launch computes these items.  The items the last forward into the same buffer reached
 * and this one does not are restored: one launch ahead of the first layer copies their outputs (a conv tile's channels
 * and its pooled tile, a transposed conv's 2 TH x 2 TW outputs, the NHWC rows of the caller's feature / bottleneck
 * pair) from a constants store, one frame of every layer buffer and of the output pair as a forward on a zero input
 * writes them.  The store is taken by the first forward that restores and again after a dodt_extractor_set_layer (that
 * forward waits for the stream), and freed with the tables.  After every forward each layer buffer holds what a
 * forward on full tables would have written.  The forwards that run full tables (see
 * above) record their input's items the same way; pyramid_fusion1 keeps the items per remembered output pair.
 * *enabled (may be NULL): 1 if the tables are on; 0 if the extractor has no skip tables or runs F(4x4,3x3) layers
 * (DODT_CONV_WINO=4: those reach block-wise), which keeps the static tables.  dodt_extractor_set_input_support
 * turns the per-frame tables off again.  While they are on, dodt_extractor_flops / _mfma_flops / _bytes wait for
 * the stream and count the items of the last finished forward. */
int dodt_extractor_set_frame_tables(dodt_extractor* ex, int on, int* enabled);
/* The work items each layer of the last forward touched from per-frame tables, computed or restored (waits for the
 * stream): items[layer] in launch order, n >= dodt_extractor_layer_count(); -1 for a layer that ran a full or static
 * table. */
int dodt_extractor_frame_items(dodt_extractor* ex, int* items, int n);
/* The same split: computed[layer] items the layer's kernels ran, restored[layer] items copied back from the constants
 * store (-1 / -1 for a layer that ran a full or static table).  dodt_extractor_flops / _mfma_flops count the
 * computed items, dodt_extractor_bytes also the copies (store read, buffer written). */
int dodt_extractor_frame_split(dodt_extractor* ex, int* computed, int* restored, int n);
/* Device memory the constants store holds (0 before the first forward that restores and after it is freed). */
long long dodt_extractor_store_bytes(const dodt_extractor* ex);
/* Host only: the per-frame rule of dodt_extractor_set_frame_tables on host masks, for one layer (0 .. 15 in launch
 * order) of the pyramid net.  masks: frames x rows x cols bytes, non-zero where the frame's padded input is; items:
 * n_items x {frame, channel tile, y0, x0} in table order, each writing th x tw outputs of the layer's GEMM grid
 * (transposed convs: 2 th x 2 tw outputs); prev (may be NULL): n_items bytes, the items the last forward reached.
 * run (room for n_items x 4 ints) receives the items of this input or of prev, in table order, *n_run their count. */
int dodt_frame_tables_host(const uint8_t* masks, int frames, int rows, int cols, int layer, int th, int tw,
                           const int* items, int n_items, const uint8_t* prev, int* run, int* n_run);
/* The two lists a forward takes, each in table order: run = the items of this input (the kernels compute them),
 * restore = the items of prev that are not of this input (copied back from the constants store); both with room for
 * n_items x 4 ints. */
int dodt_frame_lists_host(const uint8_t* masks, int frames, int rows, int cols, int layer, int th, int tw,
                          const int* items, int n_items, const uint8_t* prev, int* run, int* n_run, int* restore,
                          int* n_restore);
/* Host only: the copy the restore launch makes for one item {frame, channel tile, y0, x0} of a table with th x tw
 * tiles (f = 2: a transposed conv's, 2 th x 2 tw outputs from (2 y0, 2 x0)) and bn channels per tile from channel ch0,
 * run by the functions the device runs.  pad_top < 0: dst is a channel-blocked map of frames x [channels / 8][rows]
 * [cols][8] floats, src one frame of it; dst2 / src2 (may both be NULL) the 2x2-pooled maps of the same channels.
 * pad_top >= 0: dst is the NHWC feature map of frames x (rows - pad_top) x cols x channels (row pad_top of the layer's
 * grid is its row 0), src one frame of it, dst2 / src2 (may both be NULL) the bottleneck maps, one float per cell. */
int dodt_frame_restore_host(const int* item, int f, int th, int tw, int bn, int ch0, int rows, int cols, int channels,
                            int pad_top, float* dst, const float* src, float* dst2, const float* src2);
/* Size of the feature map forward() returns: (in_h, in_w, 32) for the pyramid,
 * (in_h / 8 * 4, in_w / 8 * 4, 256) for DODT_EXTRACTOR_VGG. */
int dodt_extractor_output_shape(const dodt_extractor* ex, int* h, int* w, int* c);
/* 1 when conv1_1 runs folded into conv1_2's launch (bf16 conv path, the default there; bev_vgg_pyramid.py:63-66's two convs in
 * one kernel): conv1_1's map is then not stored (dodt_extractor_read_activation refuses it) and its arithmetic is the bf16
 * MFMA's at fp32 grade (x and w as hi + lo bf16 pairs, three MFMAs per product term) instead of the fp32 MFMA's.  0 otherwise
 * (fp32 / split conv paths, or DODT_CONV_BF16_FIRST2=0); a negative DODT_ERR_* code for a NULL extractor. */
int dodt_extractor_first_layers_folded(const dodt_extractor* ex);
/* Debug/test access to an intermediate activation by layer name: copies the
 * (batch, h, w, c) float32 tensor to host memory `dst` (NULL to query shape).  "store:<layer>" reads the constants
 * store of the per-frame tables instead (its one frame for every frame of the batch; "store:pyramid_fusion1" and
 * "store:bottleneck": the store's output pair). */
int dodt_extractor_read_activation(dodt_extractor* ex, const char* name, float* dst,
                                   int* h, int* w, int* c);
/* FLOPs of one forward call (2*M*N*K summed over conv layers, all frames): the ALGORITHMIC
 * count of the direct form, whatever kernel computes a layer.  With skip tables
 * (dodt_extractor_set_input_support) this, dodt_extractor_mfma_flops and dodt_extractor_bytes count the work of a
 * steady-state forward: skipped items are not counted. */
double dodt_extractor_flops(const dodt_extractor* ex);
/* FLOPs the matrix pipe executes for one forward.  The fp32 3x3 stride-1 layers run as Winograd
 * minimal filtering, fp32 throughout: F(4x4,3x3) (36 multiplications per 4x4 outputs and channel pair
 * where the direct form needs 144) or F(2x2,3x3) (16 per 2x2 outputs instead of 36), selected by
 * DODT_CONV_WINO=4|2 in the environment (0: the direct kernels; DESIGN.md 5.0 states the default and
 * each form's distance to the direct result); split mode issues three bf16 MFMAs per product. */
double dodt_extractor_mfma_flops(const dodt_extractor* ex);
/* Algorithmic HBM bytes of one forward (each map and the weights read / written once). */
double dodt_extractor_bytes(const dodt_extractor* ex);
/* What a forward is made of, layer by layer in launch order, and how long each layer's launches
 * took in one forward (a HIP event pair around every layer on the extractor's stream; the call
 * waits for the stream).  bench.py's roofline object is built from this: `kernel` is the
 * __global__ function a rocprofv3 kernel trace lists, flops_executed what the matrix pipe issues
 * for the layer (see dodt_extractor_mfma_flops), bytes the layer's share of dodt_extractor_bytes. */
/* (items, launches, flops and bytes: what that forward ran -- a forward on skip tables reports the kept items.) */
typedef struct dodt_layer_info {
    char name[32];          /* TF variable scope of the layer */
    char kernel[48];
    int32_t launches;       /* 1, or 2 when a tail launch evens out the last round */
    int32_t items;          /* work items (tiles x channel tiles x frames) */
    double flops_direct;    /* 2 M N K of the direct form */
    double flops_executed;
    double bytes;
    float ms;
    int32_t reserved_;
} dodt_layer_info;
int dodt_extractor_layer_count(const dodt_extractor* ex);
/* The kernel-variant table the layers choose from. */
#define DODT_VARIANT_DECONV 0x1       /* transposed conv */
#define DODT_VARIANT_SMALL_CIN 0x2    /* first-layer kernel (4 / 6 input channels) */
#define DODT_VARIANT_TAIL_ONLY 0x4    /* quarter tiles: never a layer's main variant */
#define DODT_VARIANT_BF16 0x8
#define DODT_VARIANT_SPLIT 0x10       /* hi + lo bf16 pairs */
#define DODT_VARIANT_WINO 0x20        /* Winograd, F(2x2,3x3) unless ... */
#define DODT_VARIANT_WINO43 0x40      /* ... F(4x4,3x3) */
#define DODT_VARIANT_DMA 0x80         /* bf16 3x3 kernels with LDS-DMA staging */
#define DODT_VARIANT_DECONV_DMA 0x100 /* transposed conv, LDS-DMA staged */
#define DODT_VARIANT_FIRST2 0x200     /* conv1_1 folded into conv1_2 */
#define DODT_VARIANT_STREAM 0x400     /* producer wave, weights in registers */
#define DODT_VARIANT_XCD_QUEUE 0x800  /* walks one work queue per group of blocks that share an XCD (in this process) */
#define DODT_VARIANT_CAN_POOL 0x1000  /* its epilogue can write the 2x2 max pool behind the layer */
typedef struct dodt_conv_variant {
    int32_t tw, th, bn, ck;  /* output tile (transposed convs: input pixels), channels per tile, channels per chunk */
    int32_t flags;           /* DODT_VARIANT_* */
    int32_t blocks_per_cu;   /* resident workgroups per CU its grids are sized by */
    int32_t lds_bytes;
    int32_t reserved_;
    char kernel[48];         /* the __global__ function */
} dodt_conv_variant;
int dodt_conv_variant_count(void);
int dodt_conv_variant_info(int i, dodt_conv_variant* out);
/* What the host decides about one layer before anything runs: [0] its main launch, [1] its tail launch. */
typedef struct dodt_conv_layer_plan {
    char name[32];
    int32_t h, w, cin, cout; /* the layer's GEMM grid (transposed convs: the input's size) and channels */
    int32_t variant[2];   /* index into the variant table; -1: no such launch */
    int32_t items[2];     /* work items of the full tables */
    int32_t grid[2];      /* workgroups launched for them */
    int32_t pool_fused;   /* the 2x2 max pool behind the layer runs in its epilogue */
    int32_t bneck_fused;  /* pyramid_fusion1: the 1x1 bottleneck runs in its epilogue */
    int32_t folded;       /* conv1_1: computed inside conv1_2's launch (no launch of its own; conv1_2's main variant is then
                           * the folding kernel) */
    int32_t reserved_;
} dodt_conv_layer_plan;
/* Host only: the plan dodt_extractor_create makes for these arguments (kind with its flag bits) on a device of num_cus
 * CUs, in launch order; *n_layers (may be NULL) receives the layer count, out (may be NULL) has room for n_out records.
 * The environment switches of the conv path apply as they do to an extractor of this process. */
int dodt_conv_plan_host(int kind, int in_h, int in_w, int in_c, int pad_top, int batch, int num_cus,
                        dodt_conv_layer_plan* out, int n_out, int* n_layers);
/* The same records from a live extractor. */
int dodt_extractor_layer_plan(const dodt_extractor* ex, dodt_conv_layer_plan* out, int n_out, int* n_layers);
int dodt_extractor_forward_timed(dodt_extractor* ex, const float* d_in, float* d_feat_out,
                                 float* d_bottleneck_out, dodt_layer_info* info, int n_info);

/* ---- a11: ROI crop ------------------------------------------------------------------
 * tf.image.crop_and_resize(image, boxes, box_ind=0, crop_size) call sites
 * models/dt_rpn_model.py:418-428 and models/dt_avod_model.py:253-273.
 * d_image (H,W,C); d_boxes (n,4) [y1,x1,y2,x2] normalised; d_out (n,ch,cw,C);
 * *d_n (may be NULL) overrides n on the device. */
int dodt_crop_and_resize(dodt_ctx* ctx, const float* d_image, int H, int W, int C,
                         const float* d_boxes, int n, const int32_t* d_n, int crop_h,
                         int crop_w, float* d_out);
/* The same with box b's crop written at d_out + b * out_box_stride floats (>= ch*cw*C; the floats
 * between crops are left untouched): the flattened crops become rows of a matrix whose row length is
 * padded for the fully connected layer that reads them (the correlation head's fc6 has K = 7*7*25 =
 * 1225; rows of 1248 zero-padded floats let it run on the LDS-DMA GEMM). */
int dodt_crop_and_resize_strided(dodt_ctx* ctx, const float* d_image, int H, int W, int C,
                                 const float* d_boxes, int n, const int32_t* d_n, int crop_h,
                                 int crop_w, float* d_out, long long out_box_stride);
/* The strided form with a row index: row j of d_out (j < min(n, *d_n)) is the crop at box d_box_idx[j] of the
 * n_boxes boxes -- the gather folded into the crop, no launch of its own.  Same kernel and float expressions:
 * a row is bit-equal to the un-indexed crop of that box.  An index outside [0, n_boxes) gives a zero crop. */
int dodt_crop_and_resize_indexed(dodt_ctx* ctx, const float* d_image, int H, int W, int C,
                                 const float* d_boxes, int n_boxes, const int32_t* d_box_idx, int n,
                                 const int32_t* d_n, int crop_h, int crop_w, float* d_out,
                                 long long out_box_stride);

/* ---- T branch: correlation of the two frames' BEV feature maps ------------------------
 * Stands behind avod/core/corr_layers/correlation.py:7-27 -> the Correlation custom op
 * (avod/core/ops/correlation/correlation_op.cc:53-62, kernel correlation_kernel.cu.cc:
 * 21-119, padding pad.cu.cc:14-73) with kernel_size 1 and stride_1 1.
 * d_a, d_b: (H,W,C) float32, C = 32; d_out: (H+2*pad-2*max_displacement,
 * W+2*pad-2*max_displacement, (2*(max_displacement/stride_2)+1)^2). */
int dodt_correlation(dodt_ctx* ctx, const float* d_a, const float* d_b, int H, int W, int C,
                     int max_displacement, int stride_2, int pad, float* d_out);
/* The map at the tiles a set of crops reads, for callers that read the map through those crops only (the T
 * branch at the kept detections).
 * dodt_correlation_tile_list: one launch.  For boxes d_box_idx[0 .. min(n, *d_n)) of d_boxes (n_boxes, 4) -- or
 * boxes 0.. when d_box_idx is NULL -- flags the 16 x 16 tiles of the (OH, OW) map that meet the pixel rectangle a
 * crop_h x crop_w crop of the box can read (floor of the smallest sample coordinate to floor of the largest + 1,
 * clipped to the map, one pixel wider on every side; the coordinates are the crop kernel's own), and writes them
 * to d_tiles (capacity >= the map's tile count) in the order the kernel walks the full map, their number to
 * *d_n_tiles.
 * dodt_correlation_tiles: dodt_correlation over d_tiles[0 .. min(capacity, *d_n_tiles)) only.  A listed tile is
 * bit-equal to the full map's; nothing is written outside the listed tiles.  Only the configuration's grid
 * (stride_2 2, max_displacement / stride_2 == 2); anything else is DODT_ERR_UNSUPPORTED. */
int dodt_correlation_tile_list(dodt_ctx* ctx, int OH, int OW, const float* d_boxes, int n_boxes,
                               const int32_t* d_box_idx, int n, const int32_t* d_n, int crop_h, int crop_w,
                               int32_t* d_tiles, int capacity, int32_t* d_n_tiles);
int dodt_correlation_tiles(dodt_ctx* ctx, const float* d_a, const float* d_b, int H, int W, int C,
                           int max_displacement, int stride_2, int pad, const int32_t* d_tiles, int capacity,
                           const int32_t* d_n_tiles, float* d_out);

/* ---- dense heads: fully connected layers (fp32 MFMA) ------------------------------------
 * y[M][N] = act(x[M][K] . w[K][N] + bias[N]); stands behind slim.fully_connected / the 1x1
 * and VALID 3x3 slim.conv2d of the heads: avod/core/models/dt_rpn_model.py:445-537 (anchor
 * predictor), avod/core/avod_fc_layers/fusion_fc_layers.py:136-180 (early fusion heads),
 * avod/builders/avod_corr_layers_builder.py (correlation offsets head).
 * w: host, row-major (K,N) = the TF variable's layout (conv kernels reshaped to (kh*kw*cin,
 * cout)); relu != 0 applies ReLU.  d_x2 (may be NULL): x = (x + x2) / 2, the "mean" fusion
 * of BEV and image crops.  ldx, ldy: row strides in floats; *d_m (may be NULL) overrides M
 * on the device.  ctx == NULL in forward uses the creating context's stream. */
/* d_out[r][k] = (d_a[r][k] + d_b[r][k]) / 2 for r < min(*d_n, rows): the "mean" fusion of the BEV and
 * image crops (avod/core/avod_fc_layers/avod_fc_layer_utils.py:38-41, dt_rpn_model.py:434-439 with
 * both path-drop masks 1) as a pass of its own, in front of a layer that then runs without d_x2 (the
 * GEMM with the fusion inside its K loop is half as fast at the stage-2 head's size).  row_floats a
 * multiple of 4, blocks 16-byte aligned and contiguous. */
int dodt_mean_fusion(dodt_ctx* ctx, const float* d_a, const float* d_b, int rows, const int32_t* d_n,
                     int row_floats, float* d_out);
typedef struct dodt_fc dodt_fc;
int dodt_fc_create(dodt_ctx* ctx, int K, int N, const float* w, const float* bias, int relu,
                   dodt_fc** out);
/* flags: DODT_FC_RELU; DODT_FC_BF16 = x rounded to bf16 on load, weights stored as bf16,
 * bf16 MFMA with fp32 accumulation, bias + activation and the output in fp32 (the heads'
 * counterpart of DODT_EXTRACTOR_BF16; not the reference's arithmetic). */
#define DODT_FC_RELU 1
#define DODT_FC_BF16 2
int dodt_fc_create_ex(dodt_ctx* ctx, int K, int N, const float* w, const float* bias, int flags,
                      dodt_fc** out);
int dodt_fc_destroy(dodt_fc* fc);
int dodt_fc_forward(dodt_fc* fc, dodt_ctx* ctx, const float* d_x, const float* d_x2, int ldx,
                    int M, const int32_t* d_m, float* d_y, int ldy);
/* A layer whose columns go to `parts` (1..3) dense arrays d_ys[p] of (M, widths[p]) floats, widths summing to
 * the layer's N: the output layers of a head (fusion_fc_layers.py:94-133 build_output_layers: cls | offsets |
 * angle vectors from the same fc_drop) created as ONE layer with concatenated weights and run as one launch.
 * Layers with N <= 32, K a multiple of 16 and 16-byte aligned rows (ldx % 4 == 0); else
 * DODT_ERR_UNSUPPORTED. */
int dodt_fc_forward_split(dodt_fc* fc, dodt_ctx* ctx, const float* d_x, int ldx, int M, const int32_t* d_m,
                          int parts, const int* widths, float* const* d_ys);
/* bf16 heads with bf16 activations in HBM (round 4).  A DODT_FC_BF16 layer also takes input rows that are
 * ALREADY bf16 (ldx in elements; dodt_fc_bf16_row_elems(fc) of them per row, zeros beyond K; 0 = no such path for
 * this layer) and writes bf16 rows (y_bf16 != 0, ldy in elements; rounded to nearest even -- the rounding the next
 * layer's load would apply, so the arithmetic is the one of dodt_fc_forward on DODT_FC_BF16 layers) or float32.
 * Layers with N % 128 == 0 and K >= 128 (both operands staged by LDS-DMA), and the output layers dodt_fc_forward_split
 * takes (float32 output).  dodt_rows_to_bf16 makes the first layer's rows: bf16((a + b) / 2) -- the heads' mean
 * fusion, avod_fc_layer_utils.py:38-41 -- or bf16(a) when d_b is NULL, zero tail up to out_ld. */
int dodt_fc_bf16_row_elems(const dodt_fc* fc);
int dodt_fc_forward_bf16(dodt_fc* fc, dodt_ctx* ctx, const void* d_x_bf16, int ldx, int M, const int32_t* d_m,
                         void* d_y, int ldy, int y_bf16);
int dodt_fc_forward_split_bf16(dodt_fc* fc, dodt_ctx* ctx, const void* d_x_bf16, int ldx, int M, const int32_t* d_m,
                               int parts, const int* widths, float* const* d_ys);
int dodt_rows_to_bf16(dodt_ctx* ctx, const float* d_a, const float* d_b, int rows, const int32_t* d_n,
                      int row_floats, int in_ld, void* d_out_bf16, int out_ld);
double dodt_fc_flops(const dodt_fc* fc, int M);
/* Which kernel a call of a layer runs.  One selector decides it from the layer's (K, N, flags) and the call's strides,
 * pointer alignments and row types; these two entries report its answer and launch nothing. */
#define DODT_FC_FORM_NONE 0              /* bf16 rows that no kernel of the layer reads: the call is refused */
#define DODT_FC_FORM_SMALLK 1            /* K <= 16, N >= 64, N % 4 == 0: vector ALU */
#define DODT_FC_FORM_SKINNY 2            /* N <= 32, K % 16 == 0: K split over the waves */
#define DODT_FC_FORM_SKINNY_BF16 3
#define DODT_FC_FORM_SKINNY_BF16_ROWS 4
#define DODT_FC_FORM_DMA_NT1 5           /* fp32, LDS-DMA staged, 64 x 64 tiles */
#define DODT_FC_FORM_DMA_NT2 6           /* ... 64 x 128 tiles */
#define DODT_FC_FORM_DMA_FUSED 7         /* ... the mean of two inputs inside */
#define DODT_FC_FORM_BF16_ROWS_DMA32 8   /* bf16 rows, LDS-DMA staged, 32-k stages */
#define DODT_FC_FORM_BF16_ROWS_DMA64 9   /* ... 64-k stages */
#define DODT_FC_FORM_TILED_64X128 10     /* register-staged */
#define DODT_FC_FORM_TILED_128X32 11
#define DODT_FC_FORM_TILED_64X128_BF16 12
#define DODT_FC_FORM_TILED_128X32_BF16 13
typedef struct dodt_fc_plan {
    int32_t form;           /* DODT_FC_FORM_* */
    char name[24];          /* the form's name in the selector, "kDmaNt1" */
    int32_t xvec, fuse;     /* register-staged forms: x loaded as float4 (else by element); the mean of x and x2 inside */
    int32_t vec_store;      /* DODT_FC_FORM_SMALLK: rows stored 16 bytes at a time (ldy % 4 == 0), else by element */
    int32_t y_bf16;         /* DODT_FC_FORM_BF16_ROWS_DMA*: the output rows are bf16 */
    int32_t grid[2];        /* workgroups of the launch, before *d_m cuts rows; 0, 0 for DODT_FC_FORM_NONE */
    /* what (K, N, flags) alone decide: padded sizes, the width the weights are blocked for, the bf16-row image */
    int32_t Kp, BN, Npad, Kd, dma_bk;
    int32_t skinny, dma, smallk, plain, bf16_rows;
} dodt_fc_plan;
/* Host only, touches no device.  x_off, x2_off, y_off: the addresses of x, x2 and y modulo 16 (x2_off < 0: no second
 * input; the split entries have no y: 0).  x_bf16: the rows are bf16 (dodt_fc_forward_bf16 and its split form), ldx in
 * elements.  bf16_bk: the stage depth the bf16-row weights are blocked for, 32 or 64 (DODT_FC_BF16_DMA_BK in the
 * process that creates the layer). */
int dodt_fc_plan_host(int K, int N, int flags, int M, int ldx, int ldy, int x_off, int x2_off, int y_off, int x_bf16,
                      int y_bf16, int bf16_bk, dodt_fc_plan* out);
/* The same record for a built layer and a call's real pointers (d_x2, d_y may be NULL). */
int dodt_fc_form(const dodt_fc* fc, const void* d_x, const void* d_x2, int ldx, int M, const void* d_y, int ldy,
                 int x_bf16, int y_bf16, dodt_fc_plan* out);

/* ---- a13: NMS -------------------------------------------------------------------------
 * tf.image.non_max_suppression(boxes, scores, max_output_size, iou_threshold),
 * call sites models/dt_rpn_model.py:587-591 and models/dt_avod_model.py:606-613.
 * Candidate order is (score descending, index ascending) -- TF leaves ties
 * unspecified.  d_sel_out: (max_out) int32 selected ORIGINAL indices in score
 * order; d_count_out: (1) int32.  *d_n (may be NULL) overrides n.
 * Scores of rows below *d_n must not be NaN (TF's comparator is undefined there); rows from *d_n on are never read. */
int dodt_nms(dodt_ctx* ctx, const float* d_boxes, const float* d_scores, int n,
             const int32_t* d_n, int max_out, float iou_threshold, int32_t* d_sel_out,
             int32_t* d_count_out);
/* What dodt_nms decides on the host for (n, max_out) before anything runs; all zero where it launches nothing
 * (n == 0 or max_out == 0). */
typedef struct dodt_nms_plan {
    int32_t n_pad;          /* keys: n rounded up to a power of two */
    int32_t nb, n_rows;     /* 64-box blocks, and the rows they hold */
    int32_t ranked;         /* 1: the order comes from counted ranks, 0: from the bitonic sort */
    int32_t sort_tiles;     /* bitonic sort: LDS tiles (workgroups of its local launches); 0 if ranked */
    int32_t first_rows, later_rows;     /* rows of the first chunk and of the chunks behind it (the last may be shorter) */
    int32_t chunk_rows;     /* the largest chunk: rows of the suppression matrix in the scratch */
    int32_t n_chunks;       /* mask + scan launch pairs */
    int32_t scan_lds_bytes; /* dynamic LDS of the scan */
    int64_t scratch_bytes;  /* what the call reserves in the context's NMS scratch */
} dodt_nms_plan;
/* Host only, touches no device: the plan dodt_nms launches from.  chunks (may be NULL with n_chunks_out 0) receives
 * (row0, rows) of the first n_chunks_out chunks, in launch order. */
int dodt_nms_plan_host(int n, int max_out, dodt_nms_plan* plan, int32_t* chunks, int n_chunks_out);
/* Bytes of the context's NMS scratch: 0 before the first call; a call whose plan needs more than there is replaces it
 * by one of scratch_bytes and a quarter more, rounded up to 256. */
long long dodt_nms_scratch_bytes(const dodt_ctx* ctx);

/* ---- a12/a14: box encoders (TF branch, float32) ------------------------------------------ */
/* anchor_encoder.offset_to_anchor (avod/core/anchor_encoder.py:99-150) */
int dodt_offset_to_anchor(dodt_ctx* ctx, const float* d_anchors, const float* d_offsets,
                          int n, const int32_t* d_n, float* d_out);
/* 2-way softmax, column 1 (models/dt_rpn_model.py:581-584) */
int dodt_softmax_fg(dodt_ctx* ctx, const float* d_logits2, int n, const int32_t* d_n,
                    float* d_scores_out);
/* One launch for the three elementwise steps between the RPN head and NMS #1 (models/dt_rpn_model.py:560-591):
 * dodt_offset_to_anchor (-> d_regressed_out (n,6)), dodt_project_anchors_f32's normalised BEV boxes of the regressed anchors
 * (-> d_bev_norm_tf_out (n,4)) and dodt_softmax_fg (-> d_scores_out (n)) -- the same arithmetic, value for value. */
int dodt_rpn_decode(dodt_ctx* ctx, const float* d_anchors, const float* d_offsets, const float* d_logits2, int n,
                    const int32_t* d_n, const float bev_extents[4], float* d_regressed_out,
                    float* d_bev_norm_tf_out, float* d_scores_out);
/* ... for the two behind NMS #1 (models/dt_rpn_model.py:593-612, dt_avod_model.py:176-200): dodt_gather_rows of the kept
 * proposals (width 6 -> d_rows_out (n,6)) and their dodt_project_anchors_f32 boxes in both views. */
int dodt_gather_project(dodt_ctx* ctx, const float* d_src, const int32_t* d_idx, int n, const int32_t* d_n,
                        const float bev_extents[4], const float p2[12], float im_w, float im_h,
                        float* d_rows_out, float* d_bev_norm_tf_out, float* d_img_norm_tf_out);
/* ... and for the four behind the stage-2 head (models/dt_avod_model.py:520-548,600-634): dodt_box_4c_decode,
 * dodt_max_fg_logit of the two-class logits (-> d_nms_scores_out), dodt_softmax_fg (-> d_det_scores_out) and, with
 * d_angle_vectors, dodt_angle_vector_to_orientation (-> d_orientations_out; both NULL for box_4c). */
int dodt_final_decode(dodt_ctx* ctx, const float* d_top_anchors, const float* d_offsets, const float* d_cls_logits2,
                      const float* d_angle_vectors, int n, const int32_t* d_n, const float plane[4],
                      const float bev_extents[4], float* d_boxes_3d_out, float* d_pred_anchors_out,
                      float* d_bev_tf_out, float* d_nms_scores_out, float* d_det_scores_out,
                      float* d_orientations_out);
/* out[i] = src[idx[i]] rows of `width` floats (tf.gather call sites
 * dt_rpn_model.py:593-597, dt_avod_model.py:616-640) */
int dodt_gather_rows(dodt_ctx* ctx, const float* d_src, int width, const int32_t* d_idx,
                     int n, const int32_t* d_n, float* d_out);
/* NMS #2 score: max over the non-background logits, column 1.. of (n,n_cls)
 * (models/dt_avod_model.py:606: tf.reduce_max(all_cls_logits[:, 1:], axis=1)) */
int dodt_max_fg_logit(dodt_ctx* ctx, const float* d_logits, int n_cls, int n,
                      const int32_t* d_n, float* d_scores_out);
/* tf_angle_vector_to_orientation (avod/core/orientation_encoder.py:20-34; call site
 * models/dt_avod_model.py:547-548): atan2(y, x) of the stage-2 head's `ang_out` rows [x, y]
 * (box_4ca: avod/core/avod_fc_layers/avod_fc_layer_utils.py:11-17).  d_angle_vectors (n,2),
 * d_orientations_out (n,). */
int dodt_angle_vector_to_orientation(dodt_ctx* ctx, const float* d_angle_vectors, int n,
                                     const int32_t* d_n, float* d_orientations_out);
/* Detection record of one frame, the 17 columns the evaluator writes per box
 * (get_avod_predicted_boxes_3d_and_scores, avod/core/dt_evaluator.py:1134-1259): box_3d(7),
 * score, class index, the box shifted by the correlation head's offsets (x += dx, z += dz,
 * ry += dry; d_corr_offsets (n,3), frame 0 of a pair) or 7 zeros (d_corr_offsets NULL:
 * frame 1), frame mark.
 * d_orientations (n,) (may be NULL = box_4c): box_4ca's correction of each selected box by
 * the regressed angle (:1166-1212) -- difference wrapped to [-pi, pi], l/w swapped and ry
 * +-pi/2 when it lies in (pi/4, 3pi/4), ry + pi when |difference| >= 3pi/4, ry wrapped above
 * pi -- applied before the correlation shift, exactly as the evaluator orders them.
 * Rows d_sel[0..*d_count) of boxes_3d / scores / orientations (the tf.gather by nms_indices,
 * models/dt_avod_model.py:616-640); remaining rows of the (max_det,17) output are zeroed;
 * d_count_out[0] = *d_count. */
int dodt_pack_detections(dodt_ctx* ctx, const float* d_boxes_3d, const float* d_scores,
                         const float* d_orientations, const float* d_corr_offsets,
                         const int32_t* d_sel, const int32_t* d_count, int max_det,
                         float frame_mark, float* d_rec_out, int32_t* d_count_out);
/* The same with one row of offsets per detection: d_det_offsets (max_det, 3), row j belongs to box d_sel[j]
 * (the correlation head run at the kept detections only). */
int dodt_pack_detections_compact(dodt_ctx* ctx, const float* d_boxes_3d, const float* d_scores,
                                 const float* d_orientations, const float* d_det_offsets,
                                 const int32_t* d_sel, const int32_t* d_count, int max_det,
                                 float frame_mark, float* d_rec_out, int32_t* d_count_out);
/* ---- several classes (n_cls = number of classes + 1, column 0 the background; 2 <= n_cls <= 8, anything else is
 * DODT_ERR_INVALID).  A model for classes ['Pedestrian', 'Cyclist'] has n_cls == 3
 * (avod/configs/pyramid_people_example.config).  The entries above are the n_cls == 2 forms and stay as they are. ----
 * Record score and type of n rows of d_logits (n, n_cls) as the evaluator takes them from the softmax
 * (avod/core/dt_evaluator.py:1226-1255): per row a float32 tf.nn.softmax -- the row's maximum subtracted, the
 * exponentials summed in column order 0..n_cls-1, each divided by that sum --, d_scores_out (n) its largest
 * non-background value and d_types_out (n) int32 that value's index among the non-background columns: np.argmax of
 * softmax[:, 1:], so the FIRST maximum, taken over the float32 softmax values and not over the logits.  Rows at and
 * past min(n, *d_n) are left untouched. */
int dodt_class_scores(dodt_ctx* ctx, const float* d_logits, int n_cls, int n, const int32_t* d_n,
                      float* d_scores_out, int32_t* d_types_out);
/* dodt_final_decode for d_cls_logits (n, n_cls): one launch gives the box_4c decode (the same device functions), the
 * NMS #2 score -- the largest non-background LOGIT, NMS #2 is class-agnostic (models/dt_avod_model.py:606) --, the
 * score and type of dodt_class_scores (-> d_det_scores_out (n), d_det_types_out (n) int32) and the orientation.  At
 * n_cls == 2 every float output is byte-equal to dodt_final_decode's and the types are 0. */
int dodt_final_decode_classes(dodt_ctx* ctx, const float* d_top_anchors, const float* d_offsets,
                              const float* d_cls_logits, int n_cls, const float* d_angle_vectors, int n,
                              const int32_t* d_n, const float plane[4], const float bev_extents[4],
                              float* d_boxes_3d_out, float* d_pred_anchors_out, float* d_bev_tf_out,
                              float* d_nms_scores_out, float* d_det_scores_out, int32_t* d_det_types_out,
                              float* d_orientations_out);
/* dodt_pack_detections / dodt_pack_detections_compact with the record's class index, column 8: (float)d_types[d_sel[row]],
 * d_types (n,) int32 as dodt_class_scores writes them.  d_types NULL: column 8 is 0, the result of the entries above. */
int dodt_pack_detections_classes(dodt_ctx* ctx, const float* d_boxes_3d, const float* d_scores, const int32_t* d_types,
                                 const float* d_orientations, const float* d_corr_offsets, const int32_t* d_sel,
                                 const int32_t* d_count, int max_det, float frame_mark, float* d_rec_out,
                                 int32_t* d_count_out);
int dodt_pack_detections_compact_classes(dodt_ctx* ctx, const float* d_boxes_3d, const float* d_scores,
                                         const int32_t* d_types, const float* d_orientations,
                                         const float* d_det_offsets, const int32_t* d_sel, const int32_t* d_count,
                                         int max_det, float frame_mark, float* d_rec_out, int32_t* d_count_out);
/* Stage-2 decode (models/dt_avod_model.py:464-469,575-603):
 *   anchors_to_box_3d(fix_lw) -> tf_box_3d_to_box_4c -> + offsets ->
 *   tf_box_4c_to_box_3d -> tf_box_3d_to_anchor -> project_to_bev (metres) ->
 *   reorder.  (avod/core/box_3d_encoder.py:188-322, box_4c_encoder.py:85-165,
 *   369-484.)  d_top_anchors (n,6), d_offsets (n,10), plane[4] host.
 * Outputs: d_boxes_3d_out (n,7), d_pred_anchors_out (n,6), d_bev_tf_out (n,4)
 * [z1,x1,z2,x2] metres (the NMS #2 boxes).  Any output may be NULL. */
int dodt_box_4c_decode(dodt_ctx* ctx, const float* d_top_anchors, const float* d_offsets,
                       int n, const int32_t* d_n, const float plane[4],
                       const float bev_extents[4], float* d_boxes_3d_out,
                       float* d_pred_anchors_out, float* d_bev_tf_out);

/* ---- (f) temporal module "M" of S+T+M: the frames between two keyframes --------------------
 * The detector runs on keyframes t and t + tau only; the frames in between get their detections by
 * associating the two keyframes' detections by 3-D IoU and interpolating every track
 * (avod/core/dt_evaluator_stride.py:304-313 -> dt_evaluator_utils.py:212-362,
 * interpolate_non_keyframe_predicitons + interpolate_trajectory; the host form is
 * dodt_amd/core/dt_evaluator_utils.py).  Float64 throughout.
 *
 * 3-D IoU of every box of d_a (na,7) with every box of d_b (nb,7), [x,y,z,l,w,h,ry] doubles (y = bottom,
 * down positive), into d_iou_out (na,nb): bounding-sphere early exit (exactly 0), height overlap times the
 * exact overlap of the two bases (Sutherland-Hodgman) -- the reference rasterises that overlap at 1 cm
 * (wavedata/wavedata/tools/core/evaluation.py:60-75,182-261). */
int dodt_three_d_iou_matrix(dodt_ctx* ctx, const double* d_a, int na, const double* d_b, int nb,
                            double* d_iou_out);
/* One workgroup per pair.  d_records (n_pairs, 2, max_det, 17): keyframe f of a pair is slot f, the
 * pipeline's record layout, float32 (records_f64 = 0) or float64 (1), widened to float64 first;
 * d_counts (n_pairs, 2) valid rows per slot.  Rows with score (column 7) > threshold take part, in order.
 * n_frames (1..64): frames from keyframe 0 to keyframe 1 inclusive (tau + 1); 1 and 2 keep the
 * reference's short-cuts (no association).  on_conflict: DODT_CONFLICT_RAISE -- a keyframe-0 detection
 * whose best match is already taken sets d_status[pair] = 1 and that pair's counts to 0 (the reference's
 * next_idx.remove raises, dt_evaluator_utils.py:266-268); DODT_CONFLICT_NEXT_BEST -- its best still-free
 * match instead.  d_recover (n_pairs, n_frames, 13) or NULL (= identity): per pair and frame
 * [trans(3), inv(matrix) (3x3 row-major), delta] of recovery_coordinate (dt_evaluator_utils.py:189-210,
 * kitti_tracking_dataset.py:374-389), applied to frames 1..n_frames-1; calib (host, 42 doubles):
 * inv(R0_rect) (3x3), inv(Tr_velo_to_cam) (3x4), Tr_velo_to_cam (3x4), R0_rect (3x3), read before the call
 * returns.  Outputs: d_out (n_pairs, n_frames, max_out, 13) -- the records' first 13 columns, matched and
 * unmatched keyframe-0 tracks in order, then the unmatched keyframe-1 ones --, d_out_counts (n_pairs,
 * n_frames), d_status (n_pairs).  max_det <= 128, max_out >= 2 * max_det.  For n_frames >= 3 two launches: the
 * IoU of every row pair over the whole chip into a workspace the context keeps, then one workgroup per pair. */
#define DODT_CONFLICT_RAISE 0
#define DODT_CONFLICT_NEXT_BEST 1
int dodt_interpolate_pairs(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                           int n_pairs, int max_det, int n_frames, double threshold, int on_conflict,
                           const double* d_recover, const double* calib, int max_out, double* d_out,
                           int32_t* d_out_counts, int32_t* d_status);
/* The same with one calibration per pair: d_calibs (n_pairs, 42) float64 on the device, row p the 42 doubles
 * above for pair p (pairs of one launch that come from different videos).  Needs d_recover, the only reader of
 * a calibration.  The same kernels and arithmetic: with equal rows the outputs are the bytes
 * dodt_interpolate_pairs writes for that calibration; the rows are read when the launch runs. */
int dodt_interpolate_pairs_calibs(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                                  int n_pairs, int max_det, int n_frames, double threshold, int on_conflict,
                                  const double* d_recover, const double* d_calibs, int max_out, double* d_out,
                                  int32_t* d_out_counts, int32_t* d_status);

/* ---- (g) the IoU tracker of the temporal module: detections -> tracks ------------------------
 * The reference's tracking evaluation turns each pair's records into KITTI label rows
 * (encoder_tracking_dets) and links them across pairs (track_through_ious,
 * avod/core/dt_evaluator_utils.py:368-511); the host form is dodt_amd/core/dt_evaluator_utils.py
 * encode_tracking_dets + track_through_ious, reproduced with its quirks.  The tracker state of one
 * sequence lives in a device buffer the caller allocates (d_state): the active tracks, the counters,
 * the previous non-skipped pair's encoded rows, then a list of finished tracks and a log of every
 * detection that entered a track, log_capacity entries each.  A log or finish list that would run
 * past log_capacity sets the state's status word and is not written.  Nothing is downloaded: the
 * caller reads the buffer when it wants the tracks (layout: dodt_amd/tracking.py).
 *
 * Bytes of a state buffer with room for log_capacity (>= 1) log entries and finished tracks. */
int dodt_track_state_bytes(int log_capacity, size_t* bytes);
/* Start a sequence: empty state, capacity log_capacity (the value the buffer was sized for). */
int dodt_track_reset(dodt_ctx* ctx, void* d_state, int log_capacity);
/* The end of the sequence (track_through_ious' last statement): every active track with max_score >=
 * high_threshold (compared in float32) and length >= t_min is finished, in order; the active list is
 * emptied. */
int dodt_track_flush(dodt_ctx* ctx, void* d_state, double high_threshold, int t_min);
/* kitti_label_table of n_pairs record pairs, one workgroup per pair, without tracking.  d_records
 * (n_pairs, 2, max_det, 17) float32 (records_f64 = 0) or float64 (1), cast to float32 and widened to
 * float64 as the host does; d_counts (n_pairs, 2) valid rows per slot; max_det <= 128.  Rows with
 * score >= score_threshold are projected with p2 (host, 12 doubles, read before the call returns), the
 * truncation rules applied against image_w x image_h, rounded to 3 decimals and stored as float32.
 * Outputs, rows compacted in record order: d_track_out (n_pairs, 128, 23) -- the keyframe-0 row
 * [class, 0, 0, -10, x1, y1, x2, y2, h, w, l, x, y, z, ry, score] in cols 0..15 and cols 8..14 of the
 * shifted box's own row (record cols 9..15) in cols 16..22, zipped by position --; d_ious_out
 * (n_pairs, 128, 16), the keyframe-1 rows; d_counts_out (n_pairs, 4): [track items (the shorter of the
 * two keyframe-0 lists), keyframe-1 rows, skip (both keyframes empty), keyframe-0 rows]. */
int dodt_track_encode(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                      int n_pairs, int max_det, const double* p2, double image_w, double image_h,
                      double score_threshold, float* d_track_out, float* d_ious_out, int32_t* d_counts_out);
/* Encode and track n_pairs pairs of one sequence, in order, continuing the state: the encoding of
 * dodt_track_encode, then per non-skipped pair the merge, the greedy walk (argmax over the free
 * columns, a match needs IoU > iou_threshold), the finish rule (max_score >= high_threshold, length >=
 * t_min) and the new tracks.  Three launches per 16 pairs, all on ctx's stream: the encoding (one
 * workgroup per pair), every IoU the walk can read (float64, over the whole chip, into a workspace the
 * context keeps) and the walk (one workgroup). */
int dodt_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                     const int32_t* d_counts, int n_pairs, int max_det, const double* p2, double image_w,
                     double image_h, double score_threshold, double high_threshold, double iou_threshold,
                     int t_min);
/* Lanes: several sequences (videos, cameras) advance by one pair each in one call.  The distance in bytes
 * between two lanes' states in one buffer: dodt_track_state_bytes(log_capacity) rounded up to a multiple
 * of 256.  Needs no context. */
int dodt_track_lanes_stride(int log_capacity, size_t* stride);
/* Pair i of the batch belongs to lane i.  Lane i's state is the ordinary state layout at d_states +
 * i * stride (dodt_track_reset, dodt_track_flush and the host's reader work on that address unchanged);
 * d_records (n_lanes, 2, max_det, 17) and d_counts (n_lanes, 2) are one step's records, lane i consuming
 * pair i.  Host arrays, all read before the call returns: active, n_lanes bytes (non-zero: the lane takes
 * its pair) or NULL for every lane; p2s (n_lanes, 12) and image_whs (n_lanes, 2) doubles, lane i's
 * projection and image size.  For every active lane the live parts of its state afterwards -- the header,
 * act[0:n_active], prev_off[0:prev_nL], prev_k1[0:prev_n1], fin[0:n_fin], log[0:n_log] -- are byte for
 * byte what dodt_track_pairs(ctx, d_states + i * stride, pair i, n_pairs = 1, p2s[i], image_whs[i], ...)
 * leaves, the skip rule (both keyframes empty: seq_pair advances, nothing else) and the overflow status
 * included; of an inactive lane no byte is written; nothing of one lane reaches another.  Three launches
 * per 16 lanes on ctx's stream, in the workspaces dodt_track_pairs uses: the encoding (one workgroup per
 * lane, the lanes' calibrations by value in the kernel arguments), the IoU tables (each lane a batch of
 * one pair against its own state) and the walk (one workgroup per lane, the body dodt_track_pairs runs). */
int dodt_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes, const unsigned char* active,
                     const void* d_records, int records_f64, const int32_t* d_counts, int max_det,
                     const double* p2s, const double* image_whs, double score_threshold,
                     double high_threshold, double iou_threshold, int t_min);
/* Track only, from lists already encoded (the host-array form): d_track (n_pairs, max_rows, 23) and
 * d_ious (n_pairs, max_rows, 16) float32 in dodt_track_encode's layout (only the box cols 8..14, the
 * score col 15 and the offsets cols 16..22 are read; the log copies cols 0..15), d_counts (n_pairs, 2):
 * [track items, keyframe-1 rows].  Pair k's keyframe-1 rows are dets_for_ious[k + 1] of
 * track_through_ious.  No pair is skipped; max_rows <= 128. */
int dodt_track_encoded(dodt_ctx* ctx, void* d_state, const float* d_track, const float* d_ious,
                       const int32_t* d_counts, int n_pairs, int max_rows, double high_threshold,
                       double iou_threshold, int t_min);

/* ---- (h) the Kalman-filter tracker: keyframes -> tracks of filtered positions -----------------
 * The reference's second video-level tracker (avod/experiments/video_detection_kf.py kf_pipeline with
 * avod/utils/kalman_tracker.py); the host form is dodt_amd/experiments/video_detection_kf.py.  Per
 * keyframe: the detections with score >= sigma_l; the float32 matrix of 3-D IoUs between every live
 * track's last detection and every detection moved into the track's frame by the ego-motion; the optimal
 * assignment (maximum total IoU) and the gate (an assigned pair with IoU < iou_threshold is unmatched on
 * both sides); predict + update of the matched tracks with the measurement [x, y, z, z]; a new track per
 * unmatched detection (those no track was assigned to, ascending, then the gate-failed ones in ascending
 * track order; ids count from 0); the unmatched tracks coast (predict; a virtual detection at the
 * predicted position, or the end of the track once its last detection lies outside the camera's wedge);
 * tracks with no_losses > max_age leave, those with hits >= min_hits into the finished list.
 * The state of one sequence lives in a device buffer the caller allocates (layout: dodt_amd/tracking.py):
 * header, at most 256 live tracks at the start of a keyframe, the kept keyframe-1 rows, log_capacity
 * finished tracks and log entries.  At most 128 detections per keyframe.  More live tracks, or a log
 * past its capacity, set a bit of the state's status word; nothing is written out of bounds.
 * Launches per batch of up to 16 keyframes on ctx's stream, nothing downloaded: (records only) the
 * encoding of dodt_track_encode; the IoU matrix of the batch's first keyframe over the whole chip; the
 * step (one workgroup: assignment on one wave by shortest augmenting paths, gate, filter one lane per
 * track, compaction), which computes the later keyframes' matrices itself, since they depend on the
 * step before.  ego: host, 13 doubles per keyframe -- trans (3), matrix (3x3 row major), delta of
 * coordinate_transform from the keyframe BEFORE it to it; calib: host, the 42 doubles of
 * dodt_interpolate_pairs; both read before the call returns and passed to the kernels by value.
 *
 * Bytes of a state buffer with room for log_capacity (>= 1) log entries and finished tracks. */
int dodt_kf_state_bytes(int log_capacity, size_t* bytes);
/* Start a sequence: empty state, ids from 0, keyframe 0. */
int dodt_kf_reset(dodt_ctx* ctx, void* d_state, int log_capacity);
/* n_keyframes lists already encoded: d_rows (n_keyframes, max_rows, 16) float64 in the KITTI row layout
 * (boxes2d in cols 4..7, boxes3d [h,w,l,x,y,z,ry] in 8..14, score in 15; nothing else is read), d_counts
 * (n_keyframes,) rows per list; max_rows <= 128. */
int dodt_kf_track_keyframes(dodt_ctx* ctx, void* d_state, const double* d_rows, const int32_t* d_counts,
                            int n_keyframes, int max_rows, const double* ego, const double* calib,
                            double sigma_l, double iou_threshold, int max_age, int min_hits, double L,
                            double R_scaler);
/* n_pairs record pairs (dodt_track_pairs' arguments): pair j's keyframe-0 rows, encoded, are keyframe j
 * of the batch; the last pair's keyframe-1 rows are kept in the state for dodt_kf_flush (a later batch
 * replaces them).  ego[j]: the motion into pair j's keyframe 0. */
int dodt_kf_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                        const int32_t* d_counts, int n_pairs, int max_det, const double* p2, double image_w,
                        double image_h, double score_threshold, const double* ego, const double* calib,
                        double sigma_l, double iou_threshold, int max_age, int min_hits, double L,
                        double R_scaler);
/* The end of the sequence: the kept keyframe-1 rows, if any, are the final keyframe (ego: the motion
 * into it, NULL: none); then every live track with hits >= min_hits is finished, in order, and the live
 * list is emptied. */
int dodt_kf_flush(dodt_ctx* ctx, void* d_state, const double* ego, const double* calib, double sigma_l,
                  double iou_threshold, int max_age, int min_hits, double L, double R_scaler);
/* Lanes, as dodt_track_lanes: several sequences advance by one pair each in one call.  The distance in bytes
 * between two lanes' states in one buffer: dodt_kf_state_bytes(log_capacity) rounded up to a multiple of 256.
 * Needs no context. */
int dodt_kf_lanes_stride(int log_capacity, size_t* stride);
/* Pair i of the step belongs to lane i, whose state is the ordinary layout at d_states + i * stride
 * (dodt_kf_reset, dodt_kf_flush and the host's reader work on that address unchanged).  d_records
 * (n_lanes, 2, max_det, 17) and d_counts (n_lanes, 2): lane i's pair is pair i; its keyframe-0 rows are the
 * lane's next keyframe, its keyframe-1 rows are kept in the lane's state.  Host arrays, all read before
 * the call returns: active, n_lanes bytes (non-zero: the lane takes its pair) or NULL for every lane; p2s
 * (n_lanes, 12), image_whs (n_lanes, 2), egos (n_lanes, 13: the motion into lane i's current keyframe; the
 * parked row -- zero translation, the identity, delta 0 -- where it has none) and calibs (n_lanes, 42).
 * The thresholds and the filter's parameters are the same for all lanes.  An active lane's state
 * afterwards is byte for byte what dodt_kf_track_pairs(ctx, d_states + i * stride, pair i, n_pairs = 1,
 * p2s[i], image_whs[i], egos[i], calibs[i], ...) leaves, the status bits included, which are the lane's
 * own; of an inactive lane no byte is read or written.  Three launches per 8 lanes on ctx's stream, in
 * the workspaces dodt_kf_track_pairs uses: the encoding (one workgroup per lane), the IoU matrices over
 * the chip (grid.y = lane) and the step (one workgroup per lane, the body dodt_kf_track_pairs runs); the
 * lanes' constants -- 440 bytes each -- travel by value in the kernel arguments, which is what bounds a
 * chunk at 8 lanes.  A chunk without an active lane launches nothing. */
int dodt_kf_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes, const unsigned char* active,
                        const void* d_records, int records_f64, const int32_t* d_counts, int max_det,
                        const double* p2s, const double* image_whs, const double* egos, const double* calibs,
                        double score_threshold, double sigma_l, double iou_threshold, int max_age, int min_hits,
                        double L, double R_scaler);
/* The filter alone, the step kernel's device functions: n_tracks independent tracks, one lane each.
 * d_x0 (n_tracks, 4) initial positions (rates 0), d_LR (n_tracks, 3) [L0, L, R_scaler]: P0 = L0 I and
 * R = R_scaler L I (the host class keeps the P of its construction when L is set afterwards), d_ops
 * (n_tracks, max_ops) 0: predict, else predict + update with d_z (n_tracks, max_ops, 4); d_n_ops
 * (n_tracks,).  After every operation: d_x_out (n_tracks, max_ops, 8), d_P_out (n_tracks, max_ops, 64). */
int dodt_kf_filter_steps(dodt_ctx* ctx, const double* d_x0, const int32_t* d_ops, const double* d_z,
                         const int32_t* d_n_ops, const double* d_LR, int n_tracks, int max_ops,
                         double* d_x_out, double* d_P_out);
/* The assignment and the gate alone: d_iou (n_tracks <= 256, n_dets <= 128) float32 -> d_matches (k, 2)
 * [track, detection] in ascending track order, d_unmatched_dets and d_unmatched_tracks in the host's
 * order, d_counts [k, unmatched detections, unmatched tracks, 1 if no finite assignment exists]. */
int dodt_kf_assign(dodt_ctx* ctx, const float* d_iou, int n_tracks, int n_dets, double iou_threshold,
                   int32_t* d_matches, int32_t* d_unmatched_dets, int32_t* d_unmatched_tracks,
                   int32_t* d_counts);
/* The association's IoU alone: d_iou_out (n_tracks, n_dets) float32 = cal_transformed_ious of boxes
 * d_last (n_tracks, 7) and d_dets (n_dets, 7), [h,w,l,x,y,z,ry] float64, under one ego row (NULL: none). */
int dodt_kf_iou_matrix(dodt_ctx* ctx, const double* d_last, int n_tracks, const double* d_dets, int n_dets,
                       const double* ego, const double* calib, float* d_iou_out);

/* ---- the velocity-extrapolating greedy IoU tracker on the device (velocity_track.hip) -----------
 * interpolate_by_track of dodt_amd/experiments/video_detection_iou.py: greedy association in track order
 * (each live track takes the first maximum of its IoUs with the detections still free and matches it if
 * that is > sigma_iou), a track without a match extrapolated by its last displacement for up to extend_len
 * frames, then cut and finished if max_score >= sigma_h and it has >= t_min entries.  The state, the ego
 * rows (13 doubles per keyframe: the motion from the keyframe before it) and the calibration (42 doubles)
 * are those of dodt_kf_*; keyframe k is frame k * stride.  The IoU is float64 under this tracker's
 * permutation (the track's box enters with l and h swapped); speed and prediction are computed in the
 * dtype the host holds boxes3d in (float32 sums rounded to float32), scores are compared in the scores' dtype.  The log holds a
 * track's real entries (keyframe, row) and predicted entries (box); the frames between two matched
 * keyframes and the extensions at both ends are rebuilt from it on the host.  Limits: 128 detections per
 * keyframe, 256 live tracks at the start of a keyframe, log_capacity log entries and finished tracks, 1 <=
 * stride, extend_len <= 4096; running past one sets a status bit and writes nothing out of bounds, as does
 * an IoU that is not finite.
 *
 * Bytes of a state buffer with room for log_capacity (>= 1) log entries and finished tracks. */
int dodt_vt_state_bytes(int log_capacity, size_t* bytes);
/* Start a sequence: empty state, ids from 0, keyframe 0. */
int dodt_vt_reset(dodt_ctx* ctx, void* d_state, int log_capacity);
/* n_keyframes lists already encoded: d_rows (n_keyframes, max_rows, 16) float32 or float64 (rows_f64) in
 * the KITTI row layout (boxes2d in cols 4..7, boxes3d [h,w,l,x,y,z,ry] in 8..14, score in 15), d_counts
 * (n_keyframes,) rows per list; max_rows <= 128.  box_f64 / score_f64: the host holds boxes3d / the scores as
 * float64 (only with rows_f64): the dtype of the speed and prediction arithmetic / of the score comparisons;
 * the state remembers score_f64 for the finish test of dodt_vt_flush. */
int dodt_vt_track_keyframes(dodt_ctx* ctx, void* d_state, const void* d_rows, int rows_f64,
                            const int32_t* d_counts, int n_keyframes, int max_rows, const double* ego,
                            const double* calib, double sigma_l, double sigma_h, double sigma_iou, int t_min,
                            int extend_len, int stride, int box_f64, int score_f64);
/* n_pairs record pairs (dodt_track_pairs' arguments): pair j's keyframe-0 rows, encoded (float32), are
 * keyframe j of the batch; the last pair's keyframe-1 rows are kept in the state for dodt_vt_flush (a
 * later batch replaces them).  ego[j]: the motion into pair j's keyframe 0. */
int dodt_vt_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                        const int32_t* d_counts, int n_pairs, int max_det, const double* p2, double image_w,
                        double image_h, double score_threshold, const double* ego, const double* calib,
                        double sigma_l, double sigma_h, double sigma_iou, int t_min, int extend_len,
                        int stride);
/* The end of the sequence: the kept keyframe-1 rows, if any, are the final keyframe (ego: the motion
 * into it, NULL: none); then every live track with max_score >= sigma_h and >= t_min entries is finished,
 * in order, its predictions not cut, and the live list is emptied. */
int dodt_vt_flush(dodt_ctx* ctx, void* d_state, const double* ego, const double* calib, double sigma_l,
                  double sigma_h, double sigma_iou, int t_min, int extend_len, int stride);
/* Lanes: dodt_kf_lanes_stride and dodt_kf_track_lanes for this tracker's state -- the same arguments (the
 * records float32 or float64 by records_f64, the encoded rows float32 as in dodt_vt_track_pairs), the
 * same three launches per 8 lanes, an active lane left byte for byte as dodt_vt_track_pairs with n_pairs
 * = 1 leaves it, an inactive one untouched. */
int dodt_vt_lanes_stride(int log_capacity, size_t* stride);
int dodt_vt_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes, const unsigned char* active,
                        const void* d_records, int records_f64, const int32_t* d_counts, int max_det,
                        const double* p2s, const double* image_whs, const double* egos, const double* calibs,
                        double score_threshold, double sigma_l, double sigma_h, double sigma_iou, int t_min,
                        int extend_len, int stride_frames);
/* The association's IoU alone (a test entry): d_iou_out (n_tracks, n_dets) float64 = this tracker's
 * cal_transformed_ious of boxes d_last (n_tracks, 7) and d_dets (n_dets, 7), [h,w,l,x,y,z,ry] float64,
 * under one ego row (NULL: none). */
int dodt_vt_iou_matrix(dodt_ctx* ctx, const double* d_last, int n_tracks, const double* d_dets, int n_dets,
                       const double* ego, const double* calib, double* d_iou_out);

/* ---- (e) multi-GPU: the one exchange step of the path, RCCL over xGMI, no PyTorch -----------
 * The reference runs on ONE device (avod/experiments/run_tracking_inference.py:109-128 sets a
 * single CUDA_VISIBLE_DEVICES and walks the sequences in a loop), so there is no reference
 * collective to replace: frame pairs shard over ranks (pair i -> rank i mod N) and the
 * sequential temporal module (avod/core/dt_evaluator_utils.py:189-362) needs every rank's detection
 * records in sequence order.  One process per GPU; librccl.so is dlopen'ed by the first of these
 * calls (a single-GPU process never maps it).
 *   id          DODT_COMM_ID_BYTES opaque bytes (an ncclUniqueId) made by ONE rank with
 *               dodt_comm_unique_id and handed to the others by the launcher's means (a file, an
 *               environment variable, a socket: dodt_amd/sharding.py uses a file next to the
 *               rendezvous port).
 *   create      ncclCommInitRank on ctx's device + a side stream that every collective runs on.
 *   all_gather  waits (event) for what `producer` has enqueued so far, then gathers
 *               float32 [pairs][frames][max_det][cols] + int32 [pairs][frames] of every rank into
 *               d_all_records / d_all_counts ([world][pairs]...; rank major) in one RCCL group, and
 *               signals `slot`'s event (slots 0..3: the caller's ring of send buffers).  The
 *               producer's stream is NOT made to wait: call dodt_comm_join(comm, slot, consumer)
 *               on the context that is about to overwrite that slot's send buffer or read the
 *               gathered data on the device, dodt_comm_sync for the host.
 *   barrier     all ranks have arrived (and the side stream is drained);
 *   max_f64     *value = max over ranks (the bench's max-over-ranks timing). */
typedef struct dodt_comm dodt_comm;
#define DODT_COMM_ID_BYTES 128
int dodt_comm_unique_id(uint8_t* id_out);
int dodt_comm_create(dodt_ctx* ctx, int rank, int world, const uint8_t* id, dodt_comm** out);
int dodt_comm_destroy(dodt_comm* comm);
/* From now on the communicator's collectives run on ctx's stream instead of a stream of their own (every stream
 * beyond four costs this runtime throughput): they then sit in that stream's order, between the
 * caller's kernels.  ctx must outlive the communicator. */
int dodt_comm_attach(dodt_comm* comm, dodt_ctx* ctx);
int dodt_comm_rank(const dodt_comm* comm, int* rank, int* world);
/* Measurement aid: from now on every dodt_all_gather_records is preceded, on the stream that
 * carries the collectives, by a one-wave kernel that idles for `microseconds` -- what that stream sees when a peer
 * reaches the rendezvous late.  0 switches it off.  At most 100 000 us. */
int dodt_comm_set_late_peer(dodt_comm* comm, double microseconds);
int dodt_all_gather_records(dodt_comm* comm, dodt_ctx* producer, int slot, const float* d_records,
                            const int32_t* d_counts, int pairs, int frames, int max_det, int cols,
                            float* d_all_records, int32_t* d_all_counts);
int dodt_comm_join(dodt_comm* comm, int slot, dodt_ctx* consumer);
int dodt_comm_sync(dodt_comm* comm);
int dodt_comm_barrier(dodt_comm* comm);
int dodt_comm_max_f64(dodt_comm* comm, double* value);

#ifdef __cplusplus
}
#endif
#endif /* DODT_HIP_H */
