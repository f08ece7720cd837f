/*
 * dtfill.h -- C ABI of libdtfill.so: the MI355X (gfx950) distance-transform + nearest-valid-depth
 * fill operator.  Plain pointers and sizes only; no torch / HIP types in the signatures
 * (`stream` is a hipStream_t passed as void*, NULL = the default stream).
 *
 * What each entry point replaces in the reference (placeforyiming/DistanceTransform-DepthCompletion):
 *
 *   dtfill_batch()            the per-frame body of DT_complete_batch(), solution_DeepNet/tools.py:13-35
 *                             (live copy demo.py:84-106), and Distance_Transform(),
 *                             solution_DeepNet/eval_NYU.py:120-133, for B frames at once:
 *                               nearest_point()                      tools.py:7-10 / eval_NYU.py:114-117
 *                                 value_mask = uint8((1.0 - x) > src_thr)
 *                                 cv2.distanceTransformWithLabels(value_mask, DIST_L1, 5, DIST_LABEL_PIXEL)
 *                               with_value = x > val_thr ; depth_list = x[with_value]   tools.py:22,24
 *                               out = depth_list[lbl - 1]                               tools.py:26
 *                             out_dt / out_index are the (dt, lbl) pair nearest_point() returns.
 *   dtfill_workspace_bytes()  the temporaries numpy/cv2 allocate implicitly (cv2's (H+4)x(W+4) int32
 *                             `temp`, the masks, depth_list); here the caller owns them.
 *   dtfill_strerror()         the numpy / cv2 exceptions the reference surfaces (tools.py:26 IndexError).
 *
 * All pointers are DEVICE pointers unless stated otherwise.  Frames are float32, C-contiguous
 * [B, H, W] (the shim slices channel 0 of the reference's [B,H,W,1] layout).  The library keeps
 * no global state, allocates nothing, and every call is ordered on `stream` only: it is safe to
 * call from several host threads on different streams / devices with different workspaces.
 */
#ifndef DTFILL_H
#define DTFILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTFILL_ABI_VERSION 1

/* metric */
#define DTFILL_METRIC_L1_CV 0 /* reference parity: OpenCV L1 5x5 chamfer + its label tie-break order */
#define DTFILL_METRIC_L2    1 /* exact Euclidean transform, tie-break = smallest raster index of the source
                                 (not in the reference, which is L1 only; BASELINE.json's north_star asks for it) */

/* return codes */
#define DTFILL_OK               0
#define DTFILL_ERR_NULL        -1 /* x, workspace or every output is NULL */
#define DTFILL_ERR_SHAPE       -2 /* B,H,W < 1, B > 65535, B*H*W >= 2^31, or H+W-2 >= 8192 (cv2's Q16 INIT_DIST0 range) */
#define DTFILL_ERR_WORKSPACE   -3 /* ws_bytes < dtfill_workspace_bytes() or workspace not 256-B aligned */
#define DTFILL_ERR_METRIC      -4 /* unknown metric */
#define DTFILL_ERR_LAUNCH      -5 /* a HIP launch failed (hipGetLastError) */
#define DTFILL_ERR_NO_DEVICE   -6 /* no usable HIP device */

/* per-frame status written to frame_status[b] (device int32): a bit set */
#define DTFILL_FRAME_OK           0
#define DTFILL_FRAME_INDEX_ERROR  1 /* numpy would raise IndexError in depth_list[lbl-1] (tools.py:26):
                                       a label addresses past the value list, or label 0 (no source in
                                       the frame) with an empty value list.  out_depth of that frame is
                                       then unspecified; out_dt / out_index are still exact. */
#define DTFILL_FRAME_NO_SOURCE    4 /* dtfill_nearest_gather[_backward]: the frame has no source pixel */
#define DTFILL_FRAME_GENERAL_PATH 2 /* informational (l1_cv): the frame, or some of its rows, was computed outside the LDS
                                       window kernel -- by the any-distance kernels (sparse frame, rows with a pixel
                                       farther than the halo from every source), k_sky (the rows above every source)
                                       or k_pts (a handful of sources); results are identical. */

/* flags of dtfill_batch_flags(): path selection, for tests and benchmarks */
#define DTFILL_FLAG_GENERAL_ONLY 1u /* skip the window kernel, every frame takes the any-distance kernels */
#define DTFILL_FLAG_FUSED_ONLY   2u /* skip the any-distance kernels: frames that need them are left
                                       undefined and carry DTFILL_FRAME_GENERAL_PATH in their status */
/* ... and one that changes the result: the loader's outlier_removal() (data_read.py:103-128, applied to the sparse map
   before anything else sees it, data_read.py:168-169) in front of the predicates.  The pass then equals
   dtfill_outlier_removal() followed by dtfill_batch() on its output, without the filtered map ever being written:
   a removed pixel stops being a source / value, the surviving ones are gathered from x.  Needs H, W >= 4. */
#define DTFILL_FLAG_OUTLIER_REMOVAL 4u
/* ... and one that changes only how the l1_cv pass is launched, for tests and A/B timing: the frame facts in a k_frame launch
   of their own in front of the window kernel (seven launches) instead of inside the window kernel's launch (six; the
   default for frames of up to DTFILL_FRAME_RIDE_MAX_H rows).  Results are identical; dtfill_batch_timed() reports a k_frame
   slot only then (0 ms otherwise). */
#define DTFILL_FLAG_SEPARATE_FRAME 8u
#define DTFILL_FRAME_RIDE_MAX_H 512

int dtfill_abi_version(void);
const char *dtfill_strerror(int code);

/* Bytes of scratch dtfill_batch() needs for this shape (0 on a bad shape). 256-B aligned carve. */
size_t dtfill_workspace_bytes(int B, int H, int W, int metric);

/*
 * One pass of the hot path over B frames.
 *   x            float32 [B,H,W], never written.
 *   src_thr      a pixel is a SOURCE iff NOT((1.0f - x) > src_thr) in float32   (tools.py:8: 0.1,
 *                eval_NYU.py:115: 0.001).  NaN is therefore a source, as in numpy.
 *   val_thr      a pixel enters the value list iff x > val_thr                  (tools.py:22: 0.1)
 *   out_depth    float32 [B,H,W] filled depth  = depth_list[lbl-1]              (nullable)
 *   out_dt       float32 [B,H,W] distance map  (l1_cv: integer-valued L1, 8192.0 in a frame with
 *                no source; l2: sqrtf of the exact squared distance, +inf if no source) (nullable)
 *   out_index    int32 [B,H,W]: l1_cv: cv2's label (1-based raster rank of the nearest source under
 *                cv2's tie-break, 0 = no source); l2: the same 1-based rank under the canonical
 *                tie-break                                                      (nullable)
 *   frame_status int32 [B] (nullable): DTFILL_FRAME_*
 *   workspace    ws_bytes >= dtfill_workspace_bytes(B,H,W,metric), 256-B aligned
 * Returns DTFILL_OK or a negative DTFILL_ERR_*.  Asynchronous: outputs are valid after `stream`
 * has been synchronised.
 */
int dtfill_batch(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                 float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                 void *workspace, size_t ws_bytes, void *stream);

/* dtfill_batch() with explicit path selection (DTFILL_FLAG_*); flags = 0 is dtfill_batch(). */
int dtfill_batch_flags(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                       float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                       void *workspace, size_t ws_bytes, void *stream, unsigned flags);

/*
 * dtfill_batch_flags() with the drivers' post-fill steps folded into the depth stores (l1_cv only):
 *   depth_row0  out_depth holds rows [depth_row0, H) of every frame: float32 [B, H - depth_row0, W]
 *               (demo.py:292-293: lidar_batch = lidar_batch[:, 96:, :, :] right after DT_complete_batch)
 *   use_floor   out_depth = relu(d - floor_) + floor_ in float32, both roundings kept
 *               (eval_NYU.py:205, test.py:133: the 0.9 m depth floor)
 * out_dt / out_index stay whole frames.  Saves the separate dtfill_crop_floor() pass over the filled depth.
 * depth_row0 = 0 and use_floor = 0 is dtfill_batch_flags().  DTFILL_ERR_METRIC for the l2 metric with an epilogue.
 */
int dtfill_batch_epilogue(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                          float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                          void *workspace, size_t ws_bytes, void *stream, unsigned flags, int depth_row0,
                          int use_floor, float floor_);

/*
 * Same pass, instrumented for bench.py: records a HIP event on `stream` before and after every
 * kernel, synchronises, and returns each kernel's duration in milliseconds in kernel_ms (HOST
 * float[dtfill_num_kernels(metric)]; 0 for kernels the flags skip).  Not for production use (it blocks).
 */
int dtfill_num_kernels(int metric);
const char *dtfill_kernel_name(int metric, int k);
int dtfill_batch_timed(const float *x, int B, int H, int W, float src_thr, float val_thr, int metric,
                       float *out_depth, float *out_dt, int32_t *out_index, int32_t *frame_status,
                       void *workspace, size_t ws_bytes, void *stream, unsigned flags, float *kernel_ms);

/*
 * Which kernel family owned how many pixels in the LAST pass run in `workspace` (same B, H, W, metric) -- for bench.py's
 * per-kernel roofline figures: a kernel is credited with the bytes of the pixels it processed, not with the whole batch.
 * out_px: DEVICE int64[DTFILL_STATS_N], written on `stream`:
 *   [DTFILL_STATS_ALL]     B*H*W
 *   [DTFILL_STATS_WINDOW]  pixels of the rows the window kernel kept (l1_cv: k_fused; l2: k_l2win, rows it did not hand on)
 *   [DTFILL_STATS_ANYDIST] pixels of the rows the any-distance kernels stored (l1_cv: k_rows / k_fin; l2: k_l2env's rows)
 *   [DTFILL_STATS_SKY]     l1_cv: pixels of the rows k_sky stored
 *   [DTFILL_STATS_POINTS]  pixels of the frames with a handful of sources (l1_cv: k_pts; l2: k_l2env's tiles)
 *   [DTFILL_STATS_COLT]    pixels of the frames k_colT ran for
 */
#define DTFILL_STATS_ALL 0
#define DTFILL_STATS_WINDOW 1
#define DTFILL_STATS_ANYDIST 2
#define DTFILL_STATS_SKY 3
#define DTFILL_STATS_POINTS 4
#define DTFILL_STATS_COLT 5
#define DTFILL_STATS_N 6
int dtfill_pass_stats(const void *workspace, size_t ws_bytes, int B, int H, int W, int metric, long long *out_px, void *stream);

/*
 * outlier_removal() of the reference's loader, data_read.py:103-128 (applied in front of the path when
 * if_removal=True, data_read.py:168-169): two 7x7-diamond cv2.filter2D sums (values, valid counts;
 * BORDER_REFLECT_101), out = x where NOT (x - sum/(count + 1e-5) > 1.0), else 0.  The float32 sum is
 * accumulated over the taps in kernel row-major order, the mean and the test in float64, as
 * numpy/OpenCV do.  x, out: float32 [B,H,W] device pointers (out may not alias x).  Needs H, W >= 4.
 */
int dtfill_outlier_removal(const float *x, int B, int H, int W, float *out, void *stream);

/*
 * generate_multi_channel() of the reference's models, solution_DeepNet/net.py:83-122 (weights
 * create_weight_matrix, net.py:71-81): the in-network windowed nearest fill.  Step k: over the
 * table_size^2 window (zero padding), s = mask * (table_size - |di| - |dj|); out = sum of the inputs where s
 * equals its window maximum / (1e-6 + their count); the next step's mask is (out > 0.001).
 * The maximum runs over all table_size^2 taps, the padding's included: any finite mask is legal, negative
 * values included (a window whose every product is negative selects its largest one); a NaN mask tap is never
 * selected.  Non-finite data deviates from net.py on purpose: an input is added only where it is selected,
 * while net.py's sum(data * selected) makes every window that holds a +-inf or NaN input NaN (inf * 0).
 * Following net.py there would stop a pixel's value from being carried on through the later steps.
 * data, mask: float32 [B,H,W] (the reference's [B,H,W,1]); out2/out3/out4: the reference's lidar_2..4
 * (those beyond scale_num may be NULL); lidar_1 is the input itself.  table_size odd, <= 15; scale_num 1..4.
 * float32; the window sum is accumulated in tap (row-major) order.
 */
int dtfill_generate_multi_channel(const float *data, const float *mask, int B, int H, int W, int table_size,
                                  int scale_num, float *out2, float *out3, float *out4, void *stream);

/*
 * The backward pass of dtfill_generate_multi_channel(): the gradient of a loss with respect to `data`, given its gradients
 * with respect to lidar_1..4.  In the reference the operator sits inside the trained graph: with if_correct its input is the
 * output of four learned convolutions (net.py:469-486), its outputs feed the encoder (net.py:489), and the gradient is cut
 * only when joint_train is off (net.py:491-496).  tf.equal, tf.cast and tf.greater have no gradient, so the selection of a
 * step and the re-masking between the steps (net.py:95-96) are constants, every step is a fixed sparse linear map A_k of its
 * input, and the backward applies the transposes.  It needs the masks and the forward outputs, never the data.  The mask
 * receives no gradient.
 *
 * One forward step, input d, mask m, ts = table_size, w(t) = ts - |di| - |dj| (as above):
 *   mx_p  = max over all ts^2 taps t of m[p+t] * w(t); padding taps count, with product 0; a NaN product is never selected;
 *   sel_p(t) = (m[p+t] * w(t) == mx_p);  cnt_p = the number of selected taps;
 *   out_p = sum_t sel_p(t) * d[p+t] / (1e-6f + cnt_p).
 * Its transpose applied to an upstream gradient G, for an in-image pixel q, in float32:
 *   c_p      = G_p / (1e-6f + (float)cnt_p), one IEEE division per p;
 *   (A^T G)_q = the sum, starting from +0, over the in-image p with |p - q|_inf <= (ts-1)/2, in ascending raster order of
 *              p, of c_p where m[q] * w(q - p) == mx_p.
 * A c_p is added only where it is selected (as the forward adds an input only where it is selected): a non-finite G_p does
 * not spread to pixels that did not select it.  Gradient sent to padding taps is dropped.  "Ascending raster order of p" is
 * this library's contract, as the forward's tap order is: TensorFlow's own order is not documented, and where one window
 * selects a pixel every order gives the same bits.
 *
 * The whole call: g1..g4 are the gradients of lidar_1..4 (lidar_1 is the data itself), m_1 = mask, m_k = (lidar_k > 0.001f)
 * for k >= 2, derived from out2 / out3 while they are read, never stored.  For scale_num 4
 *   G_3 = g3 + A_3^T g4;  G_2 = g2 + A_2^T G_3;  grad_data = g1 + A_1^T G_2,
 * each + one float32 add of g_k and the finished transpose sum; shorter chains for scale_num 3 and 2; scale_num 1 gives
 * grad_data = g1.  A NULL g_k is a zero gradient and adds nothing (scale_num 1 with a NULL g1: all +0).  grad_data is
 * always fully overwritten.
 *
 * mask: float32 [B,H,W], the forward's.  out2, out3: the forward's lidar_2 and lidar_3, needed where a later step's mask
 * derives from them (out2 for scale_num >= 3, out3 for scale_num 4; NULL otherwise is fine).  g1..g4: float32 [B,H,W], each
 * nullable.  grad_data: float32 [B,H,W], may not alias any input.  workspace: at least
 * dtfill_generate_multi_channel_backward_workspace_bytes(B,H,W,scale_num) bytes (at most two [B,H,W] float frames, G_3 and
 * G_2; 0 for scale_num <= 2, when workspace may be NULL), 256-B aligned, the caller's, no initialisation needed, nothing kept
 * between calls.  Asynchronous on `stream`; no allocation; no atomics, so two calls give the same bits.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL mask, a NULL grad_data, a NULL required out_k or a NULL
 * workspace where one is needed; DTFILL_ERR_SHAPE for an even table_size or one outside 1..15, scale_num outside 1..4, B, H
 * or W < 1, or B*H*W >= 2^31; DTFILL_ERR_WORKSPACE for a workspace that is too small or not aligned.
 */
size_t dtfill_generate_multi_channel_backward_workspace_bytes(int B, int H, int W, int scale_num); /* 0 on a bad shape */
int dtfill_generate_multi_channel_backward(const float *mask, const float *out2, const float *out3,
                                           int B, int H, int W, int table_size, int scale_num,
                                           const float *g1, const float *g2, const float *g3, const float *g4, /* each nullable */
                                           float *grad_data, void *workspace, size_t ws_bytes, void *stream);

/*
 * generate_multi_channel() and generate_multi_channel_with_image() of the reference's demo driver,
 * solution_DeepNet/demo.py:108-149 and :151-198 (weights create_weight_matrix, demo.py:65-75): what demo.py runs with its
 * default --model_type DT.  Not the net.py form above: the weights are powers of ten, the selection runs on data * w (the
 * data is its own mask, nothing is re-masked between the steps, so a farther but larger depth can beat a nearer one),
 * the divisor counts the non-zero selected inputs, and every output is divided by scale_range.
 *
 * lidar: float32 [B,H,W].  ts = table_size (odd, 1..15), raw_1 = lidar.  Step k (2..scale_num), per pixel, in float32:
 *   taps   the ts x ts window over the zero-padded frame, as tf.image.extract_patches(padding='SAME') reads it, in
 *          row-major order;
 *   w      (float)10^(ts - |di| - |dj|): the double 10^e (exact for e <= 22) rounded to float32 once (exact for
 *          e <= 10; 10^11 .. 10^15 are not);
 *   p      d * w, one rounded multiply, contracted into nothing;
 *   mx     the maximum of p over all ts^2 taps; padding taps count, with p = 0;
 *   sel    p == mx;
 *   sum    the float32 sum of d over the selected taps in tap order, starting from +0 (unselected taps may add +0: the
 *          only trace is a -0 sum coming out as +0; the two compare equal, here and in every later step);
 *   cnt    the number of selected taps with d != 0: it is 0 exactly when mx == 0;
 *   raw_k  sum / (1e-6f + (float)cnt); an all-zero window gives 0 / 1e-6 = 0.
 * The next step reads raw_k.  Outputs for k = 1..scale_num, sr = scale_range:
 *   rgb == NULL   out_k float32 [B,H,W]     = raw_k / sr
 *   rgb given     out_k float32 [B,H,W,C+1]: channels 0..C-1 = rgb / sr; channel C = (raw_k / sr) / sr, both roundings
 *                 kept -- demo.py:172-173 divides the lidar channel, :198 the concatenated tensor again.  rgb: float32
 *                 [B,H,W,C], channel-last.
 * Every division is an IEEE-rounded division, not a multiply by a reciprocal.
 * Defined for finite inputs with |d| * 10^ts finite.  Beyond that: a NaN product is never selected, and an input is added
 * only where it is selected (demo.py's reduce_sum(data * selected) would make every window that holds a +-inf or NaN
 * input NaN; the same deliberate deviation as dtfill_generate_multi_channel's); nothing faults.
 * TensorFlow's reduce_sum does not document its summation order and the reference could not be run where this was
 * written, so "tap order" is this library's contract, not a measured property of the reference: with one selected tap
 * (the common case) every order gives the same bits; with more, TensorFlow may differ in the last place.
 *
 * out1..out4: those beyond scale_num may be NULL; none may alias lidar or rgb.  workspace: at least
 * dtfill_demo_multi_channel_workspace_bytes(B,H,W,scale_num) bytes (at most two [B,H,W] float frames for the raw
 * intermediates a later step reads; 0 for scale_num <= 2, when workspace may be NULL), 256-B aligned, the caller's, no
 * initialisation needed, nothing kept between calls.  Asynchronous on `stream`.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL lidar, a NULL required output or a NULL workspace
 * where one is needed; DTFILL_ERR_SHAPE for an even table_size or one outside 1..15, scale_num outside 1..4, scale_range
 * zero or not finite, rgb given with C < 1, B, H or W < 1, or B*H*W*(C+1) >= 2^31 (C = 0 without rgb);
 * DTFILL_ERR_WORKSPACE for a workspace that is too small or not aligned.
 */
size_t dtfill_demo_multi_channel_workspace_bytes(int B, int H, int W, int scale_num); /* 0 on a bad shape */
int dtfill_demo_multi_channel(const float *lidar, const float *rgb /* nullable */, int C, int B, int H, int W,
                              int table_size, int scale_num, float scale_range,
                              float *out1, float *out2, float *out3, float *out4,
                              void *workspace, size_t ws_bytes, void *stream);

/*
 * What the reference's drivers do with a filled frame.
 *
 * dtfill_crop_floor: out[b, i, j] = f(x[b, r0+i, c0+j]) for rows [r0, r1), columns [c0, c1); f is the depth
 * floor relu(d - floor) + floor in float32, both roundings kept (eval_NYU.py:205, test.py:133: floor 0.9), when
 * use_floor != 0, the identity otherwise.  Replaces lidar_batch[:, 96:, :, :] (demo.py:292-293), the NYU
 * evaluation crop [6:234, 8:312] (eval_NYU.py:202-203) and the KITTI depth floor (eval_NYU.py:205).
 * x: float32 [B,H,W]; out: float32 [B, r1-r0, c1-c0], may not alias x.
 *
 * dtfill_png16: test.py:133-148 -- depth floor (if use_floor), clip to [lo, hi] (0, 100), pad_top (96) copies
 * of the first row on top, * scale (256), cast to uint16.  out: uint16 [B, pad_top+H, W].  Defined for
 * lo * scale and hi * scale within [0, 65535].
 *
 * NaN: the depth floor keeps a NaN depth NaN (relu = max(x, 0), as in TF and numpy), here and in
 * dtfill_batch_epilogue(); dtfill_png16 clips it to NaN and writes it as 0.
 */
int dtfill_crop_floor(const float *x, int B, int H, int W, int r0, int r1, int c0, int c1, int use_floor, float floor_,
                      float *out, void *stream);
int dtfill_png16(const float *x, int B, int H, int W, int pad_top, int use_floor, float floor_, float lo, float hi,
                 float scale, uint16_t *out, void *stream);

/*
 * Scan-line subsampling of a projected LiDAR frame: the 32- and 16-line inputs subsample_Lidar_train.py /
 * subsample_Lidar_val.py build (get_all_points -> calculate_angle -> sample -> map_points_on_image), per frame b:
 *   a pixel (row v, column u) is VALID iff x > 0.1f (float32 compare: NaN, -inf and (0, 0.1] are not points);
 *   for a valid pixel, in float64 with d = (double)x:  p_cam = K^-1 [u, v, 1]^T d,  p = (E^-1 [p_cam; 1])[0:3],
 *     pitch = asin(p.z / |p|)   (K^-1, E^-1: general inverses, partial pivoting, computed on the device);
 *   pmin, pmax over the frame's valid pixels (NaN if any pitch is NaN, as np.min / np.max), interval = (pmax - pmin) / n_bins;
 *   label = ceil((pitch - pmin) / interval), not clamped (the minimum has label 0; for a power-of-two n_bins the maximum
 *     has label n_bins); a valid pixel is KEPT iff label mod keep_every == 0 (keep_every = 1 / keep_ratio: 2 gives the
 *     reference's 32 lines, 4 its 16).
 *   out[b] holds x at the kept pixels, bit for bit, and +0.0f everywhere else.  The reference re-projects the kept points
 *   through the same K and E, which is the identity in exact arithmetic, so nothing is scattered.
 *   frame_status[b]: DTFILL_LINES_* bits; when any is set, out[b] is all zeros.
 * x: float32 [B,H,W]; K: float64 [B,3,3] intrinsics; E: float64 [B,4,4] velo->cam extrinsics; out: float32 [B,H,W], may
 * not alias x; frame_status: int32 [B]; workspace: ws_bytes >= dtfill_line_subsample_workspace_bytes(B,H,W), 256-B
 * aligned, no initialisation needed, nothing kept between calls.  Asynchronous on `stream`.
 * Returns DTFILL_ERR_NULL for a NULL pointer, n_bins < 1 or keep_every < 1; DTFILL_ERR_SHAPE for B,H,W < 1, B > 65535 or
 * B*H*W >= 2^31; DTFILL_ERR_WORKSPACE; all checked before any HIP call.
 */
#define DTFILL_LINES_NO_POINTS     1 /* no valid pixel (the reference's np.max raises ValueError) */
#define DTFILL_LINES_BAD_INTERVAL  2 /* interval 0 or not finite: one point, one pitch, a +inf depth (the reference's NaN
                                        labels keep nothing) */
#define DTFILL_LINES_SINGULAR      4 /* K or E singular: a zero pivot (np.linalg.inv raises LinAlgError) */
size_t dtfill_line_subsample_workspace_bytes(int B, int H, int W);
int dtfill_line_subsample(const float *x, int B, int H, int W, const double *K, const double *E, int n_bins, int keep_every,
                          float *out, int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream);


/*
 * depth_read() of the reference's loader, data_read.py:81-99 (KITTI_demo_loader.depth_read, :404-422, is the same), on the
 * decoded 16-bit PNG values of B frames; the host keeps the PNG decode.  Frame b holds (h_b, w_b) pixels, every output
 * frame H x W.  Per frame, in IEEE double (Pillow's NEAREST resize, ImagingScaleAffine's running sum, not a closed form):
 *   ay = (double)h_b / H;  y = 0.5 * ay;  for i = 0 .. H-1: ry[i] = (int)y (truncation); y += ay   (the same for rx with w_b / W)
 *   out[b, i, j] = (float)raw[b, ry[i], rx[j]] * 2^-8   (exact, and equal to the reference's float64 value / 256 after
 *                                                        its PIL mode-F round trip)
 * Same size in and out is the identity.  An index is clamped to h_b - 1 / w_b - 1, which never binds below 2^26 rows or columns.
 * raw: uint16 [B, hmax, wmax], row pitch wmax; nothing beyond (h_b, w_b) is read.  dims: int32 [B, 2] holding (h_b, w_b), or
 * NULL for hmax x wmax everywhere.  out: float32 [B, H, W], may not alias raw.  frame_status: int32 [B] (nullable),
 * DTFILL_READ_* bits, final when the stream reaches the end of the call.  workspace: ws_bytes >=
 * dtfill_depth_read_workspace_bytes(B, H, W), 256-B aligned, no initialisation needed, nothing kept between calls.
 * Asynchronous on `stream`; no allocation.
 * Returns DTFILL_ERR_NULL for a NULL raw, out or workspace; DTFILL_ERR_SHAPE for B, hmax, wmax, H, W < 1, B > 65535,
 * B*hmax*wmax >= 2^31 or B*H*W >= 2^31; DTFILL_ERR_WORKSPACE; all checked before any HIP call.
 */
#define DTFILL_READ_NOT_16BIT 1 /* every one of the frame's h_b x w_b values is <= 255 (the reference's
                                   assert np.max(depth_png) > 255, taken before the resize); out[b] is still written */
#define DTFILL_READ_BAD_DIMS  2 /* dims[b] outside [1, hmax] x [1, wmax]: out[b] is all +0.0 (and the other bit is not set) */
size_t dtfill_depth_read_workspace_bytes(int B, int H, int W);
int dtfill_depth_read(const uint16_t *raw, const int32_t *dims, int B, int hmax, int wmax, int H, int W, float *out,
                      int32_t *frame_status, void *workspace, size_t ws_bytes, void *stream);

/*
 * rgb_read() of the reference's loader, data_read.py:66-73 (KITTI_demo_loader.rgb_read, :395-402, is the same), and the two
 * lines every driver puts behind it (rgb = img_batch[:, 96:, :, :] / 255.0 as float32: train.py:213-214, eval.py:158-159,
 * eval_NYU.py:159-160, test.py:118-119, demo.py:296-297), on the decoded uint8 images of B frames with C interleaved
 * channels; the host keeps the PNG decode.  Frame b holds (h_b, w_b) pixels, every output frame (H - first_row) x W.
 *   ry[0..H), rx[0..W): dtfill_depth_read's maps (Pillow's NEAREST resize, the running double sum, clamped to h_b - 1 / w_b - 1)
 *   for i in [first_row, H), j in [0, W), c in [0, C):   v = raw[b, ry[i], rx[j], c]
 *     out_u8[b, i - first_row, j, c] = v
 *     out_f32[...]                   = normalize ? (float)v / 255.0f : (float)v     in the layout asked for
 *   The division is the correctly rounded float32 division, whose bits equal the reference's float32(float64(v) / 255.0)
 *   for all 256 values (v * (1 / 255.0f) differs for 126 of them).
 * raw: uint8 [B, hmax, wmax, C], row pitch wmax * C bytes, any alignment.  Only the first w_b * C bytes of the source rows
 * that ry samples are read: no byte of the padding of a ragged batch, no row that no output row samples (there is no
 * whole-frame check as in dtfill_depth_read), nothing beyond raw.  dims: int32 [B, 2] holding (h_b, w_b), or NULL for
 * hmax x wmax everywhere.  out_u8: uint8 [B, H - first_row, W, C]; out_f32: float32 in `layout`; either may be NULL, both are
 * only element-aligned, neither may alias raw.  frame_status: int32 [B] (nullable): 0, or DTFILL_READ_BAD_DIMS for dims
 * outside [1, hmax] x [1, wmax], and then the frame's outputs are all 0 / +0.0f.  workspace: ws_bytes >=
 * dtfill_rgb_read_workspace_bytes(B, H, W), 256-B aligned, no initialisation needed, nothing kept between calls.
 * Asynchronous on `stream`; no allocation, no host synchronisation, re-entrant across streams.
 * Returns DTFILL_ERR_NULL for a NULL raw or workspace or both outputs NULL; DTFILL_ERR_SHAPE for B, hmax, wmax, H, W < 1,
 * B > 65535, C outside 1..4, first_row outside [0, H), a layout that is neither of the two, B*hmax*wmax*C >= 2^31,
 * B*(H-first_row)*W*C >= 2^31 or B*H*W >= 2^31 (the maps); DTFILL_ERR_WORKSPACE for a workspace too small or not
 * aligned; all checked before any HIP call.
 */
#define DTFILL_RGB_NHWC 0 /* out_f32: [B, H - first_row, W, C]  (the drivers' array; dtfill_demo_multi_channel's rgb) */
#define DTFILL_RGB_NCHW 1 /* out_f32: [B, C, H - first_row, W]  (dtfill_nearest_gather's values; a PyTorch conv) */
size_t dtfill_rgb_read_workspace_bytes(int B, int H, int W); /* 0 on a bad shape */
int dtfill_rgb_read(const uint8_t *raw, const int32_t *dims, int B, int hmax, int wmax, int C, int H, int W, int first_row,
                    int normalize, int layout, uint8_t *out_u8, float *out_f32, int32_t *frame_status, void *workspace,
                    size_t ws_bytes, void *stream);

/*
 * The per-sample work of the reference's NYU loaders (Data_load_NYU.read_batch, data_read.py:295-335; read_one_val_NYU,
 * :337-371; the two copies at :443-473 and :485-580) on B stored samples at once: the transpose of the image, the anti-aliased
 * skimage.transform.resize of image and dense depth from hin x win to H x W, the sparse sampling depth = gt * Mask, the
 * loader's rgb * 255 and, on request, the drivers' rgb / 255.0 (eval_NYU.py:164-165).  The host keeps the h5 read and the
 * random draws.  For a reduction that resize is scipy.ndimage.gaussian_filter(mode='mirror') followed by
 * scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True), and this is the arithmetic of those two, bit for bit:
 *
 * Geometry, per axis (n_in -> n_out, n_out <= n_in):  f = (double)n_in / n_out;  sigma = (f - 1) / 2;
 *   radius r = int(4 sigma + 0.5), the filter's half width.  r == 0 (sigma < 0.125; f == 1 among them): the axis has no pass.
 * Taps: the CALLER computes the half kernel w[0..r] (w[k] = exp(-0.5 / sigma^2 * k^2) over the sum of all 2r + 1, as scipy's
 *   _gaussian_kernel1d does in numpy: tools.nyu_taps) and passes it with r, so that no exp of a C library enters the bits.
 *   wy / wx are HOST pointers, read before the call returns; NULL exactly when the axis' r is 0; r <= DTFILL_NYU_MAX_RADIUS
 *   (factors below 5.25).  The call does not check the taps against the geometry: any symmetric kernel is filtered with.
 * m(i): scipy's 'mirror' into [0, n): period 2 (n - 1), the edge sample not repeated, n == 1 -> 0; it holds for r > n - 1,
 *   where an index reflects several times.
 * Filter pass along an axis (axis 0 = rows first, then axis 1), accumulated in double, no contraction:
 *   acc = x[i] * w[0];  for k = r .. 1 (the outermost pair first, scipy's order):  acc += (x[m(i - k)] + x[m(i + k)]) * w[k]
 * Resample, in double, no contraction, per axis c = (j + 0.5) * f - 0.5, i0 = floor(c), t = c - i0, neighbours m(i0), m(i0 + 1):
 *   v = 0.0 + (x00 * (1 - tr)) * (1 - tc);  v += (x01 * (1 - tr)) * tc;  v += (x10 * tr) * (1 - tc);  v += (x11 * tr) * tc
 *   (scipy's: each sample times its row weight, then its column weight, summed in this order from 0.0 on).  A neighbour of
 *   weight 0 is still read and multiplied (f == 1, where i0 + 1 may mirror): a NaN there propagates, as in scipy.
 * Depth (float32 [B, hin, win], as the files store it): each filter pass is rounded to float32 (scipy on a float32 array;
 *   skimage >= 0.19 keeps float32), the resample runs on those values in double and is rounded once: out_gt float32 [B, H, W].
 *   out_lidar[p] = marked(p) ? gt[p] : gt[p] * 0.0f, the product as it stands: -0.0 under a negative gt, NaN under a
 *   non-finite one, as gt * Mask gives them.  samples: int32 [B, n, 2] holding (row, col), the loaders' + 6 / + 8 already
 *   added, duplicates allowed; a sample outside [0, H) x [0, W) is skipped and sets DTFILL_NYU_INDEX_ERROR in its frame's
 *   status (numpy would raise IndexError).  samples == NULL or n == 0: out_lidar is gt * 0.0f everywhere.
 * Image (uint8 [B, C, hin, win], the stored layout; the loaders' transpose is folded in; C in 1..4): per channel
 *   x = (double)u8 * (1.0 / 255.0) (img_as_float's multiply by the reciprocal), both passes and the resample in double -> r;
 *   out_rgb = (float)(r * 255.0), data_read.py:329,335; with normalize, (float)((double)(float)(r * 255.0) / 255.0).
 *   Layout DTFILL_RGB_NHWC [B, H, W, C] (the reference's) or DTFILL_RGB_NCHW [B, C, H, W].
 * The limit of the claim: what the tests pin, bit for bit, is scipy (gaussian_filter and zoom as above, float32 and float64).
 *   That skimage's resize is those two calls, that img_as_float multiplies by 1.0 / 255, and that skimage's 'reflect' is
 *   scipy's 'mirror' are restated from skimage >= 0.19's source, not tested: skimage is not a dependency.  skimage < 0.19
 *   resampled with its own warp(), which associates the four products differently and returned float64 for float32 input.
 * rgb and depth are each nullable, not both; an output whose input is NULL must be NULL, and an input needs an output (out_rgb;
 * out_gt or out_lidar).  Inputs and outputs are only element-aligned; no output may alias an input.  Nothing outside the
 * rows and columns the taps reach is read.  frame_status: int32 [B], nullable, 0 or DTFILL_NYU_INDEX_ERROR, final when the
 * stream reaches the end of the call.  workspace: ws_bytes >= dtfill_nyu_read_workspace_bytes(B, H, W), 256-B aligned, no
 * initialisation needed, nothing kept between calls.  Asynchronous on `stream`; no allocation, no host synchronisation,
 * re-entrant across streams.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for rgb and depth both NULL, an output without its input, an input
 * without an output, or a NULL workspace; DTFILL_ERR_SHAPE for B, hin, win, H, W < 1, B > 65535, H > hin, W > win, a radius
 * outside [0, DTFILL_NYU_MAX_RADIUS], taps that are NULL with r > 0 or not NULL with r == 0, C outside 1..4 (with rgb), an
 * unknown layout, n < 0, or B*C*hin*win, B*hin*win, B*H*W*C, B*H*W or B*n*2 >= 2^31; DTFILL_ERR_WORKSPACE for a workspace too
 * small or not aligned; then DTFILL_ERR_LAUNCH if a launch failed.
 */
#define DTFILL_NYU_MAX_RADIUS 8  /* the largest filter radius per axis: sigma < 2.125, factors below 5.25 */
#define DTFILL_NYU_INDEX_ERROR 1 /* status bit: a sample of the frame lies outside [0, H) x [0, W) and was skipped */
size_t dtfill_nyu_read_workspace_bytes(int B, int H, int W); /* 0 on a bad shape */
int dtfill_nyu_read(const uint8_t *rgb, const float *depth, int B, int C, int hin, int win, int H, int W, const double *wy,
                    int ry, const double *wx, int rx, const int32_t *samples, int n, int normalize, int layout,
                    float *out_rgb, float *out_gt, float *out_lidar, int32_t *frame_status, void *workspace, size_t ws_bytes,
                    void *stream);

/*
 * map_points_on_image() of subsample_Lidar_train.py:180-193 / subsample_Lidar_val.py:167-180, on B point clouds at once: points
 * in the Velodyne frame through E and K, rounded to a pixel, depth_map[v, u] = z.  The front of the pipeline for a caller who
 * holds point clouds (KITTI raw .bin: float32 x, y, z, reflectance) and not frames; dtfill_line_subsample() skips this step
 * because there the points came from a frame.  Two modes: the reference's assignment literally, and the z-buffered projection
 * (nearest return per pixel) that sparse-depth maps are built with.
 *
 * points: float32 [B, N, stride], stride 3 or 4 (the 4th float is carried and ignored: a .bin buffer needs no repacking), only
 * element-aligned.  counts: int32 [B], counts[b] = n_b, the number of frame b's records in use; NULL means N everywhere.  Only
 * floats of the first n_b records of a frame are read: no padding record of a ragged batch.  K: float64 [B,3,3] intrinsics;
 * E: float64 [B,4,4] velo->cam extrinsics (dtfill_line_subsample's conventions; row 3 of E is not read).
 *
 * Per point i < n_b, everything in IEEE double, no contraction, left to right as written:
 *   X, Y, Z = the three floats widened;
 *   c_r = E[r][0]*X + E[r][1]*Y + E[r][2]*Z + E[r][3]   for r = 0..2;
 *   h_r = K[r][0]*c_0 + K[r][1]*c_1 + K[r][2]*c_2;
 *   z = h_2,  u = rint(h_0 / z),  v = rint(h_1 / z), round half to even as np.round does.
 *
 * DTFILL_PROJ_REFERENCE: map_points_on_image literally.  A frame is valid when every point has finite u, v with u in [-W, W)
 *   and v in [-H, H); a negative index wraps (u += W, v += H), as numpy's does.  Any point that violates this makes the frame
 *   an index-error frame (the reference's assignment raises IndexError): its outputs are all +0.0 and its status
 *   DTFILL_PROJ_INDEX_ERROR.  In a valid frame a pixel holds the z of the LARGEST i that landed on it (numpy assigns in order:
 *   the last writer wins); any z is written, whatever its sign, +-inf included; pixels no point reached are +0.0.  min_z is
 *   ignored.  INSIDE counts every one of the n_b points, BEHIND and OUTSIDE are 0.
 * DTFILL_PROJ_ZBUFFER: a point is dropped in exactly these cases, checked in this order:
 *   1. X, Y or Z is not finite, or z is not finite, or !(z > (double)min_z): counted as BEHIND;
 *   2. u or v is not finite or lies outside [0, W) x [0, H) (no wrap): counted as OUTSIDE.
 *   Among the points that land on a pixel the SMALLEST z wins, compared as doubles; among equal z the largest i (they hold
 *   the same bits).  min_z must be finite and >= 0, else DTFILL_ERR_SHAPE.
 * Both modes:
 *   counts[b] outside [0, N]: DTFILL_PROJ_BAD_COUNT, outputs all +0.0, nothing of that frame is read;
 *   DTFILL_PROJ_NO_POINTS is set when nothing landed (REFERENCE: n_b == 0); the outputs are then all +0.0 anyway;
 *   out_f64[b][v][u] holds the winner's z bit for bit (the reference's float64 map; its callers' (map * 256).astype(np.uint16)
 *     stays on the host); out_f32 holds (float)z, one round-to-nearest-even conversion: what dtfill_batch() takes.  Not both
 *     NULL; both fully overwritten; neither may alias an input;
 *   frame_status: int32 [B], nullable, DTFILL_PROJ_* bits; frame_counts: int32 [B, DTFILL_PROJ_N], nullable, columns PIXELS
 *     (distinct pixels written), INSIDE (points that landed), BEHIND, OUTSIDE; all four are zero in a frame with a status bit
 *     other than NO_POINTS.
 * workspace: at least dtfill_project_points_workspace_bytes(B, N, H, W) bytes, 256-B aligned, the caller's, no initialisation
 * needed (the kernels clear what they accumulate into), nothing kept between calls.  Asynchronous on `stream`; no allocation, no
 * host synchronisation, re-entrant across streams.  The winner is decided by integer comparisons (a max of i + 1, a min of z's
 * bit pattern), never by the order in which atomics arrive: the same bits on every run.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL points, K, E or workspace, or both outputs NULL;
 * DTFILL_ERR_SHAPE for B, N, H, W < 1, B > 65535, stride not 3 or 4, B*N*stride >= 2^31, B*H*W >= 2^31, an unknown mode or a
 * bad min_z; DTFILL_ERR_WORKSPACE for a workspace too small or not aligned; then DTFILL_ERR_LAUNCH if a launch failed.
 */
#define DTFILL_PROJ_REFERENCE 0 /* mode: the reference's in-order assignment, negative indices wrap */
#define DTFILL_PROJ_ZBUFFER   1 /* mode: nearest return per pixel, points behind min_z or outside the frame dropped */
#define DTFILL_PROJ_NO_POINTS   1 /* status bit: nothing landed in the frame */
#define DTFILL_PROJ_INDEX_ERROR 2 /* status bit (REFERENCE): a point's pixel lies outside the wrap range or is not finite */
#define DTFILL_PROJ_BAD_COUNT   4 /* status bit: counts[b] outside [0, N] */
#define DTFILL_PROJ_PIXELS  0 /* frame_counts columns */
#define DTFILL_PROJ_INSIDE  1
#define DTFILL_PROJ_BEHIND  2
#define DTFILL_PROJ_OUTSIDE 3
#define DTFILL_PROJ_N 4
size_t dtfill_project_points_workspace_bytes(int B, int N, int H, int W); /* 0 on a bad shape (B*N*3 >= 2^31 included) */
int dtfill_project_points(const float *points, const int32_t *counts /* nullable */, int B, int N, int stride,
                          int H, int W, const double *K, const double *E, int mode, float min_z,
                          float *out_f32 /* nullable */, double *out_f64 /* nullable */,
                          int32_t *frame_status /* nullable */, int32_t *frame_counts /* nullable */,
                          void *workspace, size_t ws_bytes, void *stream);

/*
 * Back-projection, the inverse of dtfill_project_points: depth frames to ordered point clouds in the Velodyne frame.  With
 * keep_every == 0 it is get_all_points() of subsample_Lidar_train.py:125-141 / subsample_Lidar_val.py:112-128, with
 * keep_every >= 1 the scripts' get_all_points -> calculate_angle -> sample (their `left_points`); a dense frame (a fill's
 * depth output) gives the pseudo-LiDAR cloud.
 *
 * x: float32 [B,H,W]; payload: float32 [B,H,W], nullable (any per-pixel scalar to carry: an intensity, a confidence);
 * K: float64 [B,3,3]; E: float64 [B,4,4] (dtfill_line_subsample's conventions).
 * VALID: pixel (row v, column u) of frame b is valid iff x > val_thr, a float32 compare: NaN is never valid, +inf is.  val_thr
 *   must not be NaN; the reference's literal is 0.1f.
 * THE POINT of a valid pixel, in IEEE double, no contraction, in exactly dtfill_line_subsample's order, d = (double)x:
 *     p_cam = K^-1 [u, v, 1]^T d,  p = (E^-1 [p_cam; 1])[0:3],  pitch = asin(p.z / |p|)
 *   with K^-1, E^-1 from the same on-device Gauss-Jordan (partial pivoting).  Each coordinate is stored as (float)p_r, one
 *   round-to-nearest-even conversion; pitch[b, i] holds the double bit for bit: the bits dtfill_line_subsample labels with.
 * SELECTION.  keep_every == 0: every valid pixel; n_bins is ignored.  keep_every >= 1 (n_bins >= 1): the valid pixels that
 *   dtfill_line_subsample keeps: pmin, pmax over the frame's valid pixels, interval = (pmax - pmin) / n_bins, kept iff
 *   ceil((pitch - pmin) / interval) mod keep_every == 0, the label not clamped.  With val_thr == 0.1f these are exactly the
 *   non-zero pixels of dtfill_line_subsample's output.
 * ORDER AND LAYOUT.  A frame's selected pixels go out in raster order (row-major), as numpy's boolean-mask indexing yields
 *   them.  Record i of frame b is points[(b*N + i)*stride .. +stride), stride 3 or 4: what dtfill_project_points reads, so
 *   the two calls chain with no repacking.  With stride == 4 the fourth float is payload[b, v, u] bit for bit, +0.0f when
 *   payload is NULL.  pixel[b, i] = v*W + u.  pitch: float64 [B,N], nullable; pixel: int32 [B,N], nullable.
 *   counts: int32 [B, 2]: column DTFILL_UNPROJ_WRITTEN holds n_b = min(total_b, N), column DTFILL_UNPROJ_TOTAL the number of
 *   selected pixels total_b.  When total_b > N the first N points in raster order are written and DTFILL_UNPROJ_OVERFLOW is
 *   set.  Records, pitches and pixels at i >= n_b are NOT written: the caller's bytes stay.  The placement is decided by
 *   counts and prefix sums, never by the order in which atomics arrive: the same bytes on every run.
 * STATUS.  frame_status: int32 [B], nullable, DTFILL_UNPROJ_* bits.  NO_POINTS, BAD_INTERVAL (keep_every >= 1 only) and
 *   SINGULAR have the meanings and values of DTFILL_LINES_*.  A frame with SINGULAR or BAD_INTERVAL writes nothing and has
 *   both counts 0.
 * No output may alias an input.  workspace: at least dtfill_unproject_workspace_bytes(B, H, W) bytes, 256-B aligned, the
 * caller's, no initialisation needed, nothing kept between calls.  Asynchronous on `stream`; no allocation, no host
 * synchronisation, re-entrant across streams.  Every byte offset is a size_t: B*N*stride floats may pass 4 GiB.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, K, E, points, counts or workspace; DTFILL_ERR_SHAPE
 * for B, H, W or N < 1, B > 65535, B*H*W >= 2^31, stride not 3 or 4, B*N*stride >= 2^31 (dtfill_project_points' rule: a legal
 * output is a legal input there), keep_every < 0, keep_every >= 1 with n_bins < 1, or a NaN val_thr; DTFILL_ERR_WORKSPACE for
 * a workspace too small or not aligned; then DTFILL_ERR_LAUNCH if a launch failed.
 *
 * dtfill_unproject_backward: the gradients of a loss with respect to x and payload, given its gradient with respect to the
 * records.  The map is affine in the depth, so x is not needed.  grad_points: float32 [B, N, stride]; pixel and counts as the
 * forward wrote them; grad_x: float32 [B,H,W]; grad_payload: float32 [B,H,W], nullable.
 *   For i < counts[b].WRITTEN and (v, u) decoded from pixel[b, i], in double, left to right:
 *     k = K^-1 [u, v, 1]^T;  j_r = Einv[r][0]*k_0 + Einv[r][1]*k_1 + Einv[r][2]*k_2;
 *     grad_x[b, v, u] = (float)(gX*j_0 + gY*j_1 + gZ*j_2),  gX, gY, gZ the record's three floats widened.
 *   Every other pixel of grad_x is +0.0f.  With stride == 4 and grad_payload non-NULL, grad_payload[b, v, u] is the fourth
 *   float bit for bit, +0.0f elsewhere (and everywhere with stride == 3).
 *   A frame's pixel list must be strictly increasing and inside [0, H*W), as the forward writes it; one that is not sets
 *   DTFILL_UNPROJ_BAD_PIXEL and that frame's gradients are all +0.0f.  A DTFILL_UNPROJ_SINGULAR frame gets all-zero
 *   gradients.  counts[b].WRITTEN outside [0, N] sets DTFILL_UNPROJ_BAD_COUNT: all-zero gradients, nothing of that frame is
 *   read.  A scatter to distinct pixels: no atomics on the gradients, no float accumulation, the same bits on every run.
 * Workspace, stream and aliasing rules as the forward's.  Returns DTFILL_ERR_NULL for a NULL grad_points, pixel, counts, K, E,
 * grad_x or workspace; DTFILL_ERR_SHAPE for B, N, H, W < 1, B > 65535, B*H*W >= 2^31, stride not 3 or 4 or
 * B*N*stride >= 2^31; DTFILL_ERR_WORKSPACE; all before any HIP call; then DTFILL_ERR_LAUNCH.
 */
#define DTFILL_UNPROJ_NO_POINTS    1 /* status bit: no valid pixel in the frame */
#define DTFILL_UNPROJ_BAD_INTERVAL 2 /* status bit (keep_every >= 1): the pitch interval is 0 or not finite */
#define DTFILL_UNPROJ_SINGULAR     4 /* status bit: K or E singular */
#define DTFILL_UNPROJ_OVERFLOW     8 /* status bit: total_b > N, only the first N points were written */
#define DTFILL_UNPROJ_BAD_PIXEL   16 /* status bit (backward): the pixel list is not strictly increasing inside [0, H*W) */
#define DTFILL_UNPROJ_BAD_COUNT   32 /* status bit (backward): counts[b].WRITTEN outside [0, N] */
#define DTFILL_UNPROJ_WRITTEN 0 /* counts columns */
#define DTFILL_UNPROJ_TOTAL   1
size_t dtfill_unproject_workspace_bytes(int B, int H, int W); /* 0 on a bad shape */
int dtfill_unproject(const float *x, const float *payload /* nullable */, int B, int H, int W, float val_thr,
                     const double *K, const double *E, int n_bins, int keep_every /* 0: every valid pixel */,
                     int N, int stride, float *points, double *pitch /* nullable */, int32_t *pixel /* nullable */,
                     int32_t *counts, int32_t *frame_status /* nullable */,
                     void *workspace, size_t ws_bytes, void *stream);
size_t dtfill_unproject_backward_workspace_bytes(int B, int H, int W); /* 0 on a bad shape */
int dtfill_unproject_backward(const float *grad_points, const int32_t *pixel, const int32_t *counts,
                              int B, int N, int stride, int H, int W, const double *K, const double *E,
                              float *grad_x, float *grad_payload /* nullable */, int32_t *frame_status /* nullable */,
                              void *workspace, size_t ws_bytes, void *stream);

/*
 * Error metrics of evaluation.py, one row per frame:
 *   DTFILL_METRICS_KITTI  Result.evaluate, evaluation.py:82-123 (metres -> mm for mse/rmse/mae, -> 1/km for
 *                         irmse/imae; the deltas stay 0 as in the reference);
 *   DTFILL_METRICS_NYU    Result_NYU.evaluate, evaluation.py:196-239 (no unit change, mae = mean(|d|/target),
 *                         delta1..3 = mean(max(o/t, t/o) < 1.25^k)).
 * Elements with output > 0.01 and target > 0.01 count.  Per element the float32 arithmetic of the numpy
 * expressions; the means accumulate in float64 in a fixed order (numpy: float32 pairwise sums), so a result is
 * reproducible, within ~1e-13 relative of the exact (math.fsum) mean of those float32 terms, and within ~1e-6
 * relative of numpy's.  count and delta1..3 are exact.  No valid element: NaN (numpy's mean of nothing).
 * output, target: float32 [B, n] device pointers; out: float64 [B, DTFILL_METRICS_N] device pointer, columns
 * mse, rmse, mae, irmse, imae, delta1, delta2, delta3, count.  workspace: device scratch of at least
 * dtfill_metrics_workspace_bytes(B) bytes.
 */
#define DTFILL_METRICS_KITTI 0
#define DTFILL_METRICS_NYU 1
#define DTFILL_METRICS_N 9
size_t dtfill_metrics_workspace_bytes(int B);
int dtfill_metrics(const float *output, const float *target, int B, long long n, int kind, double *out, void *workspace,
                   size_t ws_bytes, void *stream);

/*
 * The objective of the reference's training step, solution_DeepNet/train.py:210-251, and its gradient: the masked squared
 * error of the prediction and, with --correct, the squared-plus-absolute error of the corrected LiDAR, each divided by a
 * count taken over the whole batch.  pred, corr: the network's depth_predicted and lidar_correction; gt, lidar: the loader's
 * frames after the driver's row crop (train.py:211-212); all float32 [B,H,W].
 *   m  = gt > gt_thr              train.py:215 (KITTI 0.1) / :220 (NYU 0.0001)
 *   mi = m && lidar > in_thr      train.py:216 (0.1) / :221 (0.001), :227
 *   n_gt = |m|, n_in = |mi|, over the batch and the WHOLE frame                                        (:224, :228)
 *   S_main = sum of (pred - gt)^2 over m inside rows [r0, r1) x columns [c0, c1)                       (:240)
 *   S_aux  = sum of (corr - gt)^2 + |corr - gt| over mi, always the whole frame                        (:248)
 *   main = S_main / n_gt (DTFILL_LOSS_KITTI, :244, window 0,H,0,W) or sqrt(S_main / n_gt) (DTFILL_LOSS_NYU, :242, window
 *          6,228,8,304: the sum runs over the window, the count over the frame, as the reference has it)
 *   aux  = S_aux / n_in                                                                                (:249)
 * total = main + aux (:251) is the caller's add.  Both compares are float32 compares, so a NaN is in no mask; the masks are
 * derived while the inputs are read and never stored.
 * Per element float32, one rounding per operation, nothing contracted: t = pred - gt, e = t * t; u = corr - gt,
 * a = u * u + fabsf(u).  A term is added only where its mask (and, for e, the window) selects it, so a non-finite pred or
 * corr at an unselected pixel leaves no trace: the same deliberate deviation from the reference's x * mask as
 * dtfill_generate_multi_channel's.  S_main and S_aux accumulate in float64 in an order that is a function of B*H*W alone (no
 * atomics; neither the pointers' alignment nor the window changes it): two calls give the same bits, within n_terms * 2^-53
 * relative of the exact sum of those float32 terms.  TensorFlow sums in float32 in an order it does not document, so the order
 * is this library's contract, not a property of the reference.  n_gt and n_in are exact.
 * stats: DEVICE double[DTFILL_LOSS_N] = main, aux, n_gt, n_in, S_main, S_aux; the divisions and the root in double; an empty
 * mask gives 0 / 0 = NaN, like the reference.  corr == NULL (no --correct): aux, n_in and S_aux are +0 and lidar is not read.
 * workspace: at least dtfill_train_loss_workspace_bytes(B,H,W) bytes, 256-B aligned, the caller's, no initialisation needed,
 * nothing kept between calls.
 *
 * dtfill_train_loss_backward: the gradients of g_main * main + g_aux * aux, in float32 (2 * t is exact):
 *   k_main = (float)(g_main / n_gt)  (KITTI)  or  (float)(g_main / ((2 * main) * n_gt))  (NYU: main == 0 gives 0 * inf = NaN)
 *   k_aux  = (float)(g_aux / n_in)
 *   grad_pred = (2 * t) * k_main where m inside the window, +0.0f elsewhere
 *   grad_corr = (2 * u + sgn(u)) * k_aux where mi, +0.0f elsewhere; sgn(0) = 0; one rounded add, one rounded multiply
 * The divisions are in double, from stats (what dtfill_train_loss wrote for the same arguments) and the DEVICE float scalars
 * g_main and g_aux, and are rounded to float32 once.  A NULL g_* is a zero gradient: that output is all +0.  grad_pred and
 * grad_corr: float32 [B,H,W], each nullable but not both, always fully overwritten, may alias no input.  gt and lidar get no
 * gradient.
 *
 * Both calls are asynchronous on `stream`, read stats and g_* on the device, and neither synchronises nor allocates.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL pred, gt or stats, a NULL workspace, corr without lidar,
 * grad_corr without corr, or both gradients NULL; DTFILL_ERR_SHAPE for B, H or W < 1, B*H*W >= 2^31, or a window that is empty
 * or not inside the frame; DTFILL_ERR_METRIC for an unknown kind; DTFILL_ERR_WORKSPACE for a workspace that is too small or
 * not aligned.
 */
#define DTFILL_LOSS_KITTI 0 /* main = S_main / n_gt        train.py:244 */
#define DTFILL_LOSS_NYU   1 /* main = sqrt(S_main / n_gt)  train.py:242 */
#define DTFILL_LOSS_N 6     /* stats columns: main, aux, n_gt, n_in, S_main, S_aux */
size_t dtfill_train_loss_workspace_bytes(int B, int H, int W); /* 0 on a bad shape */
int dtfill_train_loss(const float *pred, const float *corr /* nullable */, const float *gt,
                      const float *lidar /* nullable iff corr is */, int B, int H, int W, int kind, float gt_thr, float in_thr,
                      int r0, int r1, int c0, int c1, double *stats, void *workspace, size_t ws_bytes, void *stream);
int dtfill_train_loss_backward(const float *pred, const float *corr, const float *gt, const float *lidar, int B, int H, int W,
                               int kind, float gt_thr, float in_thr, int r0, int r1, int c0, int c1, const double *stats,
                               const float *g_main, const float *g_aux /* device scalars, each nullable */,
                               float *grad_pred, float *grad_corr /* each nullable, not both */, void *stream);

/*
 * The backward pass of the exact fill out_depth = depth_list[lbl - 1] (tools.py:22-26): the gradient of a loss with respect to
 * x, given its gradient with respect to out_depth.  The reference runs this gather in numpy outside the graph; here it can sit
 * behind a learned correction.  x and index are dtfill_batch()'s input and out_index (either metric: a label means the same
 * thing in both).  The predicates and the labels are constants of the differentiation, so the backward is the gather transposed
 * literally: the k-th VALUED pixel receives the gradient of every pixel that read depth_list[k] -- not the nearest source,
 * wherever the source and the value predicate disagree.  Per frame:
 *   the value list is the pixels with x > val_thr in raster order; n its length, v_k the pixel of its k-th entry;
 *   idx(p) = index[p] - 1, and idx(p) += n if it is negative: numpy's wrap, so label 0 in a frame with a non-empty value list
 *     addresses the LAST value;
 *   if any pixel's idx falls outside [0, n) -- n == 0, or a label larger than n -- the frame is an index-error frame: grad_x is
 *     +0.0 everywhere in it and frame_status[b] = DTFILL_FRAME_INDEX_ERROR; otherwise frame_status[b] = 0.  The call derives
 *     this itself, it does not take the forward's status, and any 32-bit content of index is memory-safe;
 *   otherwise grad_x[v_k] = S(C_k) for the cell C_k = {grad_depth[p] : idx(p) = k}, and +0.0 at every pixel outside the list.
 *
 * The cell sum S(C), defined so that it does not depend on the order of the additions:
 *   an empty cell, or one whose terms are all +-0: +0.0;
 *   a cell with any NaN term, or with both +inf and -inf: the quiet NaN 0x7FC00000;
 *   otherwise a cell with any +inf: +inf; with any -inf: -inf;
 *   otherwise E = the largest true binary exponent floor(log2 |g|) over the cell's non-zero terms (a subnormal counts by its
 *     true exponent), q = E - 37;
 *   every term becomes the integer t = rint(g * 2^-q), round half to even: exact for every term within 14 binades of the
 *     largest; |t| < 2^38;
 *   T = the sum of the t in integers (no int64 overflow: H + W - 2 < 8192 keeps a frame below 2^24.001 pixels);
 *   S = ldexpf(f32(T), q), f32(T) the single round-to-nearest-even conversion of the integer, the scaling IEEE (exact unless
 *     it lands in the subnormal range or overflows); T = 0 gives +0.0.
 * So |S - exact sum| <= |C| * 2^(E-38) + 2^-24 * |exact sum| + 2^-149, and [1e8, 1, -1e8] gives 1.0 where a float32 running
 * sum gives 0.0.  The accumulators are integers (a max, an OR, a 64-bit add, all by atomics): two calls give the same bits.
 *
 * x, grad_depth, grad_x: float32 [B,H,W]; index: int32 [B,H,W]; grad_x is always fully overwritten and may alias no input;
 * frame_status: int32 [B], nullable.  workspace: at least dtfill_fill_backward_workspace_bytes(B,H,W) bytes, 256-B aligned,
 * the caller's, no initialisation needed (the kernels clear what they accumulate into), nothing kept between calls.
 * Asynchronous on `stream`; no allocation, no host synchronisation.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, index, grad_depth, grad_x or workspace;
 * DTFILL_ERR_SHAPE for dtfill_batch()'s shape rule; DTFILL_ERR_WORKSPACE for a workspace that is too small or not aligned;
 * then DTFILL_ERR_LAUNCH if a launch failed.
 */
size_t dtfill_fill_backward_workspace_bytes(int B, int H, int W); /* 0 on a bad shape; the forward's shape rule */
int dtfill_fill_backward(const float *x, const int32_t *index, const float *grad_depth, int B, int H, int W,
                         float val_thr, float *grad_x, int32_t *frame_status /* nullable */,
                         void *workspace, size_t ws_bytes, void *stream);

/*
 * Label -> source pixel: any channels filled from the nearest source, and the nearest-source pixel map itself.  A label of
 * dtfill_batch()'s out_index is a raster rank among the frame's sources (either metric: a label means the same thing in both);
 * this call turns it back into the source's pixel and copies C channels of a second tensor from there.  So the sources are
 * decided by one tensor (x) and the payload is read from another (values): the exact fill behind a learned correction
 * (net.py:131-155: the mask from input_lidar, the values from lidar_correct), many channels behind one dtfill_batch() pass, and
 * what scipy.ndimage.distance_transform_edt(return_indices=True) returns (the l2 metric).  Per frame b:
 *   the source list is the pixels with NOT((1.0f - x) > src_thr), evaluated in float32, in raster order: dtfill_batch()'s
 *     source predicate, a NaN is a source; m its length, s_k the flat pixel row*W + col of its k-th entry;
 *   a pixel p with L = index[b][p], 1 <= L <= m: out_pixel[b][p] = s_{L-1}, and out_values[b][c][p] has the bits of
 *     values[b][c][s_{L-1}] for every channel c: a copy, so NaN payloads, -0.0 and subnormals come through unchanged;
 *   L == 0 (dtfill_batch()'s label in a frame without a source): out_pixel = -1 and out_values = +0.0.  There is no numpy wrap
 *     here: that belongs to depth_list[lbl - 1], which dtfill_batch()'s out_depth keeps reproducing;
 *   L < 0 or L > m: that pixel gets -1 / +0.0 and the frame's status DTFILL_FRAME_INDEX_ERROR.  The rule is per pixel, the
 *     frame's other pixels are served, and any 32-bit content of index is memory-safe, INT32_MIN and INT32_MAX included;
 *   frame_status[b] = (m == 0 ? DTFILL_FRAME_NO_SOURCE : 0) | (a label outside [0, m] ? DTFILL_FRAME_INDEX_ERROR : 0).
 * With DTFILL_FLAG_OUTLIER_REMOVAL in the forward the x to pass is the filtered one (dtfill_outlier_removal()'s output): the
 * labels count the sources the forward saw.
 *
 * x: float32 [B,H,W]; index, out_pixel: int32 [B,H,W]; values, out_values: float32 [B,C,H,W], 0 <= C <= DTFILL_NEAR_MAX_C.
 * values and out_values are NULL together, out_pixel may be NULL, not both outputs; with C == 0 values and out_values are NULL
 * and the call produces the pixel map alone.  Every output given is fully overwritten and may alias no input.
 * frame_status: int32 [B], nullable.  workspace: at least dtfill_nearest_gather_workspace_bytes(B,H,W) bytes, 256-B aligned,
 * the caller's, no initialisation needed, nothing kept between calls.  Asynchronous on `stream`; no allocation, no host
 * synchronisation.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, index or workspace, both outputs NULL, or exactly one
 * of values / out_values NULL; DTFILL_ERR_SHAPE for dtfill_batch()'s shape rule, C outside [0, DTFILL_NEAR_MAX_C], or C == 0
 * with values; DTFILL_ERR_WORKSPACE for a workspace that is too small or not aligned; then DTFILL_ERR_LAUNCH if a launch failed.
 */
#define DTFILL_NEAR_MAX_C 64
size_t dtfill_nearest_gather_workspace_bytes(int B, int H, int W); /* 0 on a bad shape; the forward's shape rule */
int dtfill_nearest_gather(const float *x, const int32_t *index, const float *values /* nullable */, int C,
                          int B, int H, int W, float src_thr,
                          float *out_values /* nullable */, int32_t *out_pixel /* nullable */,
                          int32_t *frame_status /* nullable */, void *workspace, size_t ws_bytes, void *stream);

/*
 * The backward of dtfill_nearest_gather() with respect to values, given the gradient with respect to out_values.  x and index
 * are constants of the differentiation, so it is the gather transposed literally, with the source list, m and s_k as above:
 *   grad_values[b][c][s_k] = S({grad_out[b][c][p] : index[b][p] - 1 == k}) for every source, S the cell sum stated at
 *     dtfill_fill_backward() (integer accumulators: the same bits on every run), and +0.0 at every pixel that is not a source;
 *   labels outside [1, m] contribute nowhere; the status is the forward's, derived here again.
 * grad_out, grad_values: float32 [B,C,H,W], 1 <= C <= DTFILL_NEAR_MAX_C; grad_values is fully overwritten and may alias no
 * input.  workspace: at least dtfill_nearest_gather_backward_workspace_bytes(B,H,W,C) bytes, 256-B aligned, no initialisation
 * needed.  The channels run in rounds that share one set of accumulators, so that size is non-decreasing in C and for every C
 * no larger than its value at C = 4.  Asynchronous on `stream`; no allocation, no host synchronisation.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, index, grad_out, grad_values or workspace;
 * DTFILL_ERR_SHAPE for dtfill_batch()'s shape rule or C outside [1, DTFILL_NEAR_MAX_C]; DTFILL_ERR_WORKSPACE; then
 * DTFILL_ERR_LAUNCH if a launch failed.
 */
size_t dtfill_nearest_gather_backward_workspace_bytes(int B, int H, int W, int C); /* 0 on a bad shape */
int dtfill_nearest_gather_backward(const float *x, const int32_t *index, const float *grad_out, int C,
                                   int B, int H, int W, float src_thr, float *grad_values,
                                   int32_t *frame_status /* nullable */, void *workspace, size_t ws_bytes, void *stream);

/*
 * dtfill_conv2d_backward_data and dtfill_conv2d_backward_weights: the gradients of dtfill_conv2d with respect to x, and to w
 * and bias, in float32 with every output bit fixed by this statement, so that the layers of SparsityCNN can be trained
 * (train.py:232-254: a forward under a tape, the masked loss, the gradients of every variable).  The domain is
 * dtfill_conv2d's: ksize 1, 3, 5 or 7, Cin 1, 16, 32, 48 or 64, Cout 1 or 16, stride 1, 'same', NHWC.
 *
 * dy: float32 [B,H,W,dy_channels], the gradient of the loss with respect to the layer's output, read at the channels
 * dy_offset .. dy_offset + Cout - 1 (the counterpart of out_channels and out_offset: each stem reads its 16 channels of
 * conv1a's 64-wide input gradient).  y: float32 [B,H,W,y_channels], the forward's output, read at y_offset likewise; NULL is
 * allowed when act is DTFILL_CONV_LINEAR, and y is not read then.  x, w: the forward's.  Nothing else of dy's or y's tensor
 * is read or written.
 *
 * THE CONTRACTS.
 * The activation's derivative, per (b, h, v, o):
 *   g = act == DTFILL_CONV_LEAKY ? (y > 0 ? dy : dy * alpha) : dy
 * a float32 compare on the forward OUTPUT and one rounded multiply: tf.nn.leaky_relu's gradient.  With alpha >= 0 the sign of
 * y is the sign of the pre-activation, so it is the derivative at the pre-activation too; alpha < 0 is refused.  y == +-0
 * and a NaN y take the alpha branch.
 *
 * dtfill_conv2d_backward_data.  dx: float32 [B,H,W,dx_channels], written at dx_offset .. dx_offset + Cin - 1, the rest left
 * untouched.  dx is dtfill_conv2d's own chain applied to g under the kernel flipped and its channel axes exchanged,
 *   wT[i, j, o, c] = w[ksize - 1 - i, ksize - 1 - j, c, o],
 * without bias or activation.  Per (b, h, v, c), r = (ksize - 1) / 2:
 *   acc = +0
 *   for G in 0 .. ceil(Cout / 16) - 1:                         groups of 16 of the Cout channels, outermost
 *     for i in 0 .. ksize - 1:  for j in 0 .. ksize - 1:       the taps in raster order
 *       for o in 16 G .. min(16 G + 15, Cout - 1):
 *         a = g[b, h + i - r, v + j - r, o] inside the frame, +0.0f outside it
 *         acc = fmaf(a, wT[i, j, o, c], acc)
 *   dx[b, h, v, c] = acc
 * So dx equals dtfill_conv2d(g, wT) (Cin of 32, 48 or 64: dtfill_conv2d_strided(g, wT) at stride 1) bit for bit.
 *
 * dtfill_conv2d_backward_weights.  dw: float32 [ksize,ksize,Cin,Cout]; db: float32 [Cout], nullable; both fully overwritten.
 * A sum over all B H W pixels, in two levels.  A segment (b, t, s) is frame b, rows [R t, R t + R), columns [C s, C s + C),
 * cut at the frame's edges, R = DTFILL_CONV_BW_ROWS and C = DTFILL_CONV_BW_COLS; there are ceil(H / R) ceil(W / C) a frame.
 *   level 1, per segment and per (i, j, c, o):
 *     p = +0
 *     for (h, v) in the segment's pixels, in raster order:
 *       a = x[b, h + i - r, v + j - r, c] inside the frame, +0.0f outside it
 *       p = fmaf(a, g[b, h, v, o], p)
 *   level 2:
 *     acc = +0
 *     for b: for t: for s:  acc = acc + p(b, t, s)            one rounded add each
 *     dw[i, j, c, o] = acc
 * db[o] is the same with a = 1.0f everywhere.  The segment size is part of the contract: it fixes the bits.  It is not a
 * tuning parameter of a device, and the bits do not depend on the grid, the CU count, the stream or the run.
 * +0 and -0 count as equal (zero operands pad a matrix-core step at a row's end; level 2 starts from +0).  Non-finite values
 * follow fmaf.  A float32 evaluation in any other order lies within gamma_(R C + S) sum |x| |g| of dw, S the number of
 * segments, gamma_n as in dtfill_conv2d.
 *
 * workspace: dtfill_conv2d_backward_workspace_bytes(B, H, W, Cin, ksize, Cout) bytes, 256-byte aligned; one size serves both
 * calls (g and wT for the data gradient: 4 (B H W Cout + ksize^2 Cin Cout) bytes and alignment; the segments' partials for
 * the weights': 4 S (ksize^2 Cin + 1) Cout bytes).  Pure host arithmetic; 0 for a shape outside the domain.
 * Pointers need float alignment only.  Both calls are asynchronous on `stream`: no allocation, no float atomics, no host
 * synchronisation.  dx may not alias dy or y.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL dy, w, dx (x, dy, dw for the weights), workspace, or a
 * NULL y under DTFILL_CONV_LEAKY; DTFILL_ERR_SHAPE unless the shape is in dtfill_conv2d's domain, every offset lies in its
 * tensor (0 <= offset, offset + channels <= width), B H W max(Cin, every width) < 2^31, act is one of the two values and
 * alpha is finite and >= 0; DTFILL_ERR_WORKSPACE for a workspace too small or not aligned; then DTFILL_ERR_LAUNCH.
 */
enum {
    DTFILL_CONV_BW_ROWS = 32, /* R: rows of a segment of the weight gradient's sum */
    DTFILL_CONV_BW_COLS = 64  /* C: columns of it */
};
size_t dtfill_conv2d_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout);
int dtfill_conv2d_backward_data(const float *dy, int dy_channels, int dy_offset,
                                const float *y /* nullable if linear */, int y_channels, int y_offset,
                                const float *w, int B, int H, int W, int Cin, int ksize, int Cout,
                                int act, float alpha,
                                float *dx, int dx_channels, int dx_offset,
                                void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_backward_weights(const float *x,
                                   const float *dy, int dy_channels, int dy_offset,
                                   const float *y /* nullable if linear */, int y_channels, int y_offset,
                                   int B, int H, int W, int Cin, int ksize, int Cout,
                                   int act, float alpha,
                                   float *dw, float *db /* nullable */,
                                   void *workspace, size_t ws_bytes, void *stream);

/*
 * dtfill_conv2d_strided_backward_data, _weights and dtfill_conv2d_transpose_backward_data, _weights: the gradients of the wide
 * layers below, dtfill_conv2d_strided and dtfill_conv2d_transpose, in the same sense as the two calls above, whose statements
 * they extend: every output bit is fixed here, so that ResNet18_NO_BN_l2 can be trained (train.py:113, 232-254).  The
 * reference declares kernel_regularizer=l2(0.05) on its layers, and train.py:253 differentiates total_loss alone without
 * depth_network.losses: the gradient to reproduce has no weight-decay term, and nothing here adds one.
 *
 * B, H, W, Cin: the FORWARD's input shape, as in the forward calls; x: [B,H,W,Cin].  dy and y live on the forward's output
 * frame, [B,Ho,Wo,.] with Ho = ceil(H / stride) for the strided layer and [B,2H,2W,.] for the transposed one, and are read at
 * a channel offset of a wider tensor, as above.  g = y > 0 ? dy : dy * alpha, as above, on that frame.
 * The domain: Cin and Cout multiples of 16 and at least 16.  Stride 1: ksize 1, 3, 5 or 7.  Stride 2: ksize 1 or 3, and H and
 * W EVEN for both strided backward calls: narrower than the forward's domain, which takes odd frames (pt = 1 there); the
 * reference's networks cannot run on them, because their own concat fails.  An odd frame at stride 2 is DTFILL_ERR_SHAPE.
 * With H and W even, pt = pl = 0 at stride 2.  The transposed layer is the forward's: 3x3, stride 2.
 *
 * THE CONTRACTS.
 * dresidual (strided data call, nullable): float32 [B,Ho,Wo,Cout], dense; dresidual = g.  The forward adds the residual in
 * front of the activation, so the residual's gradient is g itself.
 *
 * dx of dtfill_conv2d_strided, stride 1: the statement of dtfill_conv2d_backward_data with Cout any multiple of 16: groups of
 * 16 of the Cout channels outermost, the taps in raster order, wT[i, j, o, c] = w[ksize - 1 - i, ksize - 1 - j, c, o].  dx
 * equals dtfill_conv2d_strided(g, wT) at stride 1 bit for bit.  A float32 evaluation in any other order lies within
 * gamma_K sum |g| |w|, K = ksize^2 Cout.
 *
 * dx of dtfill_conv2d_strided, stride 2, 3x3, H and W even: dtfill_conv2d_transpose's chain over g [B,H/2,W/2,Cout] under
 *   wX[ky, kx, o, c] = w[ky, kx, c, o]                          the channel axes exchanged, NO flip
 * without bias or activation.  Per (b, h, v, c):
 *   acc = +0
 *   for G in 0 .. Cout / 16 - 1:
 *     for ky in 0 .. 2:  for kx in 0 .. 2:                     only the taps with h - ky and v - kx both even
 *       for o in 16 G .. 16 G + 15:
 *         a = g[b, (h - ky) / 2, (v - kx) / 2, o] inside the frame, +0.0f outside it (index -1, at h = 0 or v = 0 under tap 2)
 *         acc = fmaf(a, w[ky, kx, c, o], acc)
 *   dx[b, h, v, c] = acc
 * (pt = pl = 0: exactly the case dtfill_conv2d_transpose's contract was written for.)  Within gamma_K sum |g| |w|, K = 4 Cout.
 *
 * dx of dtfill_conv2d_strided, stride 2, 1x1: the same chain with the single tap (0, 0).  For h and v both even
 *   acc = +0;  for o in 0 .. Cout - 1:  acc = fmaf(g[b, h / 2, v / 2, o], w[0, 0, c, o], acc);  dx[b, h, v, c] = acc
 * and every other dx is +0.0f, also where g is not finite elsewhere: no zero weight stands in for a missing tap.
 * Within gamma_Cout sum |g| |w|.
 *
 * dx of dtfill_conv2d_transpose.  w is the packed [3,3,Cin,Cout] the forward takes.  dx equals dtfill_conv2d_strided(g, wX,
 * stride 2) on the [2H,2W] frame with wX[ky, kx, o, c] = w[ky, kx, c, o] bit for bit.  Per (b, h, v, c):
 *   acc = +0
 *   for G in 0 .. Cout / 16 - 1:  for ky in 0 .. 2:  for kx in 0 .. 2:  for o in 16 G .. 16 G + 15:
 *     a = g[b, 2 h + ky, 2 v + kx, o] inside [2H,2W], +0.0f outside it (row 2H, column 2W)
 *     acc = fmaf(a, w[ky, kx, c, o], acc)
 * Within gamma_K sum |g| |w|, K = 9 Cout.
 *
 * dw and db of dtfill_conv2d_strided: the two levels of dtfill_conv2d_backward_weights with the segments laid over the OUTPUT
 * frame [Ho,Wo]; R and C are the same constants.  pt and pl are the forward's ((ksize - 1) / 2 at stride 1, 0 at stride 2).
 *   level 1, per segment and per (i, j, c, o):
 *     p = +0
 *     for (h, v) in the segment's output pixels, in raster order:
 *       a = x[b, stride h + i - pt, stride v + j - pl, c] inside the frame, +0.0f outside it
 *       p = fmaf(a, g[b, h, v, o], p)
 *   level 2: acc = +0;  for b: for t: for s:  acc = acc + p(b, t, s);  dw[i, j, c, o] = acc
 * db[o] with a = 1.0f.  At stride 1 with Cout == 16 (Cin 16 .. 64) these are the bits of dtfill_conv2d_backward_weights.
 * Within gamma_(min(R C, Ho Wo) + S) sum |x| |g|, S the number of segments.
 *
 * dw and db of dtfill_conv2d_transpose: the segments lie over the INPUT frame [H,W], the small one; dw is in the packed layout
 * [3,3,Cin,Cout] (Keras's kernel gradient is dw with its last two axes exchanged).
 *   level 1, per segment and per (ky, kx, c, o):
 *     p = +0
 *     for (h, v) in the segment's input pixels, in raster order:
 *       p = fmaf(x[b, h, v, c], g[b, 2 h + ky, 2 v + kx, o] inside [2H,2W] else +0.0f, p)
 *   db, per segment and per o: four chains q[ky][kx], ky, kx in {0, 1}, over the same pixels in the same order,
 *       q[ky][kx] = fmaf(1.0f, g[b, 2 h + ky, 2 v + kx, o], q[ky][kx])
 *     and the segment's partial is ((q[0][0] + q[0][1]) + q[1][0]) + q[1][1], each a rounded add: every output pixel is
 *     counted exactly once.
 *   level 2 as above.
 * Within gamma_(min(R C, H W) + S) sum |x| |g| for dw and gamma_(min(R C, H W) + S + 3) sum |g| for db.
 * +0 and -0 count as equal; non-finite values follow fmaf; the bits depend on the inputs and the shape alone.
 *
 * workspace: dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, Cin, ksize, Cout, stride, transposed) bytes, 256-byte
 * aligned; transposed != 0 asks for ksize 3 and stride 2.  One size serves the data and the weights call of a layer: g and the
 * repacked weights (and, 1x1 at stride 2, the chain's B Ho Wo Cin values before they are spread) for the data gradient, the
 * partials 4 S (ksize^2 Cin + 1) Cout bytes for the weights'.  Pure host arithmetic; 0 outside the domain.
 * Pointers need float alignment only.  All four calls are asynchronous on `stream`: no allocation, no float atomics, no host
 * synchronisation.  dx and dresidual may not alias dy, y or each other.
 * Returns, all checked before any HIP call and in the order of the calls above: DTFILL_ERR_NULL for a NULL dy, w, dx (x, dy,
 * dw for the weights), workspace, or a NULL y under DTFILL_CONV_LEAKY; DTFILL_ERR_SHAPE unless the shape is in the domain
 * above, every offset lies in its tensor, every tensor has fewer than 2^31 elements (B H W max(Cin, dx_channels), B Ho Wo
 * max(Cout, dy_channels, y_channels), (ksize^2 Cin + 1) Cout), act is one of the two values and alpha is finite and >= 0;
 * DTFILL_ERR_WORKSPACE for a workspace too small or not aligned; then DTFILL_ERR_LAUNCH.
 */
size_t dtfill_conv2d_wide_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout, int stride, int transposed);
int dtfill_conv2d_strided_backward_data(const float *dy, int dy_channels, int dy_offset,
                                        const float *y /* nullable if linear */, int y_channels, int y_offset,
                                        const float *w, int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                        int act, float alpha,
                                        float *dx, int dx_channels, int dx_offset, float *dresidual /* nullable */,
                                        void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_strided_backward_weights(const float *x,
                                           const float *dy, int dy_channels, int dy_offset,
                                           const float *y /* nullable if linear */, int y_channels, int y_offset,
                                           int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                           int act, float alpha,
                                           float *dw, float *db /* nullable */,
                                           void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_transpose_backward_data(const float *dy, int dy_channels, int dy_offset,
                                          const float *y /* nullable if linear */, int y_channels, int y_offset,
                                          const float *w /* packed [3,3,Cin,Cout] */, int B, int H, int W, int Cin, int Cout,
                                          int act, float alpha,
                                          float *dx, int dx_channels, int dx_offset,
                                          void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_transpose_backward_weights(const float *x,
                                             const float *dy, int dy_channels, int dy_offset,
                                             const float *y /* nullable if linear */, int y_channels, int y_offset,
                                             int B, int H, int W, int Cin, int Cout,
                                             int act, float alpha,
                                             float *dw /* packed layout */, float *db /* nullable */,
                                             void *workspace, size_t ws_bytes, void *stream);

/*
 * dtfill_conv2d_image and dtfill_conv2d_image_backward_weights: the layer that reads the image, img_conv = Conv2D(64, (3,3)) of
 * ResNet18_NO_BN_l2_image (solution_DeepNet/net.py:3407, 3645) and of its _light_image and _large_image kin, on the [B,H,W,3]
 * tensor dtfill_rgb_read() emits, in the same sense as dtfill_conv2d below: every output bit is fixed here.
 *
 * dtfill_conv2d_image.  Stride 1, 'same', NHWC.  x: float32 [B,H,W,Cin], Cin 2, 3 or 4; w: float32 [ksize,ksize,Cin,Cout], a
 * Keras Conv2D.kernel as stored (cross-correlation); ksize 1, 3, 5 or 7; Cout a multiple of 16, at least 16; bias: [Cout],
 * nullable; act, alpha, out, out_channels and out_offset as in dtfill_conv2d.
 * THE CONTRACT is dtfill_conv2d's statement with its single group (Cin < 16).  Per output (b, h, v, o), r = (ksize - 1) / 2:
 *   acc = +0
 *   for i in 0 .. ksize - 1:  for j in 0 .. ksize - 1:         the taps in raster order
 *     for c in 0 .. Cin - 1:
 *       a = x[b, h + i - r, v + j - r, c] inside the frame, +0.0f outside it        (padding taps are links of the chain)
 *       acc = fmaf(a, w[i, j, c, o], acc)
 *   y = acc + bias[o]                                          one rounded add; skipped when bias is NULL
 *   y = act == DTFILL_CONV_LEAKY ? (y > 0 ? y : y * alpha) : y
 * The chain has ksize^2 Cin links, 27 for the RGB stem, which do not fill whole matrix-core steps of four: a link that pads
 * the last step has +0 as BOTH operands.  So only the sign of a zero can change, +0 and -0 count as equal, and no zero ever
 * meets a non-finite partner: an infinite input or weight makes NaN only where the statement above does.  Non-finite values
 * follow fmaf.  The bits are a function of the inputs and the shape alone, never of the tiling, the grid or the position in
 * the batch.  A float32 evaluation in any other order lies within gamma_(K+2) (sum |x| |w| + |bias|), K = ksize^2 Cin.
 * Pointers need float alignment only.  Asynchronous on `stream`; no workspace, no allocation, no atomics, no host
 * synchronisation.  out may not alias x.
 * Returns, all checked before any HIP call and in this order: DTFILL_ERR_NULL for a NULL x, w or out; DTFILL_ERR_SHAPE unless
 * ksize is 1, 3, 5 or 7, Cin is 2, 3 or 4, Cout is a multiple of 16 and at least 16, 0 <= out_offset and out_offset + Cout <=
 * out_channels, B, H, W >= 1, B H W max(Cin, out_channels) < 2^31, act is one of the two values and alpha is finite; then
 * DTFILL_ERR_LAUNCH if a launch failed.
 *
 * dtfill_conv2d_image_backward_weights.  dw: float32 [ksize,ksize,Cin,Cout]; db: float32 [Cout], nullable; both fully
 * overwritten.  THE CONTRACT is dtfill_conv2d_backward_weights' two-level statement with Cout any multiple of 16:
 * g = y > 0 ? dy : dy * alpha; level 1 an fmaf chain per segment of DTFILL_CONV_BW_ROWS x DTFILL_CONV_BW_COLS pixels in raster
 * order, p = fmaf(x[b, h + i - r, v + j - r, c] or +0.0f, g[b, h, v, o], p); level 2 the segments' partials added in (b, t, s)
 * order from +0, one rounded add each; db with a = 1.0f.  dy, y, their widths and offsets, act and alpha as there.
 * THERE IS NO DATA GRADIENT: the image is data.  train.py:253 differentiates with respect to the model's variables only, and
 * nothing upstream of img_conv has one.
 * workspace: dtfill_conv2d_image_backward_workspace_bytes(B, H, W, Cin, ksize, Cout) bytes, 256-byte aligned: the segments'
 * partials, 4 S (ksize^2 Cin + 1) Cout bytes with S = B ceil(H / R) ceil(W / C), rounded up to 256.  Pure host arithmetic; 0
 * for a shape outside the domain.  Asynchronous on `stream`: no allocation, no float atomics, no host synchronisation.
 * Returns as dtfill_conv2d_backward_weights, all checked before any HIP call and in this order: DTFILL_ERR_NULL for a NULL x,
 * dy, dw, workspace, or a NULL y under DTFILL_CONV_LEAKY; DTFILL_ERR_SHAPE unless the shape is in dtfill_conv2d_image's domain,
 * every offset lies in its tensor, B H W max(Cin, Cout, dy_channels, y_channels) < 2^31, (ksize^2 Cin + 1) Cout < 2^31, act is one
 * of the two values and alpha is finite and >= 0; DTFILL_ERR_WORKSPACE for a workspace too small or not aligned; then
 * DTFILL_ERR_LAUNCH.
 */
size_t dtfill_conv2d_image_backward_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout);
int dtfill_conv2d_image_backward_weights(const float *x,
                                         const float *dy, int dy_channels, int dy_offset,
                                         const float *y /* nullable if linear */, int y_channels, int y_offset,
                                         int B, int H, int W, int Cin, int ksize, int Cout,
                                         int act, float alpha,
                                         float *dw, float *db /* nullable */,
                                         void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_image(const float *x, int B, int H, int W, int Cin,
                        const float *w, const float *bias /* nullable */, int ksize, int Cout,
                        int act, float alpha,
                        float *out, int out_channels, int out_offset, void *stream);

/*
 * dtfill_max_pool_pyramid and dtfill_max_pool_pyramid_backward: tf.nn.max_pool of ONE tensor by 2, 4 and 8 (ksize = strides,
 * padding 'SAME') in one pass, which is what ResNet18_NO_BN_l2_light_image does with the output of conv1_pre
 * (solution_DeepNet/net.py:4285, 4320, 4353), and its gradient.  The forward reads x once and writes up to three tensors; the
 * backward writes dx once, in a fixed order.  With two of the three levels NULL a call is a plain max_pool of size 2, 4 or 8.
 *
 * x: float32 [B,H,W,x_channels], NHWC, of which the channels x_offset .. x_offset + C - 1 are pooled.  out_k (k = 2, 4, 8):
 * float32 [B,H/k,W/k,out_k_channels], of which only the channels out_k_offset .. out_k_offset + C - 1 are written and the
 * others left as they were (tf.concat); a NULL out_k skips that level, and its width and offset are then not looked at.
 * H and W must be multiples of the largest requested k.  Under that rule TensorFlow's 'SAME' pads nothing and equals 'VALID';
 * the network cannot run at any other size anyway, since its transposed layers double (ResNet18's multiples-of-8 rule).
 *
 * THE CONTRACT, forward.  For level k, output (b, h, v, c), the window is the pixels (k h + i, k v + j), 0 <= i, j < k,
 * scanned in raster order, i outermost:
 *   best = the first element
 *   for every later element e:  if best is not NaN and (e > best or e is NaN): best = e
 * So the first NaN of the window wins if there is one; otherwise the first element that no other exceeds.  +0 and -0 compare
 * equal, so the earlier of the two wins.  The output is the winner's own bits.  Every level's winner is the raster-first one
 * of ITS window: a level-8 winner is not the first in any order of 2x2 or 4x4 blocks.  (Maxima at pixels (1,0) and (0,2) of
 * one 4x4 window lie in its 2x2 blocks 0 and 1; the winner is (0,2).)
 *
 * THE CONTRACT, backward.  Winners are recomputed from x; no argmax tensor is stored.  dy_k: float32 [B,H/k,W/k,dy_k_channels]
 * read at dy_k_offset .. + C - 1, nullable; dx: float32 [B,H,W,C], dense.  Per input element p, in float32:
 *   t_k   = dy_k at p's level-k window, if p is that window's winner and dy_k is not NULL;  +0 otherwise
 *   dx[p] = (t_2 + t_4) + t_8                                  two rounded adds, in this grouping
 * Every element of dx is written, zeros included.  The windows of one level are disjoint: no atomics, no workspace, and
 * the bits are a function of the inputs alone.  H and W must be multiples of the largest k whose dy is not NULL; with every
 * dy NULL any frame is taken and dx is all +0.
 * That first-in-scan-order is TensorFlow's own choice of winner is restated here from its CPU kernel's loop, not tested:
 * TensorFlow is not part of this project's tests.  What the tests pin is this statement, and torch where torch is unambiguous
 * (values without NaN; gradients without ties).
 *
 * Pointers need float alignment only; when x, dx and every out or dy are 16-byte aligned, all accesses are 16-byte ones.
 * No out may alias x; dx may not alias x or any dy.  Asynchronous on `stream`; no workspace, no allocation, no atomics, no
 * host synchronisation.
 * Returns, all checked before any HIP call and in this order: DTFILL_ERR_NULL for a NULL x, a NULL dx, or (forward) every out
 * NULL; DTFILL_ERR_SHAPE unless B, H, W >= 1, H and W are multiples of the largest requested k, C >= 4, C, x_channels,
 * x_offset and the width and offset of every requested level are multiples of 4, 0 <= offset and offset + C <= width for x and
 * for every requested level, B H W x_channels < 2^31 and B (H/k) (W/k) width_k < 2^31; then DTFILL_ERR_LAUNCH if a launch
 * failed.
 */
int dtfill_max_pool_pyramid(const float *x, int B, int H, int W, int C, int x_channels, int x_offset,
                            float *out2 /* nullable */, int out2_channels, int out2_offset,
                            float *out4 /* nullable */, int out4_channels, int out4_offset,
                            float *out8 /* nullable */, int out8_channels, int out8_offset, void *stream);
int dtfill_max_pool_pyramid_backward(const float *x, int B, int H, int W, int C, int x_channels, int x_offset,
                                     const float *dy2 /* nullable */, int dy2_channels, int dy2_offset,
                                     const float *dy4 /* nullable */, int dy4_channels, int dy4_offset,
                                     const float *dy8 /* nullable */, int dy8_channels, int dy8_offset,
                                     float *dx /* dense [B,H,W,C] */, void *stream);

/*
 * dtfill_adam_step: the optimizer step of the reference's training loop, train.py:169 and :253-254 --
 * tf.keras.optimizers.Adam(lr, beta_1 = 0.9), the "epsilon-hat" rule with eps = 1e-7 -- for every variable of a network in one
 * fused pass, with every bit fixed here.  tests/adam_ref.py is this statement in numpy.
 *
 * params, grads, counts: HOST arrays of n entries; params[i] and grads[i] are DEVICE pointers to counts[i] float32 each.  A NULL
 * grads[i] says that variable i has no gradient in this step: its values and its moments are left as they are, and its
 * params[i] is not dereferenced (it must still not be NULL).  The arrays are read during the call and may be freed after it.
 * m, v: two flat float32 device buffers of dtfill_adam_state_floats(counts, n) floats each, owned by the caller, zero at the
 * start.  Variable i's moments lie at offset o_i in both: o_0 = 0, o_(i+1) = o_i + counts[i] rounded up to a multiple of 4, over
 * ALL n entries, the skipped ones too, so a variable's segment does not depend on who has a gradient.  The padding floats are
 * never read and never written.
 * record: dtfill_adam_record_bytes() device bytes, 8-byte aligned: { int64 t; float64 b1p; float64 b2p }, the step count and
 * the running powers beta1^t, beta2^t.  dtfill_adam_init() sets it to { 0, 1.0, 1.0 } on `stream`; zero bytes are NOT a valid
 * record.  lr, beta1, beta2, eps: float32, as launch arguments: a schedule changes lr from one call to the next.
 *
 * THE CONTRACT.  Scalars, float64, one rounding per operation:
 *   b1p' = b1p * (double)beta1;   b2p' = b2p * (double)beta2;   t' = t + 1           one product each, no pow
 *   alpha = (float)( ((double)lr * sqrt(1 - b2p')) / (1 - b1p') )                    correctly rounded sqrt and divide, then
 *                                                                                    ONE rounding to float32
 *   c1 = 1.0f - beta1;   c2 = 1.0f - beta2                                           float32 subtractions
 * Every element of every variable that has a gradient, float32, one rounding per operation, nothing contracted into an FMA:
 *   m' = m + c1 * (g - m)
 *   v' = v + c2 * (g * g - v)
 *   p' = p - (alpha * m') / (sqrtf(v') + eps)                                        correctly rounded sqrt and divide
 * Denormals are kept (g = 1e-20f gives v' = 0x00000047 after one step), NaN and Inf go where IEEE sends them (any NaN counts
 * as any other), and no element is skipped or clamped.  The record holds t', b1p', b2p' after the call.
 * Keras forms alpha in float32 with a pow; this one is the correctly rounded value of the same expression in the running
 * products (a float32 restatement of Keras' differs from it by up to 54 ulp of alpha in the first 20 000 steps: the
 * cancellation in 1 - 0.999^t).  The element rule is restated from TensorFlow's ApplyAdam functor from memory; TensorFlow
 * is not part of this project's tests.
 *
 * How it runs: up to DTFILL_ADAM_GROUP variables per launch, their pointers, counts and offsets by value in the launch's
 * arguments -- no device table, no copy, nothing that outlives the call -- and more variables in more launches of the same
 * kernel; a block owns DTFILL_ADAM_CHUNK consecutive elements of one variable.  The update launches only read the record; a
 * one-wave launch behind the last of them, on the same stream, advances it.  Where params[i], grads[i], m and v are all 16-byte
 * aligned, variable i moves in 16-byte accesses; any float-aligned pointer is legal.  Asynchronous on `stream`; no workspace,
 * no allocation, no atomics, no host synchronisation.  Two calls on one record must be ordered by their streams.
 *
 * Returns, all checked before any HIP call and in this order: DTFILL_ERR_NULL for a NULL params, grads, counts, m, v or
 * record; DTFILL_ERR_SHAPE for n < 1; DTFILL_ERR_NULL for a NULL params[i], or when every grads[i] is NULL; DTFILL_ERR_SHAPE for
 * a count < 1 or >= 2^31, more than 2^34 - 4 state floats, an lr or eps that is negative or not finite, a beta outside [0, 1),
 * or a params[i] whose counts[i] floats overlap its grads[i]'s; then DTFILL_ERR_LAUNCH if a launch failed.
 * dtfill_adam_state_floats: the floats EACH of m and v holds; 0 for a list dtfill_adam_step would refuse.
 * dtfill_adam_init: DTFILL_ERR_NULL for a NULL record, DTFILL_ERR_LAUNCH if the launch failed.
 */
#define DTFILL_ADAM_GROUP 128  /* variables per launch: 128 x 28 bytes of table + 48 of scalars = 3632 < HIP's 4096 of arguments */
#define DTFILL_ADAM_CHUNK 4096 /* elements per block: 256 lanes x four 16-byte accesses per array */
size_t dtfill_adam_state_floats(const long long *counts, int n);
size_t dtfill_adam_record_bytes(void);
int dtfill_adam_init(void *record, void *stream);
int dtfill_adam_step(float *const *params, const float *const *grads /* entries nullable */, const long long *counts, int n,
                     float *m, float *v, void *record,
                     float lr, float beta1, float beta2, float eps, void *stream);

/*
 * dtfill_conv2d_strided_bf16 and dtfill_conv2d_transpose_bf16: the two calls below on the bf16 matrix cores with float32
 * accumulation, the opt-in inference precision of the three ResNets (precision = "bf16").  The float32 calls stay the default
 * (training under bf16: the backward calls further down).  The argument lists and tensors are the twins': x, bias, residual and out stay float32 in
 * memory, out_channels and out_offset behave as there, and the output size and the padding are the same 'same' rule.  w is NOT
 * the float32 kernel but the packed bf16 array dtfill_conv2d_pack_bf16() makes of it, 16-byte aligned.
 * Accepted shapes: ksize 1 or 3; stride 1 or 2 (the transposed form is always 3x3, stride 2); Cin a multiple of 16 and at
 * least 16; Cout a multiple of 16 and at least 16.  The kernel works in groups of 32 input channels; a trailing half group
 * (Cin = 16 or 48 mod 32: conv1a at scale_num 1 or 3) has +0 on both sides, x and w.
 *
 * THE CONTRACT.  bf16(.) is round-to-nearest-even on the float32 value to 8 significand bits; NaN stays NaN and a value that
 * rounds past the largest finite bf16 goes to +-inf.  Per output:
 *   acc = the float32-accumulated sum of bf16(x) * bf16(w) over the same taps and channels as the float32 contract, padding
 *         taps +0
 *   y = acc + bias[o];  y = y + residual[..];  y = leaky(y)     the float32 finish of the twins, unchanged, in this order
 * A product of two bf16 values has 16 significant bits and is exact in float32 where it is at least 2^-126 in magnitude (or
 * +-0); below that float32 keeps only the bits from 2^-149 up, so a smaller product is rounded once, by less than 2^-149
 * (two normal operands near 2^-70 already give one).  The order and the rounding of the additions
 * INSIDE one bf16 MFMA (v_mfma_f32_16x16x32_bf16: 32 products and the accumulator) are the hardware's and are not documented,
 * so the output bits are NOT stated by a chain, as the float32 contract's are.  What is promised:
 *   (a) The sequence of MFMAs per output is fixed: groups of 32 input channels outermost, then the taps in raster order (the
 *       transposed form: the taps of the output's parity in raster order), one k-step per (group, tap).  The bits are a
 *       function of the inputs and the shape alone: not of the tile, the grid, the position in the batch or the run.
 *   (b) |y - exact| <= 2 n 2^-23 (S + |bias| + |residual|) + n 2^-149, S = sum |bf16(x)| |bf16(w)| over the output's terms,
 *       n = ksize^2 32 ceil(Cin / 32), where exact is the sum and the finish in real arithmetic.  The bound holds for a
 *       sequential or a tree order, for rounding to nearest or truncation of every internal addition, and for alignment of an
 *       instruction's 33 addends to the largest of them.  The absolute term is the products': at most n of them, each rounded
 *       or truncated once by less than 2^-149 where it lies below 2^-126.  It stands for gradual underflow, which is what the
 *       matrix cores do (measured on an MI355X with normal operands near 2^-70 and 2^-60: no small product or partial sum is
 *       flushed, and the worst error is 0.036 of this bound; with S below 2^-126, where every addition is exact, it is
 *       6.7 x 2^-149 at n = 288: the products are rounded, not truncated).  An addition
 *       whose result is below 2^-126 is exact, and one above is within the first term.  Where all partial sums are exactly
 *       representable (small integers) the result is exact.  With S below FLT_MAX no partial sum in any order overflows and
 *       y is finite unless the finish overflows; where every product of an output has one sign and the exact sum lies beyond
 *       FLT_MAX by more than the bound, y is the infinity of that sign.  Sums of mixed signs with S beyond FLT_MAX are open:
 *       an inner order may meet inf - inf.
 * Subnormal bf16 operands may be flushed by the hardware; the contract leaves them open (an MI355X keeps them, in x and in w;
 * the tests take either, but one of the two throughout a call).  +0 and -0 count as equal.
 * residual may alias x; neither may alias out.
 *
 * dtfill_conv2d_pack_bf16: a small device kernel that rounds w to bf16 and lays it out as the matrix cores' B fragments.
 * w: float32 in the form the float32 entry point takes, [ksize,ksize,Cin,Cout]; for the transposed layer the already
 * exchanged [3,3,Cin,Cout].  out: dtfill_conv2d_bf16_packed_elems(ksize, Cin, Cout) bf16 elements (2 bytes each), 16-byte
 * aligned.  The layout, for the record; callers must go through this function and treat the array as opaque:
 *   out[(((T G + g) N + n) 64 + 16 kq + m) 8 + j] = bf16(w[T][32 g + 8 kq + j][16 n + m]),  +0 where 32 g + 8 kq + j >= Cin
 *   T = tap (ky ksize + kx), G = ceil(Cin / 32) groups, N = Cout / 16 N-tiles, kq < 4, m < 16, j < 8:
 * a lane's 8 k-values of one output channel are 16 contiguous bytes, the 16 channels of an N-tile 256 contiguous bytes, the
 * fragment of one (tap, group, N-tile) 1024 contiguous bytes; half groups are zero-filled.
 * dtfill_conv2d_bf16_packed_elems = ksize^2 G N 512; 0 for a shape the calls refuse.
 *
 * All three: asynchronous on `stream`; no workspace, no allocation, no atomics, no host synchronisation.  x needs float
 * alignment only and is read by 16-byte loads where its address allows.
 * Returns, all checked before any HIP call.  The two convolutions: as their twins', with ksize 1 or 3 only, and
 * DTFILL_ERR_SHAPE for a w that is not 16-byte aligned.  dtfill_conv2d_pack_bf16: DTFILL_ERR_NULL for a NULL w or out;
 * DTFILL_ERR_SHAPE unless ksize is 1 or 3, Cin and Cout are multiples of 16 and at least 16, the packed array has fewer than
 * 2^31 elements and out is 16-byte aligned; then DTFILL_ERR_LAUNCH if the launch failed.
 */
size_t dtfill_conv2d_bf16_packed_elems(int ksize, int Cin, int Cout);
int dtfill_conv2d_pack_bf16(const float *w, int ksize, int Cin, int Cout, void *out, void *stream);
int dtfill_conv2d_strided_bf16(const float *x, int B, int H, int W, int Cin,
                               const void *w /* packed bf16 */, const float *bias /* nullable */, int ksize, int Cout, int stride,
                               const float *residual /* nullable */, int act, float alpha,
                               float *out, int out_channels, int out_offset, void *stream);
int dtfill_conv2d_transpose_bf16(const float *x, int B, int H, int W, int Cin,
                                 const void *w /* packed bf16 */, const float *bias /* nullable */, int Cout,
                                 int act, float alpha,
                                 float *out, int out_channels, int out_offset, void *stream);

/*
 * The backward of the wide layers on the bf16 matrix cores with float32 accumulation: what precision = "bf16" trains with.
 * The four calls below are dtfill_conv2d_strided_backward_data / _weights and dtfill_conv2d_transpose_backward_data / _weights
 * with the same argument lists, and dtfill_conv2d_wide_backward_bf16_workspace_bytes is their size function (0 for a shape
 * they refuse).  x, dy, y, w, dx, dresidual, dw and db are float32 in memory; dy and y are read at a channel offset of a wider
 * tensor and dx is written at one, as there.  w is the PLAIN float32 kernel the float32 calls take ([ksize,ksize,Cin,Cout], the
 * exchanged [3,3,Cin,Cout] of the transposed layer): the weights change every step, so the data call packs what it needs
 * into the workspace itself.  Domain: ksize 1 or 3, stride 1 or 2, Cin and Cout multiples of 16 and at least 16, H and W even
 * at stride 2; pixel and element limits, the workspace rule (256-byte aligned, at least the size function's bytes) and the
 * order of the return codes are the twins'.  The float32 calls stay the default.
 *
 * g = dy * act'(y) is the float32 calls' g, computed in float32 (a compare on y and one rounded product), and dresidual = g is
 * exact, from the same pass.  x^ = bf16(x), g^ = bf16(g), w^ = bf16(w): dtfill_conv2d_strided_bf16's rounding (to nearest even,
 * NaN kept, past the largest finite bf16 to +-inf), made in registers while staging; nothing bf16 is kept in memory but the
 * packed kernel in the workspace.
 *
 * dx, by identity with the bf16 forward calls over the dense g [B,Ho,Wo,Cout], linear, no bias:
 *   stride 1          == dtfill_conv2d_strided_bf16(g, pack(wT), stride 1),  wT[i][j][o][c] = w[ksize-1-i][ksize-1-j][c][o]
 *   3x3, stride 2     == dtfill_conv2d_transpose_bf16(g, pack(wX)),          wX[i][j][o][c] = w[i][j][c][o]
 *   transposed layer  == dtfill_conv2d_strided_bf16(g, pack(wX), 3x3, stride 2)
 *   1x1, stride 2     the 1x1 stride-1 bf16 call over g under pack(wX) at the even pixels of dx, +0 literally at the others
 * bit for bit, so dx has that contract: a fixed sequence of MFMAs per output and its bound (b) with n = ksize^2 32
 * ceil(Cout / 32) and S = sum |g^| |w^| over the output's terms.
 *
 * dw and db.  Not a chain either, for the reason given there.  What is promised:
 *   (a) A fixed sequence.  Segments of DTFILL_CONV_BW_ROWS x DTFILL_CONV_BW_COLS pixels lie over the small frame exactly as
 *       in dtfill_conv2d_strided_backward_weights (the output frame of a strided layer, the input frame of the transposed
 *       one).  Inside a segment the rows go in order; inside a row, k-steps of 32 consecutive pixels go in order, and a
 *       position of a k-step past the frame is +0 on BOTH operands (a segment's row is two whole k-steps: none crosses a
 *       segment).  Per (k-step, tap, 16 x 16 tile of (input channel, output channel)) there is ONE v_mfma_f32_16x16x32_bf16
 *       into a float32 accumulator that lives from +0 across the whole segment; operand pixel u of the step sits at the
 *       MFMA's k index 8 (u / 4 % 4) + 4 (u / 16) + u % 4 on both operands.  db[o] is the same sequence with the other
 *       operand 1.0 (exact in bf16), the sum of g^; the transposed layer keeps its four chains, ((q00 + q01) + q10) + q11 in
 *       float32.  The segments' partials [segment][tap][Cin][Cout] (+ db) are then added in float32 in (frame, segment row,
 *       segment column) order, from +0, one rounding each.  So the bits are a function of the inputs and the shape alone:
 *       not of the grid, the pass, the position in the batch beyond the order just stated, the run or the stream.
 *   (b) |dw[e] - exact| <= 2 n 2^-23 S + n 2^-149,  exact = the sum of x^ g^ over the element's terms in real arithmetic,
 *       S = sum |x^| |g^| over them, n = P + N: P the padded pixel count, sum over the frames' segments of (rows of the
 *       segment) x 32 ceil(columns of the segment / 32), N = B segs_y segs_x the number of segments.  Derivation, as for
 *       dtfill_conv2d_strided_bf16.  The value is made by P additions of a product inside MFMAs (the +0 positions
 *       included) and N additions of a partial.  Each is off by at most one unit in the last place of the running sum,
 *       whether the hardware rounds to nearest or truncates, sequentially or as a tree, and every running sum is at most
 *       S (1 + o(1)) in magnitude: (P + N) 2^-23 S to first order.  An MFMA may also align its 33 addends to the
 *       largest of them and drop what falls below its last place, at most 2^-23 of that largest (<= S) per addend:
 *       another P 2^-23 S.  Together at most (2 P + N) 2^-23 S <= 2 n 2^-23 S.  The absolute term is the products': at
 *       most P of them, each rounded or truncated once by less than 2^-149 where it lies below 2^-126; an addition whose
 *       result is below 2^-126 is exact.  db: the same with x^ = 1 (for the transposed layer P counts the four chains'
 *       positions, 4 P, and N the three additions more per segment).  Where every partial sum is exactly representable
 *       (small integers) dw and db are exact.
 * Non-finite values: padding and the positions past the frame are a staged +0, so +0 * NaN = NaN as in the float32 calls,
 * and the set of NaN entries of dw and db equals theirs on the same inputs (with finite products: a bf16 overflow of a
 * finite x or g to inf is dtfill_conv2d_strided_bf16's rule).  +0 and -0 count as equal.
 *
 * The workspace holds g, the packed kernel and the 1x1 stride-2 values for the data call, the partials for the weights call;
 * either call may use the whole of it, so two calls that share one must be ordered on a stream.  Asynchronous on `stream`;
 * no allocation, no atomics, no host synchronisation.  Returns: as the twins', in their order.
 */
size_t dtfill_conv2d_wide_backward_bf16_workspace_bytes(int B, int H, int W, int Cin, int ksize, int Cout, int stride, int transposed);
int dtfill_conv2d_strided_backward_data_bf16(const float *dy, int dy_channels, int dy_offset,
                                             const float *y /* nullable if linear */, int y_channels, int y_offset,
                                             const float *w, int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                             int act, float alpha,
                                             float *dx, int dx_channels, int dx_offset, float *dresidual /* nullable */,
                                             void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_strided_backward_weights_bf16(const float *x,
                                                const float *dy, int dy_channels, int dy_offset,
                                                const float *y /* nullable if linear */, int y_channels, int y_offset,
                                                int B, int H, int W, int Cin, int ksize, int Cout, int stride,
                                                int act, float alpha,
                                                float *dw, float *db /* nullable */,
                                                void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_transpose_backward_data_bf16(const float *dy, int dy_channels, int dy_offset,
                                               const float *y /* nullable if linear */, int y_channels, int y_offset,
                                               const float *w /* packed [3,3,Cin,Cout] */, int B, int H, int W, int Cin, int Cout,
                                               int act, float alpha,
                                               float *dx, int dx_channels, int dx_offset,
                                               void *workspace, size_t ws_bytes, void *stream);
int dtfill_conv2d_transpose_backward_weights_bf16(const float *x,
                                                  const float *dy, int dy_channels, int dy_offset,
                                                  const float *y /* nullable if linear */, int y_channels, int y_offset,
                                                  int B, int H, int W, int Cin, int Cout,
                                                  int act, float alpha,
                                                  float *dw /* packed layout */, float *db /* nullable */,
                                                  void *workspace, size_t ws_bytes, void *stream);

/*
 * dtfill_conv2d_strided and dtfill_conv2d_transpose: the wide layers of ResNet18_NO_BN_l2 (solution_DeepNet/net.py:245-745),
 * in the same sense as dtfill_conv2d below, whose statement they extend: every output bit is fixed here.  Convolutions with
 * Cin == 1 or Cout == 1 (the correction branch, the stems, conv_output) stay with dtfill_conv2d.
 *
 * dtfill_conv2d_strided.  x: float32 [B,H,W,Cin]; w: float32 [ksize,ksize,Cin,Cout], a Keras Conv2D.kernel as stored
 * (cross-correlation); bias: [Cout], nullable; stride: 1 or 2; residual: float32 [B,Ho,Wo,Cout], dense, nullable; act, alpha,
 * out_channels and out_offset as in dtfill_conv2d; out: float32 [B,Ho,Wo,out_channels].  The output size and the padding are
 * TensorFlow's 'same' rule, per axis:
 *   Ho = ceil(H / stride),  pad = max((Ho - 1) stride + ksize - H, 0),  pt = pad / 2   (integer division: the smaller half
 *   in front), and Wo and pl likewise from W.  Stride 1: pt = (ksize - 1) / 2.  Stride 2, ksize 3: pt = 0 for an even H and
 *   1 for an odd one.  Stride 2, ksize 1: pt = 0.
 * THE CONTRACT.  Per output (b, h, v, o), in float32:
 *   acc = +0
 *   for g in 0 .. Cin / 16 - 1:                                groups of 16 input channels, outermost
 *     for i in 0 .. ksize - 1:  for j in 0 .. ksize - 1:       the taps in raster order
 *       for c in 16 g .. 16 g + 15:
 *         a = x[b, stride h + i - pt, stride v + j - pl, c] inside the frame, +0.0f outside it
 *         acc = fmaf(a, w[i, j, c, o], acc)
 *   y = acc + bias[o]                                          one rounded add; skipped when bias is NULL
 *   y = y + residual[b, h, v, o]                               one more rounded add; skipped when residual is NULL
 *   y = act == DTFILL_CONV_LEAKY ? (y > 0 ? y : y * alpha) : y
 * which is the order of the reference's graph: the bias inside the layer, then tensor + tensor_add, then leaky_relu.  At
 * stride 1 without a residual this is dtfill_conv2d's statement, and for Cout == 16 the two entry points give the same bits.
 * residual may alias x; neither may alias out.  +0 and -0 count as equal; non-finite values follow fmaf; the bits are a
 * function of the inputs and the shape alone.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, w or out; DTFILL_ERR_SHAPE unless stride is 1 or 2,
 * ksize is 1, 3, 5 or 7 at stride 1 and 1 or 3 at stride 2, Cin and Cout are multiples of 16 and at least 16,
 * 0 <= out_offset and out_offset + Cout <= out_channels, B, H, W >= 1, B H W Cin < 2^31 and B Ho Wo max(Cout, out_channels)
 * < 2^31, act is one of the two values and alpha is finite; then DTFILL_ERR_LAUNCH if a launch failed.
 *
 * dtfill_conv2d_transpose: tf.keras.layers.Conv2DTranspose(Cout, 3, strides=2, padding='same'), which TensorFlow defines as
 * the gradient, with respect to its input, of the stride-2 'same' 3x3 convolution of a [2H,2W] frame (pt = pl = 0 there).
 * x: float32 [B,H,W,Cin]; out: float32 [B,2H,2W,out_channels], written at out_offset .. out_offset + Cout - 1.
 * w: float32 [3,3,Cin,Cout]: Keras's Conv2DTranspose.kernel is [3,3,Cout,Cin], and w is that array with its last two axes
 * exchanged, a one-time repack on the host when the weights are loaded.  It makes the weights of four consecutive input
 * channels and sixteen output channels, a matrix-core k-step, 64 consecutive floats per k index, as dtfill_conv2d's are.
 * THE CONTRACT.  Per output (b, y, u, o), in float32:
 *   acc = +0
 *   for g in 0 .. Cin / 16 - 1:
 *     for ky in 0 .. 2:  for kx in 0 .. 2:                     raster order; only the taps with y - ky and u - kx both even
 *       for c in 16 g .. 16 g + 15:
 *         a = x[b, (y - ky) / 2, (u - kx) / 2, c] inside the frame, +0.0f outside it
 *             (only the index -1 occurs, at y = 0 or u = 0 under tap 2; it is a link of the chain like any padding tap)
 *         acc = fmaf(a, w[ky, kx, c, o], acc)
 *   y = acc + bias[o]                                          skipped when bias is NULL
 *   y = act == DTFILL_CONV_LEAKY ? (y > 0 ? y : y * alpha) : y
 * so an output has 1, 2, 2 or 4 taps by the parity of (y, u): (odd, odd) reads x[(y-1)/2, (u-1)/2] under w[1,1] alone,
 * (even, even) reads four pixels under w[0,0], w[0,2], w[2,0], w[2,2].  No residual.
 * Returns as dtfill_conv2d_strided's, with B 2H 2W max(Cout, out_channels) < 2^31 for the output.
 *
 * Both: pointers need float alignment only, x is read by 16-byte loads where its address allows; asynchronous on `stream`;
 * no workspace, no allocation, no atomics, no host synchronisation.
 */
int dtfill_conv2d_strided(const float *x, int B, int H, int W, int Cin,
                          const float *w, const float *bias /* nullable */, int ksize, int Cout, int stride,
                          const float *residual /* nullable */, int act, float alpha,
                          float *out, int out_channels, int out_offset, void *stream);
int dtfill_conv2d_transpose(const float *x, int B, int H, int W, int Cin,
                            const float *w, const float *bias /* nullable */, int Cout,
                            int act, float alpha,
                            float *out, int out_channels, int out_offset, void *stream);

/*
 * dtfill_conv2d: a stride-1 'same' convolution in float32 whose every output bit is fixed by this statement: the layers of
 * SparsityCNN (solution_DeepNet/net.py:11-242), so that the network between the fills and the losses runs here too.
 *
 * x: float32 [B,H,W,Cin], channel-last as the reference's tensors are; with Cin == 1 that is the [B,H,W] planes the fill and
 * dtfill_generate_multi_channel() emit.  w: float32 [ksize,ksize,Cin,Cout], a Keras Conv2D.kernel as stored; the operation
 * is cross-correlation, as TensorFlow's is, not a flipped convolution.  bias: float32 [Cout], nullable.  out: float32
 * [B,H,W,out_channels], of which only the channels out_offset .. out_offset + Cout - 1 are written and the others left
 * untouched (tf.concat of several layers' outputs is several calls into one tensor); out may not alias x.
 *
 * THE CONTRACT.  Per output (b, h, v, o), in float32, with r = (ksize - 1) / 2:
 *   acc = +0
 *   for g in 0 .. ceil(Cin / 16) - 1:                          groups of 16 input channels, outermost
 *     for i in 0 .. ksize - 1:  for j in 0 .. ksize - 1:       the taps in raster order
 *       for c in 16 g .. min(16 g + 15, Cin - 1):
 *         a = x[b, h + i - r, v + j - r, c] inside the frame, +0.0f outside it      (padding taps are links of the chain)
 *         acc = fmaf(a, w[i, j, c, o], acc)
 *   y = acc + bias[o]                                          one rounded add; skipped when bias is NULL
 *   y = act == DTFILL_CONV_LEAKY ? (y > 0 ? y : y * alpha) : y
 * +0 and -0 count as equal: the zero operands that fill the last matrix-core step of a Cin == 1 chain can turn a -0
 * accumulator into +0.  Non-finite values follow fmaf, so a padding tap under an infinite weight makes NaN; nothing faults.
 * The bits are a function of the inputs and the shape alone, never of the tiling, the grid or the position in the batch.
 * TensorFlow documents no summation order, so this order is the library's own, as the tap order of
 * dtfill_generate_multi_channel() is: a float32 evaluation in any other order lies within
 * gamma_(K+2) (sum |x| |w| + |bias|) of it, K = ksize^2 Cin, gamma_n = n 2^-24 / (1 - n 2^-24).
 * Why the groups are outermost: a block keeps the haloed input tile of 16 channels in LDS (34 KB for 7x7), not of all 64.
 *
 * Pointers need float alignment only; x is read by 16-byte loads where its address allows.  Asynchronous on `stream`; no
 * workspace, no allocation, no atomics, no host synchronisation.
 * Returns, all checked before any HIP call: DTFILL_ERR_NULL for a NULL x, w or out; DTFILL_ERR_SHAPE unless ksize is 1, 3, 5
 * or 7, Cin is 1, 16, 32, 48 or 64, Cout is 1 or 16, 0 <= out_offset and out_offset + Cout <= out_channels, B, H, W >= 1,
 * B H W max(Cin, out_channels) < 2^31, act is one of the two values below and alpha is finite; then DTFILL_ERR_LAUNCH if a
 * launch failed.
 */
#define DTFILL_CONV_LINEAR 0
#define DTFILL_CONV_LEAKY  1 /* y > 0 ? y : y * alpha; tf.nn.leaky_relu's alpha is 0.2f */
int dtfill_conv2d(const float *x, int B, int H, int W, int Cin,
                  const float *w, const float *bias /* nullable */, int ksize, int Cout,
                  int act, float alpha,
                  float *out, int out_channels, int out_offset, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DTFILL_H */
