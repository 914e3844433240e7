/* dcvc_hip_motion.h -- motion regions of a fixed-camera sequence: a per-pixel background model of the luma, updated
 * picture by picture on the device, and per 16 x 16 cell the number of pixels that differ from it (foreground).  The host
 * turns the counts into boxes (vcm_ts_amd/motionroi.py); this header is the device half.
 *
 * Conventions of dcvc_hip_scene.h and dcvc_hip_aq.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative
 * DCVC_E_* code, nothing launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 R, G, B with
 * explicit strides in elements:
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read in place.  H and W are the UNPADDED size, each within
 * 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.
 *
 * The model:   bg[y * W + x], H W dense uint16 with row stride W, the background luma in 8.8 fixed point.  The caller
 *   owns it; a step updates it in place.
 *
 * The counts:  counts[i * wc + j], hc wc uint16 on the grid of the q-scale maps and bit maps (dcvc_hip_roi.h, "Latent
 *   grid"): hc = 4 ceil(H / 64), wc = 4 ceil(W / 64).  Cell (i, j) covers pixel rows [16 i, 16 i + 16) and columns
 *   [16 j, 16 j + 16) INTERSECTED WITH THE PICTURE.  Every cell is WRITTEN, not added to; a cell that holds no pixel
 *   (the padding's) is written 0.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  The only floating-point operation is the one multiply of code() below; everything
 * else is integer arithmetic, exact and independent of the order of summation.
 *
 * Per pixel:   r, g, b = code(v) = (int) rint(255.0f * clamp01(v)) of the three planes (dcvc_hip_scene.h; a NaN codes
 *   as 0);  Y = (54 r + 183 g + 19 b + 128) >> 8,  0 <= Y <= 255  (the luma of dcvc_hip_scene.h).
 *
 * With init != 0:   bg[p] = Y << 8 for every pixel, every count is 0.
 *
 * With init == 0, B = bg[p]:
 *     delta = (Y << 8) - B  (int32),   a = |delta|
 *     fg    = a > (T << 8)             (strictly)
 *     k     = fg ? k_fg : k_bg
 *     s     = a >> k
 *     bg[p] = B + (delta < 0 ? -s : s)
 *     counts[cell] = the number of fg pixels of the cell, 0 .. 256.
 *   The step truncates toward zero and never overshoots: a model within 0 .. 65280 (what init leaves) stays there.
 *   k = 0 makes the model follow the picture exactly; k = 16 freezes it (a <= 65280 < 2^16).  |delta| below 2^k moves
 *   nothing.
 *
 * The bg words outside the H W range and the counts words outside the hc wc range are never touched.
 */
#ifndef DCVC_HIP_MOTION_H
#define DCVC_HIP_MOTION_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MOTION_MAX_T 254 /* T: 1 .. 254 luma codes */
#define DCVC_MOTION_MAX_K 16  /* k_bg, k_fg: 0 .. 16 */

/* One step of the model on one picture: one launch on `stream`, nothing synchronised.  A picture whose base is 16-byte
 * aligned and whose strides are multiples of 4 is read 16 bytes at a time, any other 4 bytes at a time; a model whose
 * base is 8-byte aligned and whose W is a multiple of 4 is read and written 8 bytes (4 pixels) at a time, any other 2
 * bytes at a time: same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL rgb, bg or counts; H or W not in 1 .. DCVC_ROI_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; T outside 1 .. DCVC_MOTION_MAX_T; k_bg or k_fg outside
 * 0 .. DCVC_MOTION_MAX_K (init != 0 checks them all the same); rgb not 4-byte aligned; bg or counts not 2-byte aligned. */
int dcvc_motion_step(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint16_t *bg,
                     int32_t init, int32_t T, int32_t k_bg, int32_t k_fg, uint16_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
