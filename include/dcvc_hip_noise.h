/* dcvc_hip_noise.h -- the sensor noise of a fixed-camera sequence, measured from the source alone: per 16 x 16 cell the sum
 * of the absolute luma difference of two consecutive pictures and the cell's luma, and a histogram of those cell words.  The
 * host turns the histogram into one number (vcm_ts_amd/noise.py); this header is the device half.
 *
 * Conventions of dcvc_hip_motion.h and dcvc_hip_tnr.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative
 * DCVC_E_* code, nothing launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 R, G, B with
 * explicit strides in elements:
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read in place.  H and W are the UNPADDED size, each within
 * 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  The only floating-point operation is the one multiply of code() below; everything
 * else is integer arithmetic, exact and independent of the order of summation.
 *
 * Per pixel:   r, g, b = code(v) = (int) rint(255.0f * clamp01(v)) of the three planes (dcvc_hip_scene.h; a NaN codes
 *   as 0);  Y = (54 r + 183 g + 19 b + 128) >> 8,  0 <= Y <= 255  (the luma of dcvc_hip_scene.h).
 *
 * The luma planes:  ycur and yprev are H rows of y_stride bytes (uint8), y_stride >= W and a multiple of 4, so a plane is
 *   H * y_stride bytes.  Byte (y, x) of ycur, x < W, is WRITTEN with the Y of this picture's pixel; the bytes of a row from
 *   column W on are never written (those below the next multiple of 4 may be READ from yprev, and nothing is made of them).
 *   yprev is the plane the previous call wrote, with the same stride, and is only read.  Keeping the previous picture as
 *   bytes means that a scan never holds on to a source picture, and that a pixel costs 12 + 1 bytes read and 1 written.
 *   yprev may be NULL (the first picture of a scan): then only ycur is written and every cell word is DCVC_NOISE_NONE.
 *
 * The cells:   cells[i * wc + j], hc wc uint32 words on the grid of the q-scale maps (dcvc_hip_roi.h, "Latent grid"):
 *   hc = 4 ceil(H / 64), wc = 4 ceil(W / 64).  Every word is WRITTEN, not added to.  For a cell that lies wholly inside
 *   the picture, i < H / 16 and j < W / 16 (integer division), over its 256 pixels
 *     m = sum |Y(cur) - Y(prev)|   (0 .. 65280)
 *     l = sum Y(cur)               (0 .. 65280)
 *     word = ((l >> 12) << 16) | m
 *   so the upper half is the cell's mean luma in steps of 16 codes (0 .. 15) and the lower half 256 times its mean absolute
 *   difference.  Every other cell -- one the picture's edge cuts, one of the padding -- is DCVC_NOISE_NONE: every counted
 *   cell has the same number of samples.  The words outside the hc wc range are never touched.
 *
 * The histogram:  hist[row * 512 + col], DCVC_NOISE_COUNTERS = 16 * 512 uint32 counters.  A word is SKIPPED when it is
 *   DCVC_NOISE_NONE or when its upper half exceeds 15 (nothing out of range is ever indexed).  Otherwise
 *     row = word >> 16                        the cell's mean luma in steps of 16 codes
 *     col = min((word & 0xFFFF) >> 4, 511)    the cell's mean absolute difference in 1/16 code; the last column collects
 *                                             everything from 8176 / 256 = 31.94 codes up
 *     hist[row * 512 + col] += 1.
 *   Integer adds: the result does not depend on any order.  The counters are exact while none exceeds 2^32 - 1, which is
 *   the caller's business.
 */
#ifndef DCVC_HIP_NOISE_H
#define DCVC_HIP_NOISE_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_NOISE_NONE 0xFFFFFFFFu
#define DCVC_NOISE_ROWS 16
#define DCVC_NOISE_COLS 512
#define DCVC_NOISE_COUNTERS (DCVC_NOISE_ROWS * DCVC_NOISE_COLS)
#define DCVC_NOISE_MAX_WORDS (1 << 28)

/* One picture: one launch on `stream`, nothing synchronised.  A picture whose base is 16-byte aligned and whose strides
 * are multiples of 4 is read 16 bytes at a time, any other 4 bytes at a time; the luma planes are read and written 4 bytes
 * (4 pixels) at a time wherever the four lie inside the picture, else byte by byte: same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL rgb, ycur or cells; H or W not in 1 .. DCVC_ROI_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; y_stride < W or not a multiple of 4; rgb, ycur, yprev or cells
 * not 4-byte aligned; ycur == yprev. */
int dcvc_noise_cells(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, const uint8_t *yprev,
                     uint8_t *ycur, int32_t y_stride, uint32_t *cells, void *stream);

/* ADDS the n words of `cells` (any number of pictures' cells laid end to end) into hist: one launch on `stream`, nothing
 * synchronised; n == 0 launches nothing and answers 0.
 * Refused with DCVC_E_ARG, before anything else: a NULL cells or hist; n outside 0 .. DCVC_NOISE_MAX_WORDS; cells or hist
 * not 4-byte aligned. */
int dcvc_noise_hist(const uint32_t *cells, int64_t n, uint32_t *hist, void *stream);

#ifdef __cplusplus
}
#endif
#endif
