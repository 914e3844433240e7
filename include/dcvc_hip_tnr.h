/* dcvc_hip_tnr.h -- a motion-adaptive temporal noise prefilter for fixed-camera content: every picture the codec is
 * handed is blended, pixel by pixel, with the previous filtered picture wherever the luma of the two stays close over a
 * 5 x 5 window, and passed through untouched wherever something moves.  Encoder side only: the bitstream and the decoder
 * know nothing of it.  The host side is vcm_ts_amd/tnr.py; this header is the device half.
 *
 * Conventions of dcvc_hip_motion.h and dcvc_hip_aq.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative
 * DCVC_E_* code, nothing launched (and nothing dereferenced) on a bad argument.  The three pictures are PLANAR fp32 R, G, B
 * with explicit strides in elements:
 *   element (c, y, x) = p[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read and written in place.  H and W are the UNPADDED size, each within
 * 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.
 *
 *   cur   the source picture
 *   ref   the previous filtered picture, i.e. the previous call's out (after an I picture: that picture)
 *   out   the picture the codec will see
 *   wtab  256 uint16 words on the device, each within 1 .. 256: the weight of the current picture, in 1/256ths, by the
 *         window's mean absolute difference.  The caller answers for the range of the entries.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Everything that decides a weight is integer arithmetic, exact and independent of
 * the order of summation; the only floating-point work is the one multiply of code() and the blend below.
 *
 * Per pixel p = (y, x), with code(v) = (int) rint(255.0f * clamp01(v)) (a NaN codes as 0) and the luma
 * Y = (54 r + 183 g + 19 b + 128) >> 8 of the three codes, both exactly as in dcvc_hip_scene.h / dcvc_hip_motion.h:
 *     d(p) = |Y(cur, p) - Y(ref, p)|                                     0 .. 255
 *     S(p) = the sum of d over the 5 x 5 window centred on p, coordinates clamped to the picture (replicated edges):
 *            always 25 terms,                                            0 .. 6375
 *     a    = S / 25  (integer floor)                                     0 .. 255
 *     w    = d(p) > P ? 256 : wtab[a]                                    1 .. 256
 *   and for each of the three planes
 *     out  = (w == 256) ? cur : ref + (cur - ref) * (float) w * 0x1p-8f
 *   evaluated as written, left to right, in fp32 with every operation rounded and none contracted: the difference, its
 *   product with (float) w, the scaling by 2^-8 (exact short of underflow), the sum with ref.  w == 256 copies the bits
 *   of cur.
 *
 * The cells:   sad[i * wc + j] (uint32) and held[i * wc + j] (uint16) on the grid of the q-scale maps (dcvc_hip_roi.h,
 *   "Latent grid"): hc = 4 ceil(H / 64), wc = 4 ceil(W / 64); cell (i, j) covers pixel rows [16 i, 16 i + 16) and columns
 *   [16 j, 16 j + 16) INTERSECTED WITH THE PICTURE.  sad is the sum of d(p) over the cell's pixels, held the number of
 *   them with w < 256 (0 .. 256).  Every cell is WRITTEN, not added to; a cell that holds no pixel is written 0.
 *
 * Nothing outside the H x W crop of out, nor outside the two hc wc arrays, is touched.
 */
#ifndef DCVC_HIP_TNR_H
#define DCVC_HIP_TNR_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_TNR_WINDOW 5  /* the side of the window S is taken over */
#define DCVC_TNR_MAX_P 255 /* P: 0 .. 255 luma codes (255 switches the pixel guard off) */

/* One step of the filter on one picture: one launch on `stream`, nothing synchronised.  A picture whose base is 16-byte
 * aligned and whose strides are multiples of 4 is accessed 16 bytes at a time, any other 4 bytes at a time (each of the
 * three on its own): same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref, out, wtab, sad or held; H or W not in
 * 1 .. DCVC_ROI_MAX_SIDE; a row stride < W; a plane stride < (H - 1) * row stride + W; P outside 0 .. DCVC_TNR_MAX_P;
 * cur, ref, out or sad not 4-byte aligned; wtab or held not 2-byte aligned; and an out whose extent
 * [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent of cur or of ref -- the window reads
 * neighbours, so the step cannot run in place. */
int dcvc_tnr_step(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps, float *out,
                  int32_t out_rs, int64_t out_ps, int32_t H, int32_t W, const uint16_t *wtab, int32_t P, uint32_t *sad,
                  uint16_t *held, void *stream);

#ifdef __cplusplus
}
#endif
#endif
