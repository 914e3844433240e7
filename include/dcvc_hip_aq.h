/* dcvc_hip_aq.h -- backward-adaptive quantisation: a per-cell q-scale map for a P picture, made from the reference
 * picture that encoder and decoder both hold bit for bit (the DPB's ref_frame).  The map is a pure INTEGER function of the
 * 8-bit codes of that picture, so the decoder rebuilds it on its own and the bitstream carries nothing.  It is used as the
 * q-scale map of dcvc_hip_roi.h is: one more factor on the step of the latent y, cell by cell.
 *
 * Conventions of dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 with explicit strides in
 * elements:
 *   element (c, y, x) = pic[c * plane_stride + y * row_stride + x],  row_stride >= Wp,
 *   plane_stride >= (Hp - 1) * row_stride + Wp,
 * three planes R, G, B.  It is the PADDED reference picture: Hp and Wp are positive multiples of 64, at most
 * DCVC_ROI_MAX_SIDE.  The grid is hc = Hp / 16 rows by wc = Wp / 16 columns of DCVC_ROI_CELL x DCVC_ROI_CELL pixels; cell
 * (i, j) covers pixel rows [16 i, 16 i + 16) and columns [16 j, 16 j + 16).  EVERY cell counts, the padding's included:
 * it is the same picture on both sides.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  The only floating-point operations are those of code() below and the one
 * multiply that reads a ROI factor back as hundredths; each is one correctly rounded fp32 operation in the order written
 * (no contraction), rint is round-half-to-even.  Everything else is integer arithmetic, exact and independent of the
 * order of summation.
 *
 * Per pixel:   r, g, b = code(v) = (int) rint(255.0f * clamp01(v)) of the three planes, as dcvc_hip_roi.h defines it (a
 *   NaN codes as 0);  Y = (54 r + 183 g + 19 b + 128) >> 8,  0 <= Y <= 255  (the luma of dcvc_hip_scene.h).
 *
 * Per cell of 256 pixels:   S1 = sum Y,  S2 = sum Y^2,  V = 256 S2 - S1^2  (256^2 times the variance of Y).
 *   0 <= V <= 1065369600 < 2^30: a flat cell has V = 0, a cell half 0 and half 255 the maximum.  256 S2 reaches
 *   4261478400 > 2^31: it is formed in unsigned 32-bit arithmetic.
 *
 * Activity:   v = V + 1,  e = floor(log2 v) (the position of v's leading one),  m = the 8 bits below the leading one
 *   (e >= 8: (v >> (e - 8)) & 255;  e < 8: (v << (8 - e)) & 255, zero-filled),  L = 256 e + m.
 *   L is a piecewise-linear log2 in 1/256 units: monotone in V, L = 0 for a flat cell, 0 <= L <= 7935, and
 *   0 <= 256 log2(V + 1) - L < 256 * 0.08608 + 1 < 23.04: with x = v / 2^e - 1, log2(1 + x) - x is at most
 *   1 + log2(log2 e) - log2 e = 0.086071.. (at x = 1 / ln 2 - 1), and truncating 256 x to 8 bits loses less than 1.
 *
 * Picture mean:   M = floor(sum of L over all cells / (hc wc)), the sum in unsigned 64-bit.
 *
 * Per cell:   d = L - M,  -7935 <= d <= 7935,  k_aq = ktab[d + 7935].
 *   ktab: DCVC_AQ_KTAB = 15871 uint16 built by the HOST in float64 for a strength A in hundredths, 1 <= A <= 400, and a
 *   clamp 10 <= lo <= 100 <= hi <= 1000:
 *     k(d) = min(max(rint(100 * 2^(A d / (100 * 256 * 6))), lo), hi).
 *   This is the form of x265's auto-variance mode: A / 100 is the QP offset per doubling of the variance at 6 QP per
 *   doubling of the step; a cell flatter than the picture's mean gets a finer step (k < 100), a busier one a coarser
 *   step.  k(0) = 100.  The device never evaluates an exponential.
 *
 * With a ROI map (dcvc_roi_qmap's, hc wc floats) also present:
 *     k_roi = (int) rint(100.0f * roi[cell]),   k = min(max((k_roi k_aq + 50) / 100, 10), 1000)
 *   (integer division; the product in 64-bit).  Without one, k = k_aq.
 *
 * Output:   map[cell] = ftab[k - 10],  ftab[i] = (float) (i + 10) / 100.0f for i in 0 .. DCVC_AQ_FTAB - 1 = 990 as the
 *   HOST's IEEE division gives it -- the floats of dcvc_hip_roi.h's factors; the device never computes a factor.  k = 100
 *   gives 1.0f, which codes the bits of no map at all.
 *
 * The kernels clamp d + 7935 and k - 10 to their tables before they index them: no effect on the values above, and no
 * content of L, sum or roi_map can make a kernel address anything outside the tables.
 */
#ifndef DCVC_HIP_AQ_H
#define DCVC_HIP_AQ_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_AQ_MAX_L 7935                     /* 256 * 31 - 1 */
#define DCVC_AQ_KTAB (2 * DCVC_AQ_MAX_L + 1)   /* entries of ktab, d = -7935 .. 7935 */
#define DCVC_AQ_FTAB 991                       /* entries of ftab, k = 10 .. 1000 */
#define DCVC_AQ_MAX_STRENGTH 400               /* A, in hundredths */

/* L[i * wc + j] = the activity of cell (i, j) (hc wc int32, DEVICE), and the sum of all of them ADDED to *sum (one
 * unsigned 64-bit DEVICE integer, 8-byte aligned; the caller zeroes it -- on the same stream -- before the call).  One
 * launch on `stream`, nothing synchronised.  A picture whose base is 16-byte aligned and whose strides are multiples of 4
 * is read 16 bytes at a time, any other 4 bytes at a time: same results.
 * Refused (DCVC_E_ARG): NULL pic, L or sum; Hp or Wp not a positive multiple of 64, or above DCVC_ROI_MAX_SIDE;
 * row_stride < Wp; plane_stride < (Hp - 1) * row_stride + Wp; pic or L not 4-byte aligned; sum not 8-byte aligned. */
int dcvc_aq_activity(const float *pic, int32_t row_stride, int64_t plane_stride, int32_t Hp, int32_t Wp, int32_t *L,
                     uint64_t *sum, void *stream);

/* map[cell] for the hc wc cells from L and *sum as dcvc_aq_activity left them (all DEVICE pointers: L, sum, ktab of
 * DCVC_AQ_KTAB uint16, ftab of DCVC_AQ_FTAB floats, roi_map of hc wc floats or NULL for none, map of hc wc floats).  One
 * launch on `stream`, one thread per cell, nothing synchronised.
 * Refused (DCVC_E_ARG): NULL L, sum, ktab, ftab or map; hc or wc not a positive multiple of 4, or above
 * DCVC_ROI_MAX_SIDE / 16; sum not 8-byte aligned; L, ftab, roi_map or map not 4-byte aligned; ktab not 2-byte aligned. */
int dcvc_aq_map(const int32_t *L, const uint64_t *sum, int32_t hc, int32_t wc, const uint16_t *ktab, const float *ftab,
                const float *roi_map, float *map, void *stream);

#ifdef __cplusplus
}
#endif
#endif
