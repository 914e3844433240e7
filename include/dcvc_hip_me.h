/* dcvc_hip_me.h -- block motion search and motion compensation in front of the temporal noise prefilter
 * (dcvc_hip_tnr.h): an integer-pel full search per 16 x 16 cell of the current picture in the previous filtered picture,
 * and the gather that moves every cell of that picture by its vector, so that dcvc_tnr_step, unchanged, blends a moving
 * object with where it was and not with what stood behind it.  Encoder side only, like the filter.  The host side is
 * vcm_ts_amd/tnr.py; this header is the device half.
 *
 * Conventions of dcvc_hip_tnr.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code, nothing
 * launched (and nothing dereferenced) on a bad argument.  Pictures are PLANAR fp32 R, G, B with explicit strides in
 * elements:
 *   element (c, y, x) = p[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * H and W the UNPADDED size, each within 1 .. DCVC_ROI_MAX_SIDE.
 *
 * The cells are those of the q-scale maps (dcvc_hip_roi.h, "Latent grid"): hc = 4 ceil(H / 64), wc = 4 ceil(W / 64); cell
 * (i, j), number i * wc + j, covers pixel rows [16 i, 16 i + 16) and columns [16 j, 16 j + 16) INTERSECTED WITH THE PICTURE.
 *
 * ARITHMETIC IS PART OF THE INTERFACE, and all of it is integer arithmetic, exact and independent of the order of
 * summation.  With code(v) = (int) rint(255.0f * clamp01(v)) (a NaN codes as 0) and the luma
 * Y = (54 r + 183 g + 19 b + 128) >> 8 of the three codes, both exactly as in dcvc_hip_tnr.h, and
 * clamp(v, lo, hi) = min(max(v, lo), hi):
 *
 * The search.  For a cell and a candidate vector (dy, dx), |dy| <= R and |dx| <= R:
 *     SAD(dy, dx) = the sum over the cell's pixels (y, x) of
 *                   |Y(cur, y, x) - Y(ref, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1))|          0 .. 65280
 *     J(dy, dx)   = SAD(dy, dx) + lambda * (|dy| + |dx|)                                              < 2^17
 *   The cell's vector is the candidate with the smallest key (J, |dy| + |dx|, dy, dx), the four compared in this order
 *   as signed integers (lexicographically).  No two candidates share a key, so the choice does not depend on the order in
 *   which candidates are visited.  Of equal J the shorter vector wins, of equally short ones the smaller dy, then the
 *   smaller dx.
 *     mv[2 * cell] = dy, mv[2 * cell + 1] = dx     int16
 *     cost[cell]   = SAD of the chosen vector      uint32 (without the penalty)
 *     zero[cell]   = SAD(0, 0)                     uint32
 *   Every cell is WRITTEN, not added to; a cell that holds no pixel is written 0 in all three.
 *
 * The compensation.  With (dy, dx) = (mv[2 * cell], mv[2 * cell + 1]) of the cell that holds pixel (y, x):
 *     out(c, y, x) = the bits of ref(c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1))     c = 0, 1, 2
 *   Bits are copied: a NaN keeps its payload, -0.0 its sign.  The coordinates are clamped whatever the int16 words hold,
 *   so every read is inside the H x W crop of ref; the caller answers for the words' meaning only.
 */
#ifndef DCVC_HIP_ME_H
#define DCVC_HIP_ME_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_ME_MAX_R 32        /* R: 1 .. 32 pixels in each direction */
#define DCVC_ME_MAX_LAMBDA 255  /* lambda: 0 .. 255 luma codes per pixel of vector length */

/* The search of every cell of cur in ref: one launch on `stream`, nothing synchronised.  cur and ref may be the same
 * picture.  Nothing outside the three hc wc arrays (mv: 2 hc wc words) is written.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref, mv, cost or zero; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a
 * row stride < W; a plane stride < (H - 1) * row stride + W; R outside 1 .. DCVC_ME_MAX_R; lambda outside
 * 0 .. DCVC_ME_MAX_LAMBDA; cur, ref, cost or zero not 4-byte aligned; mv not 2-byte aligned. */
int dcvc_me_search(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps, int32_t H,
                   int32_t W, int32_t R, int32_t lambda, int16_t *mv, uint32_t *cost, uint32_t *zero, void *stream);

/* ref moved cell by cell into out: one launch on `stream`, nothing synchronised.  A quad of four pixels is read as one
 * 16-byte access where ref's base and strides and the cell's dx allow it (dx a multiple of 4, the quad's source inside the
 * row) and written as one where out's base and strides do; anything else goes element by element: same bits.  Nothing
 * outside the H x W crop of out is touched.
 * Refused with DCVC_E_ARG, before anything else: a NULL ref, out or mv; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row stride
 * < W; a plane stride < (H - 1) * row stride + W; ref or out not 4-byte aligned; mv not 2-byte aligned; and an out whose
 * extent [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent of ref. */
int dcvc_me_compensate(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                       int32_t W, const int16_t *mv, void *stream);

#ifdef __cplusplus
}
#endif
#endif
