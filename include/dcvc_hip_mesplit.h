/* dcvc_hip_mesplit.h -- vectors per 8 x 8 sub-cell for the temporal noise prefilter: every quarter of a 16 x 16 cell chooses
 * again among the vectors that the search (dcvc_hip_me.h) or the refinement (dcvc_hip_mesub.h) found for its own cell and
 * the eight cells around it, and the gather moves the previous filtered picture sub-cell by sub-cell.  A cell that straddles
 * an object's edge then no longer moves all of its pixels by a vector that is right for a part of them only.  Encoder side
 * only, like the headers it stands beside: a P step of the filter is then dcvc_me_search, [dcvc_me_refine,] dcvc_me_split,
 * dcvc_me_compensate_split, dcvc_tnr_step.  The host side is vcm_ts_amd/tnr.py.
 *
 * Conventions, pictures (planar fp32 R, G, B with strides in elements), cells (16 x 16, hc x wc of them, number i * wc + j),
 * code(), Y and clamp() are those of dcvc_hip_me.h; quarter-pel components (whole part v >> 2, phase v & 3), the filters of
 * the phases, the interpolated luma YI and the fp32 folds are those of dcvc_hip_mesub.h.  0 or a negative DCVC_E_* code;
 * nothing launched and nothing dereferenced on a bad argument.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.
 *
 * Sub-cells are 8 x 8 on a grid of hs = 2 hc by ws = 2 wc.  Sub-cell (a, b), number a * ws + b, covers pixel rows
 * [8 a, 8 a + 8) and columns [8 b, 8 b + 8) INTERSECTED WITH THE PICTURE and belongs to cell (a >> 1, b >> 1).
 *
 * The input vectors mv_in are the cells', 2 hc wc int16 words, in 1 / unit pixels: unit = 1 for whole
 * pixels (dcvc_me_search's mv), unit = 4 for quarter pixels (dcvc_me_refine's mvq).  Every word is first clamped to
 * +-DCVC_ME_MAX_R at unit 1 and to +-(4 DCVC_ME_MAX_R + 3) = +-131 at unit 4, then multiplied by 4 / unit: everything below
 * is in QUARTER pixels, within -131 .. 131.
 *
 * The candidates of a sub-cell of cell (i, j) are the vectors of the cells (clamp(i + di, 0, rows - 1),
 * clamp(j + dj, 0, cols - 1)), di and dj in -1 .. 1, with rows = ceil(H / 16) and cols = ceil(W / 16), the cells that hold a
 * pixel: nine at the most, and equal candidates share a key, so duplicates change nothing.
 *     SAD8(v) = the sum over the sub-cell's pixels (y, x) of |Y(cur, y, x) - YI(ref, y, x, vy, vx)|            0 .. 16320
 *     J(v)    = 4 SAD8(v) + lambda * (|vy| + |vx|)                                                           < 2^18
 *   The sub-cell's vector is the candidate with the smallest key (J, |vy| + |vx|, vy, vx), the four compared in this order
 *   as signed integers (lexicographically): distinct candidates have distinct keys, so the choice does not depend on the
 *   order in which they are visited.
 *     mv8[2 * s] = vy, mv8[2 * s + 1] = vx     int16, ALWAYS quarter pixels, within -131 .. 131
 *     cost8[s]   = SAD8 of the chosen vector   uint32 (without the penalty)
 *   Every sub-cell is WRITTEN; a sub-cell that holds no pixel is written 0 in both.
 *   Nine equal candidates return that vector, and the four cost8 of the cell then add up to the cell's SAD of it.
 *
 * The compensation.  out(c, y, x) is exactly what dcvc_me_compensate_sub defines, with (vy, vx) = (mv8[2 s], mv8[2 s + 1]) of
 * the SUB-cell s that holds pixel (y, x): a whole vector (py == 0 and px == 0) copies the BITS of
 * ref(c, clamp(y + iy, 0, H - 1), clamp(x + ix, 0, W - 1)); a fractional one is folded in fp32, every product and every sum
 * one correctly rounded operation, none contracted, horizontal then vertical in increasing offset, a pass of phase 0 the
 * identity, the result fminf(fmaxf(a, 0.0f), 1.0f) with a zero of either sign written as +0.0f.  The coordinates are clamped
 * PER TAP whatever the int16 words hold, so every read is inside the H x W crop of ref.  With every cell's vector repeated
 * in its four sub-cells the output is dcvc_me_compensate_sub's, bit for bit.
 */
#ifndef DCVC_HIP_MESPLIT_H
#define DCVC_HIP_MESPLIT_H

#include <stdint.h>

#include "dcvc_hip_mesub.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MESPLIT_SUB 8  /* the side of a sub-cell */

/* The vector of every sub-cell, chosen among its cell's and the neighbours': one launch on `stream`, nothing synchronised.
 * mv_in: 2 hc wc int16 words in 1 / unit pixels; cur and ref may be the same picture.  Nothing outside mv8 (8 hc wc words)
 * and cost8 (4 hc wc words) is written.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref, mv_in, mv8 or cost8; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a
 * row stride < W; a plane stride < (H - 1) * row stride + W; lambda outside 0 .. DCVC_ME_MAX_LAMBDA; unit other than 1 or 4;
 * cur, ref or cost8 not 4-byte aligned; mv_in or mv8 not 2-byte aligned; the 8 hc wc words of mv8 overlapping the 2 hc wc
 * words of mv_in. */
int dcvc_me_split(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps, int32_t H,
                  int32_t W, int32_t lambda, int32_t unit, const int16_t *mv_in, int16_t *mv8, uint32_t *cost8, void *stream);

/* ref moved sub-cell by sub-cell by quarter-pel vectors into out: one launch on `stream`, nothing synchronised.  A cell whose
 * four sub-cells hold one vector is moved as dcvc_me_compensate_sub moves it.  Nothing outside the H x W crop of out is
 * touched.
 * Refused with DCVC_E_ARG, before anything else: a NULL ref, out or mv8; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row stride
 * < W; a plane stride < (H - 1) * row stride + W; ref or out not 4-byte aligned; mv8 not 2-byte aligned; and an out whose
 * extent [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent of ref. */
int dcvc_me_compensate_split(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                             int32_t W, const int16_t *mv8, void *stream);

#ifdef __cplusplus
}
#endif
#endif
