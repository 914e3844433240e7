/* dcvc_hip_mesub.h -- quarter-pel motion for the temporal noise prefilter: the refinement of dcvc_me_search's whole-pel
 * vectors to quarter pixels, and the gather that moves every cell of the previous filtered picture by such a vector through
 * a separable interpolation filter.  Encoder side only, like dcvc_hip_me.h, which they stand beside: a P step of the filter
 * is then dcvc_me_search, dcvc_me_refine, dcvc_me_compensate_sub, dcvc_tnr_step.  The host side is vcm_ts_amd/tnr.py.
 *
 * Conventions, pictures (planar fp32 R, G, B with strides in elements), cells (16 x 16, number i * wc + j), code(), Y and
 * clamp() are those of dcvc_hip_me.h.  0 or a negative DCVC_E_* code; nothing launched and nothing dereferenced on a bad
 * argument.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Vectors are in QUARTER pixels.  A component v has the whole part i = v >> 2 (the
 * floor of v / 4, an arithmetic shift) and the phase p = v & 3, so v = 4 i + p.  The interpolation filter of a phase, as
 * (offset of the first tap; the taps), each summing to 64:
 *     p = 0   ( 0;  64)                                      the sample itself
 *     p = 1   (-3;  -1,  4, -10, 58, 17,  -5,  1)
 *     p = 2   (-3;  -1,  4, -11, 40, 40, -11,  4, -1)
 *     p = 3   (-2;   1, -5,  17, 58, -10,  4, -1)
 * Tap k of a filter with first offset o reads coordinate clamp(n + i + o + k, 0, side - 1): every coordinate is clamped to
 * the picture PER TAP.
 *
 * The interpolated luma YI(ref, y, x, vy, vx), all of it integer arithmetic, exact and independent of the order of summation:
 *     h(r, x)  = the sum over the taps t_k of px of  t_k * Y(ref, r, clamp(x + ix + o + k, 0, W - 1))      no rounding;
 *                                                                                  within -6120 .. 22440: fits int16
 *     s(y, x)  = the sum over the taps t_j of py of  t_j * h(clamp(y + iy + o + j, 0, H - 1), x)
 *     YI       = clamp((s + 2048) >> 12, 0, 255)                                  (an arithmetic shift)
 *   Phase 0 is the single tap 64, so a whole vector (py = px = 0) gives Y(ref, clamp(y + iy), clamp(x + ix)) itself.
 *
 * The refinement.  For a cell, d = (clamp(mv_in[2 cell], -R, R), clamp(mv_in[2 cell + 1], -R, R)) with R = DCVC_ME_MAX_R.
 *   The candidates are the 49 vectors v = 4 d + f, f = (fy, fx) with fy and fx in -3 .. 3.
 *     SAD(v) = the sum over the cell's pixels (y, x) of |Y(cur, y, x) - YI(ref, y, x, vy, vx)|            0 .. 65280
 *     J(v)   = 4 SAD(v) + lambda * (|vy| + |vx|)                                                         < 2^19
 *   which at f = 0 is four times dcvc_me_search's J of d.  The cell's vector is the candidate with the smallest key
 *   (J, |vy| + |vx|, vy, vx), the four compared in this order as signed integers (lexicographically): no two candidates
 *   share a key, so the choice does not depend on the order in which candidates are visited.
 *     mvq[2 * cell] = vy, mvq[2 * cell + 1] = vx     int16, quarter pixels, within -131 .. 131
 *     cost[cell]    = SAD of the chosen vector       uint32 (without the penalty)
 *   Every cell is WRITTEN; a cell that holds no pixel is written 0 in both.
 *
 * The compensation.  With (vy, vx) = (mvq[2 * cell], mvq[2 * cell + 1]) of the cell that holds pixel (y, x):
 *   py == 0 and px == 0:  out(c, y, x) = the BITS of ref(c, clamp(y + iy, 0, H - 1), clamp(x + ix, 0, W - 1)), exactly as
 *     dcvc_me_compensate copies them: a NaN keeps its payload, -0.0 its sign.
 *   otherwise fp32, every product and every sum one correctly rounded operation, none contracted into a fused multiply-add,
 *   with the taps t_k = tap / 64 (exact in fp32):
 *     a pass whose phase is 0 is the identity (no arithmetic at all);
 *     a pass whose phase is not 0 folds its taps in increasing offset:  a = t_0 * x_0;  a = a + (t_k * x_k), k = 1, 2, ...
 *     horizontal first, over the samples ref(c, r, clamp(x + ix + o + k)) of each row r = clamp(y + iy + o + j) the vertical
 *     pass needs (the row r = clamp(y + iy) alone where py == 0), then vertical over those results; the horizontal result
 *     is an fp32 value, unclamped.
 *     out(c, y, x) = fminf(fmaxf(a, 0.0f), 1.0f), a zero of either sign written as +0.0f: within [0, 1], and 0 for a NaN
 *     (an infinity among the samples makes NaNs or infinities of the sums; they end as 0 or 1 like any other value).
 *   Denormals are neither flushed on the way in nor on the way out: a product or a sum that is denormal is kept as IEEE 754
 *   gives it, so a numpy float32 evaluation in this order gives the same bits.
 *   The coordinates are clamped whatever the int16 words hold, so every read is inside the H x W crop of ref.
 */
#ifndef DCVC_HIP_MESUB_H
#define DCVC_HIP_MESUB_H

#include <stdint.h>

#include "dcvc_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MESUB_UNIT 4  /* vectors are in 1 / 4 pixels */

/* The refinement of every cell's vector: one launch on `stream`, nothing synchronised.  mv_in: dcvc_me_search's mv (2 hc wc
 * int16 words, whole pixels); cur and ref may be the same picture.  Nothing outside mvq (2 hc wc words) and cost (hc wc
 * words) is written.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref, mv_in, mvq or cost; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a
 * row stride < W; a plane stride < (H - 1) * row stride + W; lambda outside 0 .. DCVC_ME_MAX_LAMBDA; cur, ref or cost not
 * 4-byte aligned; mv_in or mvq not 2-byte aligned; the 2 hc wc words of mvq overlapping those of mv_in. */
int dcvc_me_refine(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps, int32_t H,
                   int32_t W, int32_t lambda, const int16_t *mv_in, int16_t *mvq, uint32_t *cost, void *stream);

/* ref moved cell by cell by quarter-pel vectors into out: one launch on `stream`, nothing synchronised.  A cell whose vector
 * is whole is copied as dcvc_me_compensate copies it (16-byte accesses where the bases, the strides and the vector allow
 * them: same bits).  Nothing outside the H x W crop of out is touched.
 * Refused with DCVC_E_ARG, before anything else: a NULL ref, out or mvq; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row stride
 * < W; a plane stride < (H - 1) * row stride + W; ref or out not 4-byte aligned; mvq not 2-byte aligned; and an out whose
 * extent [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent of ref. */
int dcvc_me_compensate_sub(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                           int32_t W, const int16_t *mvq, void *stream);

#ifdef __cplusplus
}
#endif
#endif
