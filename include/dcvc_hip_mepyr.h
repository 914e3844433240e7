/* dcvc_hip_mepyr.h -- a hierarchical motion search in front of the temporal noise prefilter: the luma of a picture reduced
 * to one or two coarser levels, an exhaustive search on the coarsest level, and a descent level by level down to whole
 * pixels.  It writes exactly the three arrays dcvc_me_search (dcvc_hip_me.h) writes -- mv, cost, zero, same types, layout
 * and meaning -- so that the compensation and everything behind it stay what they are; it reaches 128 pixels where the full
 * search stops at 32.  Encoder side only.  The host side is vcm_ts_amd/tnr.py; this header is the device half.
 *
 * Conventions of dcvc_hip_me.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code, nothing
 * launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 R, G, B with strides in elements as
 * there, H and W the UNPADDED size, each within 1 .. DCVC_ROI_MAX_SIDE.  A BYTE PLANE is one level's luma, a byte per pixel:
 *   pixel (y, x) = p[y * stride + x],  stride in bytes, >= the level's width and a multiple of 4,  p 4-byte aligned.
 * Every entry point takes the PICTURE's H and W and the search's R and derives the level's own size and range.
 *
 * ARITHMETIC IS PART OF THE INTERFACE, and all of it is integer arithmetic, exact and independent of the order of
 * summation.  Y, code, clamp, the cells, hc and wc are those of dcvc_hip_me.h; `levels` L is 1 or 2.
 *
 * Levels.  Level 0 is the 8-bit luma Y of the H x W picture.  Level l + 1 has size H_{l+1} = ceil(H_l / 2),
 *   W_{l+1} = ceil(W_l / 2), and
 *     Y_{l+1}(y, x) = (a + b + c + d + 2) >> 2,   a .. d = Y_l(min(2 y + {0, 1}, H_l - 1), min(2 x + {0, 1}, W_l - 1)).
 *   So level 2 is the rounded mean of rounded means; it is not a 4 x 4 mean.
 *
 * Level ranges.  R_0 = R, R_1 = ceil(R / 2), R_2 = ceil(R / 4).  R lies within 2 .. 64 for L = 1 and within 4 .. 128 for
 *   L = 2; the coarsest radius is therefore at most 32.
 *
 * Key.  At every level the candidate with the smallest (J, |dy| + |dx|, dy, dx) wins, the four compared in this order as
 *   signed integers, as in dcvc_me_search.  A candidate that occurs twice in a candidate set has one key, so sets are sets.
 *   len = |dy| + |dx| below.
 *
 * Coarse search, at level L, for every cell (i, j) that holds a pixel (16 i < H and 16 j < W).  The candidates are all
 *   (dy, dx) with |dy|, |dx| <= R_L.  The support is, at level 2, the 8 x 8 block centred on the cell, rows [4 i - 2, 4 i + 6)
 *   and columns [4 j - 2, 4 j + 6), and at level 1 the cell's own rows [8 i, 8 i + 8) and columns [8 j, 8 j + 8), both
 *   INTERSECTED WITH THE LEVEL.
 *     SAD(dy, dx) = the sum over the support of |Y_L(cur, y, x) - Y_L(ref, clamp(y + dy, 0, H_L - 1), clamp(x + dx, 0, W_L - 1))|
 *     J = SAD + lambda * len at level 2,   J = 2 * SAD + lambda * len at level 1
 *   (64 samples stand for 256 pixels and a level-1 pixel of vector is two picture pixels: the factor keeps the trade per
 *   picture pixel that level 0 makes.  lambda stays the untuned placeholder it is.)
 *
 * Descent to level 1 (L = 2 only).  With p the cell's own level-2 vector the candidate set is
 *     { clamp(2 p + e, -R_1, R_1) componentwise : e in {-1, 0, 1}^2 } and (0, 0),
 *   SAD is taken over the cell's rows [8 i, 8 i + 8) and columns [8 j, 8 j + 8) intersected with level 1, and
 *   J = 2 * SAD + lambda * len.
 *
 * Descent to level 0.  With p the cell's level-1 vector the candidate set is
 *     { clamp(2 p + e, -R, R) componentwise : e in {-2 .. 2}^2 } and (0, 0),
 *   SAD and J = SAD + lambda * len are exactly dcvc_me_search's, over the cell's pixels, and
 *     mv[2 * cell] = dy, mv[2 * cell + 1] = dx     int16
 *     cost[cell]   = SAD of the chosen vector      uint32 (without the penalty)
 *     zero[cell]   = SAD(0, 0)                     uint32
 *   (0, 0) is always a candidate, so static ground stays static.  2 p + e is formed in 32 bits whatever the int16 words of
 *   the incoming vectors hold, and the clamp bounds it: the caller answers for the words' meaning only.
 *
 * Cells and writes.  A cell that holds no pixel is written 0 in every array of every level and takes part in nothing.
 *   Every word is WRITTEN, not added to.  The vector arrays of all levels have the layout of dcvc_me_search's mv: 2 hc wc
 *   int16 words, (dy, dx) of cell i * wc + j, in pixels of their own level.
 */
#ifndef DCVC_HIP_MEPYR_H
#define DCVC_HIP_MEPYR_H

#include <stdint.h>

#include "dcvc_hip_me.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MEPYR_MAX_LEVELS 2   /* L: 1 or 2 */
#define DCVC_MEPYR_MAX_R 128      /* R: 2 .. 64 for L = 1, 4 .. 128 for L = 2 */

/* The planar fp32 picture to its byte planes y0 (H x W), y1 (H_1 x W_1) and, when levels = 2, y2 (H_2 x W_2): ONE launch on
 * `stream`, nothing synchronised.  The fp32 picture is read once, here and nowhere else; every later kernel reads bytes.
 * Nothing outside the planes' pixels is written (not the bytes between a row's end and its stride).  With levels = 1, y2 and
 * s2 are ignored.
 * Refused with DCVC_E_ARG, before anything else: a NULL pic, y0 or y1 (y2 with levels = 2); H or W not in
 * 1 .. DCVC_ROI_MAX_SIDE; a row stride < W; a plane stride < (H - 1) * row stride + W; levels outside 1 .. 2; pic or a plane
 * not 4-byte aligned; a plane's stride below its level's width or no multiple of 4; and a plane whose extent
 * [y, y + (H_l - 1) * stride + W_l) overlaps another plane's or the picture's. */
int dcvc_me_pyramid(const float *pic, int32_t rs, int64_t ps, int32_t H, int32_t W, int32_t levels, uint8_t *y0, int32_t s0,
                    uint8_t *y1, int32_t s1, uint8_t *y2, int32_t s2, void *stream);

/* The coarse search of every cell on the level-`levels` byte planes of cur and ref into mv (2 hc wc words, in pixels of that
 * level): one launch on `stream`, nothing synchronised.  cur and ref may be the same plane.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref or mv; H or W not in 1 .. DCVC_ROI_MAX_SIDE; levels outside
 * 1 .. 2; R outside its range for `levels`; lambda outside 0 .. DCVC_ME_MAX_LAMBDA; a stride below the level's width or no
 * multiple of 4; cur or ref not 4-byte aligned; mv not 2-byte aligned. */
int dcvc_me_coarse(const uint8_t *cur, int32_t cur_s, const uint8_t *ref, int32_t ref_s, int32_t H, int32_t W, int32_t R,
                   int32_t levels, int32_t lambda, int16_t *mv, void *stream);

/* One descent: from the vectors mv_in of level `level` + 1 to the vectors mv of level `level` (1 or 0) on that level's byte
 * planes of cur and ref: one launch on `stream`, nothing synchronised.  At level 0 it also writes cost and zero (hc wc words
 * each); at level 1 both are ignored.  Level 1 exists with levels = 2 only.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, ref, mv_in or mv (cost or zero at level 0); H or W not in
 * 1 .. DCVC_ROI_MAX_SIDE; levels outside 1 .. 2; level outside 0 .. levels - 1; R outside its range for `levels`; lambda
 * outside 0 .. DCVC_ME_MAX_LAMBDA; a stride below the level's width or no multiple of 4; cur, ref, cost or zero not 4-byte
 * aligned; mv_in or mv not 2-byte aligned; mv_in and mv the same address. */
int dcvc_me_descend(const uint8_t *cur, int32_t cur_s, const uint8_t *ref, int32_t ref_s, int32_t H, int32_t W, int32_t R,
                    int32_t levels, int32_t level, int32_t lambda, const int16_t *mv_in, int16_t *mv, uint32_t *cost,
                    uint32_t *zero, void *stream);

#ifdef __cplusplus
}
#endif
#endif
