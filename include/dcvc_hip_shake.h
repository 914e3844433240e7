/* dcvc_hip_shake.h -- the shake of a fixed camera, measured ahead of the scans that assume a static pixel stays where it is
 * (dcvc_hip_motion.h, dcvc_hip_noise.h): ONE whole-pixel vector per picture against an anchor picture, from a 2-D search on a
 * sparse sample of every 64 x 64 tile and a median vote over the tiles.  The unchanged dcvc_me_compensate (dcvc_hip_me.h) then
 * moves the picture onto the anchor.  The host side is vcm_ts_amd/shake.py; this header is the device half.
 *
 * Conventions of dcvc_hip_noise.h and dcvc_hip_me.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative
 * DCVC_E_* code, nothing launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 R, G, B with
 * explicit strides in elements:
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * H and W the UNPADDED size, each within 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  The only floating-point operation is the one multiply of code() below; everything
 * else is integer arithmetic, exact and independent of the order of summation.
 *
 * Per pixel:   r, g, b = code(v) = (int) rint(255.0f * clamp01(v)) of the three planes (dcvc_hip_scene.h; a NaN codes
 *   as 0);  Y = (54 r + 183 g + 19 b + 128) >> 8,  0 <= Y <= 255  (the luma of dcvc_hip_scene.h);
 *   clamp(v, lo, hi) = min(max(v, lo), hi)  (dcvc_hip_me.h).
 *
 * The anchor plane:  H rows of y_stride bytes (uint8), y_stride >= W and a multiple of 4: exactly the format of
 *   dcvc_noise_cells' ycur.  Byte (y, x), x < W, holds the Y of the anchor picture's pixel; the bytes of a row from column W
 *   on are never written by dcvc_shake_plane and never read by dcvc_shake_tiles.
 *
 * The tiles:   64 x 64 pixels on a picture-aligned grid, th = H / 64 rows of tw = W / 64 tiles (integer division): only
 *   tiles that lie wholly inside the picture exist, and the margin right of and below them belongs to no tile.  For tile
 *   (a, b) and every candidate (dy, dx), |dy| <= R and |dx| <= R:
 *     SAD(dy, dx) = the sum over i = 0 .. 15 and j = 0 .. 63 of
 *                   |Y(cur, 64 a + 4 i, 64 b + j) - anchor(clamp(64 a + 4 i + dy, 0, H - 1), clamp(64 b + j + dx, 0, W - 1))|
 *   1024 terms, 0 .. 261120.  Every fourth row of the tile is taken (rows stay runs of contiguous bytes); the same samples
 *   of cur are held against every whole-pixel shift of the FULL anchor, so the subsampling does not alias.
 *   The tile's vector is the candidate with the smallest key (SAD, |dy| + |dx|, dy, dx), the four compared in this order as
 *   signed integers (lexicographically), as in dcvc_hip_me.h.  No two candidates share a key, so the choice does not depend
 *   on the order in which candidates are visited.  The sign is that header's: cur(y, x) ~ anchor(y + dy, x + dx).
 *   Tile (a, b) WRITES five int32 words, tiles[5 * (a * tw + b) + 0 .. 4]:
 *     0: dy     1: dx     2: the SAD of the choice     3: the LARGEST SAD over all candidates     4: SAD(0, 0)
 *   Nothing outside the 5 th tw words is touched.
 *
 * The vote:    over n_tiles records of five words.  A tile VOTES when |dy| <= R and |dx| <= R (nothing out of range is ever
 *   indexed), its largest SAD is positive, and twice its chosen SAD does not exceed its largest: 2 * tile[2] <= tile[3].  A
 *   flat tile, with or without noise, sees the same SAD at every shift and has no opinion; a tile of exact zeros does not
 *   vote.  With n the number of voting tiles:
 *     my = the lower median of their dy: the element of rank (n - 1) / 2 in ascending order; mx = the lower median of their
 *          dx, taken independently.  Both come from counting into 2 R + 1 bins: exact whatever the order.  n == 0: both 0.
 *     agree  = the number of voting tiles whose vector equals (my, mx)  (0 is possible: the medians may come from two tiles)
 *     status = bit 0 (DCVC_SHAKE_FEW): n < min_votes;  bit 1 (DCVC_SHAKE_EDGE): |my| == R or |mx| == R -- the true motion
 *              may lie beyond the range, as in a pan
 *     (dy, dx) = (my, mx) when status == 0, else (0, 0)
 *   record[0 .. 7], int32, is WRITTEN:  dy, dx, n, agree, n_tiles, status, my, mx.
 *   Every cell of mv -- hc wc pairs of int16 on the grid of the q-scale maps (dcvc_hip_roi.h, "Latent grid"): hc = 4 ceil(H /
 *   64), wc = 4 ceil(W / 64) -- is WRITTEN (-dy, -dx): the unchanged dcvc_me_compensate(cur -> out, mv) then gives
 *     out(c, y, x) = the bits of cur(c, clamp(y - dy, 0, H - 1), clamp(x - dx, 0, W - 1)),
 *   the picture registered onto the anchor.  Nothing outside record and the 2 hc wc words of mv is touched.
 */
#ifndef DCVC_HIP_SHAKE_H
#define DCVC_HIP_SHAKE_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_SHAKE_TILE 64
#define DCVC_SHAKE_ROWS 16          /* the sampled rows of a tile: every fourth */
#define DCVC_SHAKE_MAX_R 16         /* R: 1 .. 16 pixels in each direction */
#define DCVC_SHAKE_MAX_TILES 16384  /* (DCVC_ROI_MAX_SIDE / 64)^2 */
#define DCVC_SHAKE_WORDS 5          /* int32 words per tile */
#define DCVC_SHAKE_RECORD 8         /* int32 words per picture */
#define DCVC_SHAKE_FEW 1
#define DCVC_SHAKE_EDGE 2

/* The luma of a picture as a byte plane: one launch on `stream`, nothing synchronised.  A picture whose base is 16-byte
 * aligned and whose strides are multiples of 4 is read 16 bytes at a time, any other 4 bytes at a time; the plane is written
 * 4 bytes (4 pixels) at a time wherever the four lie inside the picture, else byte by byte: same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL rgb or y; H or W not in 1 .. DCVC_ROI_MAX_SIDE; row_stride < W;
 * plane_stride < (H - 1) * row_stride + W; y_stride < W or not a multiple of 4; rgb or y not 4-byte aligned. */
int dcvc_shake_plane(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint8_t *y,
                     int32_t y_stride, void *stream);

/* The search of every tile of the picture in the anchor plane: one launch on `stream`, one workgroup per tile, nothing
 * synchronised, no global atomics.  The picture is read at a quarter of its rows only.  With no tile (H < 64 or W < 64)
 * nothing is launched, nothing is written and the answer is 0.
 * Refused with DCVC_E_ARG, before anything else: a NULL rgb, anchor or tiles; H or W not in 1 .. DCVC_ROI_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; y_stride < W or not a multiple of 4; R outside
 * 1 .. DCVC_SHAKE_MAX_R; rgb, anchor or tiles not 4-byte aligned. */
int dcvc_shake_tiles(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, const uint8_t *anchor,
                     int32_t y_stride, int32_t R, int32_t *tiles, void *stream);

/* The vote of n_tiles tile records, the picture's record and the uniform vector field: one launch of ONE workgroup on
 * `stream`, nothing synchronised.  n_tiles == 0 is a vote of nobody (tiles is then not read, but must not be NULL).
 * Refused with DCVC_E_ARG, before anything else: a NULL tiles, record or mv; n_tiles outside 0 .. DCVC_SHAKE_MAX_TILES; R
 * outside 1 .. DCVC_SHAKE_MAX_R; min_votes outside 1 .. DCVC_SHAKE_MAX_TILES; H or W not in 1 .. DCVC_ROI_MAX_SIDE; tiles
 * or record not 4-byte aligned; mv not 2-byte aligned. */
int dcvc_shake_vote(const int32_t *tiles, int32_t n_tiles, int32_t R, int32_t min_votes, int32_t H, int32_t W, int32_t *record,
                    int16_t *mv, void *stream);

#ifdef __cplusplus
}
#endif
#endif
