/* dcvc_hip_deint.h -- a motion-adaptive deinterlacer for interlaced 4:2:0 sources, on the sample planes of the file, in front
 * of the unchanged colour conversion (dcvc_hip_color.h).  Where the scene is static it weaves the two fields, and a static
 * progressive picture comes back bit for bit; where something moves it interpolates inside the field, clamped to what the
 * neighbouring fields allow.  Encoder side only: the bitstream and the decoder know nothing of it.  The host side is
 * vcm_ts_amd/deint.py; this header is the device half, and tests/deint_ref.py restates it in numpy.
 *
 * Conventions of dcvc_hip_color.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  Sample planes are 8-bit (one byte per sample) or 10-bit
 * (16-bit little-endian words read as unsigned) with row strides in SAMPLES: luma H x W, both chroma planes H/2 x W/2.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Everything is integer arithmetic on the file's own samples, applied to the Y, U and
 * V planes independently with the same rule; a 4:2:0 chroma plane's rows alternate between the fields exactly as the luma's
 * do (the plane is treated as two co-sited fields: the quarter-line vertical offset of interlaced chroma is NOT corrected).
 *
 * Fields.  Frame n holds the top field (even rows) and the bottom field (odd rows).  Field time is f = 2 n + s, s = 0 for
 * the earlier field of the frame (`second` = s); `parity` p is the row parity the field owns (top field first: p = s,
 * bottom field first: p = 1 - s).
 *
 * The output picture for field f of frame n = cur, per plane of PH rows:
 *   rows of parity p are copied from cur;
 *   for a missing row r (parity 1 - p) and column x, with
 *     (A, B) = (prev, cur) for the earlier field (second = 0), (cur, next) for the later one (second = 1) -- the frames
 *              that hold fields f - 1 and f + 1; both own row r, and one of them is cur itself,
 *     P2 = prev, N2 = next,
 *     a row index q outside 0 .. PH - 1 replaced by the nearest row inside the plane that has q's parity
 *     (q < 0: q & 1; q > PH - 1: PH - 2 + (q & 1)),
 *     >> an arithmetic shift and max = 2^depth - 1:
 *
 *     c  = cur[r-1][x]   e  = cur[r+1][x]   c3 = cur[r-3][x]   e3 = cur[r+3][x]
 *     d    = (A[r][x] + B[r][x]) >> 1
 *     td0  = |A[r][x] - B[r][x]|
 *     td1  = (|P2[r-1][x] - c| + |P2[r+1][x] - e|) >> 1
 *     td2  = (|N2[r-1][x] - c| + |N2[r+1][x] - e|) >> 1
 *     diff = max(td0 >> 1, td1, td2)
 *     pred = clip((9 (c + e) - (c3 + e3) + 8) >> 4, 0, max)
 *     out  = min(max(pred, d - diff), d + diff)
 *
 * There is no horizontal term.  A frame outside the file is replaced by the caller with cur itself: prev or next may be
 * passed equal to cur (the first and the last frame of a file have one temporal neighbour replaced by themselves).
 *
 * The count:  moved[b] (uint32), b = 0 .. ceil(H / DCVC_DEINT_BAND) - 1: the number of missing LUMA samples in luma rows
 *   [DCVC_DEINT_BAND b, DCVC_DEINT_BAND (b + 1)) with diff > 0.  Every word is WRITTEN, not added to.
 *
 * Nothing outside the three output planes' H x W (H/2 x W/2) samples, nor outside moved[0 .. n_moved), is touched, and the
 * inputs are only read.
 */
#ifndef DCVC_HIP_DEINT_H
#define DCVC_HIP_DEINT_H

#include <stdint.h>

#include "dcvc_hip_color.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_DEINT_BAND 8 /* luma rows per word of `moved` (and per workgroup) */

/* One output picture: one launch on `stream` for all three planes, nothing synchronised.  *_ys / *_cs: the row strides of
 * the luma plane and of the two chroma planes of a frame, in samples.  A plane whose bases (in all three frames, or in the
 * output) are 16-byte aligned and whose strides are multiples of 16 bytes is accessed 16 bytes at a time, any other sample
 * by sample: same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL plane or a NULL moved; H not a positive multiple of 4 (an
 * interlaced 4:2:0 chroma plane needs an even number of rows), W not positive and even, a side beyond DCVC_COLOR_MAX_SIDE;
 * a luma stride < W or a chroma stride < W / 2; a bit_depth other than 8 or 10, a parity or a `second` other than 0 or 1;
 * at 10 bits a plane that is not 2-byte aligned; a moved that is not 4-byte aligned; n_moved != ceil(H / DCVC_DEINT_BAND);
 * an output plane whose extent [base, base + (rows - 1) * stride + width) overlaps the extent of any input plane or of
 * another output plane. */
int dcvc_deinterlace420(const void *prev_y, const void *prev_u, const void *prev_v, int32_t prev_ys, int32_t prev_cs,
                        const void *cur_y, const void *cur_u, const void *cur_v, int32_t cur_ys, int32_t cur_cs,
                        const void *next_y, const void *next_u, const void *next_v, int32_t next_ys, int32_t next_cs, int32_t H,
                        int32_t W, int32_t bit_depth, int32_t parity, int32_t second, void *out_y, void *out_u, void *out_v,
                        int32_t out_ys, int32_t out_cs, uint32_t *moved, int32_t n_moved, void *stream);

#ifdef __cplusplus
}
#endif
#endif
