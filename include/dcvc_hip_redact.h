/* dcvc_hip_redact.h -- ROI redaction on the codec's input: inside the boxes of the selected classes the picture the
 * codec is handed is replaced by a mosaic (every tile of a picture-aligned grid shows the rounded mean of its own
 * pixels) or by a solid fill, and everywhere else it is the source, bit for bit.  Encoder side only: the bitstream and
 * the decoder know nothing of it.  The host side is vcm_ts_amd/redact.py; this header is the device half.
 *
 * A mosaic is NOT a security guarantee: small tiles over text can be partly inverted.  The solid fill removes the
 * content; the mosaic only makes it hard to read.
 *
 * Conventions of dcvc_hip_tnr.h and dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative
 * DCVC_E_* code, nothing launched (and nothing dereferenced) on a bad argument.  The two pictures are PLANAR fp32 R, G, B
 * with explicit strides in elements:
 *   element (c, y, x) = p[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read and written in place.  H and W are the UNPADDED size, each within
 * 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.  Boxes are dcvc_roi_box_t records as in
 * dcvc_hip_roi.h, passed twice (the host list is validated, the device list is read), 0 .. DCVC_ROI_MAX_BOXES of them.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Everything is integer arithmetic, exact and independent of the order of
 * summation; the only floating-point work is the one multiply of code().
 *
 * Region R:  the pixels inside any non-empty box (x2 > x1 and y2 > y1) whose class bit is set in class_mask
 *   ((class_mask >> cls) & 1), after the box is grown by `grow` pixels and clipped to the picture by the q-map's formulas:
 *     x1' = max(x1 - grow, 0), x2' = min(x2 + grow, W), y1' = max(y1 - grow, 0), y2' = min(y2 + grow, H).
 *   Boxes of other classes are ignored (their cls is still validated).  List order does not matter.
 *
 * Mosaic (tile in {2, 4, 8, 16, 32, 64}, fill == -1):  tiles lie on a picture-aligned grid from (0, 0) -- the grid does
 *   not move with the boxes, so a static scene does not shimmer.  Tile (I, J) covers rows [tile I, tile I + tile) and
 *   columns [tile J, tile J + tile) INTERSECTED WITH THE PICTURE; it holds n_t pixels.  Per channel
 *     S = the sum of code(src) over ALL n_t pixels of the tile, in R or not,
 *         code(v) = (int) rint(255.0f * clamp01(v)), a NaN codes as 0 (dcvc_hip_roi.h),
 *     m = (2 S + n_t) / (2 n_t)   (integer floor: the mean rounded half up, 0 .. 255),
 *     out(p) = T[m] for p in R,   T[k] = (float) k / 255.0f as the HOST's IEEE division gives it.
 *
 * Solid (tile == 0, fill in 0 .. 255):  out(p) = T[fill] for p in R.
 *
 * Outside R:  out(p) is the BITS of src(p).  A NaN stays that NaN.
 *
 * Counts:  count[i * wc + j] (uint16) on the grid of the q-scale maps (dcvc_hip_roi.h, "Latent grid"):
 *   hc = 4 ceil(H / 64), wc = 4 ceil(W / 64); cell (i, j) covers pixel rows [16 i, 16 i + 16) and columns
 *   [16 j, 16 j + 16) INTERSECTED WITH THE PICTURE.  count is the number of pixels of R in the cell (0 .. 256).  Every
 *   cell is WRITTEN, not added to; a cell that holds no pixel is written 0.
 *
 * Nothing outside the H x W crop of out, nor outside the hc wc words of count, is touched.
 */
#ifndef DCVC_HIP_REDACT_H
#define DCVC_HIP_REDACT_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_REDACT_MAX_TILE 64 /* tile sides: the powers of two 2 .. 64 */

/* One picture: one launch on `stream`, nothing synchronised.  A picture whose base is 16-byte aligned and whose strides
 * are multiples of 4 is accessed 16 bytes at a time, any other 4 bytes at a time (each of the two on its own): same
 * results.
 * Refused with DCVC_E_ARG, before anything else: a NULL src, out or count; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row
 * stride < W; a plane stride < (H - 1) * row stride + W; src or out not 4-byte aligned; count not 2-byte aligned; n
 * outside 0 .. DCVC_ROI_MAX_BOXES; NULL boxes_host or boxes_dev with n > 0; a coordinate outside [0, W] / [0, H]; a cls
 * outside 0 .. DCVC_ROI_MAX_CLASSES - 1; grow outside 0 .. DCVC_ROI_MAX_GROW; class_mask outside
 * 1 .. 2^DCVC_ROI_MAX_CLASSES - 1; anything but exactly one of the two modes (tile in the list with fill == -1, or
 * tile == 0 with fill in 0 .. 255); and an out whose extent [out, out + 2 * plane stride + (H - 1) * row stride + W)
 * overlaps the extent of src -- the mosaic reads its neighbours, so it cannot run in place. */
int dcvc_redact(const float *src, int32_t src_rs, int64_t src_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                int32_t W, const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, int32_t class_mask,
                int32_t grow, int32_t tile, int32_t fill, uint16_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif
