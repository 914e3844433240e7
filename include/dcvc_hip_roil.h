/* dcvc_hip_roil.h -- the ROI residual layer as a bitstream of its own: a box-local, lossless or near-lossless coder for
 * the residual picture of dcvc_hip_roi.h, parallel on the encode and on the decode side.  It codes only pixels inside
 * boxes.  It is NOT HEVC and no rate or quality result is claimed for it.
 *
 * Conventions of dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative code, nothing launched
 * (and nothing dereferenced) on a bad argument; pictures, strides, boxes, the 8-bit picture's two layouts and the channel
 * order are that header's.  ARITHMETIC AND FORMAT ARE PART OF THE INTERFACE; everything after code() is integer.
 *
 * Samples.  For a pixel inside the binary mask of the boxes and a channel,
 *   r = clip(code(src) - code(rec) + 128, 0, 255)            (dcvc_roi_residual's value)
 *   e = r - 128;  q = sign(e) * ((|e| + S / 2) / S)          (integer division; S: the step, 1 .. DCVC_ROIL_MAX_STEP)
 *   u = q >= 0 ? 2 q : -2 q - 1                              (0 <= u <= 255)
 *   reconstruction  r' = clip(128 + q * S, 0, 255);  |r' - r| <= S / 2;  S = 1 is lossless.
 *
 * Cells.  The 16 x 16-pixel grid over the UNPADDED picture: hc = ceil(H / 16) rows, wc = ceil(W / 16) columns, partial
 *   cells on the right and bottom edge.  A cell is ACTIVE iff a non-empty box touches it (the touch rule of the q-scale
 *   map with grow = 0).  The active cells in raster order are a = 0 .. A - 1; cell a has n_a >= 1 mask pixels (a pixel in
 *   several boxes counts once), taken in raster order inside the cell, and three SEGMENTS: channels 0, 1, 2.
 *
 * Segment of n samples.  Bit b of a segment is bit (b & 7) of its byte (b >> 3).
 *   mode m = 0 .. 7   the n low parts u_i & (2^m - 1), m bits each, LSB first; then the unary section: per sample, in
 *                     order, (u_i >> m) zero bits and a one bit.            n (m + 1) + sum(u_i >> m) bits
 *   mode 8            the n bytes u_i.                                       8 n bits
 *   mode 9            nothing; only when every u_i is 0.                     0 bits
 *   Unused bits of the last byte are 0.  L = ceil(bits / 8) bytes, L <= n <= 256.  The encoder takes the mode with the
 *   fewest bits, the smallest mode number among equals.  A decoder accepts any mode whose L is possible for n:
 *   mode 9: L == 0;  mode 8: L == n;  mode m: ceil(n (m + 1) / 8) <= L <= n.
 *   Sample i's low part sits at bit i m, and its unary part is the gap between the (i - 1)-th and the i-th set bit of the
 *   unary section (which starts at bit n m): a decoder selects, it does not parse.
 *
 * Picture record (little-endian), one per picture:
 *   bytes 0..1 'R' 'L';  byte 2 the version, 1;  byte 3 S;  bytes 4..7 A as u32;
 *   3 A u16 in cell-then-channel order: low 12 bits L, high 4 bits the mode;
 *   the segments in the same order, back to back.   Size exactly 8 + 6 A + sum L;  a picture without boxes: 8 bytes.
 *
 * What only the payload can reveal -- fewer than n set bits in a unary section, a decoded u > 255 -- ORs
 * DCVC_ROIL_BAD_STREAM into a device status word; the affected samples are then unspecified but within 0 .. 255, nothing
 * outside the record is read and nothing outside the picture is written.
 */
#ifndef DCVC_HIP_ROIL_H
#define DCVC_HIP_ROIL_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_ROIL_VERSION 1
#define DCVC_ROIL_MAX_STEP 64
#define DCVC_ROIL_HEADER 8      /* bytes before the length table */
#define DCVC_ROIL_SLOT 768      /* staging bytes per active cell: three segments of at most 256 bytes */
#define DCVC_ROIL_CELL_MAX 774  /* record bytes per active cell at most: 6 + DCVC_ROIL_SLOT */
#define DCVC_ROIL_BAD_STREAM 1u

/* what dcvc_roil_check answers (dcvc_roil_decode answers the same before it launches anything) */
#define DCVC_ROIL_E_TRUNCATED (-16) /* fewer bytes than the header, the length table or the segments need */
#define DCVC_ROIL_E_MAGIC (-17)
#define DCVC_ROIL_E_VERSION (-18)
#define DCVC_ROIL_E_STEP (-19)      /* a step outside 1 .. DCVC_ROIL_MAX_STEP */
#define DCVC_ROIL_E_CELLS (-20)     /* A is not the boxes' number of active cells */
#define DCVC_ROIL_E_MODE (-21)      /* a mode above 9 */
#define DCVC_ROIL_E_LENGTH (-22)    /* an L that is impossible for the cell's n and the mode */
#define DCVC_ROIL_E_TRAILING (-23)  /* bytes behind the last segment */

/* HOST only.  The active cells of a box list: writes the cell indexes (row * wc + column, ascending) to cells[0 .. A) and
 * the numbers of mask pixels to counts[0 .. A), and returns A.  cells and counts may both be NULL (A alone); otherwise
 * `capacity` entries must hold A.  Refused with DCVC_E_ARG: sizes and boxes as dcvc_roi_residual refuses them, one of
 * cells / counts NULL, a capacity below A. */
int dcvc_roil_cells(int32_t H, int32_t W, const dcvc_roi_box_t *boxes, int32_t n, int32_t *cells, int32_t *counts,
                    int32_t capacity);

/* HOST only.  The validation of a picture record of `size` bytes against the counts n_a of the A active cells: 0, or
 * the first of the DCVC_ROIL_E_* codes above in the order magic, version, step, A, length table present, every entry
 * (mode, then L), total size.  DCVC_E_ARG: NULL record, negative size or A, NULL counts with A > 0. */
int dcvc_roil_check(const uint8_t *record, int64_t size, const int32_t *counts, int32_t A);

/* Codes the residual layer of one picture into `record` (DEVICE, 4-byte aligned, `capacity` >= 8 + 774 A bytes) and its
 * size in bytes into *size_word (DEVICE, 4-byte aligned).  Two launches on `stream` (one without boxes), nothing
 * synchronised: one workgroup per active cell forms u, picks the modes and assembles the three segments into its slot of
 * `staging` (DEVICE, 4-byte aligned, 768 A bytes; may be NULL when A == 0); dcvc_roil_pack's launch scans the lengths
 * and gathers the slots behind the header.  Every byte of the record is written, nothing beyond 8 + 774 A is touched.
 * table_dev: DEVICE, A pairs of int32 {cell index, unused}, the cells of dcvc_roil_cells in order; A must be what
 * dcvc_roil_cells answers for boxes_host.  Whatever the device copies hold, only pixels of the picture are read and only
 * the A slots and the record are written.
 * Refused with DCVC_E_ARG: what dcvc_roi_residual refuses about pictures and boxes; a step outside 1 .. 64; a wrong A;
 * NULL table_dev or staging with A > 0; NULL or unaligned record, staging or size_word; a capacity below 8 + 774 A. */
int dcvc_roil_encode(const float *src, int32_t src_row_stride, int64_t src_plane_stride, const float *rec,
                     int32_t rec_row_stride, int64_t rec_plane_stride, int32_t H, int32_t W,
                     const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, int32_t step,
                     const int32_t *table_dev, int32_t A, uint8_t *staging, uint8_t *record, int64_t capacity,
                     uint32_t *size_word, void *stream);

/* Decodes a record into the 8-bit residual picture dcvc_roi_fuse reads (either layout, any channel order): r' inside the
 * mask, 0 outside; every one of the 3 H W elements is written.  record_host: the record in HOST memory, validated
 * against the boxes before anything is launched (dcvc_roil_check's codes); record_dev: its DEVICE copy (2-byte aligned),
 * the one the kernel reads -- bounded by `size` and by the validated form of a segment whatever it holds.
 * table_dev: DEVICE, A pairs of int32 {cell index, byte offset of the cell's first segment in the record}.
 * status: DEVICE, 4-byte aligned; DCVC_ROIL_BAD_STREAM is ORed in, the caller zeroes it.  Two launches on `stream`.
 * Refused with DCVC_E_ARG: NULL or misaligned pointers, sizes and boxes as above, a layout or order dcvc_roi_fuse
 * refuses, NULL table_dev with A > 0. */
int dcvc_roil_decode(const uint8_t *record_host, const uint8_t *record_dev, int64_t size, int32_t H, int32_t W,
                     const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, const int32_t *table_dev,
                     uint8_t *out, int64_t out_chan_stride, int64_t out_row_stride, int32_t out_pixel_stride, int32_t order0,
                     int32_t order1, int32_t order2, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
