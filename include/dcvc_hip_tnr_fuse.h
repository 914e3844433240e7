/* dcvc_hip_tnr_fuse.h -- the temporal noise prefilter (dcvc_hip_tnr.h) on a picture that has no filtered predecessor: an
 * I picture is blended, pixel by pixel and in ONE pass, with up to four reference pictures -- the pictures that FOLLOW it
 * in its GOP, moved onto it by dcvc_hip_me.h where a search is asked for -- each weighted on its own by the window and
 * weight rule of dcvc_tnr_step.  Encoder side only.  The host side is vcm_ts_amd/tnr.py; this header is the device half.
 *
 * Conventions of dcvc_hip_tnr.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code, nothing
 * launched (and nothing dereferenced) on a bad argument.  Every picture is PLANAR fp32 R, G, B with explicit strides in
 * elements, element (c, y, x) = p[c * plane_stride + y * row_stride + x], row_stride >= W, plane_stride >= (H - 1) *
 * row_stride + W.  H and W are the UNPADDED size, each within 1 .. DCVC_ROI_MAX_SIDE.
 *
 *   cur          the source picture
 *   ref0..ref3   the references in order of distance; the first n are used, ref_j for j >= n is ignored and may be NULL.
 *                They share ONE pair of strides (ref_rs, ref_ps): the host side answers for that
 *   out          the picture the codec will see
 *   wtab         the 256 uint16 words of dcvc_tnr_step: the weight of the current picture, 1 .. 256, by the window's mean
 *                absolute difference.  The caller answers for the range of the entries.
 *   rtab         DCVC_TNR_FUSE_RCP fp32 words on the device: entry U is the fp32 nearest the float64 quotient
 *                1 / (256 + U), built on the host.  The caller answers for the values.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  code(), the luma Y, the 5 x 5 window with replicated edges and the cells are
 * exactly those of dcvc_hip_tnr.h.  Per pixel p and per reference j = 0 .. n - 1, all in integers:
 *     d_j(p) = |Y(cur, p) - Y(ref_j, p)|                                 0 .. 255
 *     S_j(p) = the sum of d_j over the 5 x 5 window centred on p         0 .. 6375
 *     a_j    = S_j / 25  (integer floor)                                 0 .. 255
 *     w_j    = d_j(p) > P ? 256 : wtab[a_j]                              1 .. 256
 *     u_j    = 256 - w_j                                                 0 .. 255
 *     U      = the sum of the u_j                                        0 .. 1020
 *   and for each of the three planes
 *     acc = 0.0f
 *     for j = 0 .. n - 1 in this order, and only where u_j > 0:
 *         acc = acc + (ref_j - cur) * (float) u_j
 *     out = (U == 0) ? cur : cur + acc * rtab[U]
 *   evaluated as written in fp32 with every operation rounded and none contracted; the terms are added in increasing j.
 *   U == 0 copies the bits of cur.  A reference with u_j == 0 contributes nothing, so a NaN in it cannot reach out.  The
 *   multiply by a host table entry stands in for a division, so no division's rounding is part of the interface.  Where
 *   the arithmetic itself makes or passes on a NaN (a NaN or an infinity in cur, or in a reference with u_j > 0), out is a
 *   NaN; its sign and payload are the machine's and not part of the interface.  With
 *   n == 1 the weights are those of dcvc_tnr_step (cur weighs w / 256), the rounding is not.
 *
 * The cells (the grid of dcvc_hip_tnr.h): held[cell] (uint16) is the number of the cell's pixels with U > 0 -- the meaning
 *   held has in dcvc_tnr_step, so dcvc_grain_measure reads it unchanged -- and sad[cell] (uint32) the sum of d_0 over the
 *   cell's pixels.  Every cell is WRITTEN, not added to; a cell that holds no pixel is written 0.
 *
 * Nothing outside the H x W crop of out, nor outside the two hc wc arrays, is touched.
 */
#ifndef DCVC_HIP_TNR_FUSE_H
#define DCVC_HIP_TNR_FUSE_H

#include <stdint.h>

#include "dcvc_hip_tnr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_TNR_FUSE_MAX_REFS 4                               /* n: 1 .. 4 */
#define DCVC_TNR_FUSE_RCP (255 * DCVC_TNR_FUSE_MAX_REFS + 1)   /* the words of rtab: U = 0 .. 1020 */

/* One launch on `stream`, nothing synchronised.  A picture whose base is 16-byte aligned and whose strides are multiples of
 * 4 is accessed 16 bytes at a time, any other 4 bytes at a time (cur, out and each reference on its own): same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL cur, out, wtab, rtab, sad or held, or a NULL ref_j for j < n; n
 * outside 1 .. DCVC_TNR_FUSE_MAX_REFS; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row stride < W; a plane stride < (H - 1) *
 * row stride + W; P outside 0 .. DCVC_TNR_MAX_P; cur, out, a used reference, rtab or sad not 4-byte aligned; wtab or held
 * not 2-byte aligned; and an out whose extent [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent
 * of cur or of any of the n references.  The references may alias each other and cur. */
int dcvc_tnr_fuse(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref0, const float *ref1, const float *ref2,
                  const float *ref3, int32_t ref_rs, int64_t ref_ps, int32_t n, float *out, int32_t out_rs, int64_t out_ps,
                  int32_t H, int32_t W, const uint16_t *wtab, const float *rtab, int32_t P, uint32_t *sad, uint16_t *held,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif
