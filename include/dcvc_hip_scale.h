/* dcvc_hip_scale.h -- the resampler of the reduced-resolution base layer: a separable Lanczos-3 on planar fp32 pictures,
 * the same kernel down and up (only the tables differ).  Encoder and decoder must rebuild the same full-size picture bit
 * for bit -- the ROI residual layer is taken against it -- so the scaler is the project's own and its arithmetic is
 * stated here.
 *
 * Conventions of dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument, nothing synchronised.  Pictures are PLANAR fp32 with
 * explicit strides in elements on both sides:
 *   element (p, y, x) = ptr[p * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the crop of a padded reconstruction is read in place and the scaled picture is written straight into the interior
 * of a larger (padded, zeroed) one.  `planes` is the number of planes (3 per picture), 1 .. DCVC_SCALE_MAX_PLANES.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Every table is built on the HOST; the device evaluates no transcendental.
 *
 * Tap table of one axis, n_in -> n_out samples, built in float64 (vcm_ts_amd/scale.py taps(), tests/scale_ref.py):
 *   r = n_in / n_out,  f = max(1, r),  S = 3 f,  c_i = (i + 0.5) r
 *   lo_i = max(0, int(c_i - S + 0.5)),  hi_i = min(n_in, int(c_i + S + 0.5))           (int: truncation toward zero)
 *   w_j = L((j + 0.5 - c_i) / f)  for lo_i <= j < hi_i,   L(x) = sinc(x) sinc(x / 3) inside |x| < 3 and 0 outside,
 *         sinc(x) = sin(pi x) / (pi x), sinc(0) = 1;  the weights are divided by their sum
 *   k_j = rint(16384 w_j) as int16 (round-half-to-even); 16384 - sum k is added to the FIRST largest k_j, so every row
 *         sums to exactly DCVC_SCALE_UNIT = 16384
 *   T = max_i (hi_i - lo_i);  start_i = min(lo_i, n_in - T);  row i of the table holds its k at offset lo_i - start_i and
 *         zeros elsewhere.
 *   A table is start (int32[n_out]) and k (int16[n_out][T], row-major).  T is 12 for 1/2, 24 for 1/4, 9 for 2/3, 6 for x2.
 *   Refused by the host rule: n_in == n_out, r outside [1/4, 4], T > DCVC_SCALE_MAX_TAPS, n_in < T, sides beyond
 *   DCVC_ROI_MAX_SIDE.
 *
 * Fold, per output sample: horizontal first (W_in -> W_out on every input row), then vertical (H_in -> H_out) on the
 *   horizontal results.  In each pass
 *     acc = +0.0f;  for t = 0 .. T - 1:  acc = acc + (wf[i][t] * in[start_i + t])
 *   over ALL T entries of the row, zeros included, with wf = (float) k * 2^-14 (exact).  The product and the sum are each
 *   one correctly rounded fp32 operation (no contraction into fused multiply-adds).  The horizontal result is an fp32
 *   value, unclamped, whether it lives in LDS or in memory.  The result written is fminf(fmaxf(v, 0.0f), 1.0f) of the
 *   vertical sum: within [0, 1], and 0 for a NaN.  A numpy float32 evaluation in this order gives the same bits.
 *
 * Each table is passed twice: the HOST copy is validated before the launch (0 <= start_i, start_i + T <= n_in,
 *   1 <= T <= DCVC_SCALE_MAX_TAPS, every row sums to DCVC_SCALE_UNIT, start_i >= start_(i-1), and the window of every
 *   tile fits what a workgroup stages -- see DCVC_SCALE_TILE_* below); the DEVICE copy is what the kernel reads.  The
 *   kernel clamps every start it reads into [0, n_in - T]: whatever the device copy holds, only samples of the
 *   H_in x W_in source and of the H_out x W_out destination are touched -- a differing copy changes results, never which
 *   memory is addressed.
 */
#ifndef DCVC_HIP_SCALE_H
#define DCVC_HIP_SCALE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_SCALE_MAX_TAPS 32
#define DCVC_SCALE_UNIT 16384
#define DCVC_SCALE_MAX_PLANES 65535
/* A workgroup owns DCVC_SCALE_TILE_W output columns x DCVC_SCALE_TILE_H output rows and stages at most
 * DCVC_SCALE_TILE_COLS input columns (counted from the start of the tile's first column rounded DOWN to a multiple of 4)
 * and DCVC_SCALE_TILE_ROWS input rows: what ratios up to 4 to 1 with at most 32 taps need (64 * 4 + 32 + 8, 16 * 4 + 32).
 * A host table must satisfy, for every i0 that is a multiple of the tile side and last = min(i0 + side, n_out) - 1:
 *   horizontal:  start[last] + T - (start[i0] & ~3) <= DCVC_SCALE_TILE_COLS
 *   vertical:    start[last] + T -  start[i0]       <= DCVC_SCALE_TILE_ROWS
 * Every table of the rule above with r <= 4 does. */
#define DCVC_SCALE_TILE_W 64
#define DCVC_SCALE_TILE_H 16
#define DCVC_SCALE_TILE_COLS 296
#define DCVC_SCALE_TILE_ROWS 96

/* x_*: the table of the horizontal axis (W_in -> W_out: x_start[W_out], x_k[W_out][x_taps]); y_*: of the vertical axis
 * (H_in -> H_out).  *_host in HOST memory, *_dev the device copies.  One launch on `stream`.
 * Refused with DCVC_E_ARG: a NULL pointer; a side not in 1 .. DCVC_ROI_MAX_SIDE; planes outside
 * 1 .. DCVC_SCALE_MAX_PLANES; a row stride smaller than the row or a plane stride too small for the rows (either side);
 * taps outside 1 .. DCVC_SCALE_MAX_TAPS or larger than the input side; a host start outside [0, n_in - taps]; a host row
 * that does not sum to DCVC_SCALE_UNIT; host starts that decrease (start_i < start_(i-1)); a host table whose window
 * moves faster than a tile stages (the two DCVC_SCALE_TILE_* inequalities above: more than about 4 inputs per output). */
int dcvc_scale_planes(const float *src, int32_t src_row_stride, int64_t src_plane_stride, float *dst,
                      int32_t dst_row_stride, int64_t dst_plane_stride, int32_t planes, int32_t H_in, int32_t W_in,
                      int32_t H_out, int32_t W_out, const int32_t *x_start_host, const int16_t *x_k_host,
                      const int32_t *x_start_dev, const int16_t *x_k_dev, int32_t x_taps, const int32_t *y_start_host,
                      const int16_t *y_k_host, const int32_t *y_start_dev, const int16_t *y_k_dev, int32_t y_taps,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif
