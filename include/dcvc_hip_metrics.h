/* dcvc_hip_metrics.h -- quality metrics on the device: MS-SSIM (value and gradient) and the squared error PSNR needs.
 *
 * Conventions of dcvc_hip.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code, nothing
 * launched (and nothing dereferenced) on a bad argument.  Unlike the codec's activations these operands are PLANAR fp32
 * (N, C, H, W) -- the layout pictures and reconstructions have at the public interface -- with explicit strides in
 * elements, so the unpadded crop of a padded reconstruction is measured in place:
 *   element (n, c, y, x) = p[(n * C + c) * plane_stride + y * row_stride + x],   row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W.
 *
 * What is computed is pytorch_msssim.ms_ssim (1.0): the reference's MS_SSIM(data_range=1.0, size_average=False)
 * (DCVC_HEM/src/models/common_model.py:7,29; src/utils/common.py:63-112 in its test harness):
 *   window   11 taps, g[k] = exp(-(k-5)^2 / (2 * 1.5^2)) / sum, separable, depth-wise, NO padding: maps are (H-10, W-10)
 *   level    mu1 = G*X, mu2 = G*Y, s1 = G*(XX) - mu1^2, s2 = G*(YY) - mu2^2, s12 = G*(XY) - mu1 mu2,
 *            cs_map = (2 s12 + C2) / (s1 + s2 + C2),  ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map,
 *            C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range; cs / ssim = mean of the map per (n, c)
 *   pyramid  five levels; after levels 0..3 keep relu(cs) and replace X, Y by avg_pool2d(2, 2, padding=(H%2, W%2)) (zero
 *            padding, divisor always 4); at level 4 keep relu(ssim)
 *   result   ms[n, c] = prod_i kept_i ^ w_i, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); out_ms[n] = mean over c
 * min(H, W) <= 160 is refused like the package's assert.
 * Evaluated in fp32 with the window sums in a fixed tap order; the kernels take 2 s12 - s1 - s2 as minus the windowed
 * variance of x - y (the same number, without the cancellation), so cs_map = 1 - var(x - y) / (s1 + s2 + C2).
 *
 * Deterministic: every map is reduced per workgroup in a fixed order, the per-workgroup sums are added in a fixed order
 * by a finishing launch; no floating-point atomics anywhere.
 */
#ifndef DCVC_HIP_METRICS_H
#define DCVC_HIP_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MS_SSIM_LEVELS 5
#define DCVC_MS_SSIM_MIN_SIDE 161 /* smallest accepted min(H, W) */

/* Bytes of device workspace one call needs (pyramid, per-workgroup sums; with want_grad also the three gradient maps and
 * the per-level gradient planes).  0 for a shape the calls below would refuse. */
int64_t dcvc_ms_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t want_grad);

/* out_ms[N]; optional out_levels[5 * N * C] (level-major: the kept, i.e. relu-ed, cs of levels 0..3 and ssim of level
 * 4 per (n, c)); optional out_sse[N] = sum over (c, y, x) of (x - y)^2 taken from the same loads (PSNR without a second
 * pass).  clamp01_x != 0 clamps the FIRST operand to [0, 1] as it is loaded (a reconstruction against its source).
 * workspace: dcvc_ms_ssim_workspace_bytes(N, C, H, W, 0) bytes, 16-byte aligned, owned by the call until it completes. */
int dcvc_ms_ssim(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t x_row_stride,
                 int64_t x_plane_stride, int32_t y_row_stride, int64_t y_plane_stride, float data_range,
                 int32_t clamp01_x, void *workspace, float *out_ms, float *out_levels, float *out_sse, void *stream);

/* gx (dense N, C, H, W) = d/dx of sum_n g_ms[n] * out_ms[n].  The function is symmetric in its operands: the gradient
 * with respect to y is the same call with x and y swapped.  Recomputes the forward into the workspace (sized with
 * want_grad = 1) with the forward's own code, so the differences s1, s2, s12 are the same bits in both.  clamp01_x must
 * be 0.  Where a kept value was cut by the relu its gradient is 0. */
int dcvc_ms_ssim_grad(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t x_row_stride,
                      int64_t x_plane_stride, int32_t y_row_stride, int64_t y_plane_stride, float data_range,
                      int32_t clamp01_x, void *workspace, const float *g_ms, float *gx, void *stream);

#ifdef __cplusplus
}
#endif
#endif
