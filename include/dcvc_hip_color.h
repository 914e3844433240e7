/* dcvc_hip_color.h -- 4:2:0 Y'CbCr sample planes <-> the planar fp32 RGB pictures the codec takes and returns.
 *
 * Conventions of dcvc_hip_metrics.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  RGB is PLANAR fp32 with explicit strides in elements:
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],  row_stride >= width,
 *   plane_stride >= (height - 1) * row_stride + width,
 * so the unpadded crop of a padded reconstruction is read in place.  Sample planes are 8-bit (one byte per sample) or
 * 10-bit (16-bit little-endian words, as in Y4M C420p10) with row strides in SAMPLES: luma H x W, both chroma planes
 * H/2 x W/2.  H and W are even and at most 32768.
 *
 * Colour description.  Kr, Kb = 0.2126, 0.0722 (BT.709) or 0.299, 0.114 (BT.601); Kg = (1 - Kr) - Kb.
 * With s = 2^(depth - 8) and max = 2^depth - 1:
 *   limited: y_off = 16 s, y_range = 219 s, c_range = 224 s        full: y_off = 0, y_range = c_range = max
 *   c_off = 128 s (both)
 * dcvc_color_coeffs derives every constant in double precision and rounds it ONCE to fp32; the kernels use these fp32
 * values and never divide.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Every operation below is one correctly rounded fp32 add, subtract or multiply,
 * in the order written (no contraction into fused multiply-adds); rint is round-half-to-even; clamp01(v) =
 * min(max(v, 0), 1).  A numpy float32 evaluation in this order gives the same bits.
 *
 * dcvc_yuv420_to_rgb
 *   Chroma is upsampled bilinearly, edges clamped.  Chroma row j sits at luma row 2j + 1/2 in both sitings: luma row 2j
 *   takes 3 c[j] + c[j-1], row 2j+1 takes 3 c[j] + c[j+1] (quarters).  Columns, siting CENTER: the same (3, 1) pattern;
 *   siting LEFT (chroma column i at luma column 2i): column 2i takes 4 c[i], column 2i+1 takes 2 c[i] + 2 c[i+1].
 *   The weighted sum (weights in sixteenths) is formed in integers and converted once: c = (float) sum * 0.0625f (exact).
 *     Y' = ((float) y - y_off) * y_scale      Cb = (c_u - c_off) * c_scale      Cr = (c_v - c_off) * c_scale
 *     R = clamp01(Y' + crr * Cr)      G = clamp01((Y' - cgb * Cb) - cgr * Cr)      B = clamp01(Y' + cbb * Cb)
 *   quantize8 != 0: each value v becomes T[(int) rint(255.0f * v)], T[k] = (float) k / 255.0f as the HOST's IEEE division
 *   gives it (a compile-time table): exactly the 256 values an 8-bit RGB picture divided by 255 on the host holds.
 *   The launch also writes zeros to every output element to the right of column W and below row H (out_H x out_W is
 *   the padded picture the encoder takes).
 *
 * dcvc_rgb_to_yuv420
 *   r, g, b = clamp01 of the loaded values.
 *     Y' = (kr * r + kg * g) + kb * b      Cb = (b - Y') * icb      Cr = (r - Y') * icr        (per pixel)
 *     y  = clip(rint(Y' * y_range + y_off), 0, max)
 *   Chroma is filtered as the transpose of the siting.  CENTER: ((a + b) + (c + d)) * 0.25f with a, b the pixels
 *   (2j, 2i), (2j, 2i+1) and c, d the pixels (2j+1, 2i), (2j+1, 2i+1).  LEFT: v[x] = C(2j, x) + C(2j+1, x), then
 *   ((l + r) + (m + m)) * 0.125f with m = v[2i], r = v[2i+1], l = v[max(2i-1, 0)].
 *     c  = clip(rint(C * c_range + c_off), 0, max)
 *   With src_y, src_u, src_v (all three or none) and sse: the sums over each plane of (sample - source sample)^2 are
 *   ADDED to sse[0..2] (unsigned 64-bit; the caller zeroes them).  Integer sums: exact and order-independent.
 */
#ifndef DCVC_HIP_COLOR_H
#define DCVC_HIP_COLOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_MATRIX_BT709 0
#define DCVC_MATRIX_BT601 1
#define DCVC_RANGE_LIMITED 0
#define DCVC_RANGE_FULL 1
#define DCVC_SITING_LEFT 0
#define DCVC_SITING_CENTER 1
#define DCVC_COLOR_MAX_SIDE 32768

typedef struct {
    float y_off, c_off;          /* sample offsets */
    float y_scale, c_scale;      /* 1 / y_range, 1 / c_range */
    float crr, cgb, cgr, cbb;    /* 2 (1 - Kr),  2 Kb (1 - Kb) / Kg,  2 Kr (1 - Kr) / Kg,  2 (1 - Kb) */
    float kr, kg, kb;            /* luma weights */
    float icb, icr;              /* 1 / (2 (1 - Kb)),  1 / (2 (1 - Kr)) */
    float y_range, c_range;
    int32_t max_code;            /* 2^depth - 1 */
    int32_t bit_depth, siting, matrix, range;
} dcvc_color_coeffs_t;

/* HOST only, no GPU needed.  DCVC_E_ARG for a code that is none of the above, a depth other than 8 or 10, NULL out. */
int dcvc_color_coeffs(int32_t matrix, int32_t range, int32_t bit_depth, int32_t siting, dcvc_color_coeffs_t *out);

/* y, u, v: device sample planes (depth and siting from *cc, which is a HOST pointer read before the launch).
 * Refused: a NULL plane, cc or rgb; odd or non-positive H or W, a side beyond DCVC_COLOR_MAX_SIDE; out_H < H,
 * out_W < W; y_stride < W, c_stride < W / 2, out_row_stride < out_W, out_plane_stride too small for the rows; a *cc that
 * dcvc_color_coeffs did not fill (depth, siting). */
int dcvc_yuv420_to_rgb(const void *y, const void *u, const void *v, int32_t H, int32_t W, int32_t y_stride,
                       int32_t c_stride, const dcvc_color_coeffs_t *cc, float *rgb, int32_t out_H, int32_t out_W,
                       int32_t out_row_stride, int64_t out_plane_stride, int32_t quantize8, void *stream);

/* rgb: H x W pixels read through the strides.  y, u, v: device planes written.  src_* / sse: optional (all four or
 * none), source planes with the strides src_y_stride / src_c_stride. */
int dcvc_rgb_to_yuv420(const float *rgb, int32_t H, int32_t W, int32_t row_stride, int64_t plane_stride,
                       const dcvc_color_coeffs_t *cc, void *y, void *u, void *v, int32_t y_stride, int32_t c_stride,
                       const void *src_y, const void *src_u, const void *src_v, int32_t src_y_stride,
                       int32_t src_c_stride, uint64_t *sse, void *stream);

#ifdef __cplusplus
}
#endif
#endif
