/* dcvc_hip_grain.h -- film-grain synthesis, the other half of the temporal noise prefilter (dcvc_hip_tnr.h): the encoder
 * MEASURES what the filter took out of the cells it blended throughout (dcvc_grain_measure: eight intensity bins of second
 * moments of the luma difference and of its products with the right and the lower neighbour), and the decoder APPLIES
 * noise of that strength and shape to the picture it displays (dcvc_grain_apply: a counter-hashed white field, a separable
 * 3-tap shape, a scale by intensity).  The bitstream, the DPB and every reference picture know nothing of either.  The
 * host side -- the eight points, the two taps and the table they become -- is vcm_ts_amd/grain.py; this header is the
 * device half.
 *
 * Conventions of dcvc_hip_tnr.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code, nothing
 * launched (and nothing dereferenced) on a bad argument.  Pictures are PLANAR fp32 R, G, B with explicit strides in elements:
 *   element (c, y, x) = p[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read and written in place.  H and W are the UNPADDED size, each within
 * 1 .. DCVC_ROI_MAX_SIDE; they need not be multiples of anything.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  With code(v) = (int) rint(255.0f * clamp01(v)) (a NaN codes as 0) and the luma
 * Y = (54 r + 183 g + 19 b + 128) >> 8 of the three codes, both exactly as in dcvc_hip_tnr.h / dcvc_hip_scene.h, and the
 * cells of dcvc_hip_roi.h ("Latent grid"): hc = 4 ceil(H / 64), wc = 4 ceil(W / 64), cell (i, j) covers pixel rows
 * [16 i, 16 i + 16) and columns [16 j, 16 j + 16) INTERSECTED WITH THE PICTURE.
 *
 * ---- dcvc_grain_measure
 *   src   the source picture;   flt   what dcvc_tnr_step wrote for it;   held   the uint16 cells that step wrote
 *   acc   DCVC_GRAIN_WORDS = 32 int64 words on the device: word 4 b + k is, for the intensity bin b = 0 .. 7,
 *         k = 0 the count, 1 the sum of e^2, 2 the sum of e * e_right, 3 the sum of e * e_below.
 * A cell TAKES PART when every one of its pixels inside the picture was blended: held[i * wc + j] equals
 * min(16, H - 16 i) * min(16, W - 16 j).  Per pixel p = (y, x) of such a cell:
 *     e(p) = Y(src, p) - Y(flt, p)                                      -255 .. 255
 *     b    = Y(flt, p) >> 5                                             0 .. 7
 *     acc[4 b + 0] += 1,   acc[4 b + 1] += e(p)^2
 *     acc[4 b + 2] += e(p) * e(y, x + 1)   when x + 1 < W and (x + 1) / 16 == x / 16
 *     acc[4 b + 3] += e(p) * e(y + 1, x)   when y + 1 < H and (y + 1) / 16 == y / 16
 * A pair never leaves its cell.  acc is ADDED TO, never written: the caller zeroes it.  All sums are integers and do not
 * depend on the order of summation; a word that gains nothing is not touched.
 *
 * ---- dcvc_grain_apply
 *   in    the picture to display;   out   the grained copy (must not overlap in)
 *   t     the picture number, 0 .. 2^31 - 1;   kh, kv   the two taps, -DCVC_GRAIN_MAX_TAP .. DCVC_GRAIN_MAX_TAP
 *   stab  256 uint16 words on the device, the scale by luma code; the caller answers for their range (any uint16 is safe)
 * 1. The white field.  With uint32 arithmetic modulo 2^32 and
 *        fmix(h):  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16      (murmur3's finaliser)
 *    for every position (y, x), y in -1 .. H, x in -1 .. W:
 *        key = fmix((uint32) t ^ 0x9e3779b9)
 *        w0  = fmix((((uint32) (y + 1)) << 16 | (uint32) (x + 1)) ^ key)          (y + 1 and x + 1 are below 2^16)
 *        w1  = fmix(w0 ^ 0x9e3779b9)
 *        g(y, x) = (the sum of the four bytes of w0 and of the four bytes of w1) - 1020                 -1020 .. 1020
 *    Eight independent uniform bytes have the variance 8 (256^2 - 1) / 12 = DCVC_GRAIN_WHITE_VAR = 43690.  g depends on
 *    the position and the picture number only.
 * 2. The shape.  th = [kh, 64, kh], tv = [kv, 64, kv] (DCVC_GRAIN_CENTRE = 64):
 *        n(y, x) = sum over dy, dx in -1 .. 1 of tv[dy + 1] * th[dx + 1] * g(y + dy, x + dx)
 *    |n| <= (64 + 2 * 24)^2 * 1020 = 12 794 880 < 2^24.  The variance of n is 43690 (64^2 + 2 kh^2) (64^2 + 2 kv^2), and
 *    its lag-1 correlations are 2 * 64 kh / (64^2 + 2 kh^2) along a row and the same of kv along a column.
 * 3. Scale and add.  s = stab[Y(in, p)], 0 .. 65535; F = DCVC_GRAIN_SHIFT = 24:
 *        D = (n * s + 2^(F - 1)) >> F        in int64, arithmetic shift (floor): |n * s| < 2^24 * 2^16 = 2^40
 *    D is in 1/16 of an 8-bit code, |D| <= 49 980.  For each of the three planes
 *        out = (s == 0) ? in : fminf(fmaxf(in + (float) D * (1.0f / 4080.0f), 0.0f), 1.0f)
 *    evaluated as written in fp32, every operation rounded and none contracted: the conversion of D (exact), its product
 *    with the fp32 constant 1.0f / 4080.0f, the sum with in, the two clamps (fmaxf and fminf answer the other operand for
 *    a NaN).  s == 0 copies the bits of in.  The same D goes to all three planes: the grain is achromatic.
 * Nothing outside the H x W crop of out is touched.
 */
#ifndef DCVC_HIP_GRAIN_H
#define DCVC_HIP_GRAIN_H

#include <stdint.h>

#include "dcvc_hip_roi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_GRAIN_BINS 8          /* intensity bins of 32 luma codes */
#define DCVC_GRAIN_WORDS 32        /* int64 words of acc: 4 per bin */
#define DCVC_GRAIN_MAX_TAP 24      /* |kh|, |kv| */
#define DCVC_GRAIN_CENTRE 64       /* the middle tap */
#define DCVC_GRAIN_SHIFT 24        /* F */
#define DCVC_GRAIN_WHITE_VAR 43690 /* the variance of g */

/* The sums of one P picture: one launch on `stream`, nothing synchronised.  Each workgroup reduces its strip in registers
 * and LDS and then issues ONE 64-bit vector atomic add per word of acc it has something for; integer sums, so the result
 * does not depend on the order the workgroups arrive in.  A picture whose base is 16-byte aligned and whose strides are
 * multiples of 4 is read 16 bytes at a time, any other 4 bytes at a time (each of the two on its own): same results.
 * Refused with DCVC_E_ARG, before anything else: a NULL src, flt, held or acc; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row
 * stride < W; a plane stride < (H - 1) * row stride + W; src or flt not 4-byte aligned; held not 2-byte aligned; acc not
 * 8-byte aligned. */
int dcvc_grain_measure(const float *src, int32_t src_rs, int64_t src_ps, const float *flt, int32_t flt_rs, int64_t flt_ps, int32_t H,
                       int32_t W, const uint16_t *held, int64_t *acc, void *stream);

/* The grained copy of one picture: one launch on `stream`, nothing synchronised.  The 16-byte rule as above, for in and out
 * each on its own.
 * Refused with DCVC_E_ARG, before anything else: a NULL in, out or stab; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a row stride
 * < W; a plane stride < (H - 1) * row stride + W; in or out not 4-byte aligned; stab not 2-byte aligned; kh or kv outside
 * -DCVC_GRAIN_MAX_TAP .. DCVC_GRAIN_MAX_TAP; t < 0; and an out whose extent
 * [out, out + 2 * plane stride + (H - 1) * row stride + W) overlaps the extent of in. */
int dcvc_grain_apply(const float *in, int32_t in_rs, int64_t in_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H, int32_t W,
                     int32_t t, int32_t kh, int32_t kv, const uint16_t *stab, void *stream);

#ifdef __cplusplus
}
#endif
#endif
