/* dcvc_hip_roi.h -- the region-of-interest enhancement layer around the codec: residual picture inside boxes, fusion of
 * a decoded residual through a feathered mask, squared error inside and outside the boxes -- and the per-cell q-scale
 * map that lets the base layer itself quantise finer inside the boxes (ROI-weighted quantisation).
 *
 * Conventions of dcvc_hip_color.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  Float pictures are PLANAR fp32 with explicit strides
 * in elements:
 *   element (c, y, x) = p[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded reconstruction is read in place.  H and W are any positive sizes up to
 * DCVC_ROI_MAX_SIDE; they need not be even.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Every floating-point operation below is one correctly rounded fp32 multiply or
 * add in the order written (no contraction into fused multiply-adds); rint is round-half-to-even;
 * clamp01(v) = min(max(v, 0), 1).  A numpy float32 evaluation in this order gives the same bits.
 *
 * 8-bit code of a float picture:  code(v) = (int) rint(255.0f * clamp01(v)).  On a picture that came from 8-bit
 *   samples divided by 255 on the host it returns the sample (rint(255 T[k]) == k for all 256 quotients T[k]).
 *
 * Boxes are records {x1, y1, x2, y2, cls} of int32, half-open as numpy slices [y1:y2, x1:x2], coordinates within
 *   [0, W] and [0, H].  x2 <= x1 or y2 <= y1 is an EMPTY box, not an error.  cls indexes up to DCVC_ROI_MAX_CLASSES
 *   class records {border, shrink, feather[DCVC_ROI_MAX_BORDER]}.  At most DCVC_ROI_MAX_BOXES boxes; n == 0 is valid.
 *   Every entry point takes the list twice: `boxes_host` (HOST memory, validated before the launch: coordinates, cls)
 *   and `boxes_dev` (the DEVICE copy the kernel reads).  The kernels address nothing through a box, so a device copy
 *   that differs from the validated one changes results, never which memory is touched.
 *
 * Binary mask:  1 where any non-empty box contains the pixel.
 *
 * Feather mask:  the value at a pixel comes from the LAST box in list order that contains it (boxes are assigned one
 *   after the other; a later box's low border values overwrite an earlier box's interior).  Inside that box, with
 *   d = min(x - x1, x2 - 1 - x, y - y1, y2 - 1 - y), the value is feather[min(d, border - 1)], and 1.0 when
 *   border == 0; 0.0 outside every box.  The table is built by the HOST as
 *   feather[i] = (float) (1.0 - linspace(0.9, 0.0, border)[i]) in double precision; the device never computes it.
 *   border == 1 therefore gives 0.1 over the whole box (linspace of one point is its start).
 *
 * dcvc_roi_residual
 *   out = inside the binary mask ? clip(code(src) - code(rec) + 128, 0, 255) : 0, per channel, 8-bit.
 *   Output element (slot j, y, x) = out[j * chan_stride + y * row_stride + x * pixel_stride] holds channel order[j]
 *   of the pictures (order: a permutation of 0, 1, 2; {1, 2, 0} writes G, B, R planes).  Two layouts: planar
 *   (pixel_stride 1, row_stride >= W, chan_stride >= (H - 1) * row_stride + W) and interleaved HWC (pixel_stride 3,
 *   chan_stride 1, row_stride >= 3 W).
 *
 * dcvc_roi_fuse
 *   m the feather mask, e = (float) residual - 128.0f, b = (float) code(base):
 *     s = m * e;  v = s + b;  k = (int) min(max(v, 0.0f), 255.0f)  (truncation toward zero);  out = T[k],
 *   T[k] = (float) k / 255.0f as the HOST's IEEE division gives it (the table of dcvc_yuv420_to_rgb's quantize8).
 *   Outside every box that is T[code(base)].  The residual is read in either layout dcvc_roi_residual writes.
 *
 * dcvc_roi_sse
 *   The binary mask of the boxes SHRUNK by their class's shrink: [y1 + p : y2 - p, x1 + p : x2 - p]; a box that
 *   shrinks to nothing is empty.  ADDS three unsigned 64-bit integers to sums[0..2]: the sum over the 3 channels of
 *   (code(a) - code(b))^2 inside the mask, the same outside, and the number of PIXELS inside (a pixel in several
 *   boxes counts once).  The caller zeroes them.  Integer sums: exact and order-independent.
 *
 * Q-scale map  (ROI-weighted quantisation of the latent y; used by dcvc_scale_channels_map and by the q_map member of
 *   dcvc_dual_prior_args, include/dcvc_hip.h)
 *   Latent grid: DCVC_ROI_CELL = 16.  For a picture of H x W pixels, Hp x Wp is the size padded to multiples of 64 (as
 *   the codec pads pictures); the grid is hc = Hp / 16 rows by wc = Wp / 16 columns, and cell (i, j) covers pixel rows
 *   [16 i, 16 i + 16) and columns [16 j, 16 j + 16).
 *   Factors: an integer k of hundredths, 10 <= k <= 1000, stands for f = (float) k / 100.0f as the HOST's IEEE division
 *   gives it; the device never computes a factor.  factors[0] is the background's, factors[1 + c] class c's.
 *   Map: a non-empty box is grown by `grow` pixels, 0 <= grow <= 255, and clipped to the picture:
 *     x1' = max(x1 - grow, 0), x2' = min(x2 + grow, W), y1' = max(y1 - grow, 0), y2' = min(y2 + grow, H).
 *   The grown box TOUCHES cell (i, j) iff  x1' < 16 j + 16 && x2' > 16 j && y1' < 16 i + 16 && y2' > 16 i.
 *   map[i * wc + j] = the minimum of factors[1 + cls] over the boxes that touch the cell, factors[0] where none does:
 *   independent of list order.  Cells that lie wholly in the padding get factors[0] (a clipped box ends at W, H).
 *   Use: wherever the codec forms the step of the latent y, cq = max(q_basic[c], 0.5) * q_scale[n], the step becomes
 *   cq * map[cell] -- one more correctly rounded fp32 multiply, in that order.  It applies to the y of an I picture and
 *   to the y of a P picture; mv_y keeps its scalar.  No map means exactly the expression without the multiply, so a
 *   map of 1.0f gives the same bits as no map.
 */
#ifndef DCVC_HIP_ROI_H
#define DCVC_HIP_ROI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_ROI_MAX_SIDE 32768
#define DCVC_ROI_MAX_BOXES 1024
#define DCVC_ROI_MAX_CLASSES 4
#define DCVC_ROI_MAX_BORDER 64
#define DCVC_ROI_CELL 16
#define DCVC_ROI_MAX_GROW 255

typedef struct {
    int32_t x1, y1, x2, y2, cls;
} dcvc_roi_box_t;

typedef struct {
    int32_t border, shrink;              /* each within 0 .. DCVC_ROI_MAX_BORDER */
    float feather[DCVC_ROI_MAX_BORDER];  /* the first `border` entries are used */
} dcvc_roi_class_t;

/* Refused by all three: a NULL picture or output; H or W not in 1 .. DCVC_ROI_MAX_SIDE; a stride smaller than the row or
 * a plane stride too small for the rows; n outside 0 .. DCVC_ROI_MAX_BOXES; NULL boxes_host or boxes_dev with n > 0; a
 * coordinate outside [0, W] / [0, H]; a cls outside 0 .. n_classes - 1 (dcvc_roi_residual, which uses no class:
 * outside 0 .. DCVC_ROI_MAX_CLASSES - 1); a pixel stride other than 1 or 3, chan_stride != 1 with pixel stride 3;
 * {order0, order1, order2} not a permutation of 0, 1, 2. */
int dcvc_roi_residual(const float *src, int32_t src_row_stride, int64_t src_plane_stride, const float *rec,
                      int32_t rec_row_stride, int64_t rec_plane_stride, int32_t H, int32_t W,
                      const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, uint8_t *out,
                      int64_t out_chan_stride, int64_t out_row_stride, int32_t out_pixel_stride, int32_t order0,
                      int32_t order1, int32_t order2, void *stream);

/* classes: HOST pointer to n_classes records, read before the launch.  Also refused: n_classes outside
 * 0 .. DCVC_ROI_MAX_CLASSES, NULL classes with n_classes > 0, a border or shrink outside 0 .. DCVC_ROI_MAX_BORDER. */
int dcvc_roi_fuse(const float *base, int32_t base_row_stride, int64_t base_plane_stride, const uint8_t *residual,
                  int64_t res_chan_stride, int64_t res_row_stride, int32_t res_pixel_stride, int32_t order0, int32_t order1,
                  int32_t order2, int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev,
                  int32_t n, const dcvc_roi_class_t *classes, int32_t n_classes, float *out, int32_t out_row_stride,
                  int64_t out_plane_stride, void *stream);

/* sums: three 8-byte-aligned device integers. */
int dcvc_roi_sse(const float *a, int32_t a_row_stride, int64_t a_plane_stride, const float *b, int32_t b_row_stride,
                 int64_t b_plane_stride, int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host,
                 const dcvc_roi_box_t *boxes_dev, int32_t n, const dcvc_roi_class_t *classes, int32_t n_classes,
                 uint64_t *sums, void *stream);

/* The q-scale map above: writes exactly hc * wc floats to `map` (DEVICE), hc = 4 * ceil(H / 64), wc = 4 * ceil(W / 64).
 * One launch on `stream`, nothing synchronised.  factors: HOST pointer to 1 + n_classes floats, read before the launch.
 * Refused: NULL factors or map; H or W not in 1 .. DCVC_ROI_MAX_SIDE; grow outside 0 .. DCVC_ROI_MAX_GROW; n_classes
 * outside 0 .. DCVC_ROI_MAX_CLASSES; a factor that is not finite or not in [0.1, 10]; and what dcvc_roi_residual refuses
 * about boxes (n, NULL lists with n > 0, coordinates), with cls outside 0 .. n_classes - 1. */
int dcvc_roi_qmap(int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n,
                  int32_t grow, const float *factors, int32_t n_classes, float *map, void *stream);

#ifdef __cplusplus
}
#endif
#endif
