/* dcvc_hip_scene.h -- scene-cut detection: sixteen regional luma histograms of a picture the codec holds on the device.
 *
 * Conventions of dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  The picture is PLANAR fp32 R, G, B with explicit
 * strides in elements:
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read in place.  H and W are any sizes within 1 .. DCVC_SCENE_MAX_SIDE; they
 * need not be even.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.
 *
 * 8-bit code of a sample:  code(v) = (int) rint(255.0f * clamp01(v)),  clamp01(v) = min(max(v, 0), 1) -- the function of
 *   dcvc_hip_roi.h: one correctly rounded fp32 multiply, rint is round-half-to-even.
 *
 * Luma of a pixel, on the three integer codes r, g, b:
 *   Y = (54 * r + 183 * g + 19 * b + 128) >> 8
 *   (BT.709 weights scaled to a sum of 256; Y lies in 0 .. 255, and Y(255, 255, 255) == 255).
 *
 * Bin:  bin = Y >> 3, one of DCVC_SCENE_BINS = 32.
 *
 * Cell of pixel (y, x):  cy = (4 * y) / H,  cx = (4 * x) / W  with integer division: a DCVC_SCENE_GRID x DCVC_SCENE_GRID
 *   = 4 x 4 grid.  Cell cy holds the rows ceil(cy * H / 4) .. ceil((cy + 1) * H / 4) - 1; with H or W below 4 some cells
 *   hold no pixel.
 *
 * dcvc_scene_hist
 *   ADDS 1 to hist[(cy * 4 + cx) * 32 + bin] for every pixel of the picture: DCVC_SCENE_COUNTERS = 512 unsigned 32-bit
 *   counters in device memory.  The caller zeroes them.  Integer sums: exact, independent of order, and the same bits
 *   whatever runs beside the kernel.
 */
#ifndef DCVC_HIP_SCENE_H
#define DCVC_HIP_SCENE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_SCENE_MAX_SIDE 32768
#define DCVC_SCENE_GRID 4
#define DCVC_SCENE_BINS 32
#define DCVC_SCENE_COUNTERS (DCVC_SCENE_GRID * DCVC_SCENE_GRID * DCVC_SCENE_BINS)

/* Refused with DCVC_E_ARG, before anything else: a NULL rgb or hist; H or W not in 1 .. DCVC_SCENE_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; a pointer that is not 4-byte aligned. */
int dcvc_scene_hist(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint32_t *hist,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif
