// roi_common.h -- what the picture tools (roi.hip, roil.hip, aq.hip, motion.hip, tnr.hip, redact.hip, hash.hip, scene.hip)
// share: the 8-bit code of a float sample and the luma of three codes, the cull of a picture's box list against a rectangle
// into LDS, and the entry points' checks of pictures (size, strides, overlap, vector loads) and box lists
// (include/dcvc_hip_roi.h).
// Internal, like kernel_common.h: every unit is compiled on its own, hence the unnamed namespace.
#ifndef DCVC_ROI_COMMON_H
#define DCVC_ROI_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip_roi.h"

namespace {

__device__ __forceinline__ int code8(float v) { return (int)rintf(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); }

// the luma of dcvc_hip_scene.h on three 8-bit codes
__device__ __forceinline__ int luma8(int r, int g, int b) { return (54 * r + 183 * g + 19 * b + 128) >> 8; }

// ONE wave culls the list against the rectangle [rx0, rx1) x [ry0, ry1) into box[] / cls[] KEEPING LIST ORDER (ballot +
// prefix popcount per round of 64 boxes) and returns how many it kept.  shrink(c): what class c's boxes lose on every
// side first; a box that is empty then is dropped.
template <class Shrink>
__device__ __forceinline__ int roi_cull(const dcvc_roi_box_t *boxes, int n, int lane, int rx0, int ry0, int rx1, int ry1,
                                        int4 *box, uint8_t *cls, Shrink shrink) {
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool keep = false;
        int4 bx = make_int4(0, 0, 0, 0);
        int c = 0;
        if (i < n) {
            const dcvc_roi_box_t rec = boxes[i];
            c = rec.cls & (DCVC_ROI_MAX_CLASSES - 1);
            const int s = shrink(c);
            bx = make_int4(rec.x1 + s, rec.y1 + s, rec.x2 - s, rec.y2 - s);
            keep = bx.z > bx.x && bx.w > bx.y && bx.x < rx1 && bx.z > rx0 && bx.y < ry1 && bx.w > ry0;
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int at = count + __popcll(bal & ((1ull << lane) - 1ull));
            box[at] = bx;
            cls[at] = (uint8_t)c;
        }
        count += __popcll(bal);
    }
    return count;
}

inline bool aligned(const void *p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

inline bool size_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && H <= DCVC_ROI_MAX_SIDE && W <= DCVC_ROI_MAX_SIDE; }

inline bool planes_ok(const float *p, int32_t rs, int64_t ps, int32_t H, int32_t W) {
    return p && rs >= W && ps >= (int64_t)(H - 1) * rs + W;
}

// [p, p + 2 ps + (H - 1) rs + W) in bytes: what a picture's three planes span
inline bool extents_overlap(const float *a, int32_t ars, int64_t aps, const float *b, int32_t brs, int64_t bps, int32_t H, int32_t W) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    // (unsigned: a plane stride near 2^63 wraps instead of overflowing, and such a picture overlaps nothing real)
    const uintptr_t a1 = a0 + 4 * (2 * (uintptr_t)aps + (uintptr_t)(H - 1) * (uintptr_t)ars + (uintptr_t)W);
    const uintptr_t b1 = b0 + 4 * (2 * (uintptr_t)bps + (uintptr_t)(H - 1) * (uintptr_t)brs + (uintptr_t)W);
    return a0 < b1 && b0 < a1;
}

inline int vec_ok(const float *p, int32_t rs, int64_t ps) { return aligned(p, 16) && rs % 4 == 0 && ps % 4 == 0; }

inline bool boxes_ok(const dcvc_roi_box_t *host, const dcvc_roi_box_t *dev, int32_t n, int32_t H, int32_t W, int32_t n_classes) {
    if (n < 0 || n > DCVC_ROI_MAX_BOXES || (n > 0 && (!host || !dev))) return false;
    for (int32_t i = 0; i < n; ++i) {
        const dcvc_roi_box_t &b = host[i];
        if (b.x1 < 0 || b.x1 > W || b.x2 < 0 || b.x2 > W || b.y1 < 0 || b.y1 > H || b.y2 < 0 || b.y2 > H || b.cls < 0 ||
            b.cls >= n_classes)
            return false;
    }
    return true;
}

// an 8-bit picture in one of the two layouts, and a channel order: a permutation of 0, 1, 2
inline bool u8_layout_ok(const uint8_t *p, int64_t cs, int64_t rs, int32_t px, int32_t H, int32_t W) {
    if (!p || (px != 1 && px != 3)) return false;
    return px == 1 ? (rs >= W && cs >= (int64_t)(H - 1) * rs + W) : (cs == 1 && rs >= 3 * (int64_t)W);
}

inline bool order_ok(int32_t o0, int32_t o1, int32_t o2) {
    return !(o0 < 0 || o0 > 2 || o1 < 0 || o1 > 2 || o2 < 0 || o2 > 2 || o0 == o1 || o0 == o2 || o1 == o2);
}

}  // namespace

#endif
