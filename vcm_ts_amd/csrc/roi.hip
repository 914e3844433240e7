// roi.hip -- the region-of-interest enhancement layer (include/dcvc_hip_roi.h, which states the arithmetic and its
// order; this file only arranges it).
//
// Three streaming kernels from one template.  A workgroup is 4 waves and owns a tile of 8 rows x 256 columns, as in
// color.hip; a lane owns 4 consecutive pixels of two rows: 16-byte fp32 accesses, 4-byte accesses for planar 8-bit data,
// three 4-byte accesses for interleaved 8-bit data.  The first wave culls the picture's box list against the tile into
// LDS KEEPING LIST ORDER (ballot + prefix popcount per round of 64 boxes: the last box that holds a pixel decides its
// feather value), then every pixel walks the culled list only.  A tile whose list is empty -- nearly all of a picture --
// takes a path without the walk.  Rows whose width or pointers do not give the vector alignment, and the last partial
// block of a row, take scalar accesses guarded by the width through the same arithmetic.  The kernels address nothing
// through a box: whatever the device copy of the list holds, only pixels of the H x W picture are touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_roi.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

#include "unit8_table.h"

enum { RESIDUAL = 0, FUSE = 1, SSE = 2 };
constexpr int TILE_W = 256, TILE_H = 8;

struct RoiArgs {
    const float *a, *b;         // residual: source, reconstruction; fuse: base (b unused); sse: the two pictures
    uint8_t *u8;                // residual: output; fuse: the residual read
    float *out;                 // fuse
    unsigned long long *sums;   // sse
    const dcvc_roi_box_t *boxes;
    int64_t a_ps, b_ps, out_ps, u8_cs, u8_rs;
    int32_t a_rs, b_rs, out_rs, u8_px, H, W, n;
    int32_t order[3];
    int32_t vec_a, vec_b, vec_out, vec_u8;
    dcvc_roi_class_t cls[DCVC_ROI_MAX_CLASSES];
};

struct Tile {
    int4 box[DCVC_ROI_MAX_BOXES];  // the culled list, in list order (sse: already shrunk)
    uint8_t cls[DCVC_ROI_MAX_BOXES];
    float feather[DCVC_ROI_MAX_CLASSES * DCVC_ROI_MAX_BORDER];
    int border[DCVC_ROI_MAX_CLASSES], shrink[DCVC_ROI_MAX_CLASSES];
    int count;
    unsigned part[4][3];
};

// the 8-bit codes of this lane's four pixels of one row and plane (0 beyond the width)
__device__ __forceinline__ void load_codes(const float *row, int x0, int W, int vec, int k[4]) {
    if (vec && x0 + 4 <= W) {
        const float4 f = *reinterpret_cast<const float4 *>(row + x0);
        k[0] = code8(f.x), k[1] = code8(f.y), k[2] = code8(f.z), k[3] = code8(f.w);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = x0 + q < W ? code8(row[x0 + q]) : 0;
    }
}

// four pixels x three slots of 8-bit data at `at` (the element of slot 0, pixel x0), planar or interleaved
__device__ __forceinline__ void store_u8(uint8_t *at, int64_t cs, int px, int x0, int W, int vec, const int v[3][4]) {
    if (vec && x0 + 4 <= W) {
        if (px == 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                *reinterpret_cast<uint32_t *>(at + j * cs) =
                    (uint32_t)v[j][0] | ((uint32_t)v[j][1] << 8) | ((uint32_t)v[j][2] << 16) | ((uint32_t)v[j][3] << 24);
        } else {  // 12 bytes: p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
            uint32_t *w = reinterpret_cast<uint32_t *>(at);
            w[0] = (uint32_t)v[0][0] | ((uint32_t)v[1][0] << 8) | ((uint32_t)v[2][0] << 16) | ((uint32_t)v[0][1] << 24);
            w[1] = (uint32_t)v[1][1] | ((uint32_t)v[2][1] << 8) | ((uint32_t)v[0][2] << 16) | ((uint32_t)v[1][2] << 24);
            w[2] = (uint32_t)v[2][2] | ((uint32_t)v[0][3] << 8) | ((uint32_t)v[1][3] << 16) | ((uint32_t)v[2][3] << 24);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < W) {
#pragma unroll
                for (int j = 0; j < 3; ++j) at[j * cs + (int64_t)q * px] = (uint8_t)v[j][q];
            }
    }
}

__device__ __forceinline__ void load_u8(const uint8_t *at, int64_t cs, int px, int x0, int W, int vec, int v[3][4]) {
    if (vec && x0 + 4 <= W) {
        if (px == 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(at + j * cs);
                v[j][0] = w & 255u, v[j][1] = (w >> 8) & 255u, v[j][2] = (w >> 16) & 255u, v[j][3] = w >> 24;
            }
        } else {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(at);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            v[0][0] = w0 & 255u, v[1][0] = (w0 >> 8) & 255u, v[2][0] = (w0 >> 16) & 255u, v[0][1] = w0 >> 24;
            v[1][1] = w1 & 255u, v[2][1] = (w1 >> 8) & 255u, v[0][2] = (w1 >> 16) & 255u, v[1][2] = w1 >> 24;
            v[2][2] = w2 & 255u, v[0][3] = (w2 >> 8) & 255u, v[1][3] = (w2 >> 16) & 255u, v[2][3] = w2 >> 24;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 3; ++j) v[j][q] = x0 + q < W ? (int)at[j * cs + (int64_t)q * px] : 0;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void roi_kernel(const RoiArgs p) {
    __shared__ Tile t;
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int x0 = tx0 + lane * 4, y0 = ty0 + wave * 2;

    if (MODE != RESIDUAL) {  // the class records, where a lane can index them
        t.feather[tid] = p.cls[tid >> 6].feather[tid & 63];
        if (tid < DCVC_ROI_MAX_CLASSES) t.border[tid] = p.cls[tid].border, t.shrink[tid] = p.cls[tid].shrink;
        __syncthreads();
    }
    if (wave == 0) {  // cull the list against this tile, in order (roi_common.h)
        const int count = roi_cull(p.boxes, p.n, lane, tx0, ty0, tx0 + TILE_W, ty0 + TILE_H, t.box, t.cls,
                                   [&](int c) { return MODE == SSE ? t.shrink[c] : 0; });
        if (lane == 0) t.count = count;
    }
    __syncthreads();
    const int count = t.count;

    // per pixel: residual / sse: inside any box; fuse: the feather value of the last box that holds it
    bool in[2][4];
    float m[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) in[r][q] = false, m[r][q] = 0.0f;
    for (int j = 0; j < count; ++j) {  // (count == 0, nearly every tile: no walk)
        const int4 bx = t.box[j];
        if (x0 + 4 <= bx.x || x0 >= bx.z || y0 + 2 <= bx.y || y0 >= bx.w) continue;
        const int c = t.cls[j];
        const int border = MODE == FUSE ? t.border[c] : 0;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int x = x0 + q, y = y0 + r;
                if (x < bx.x || x >= bx.z || y < bx.y || y >= bx.w) continue;
                in[r][q] = true;
                if (MODE == FUSE) {
                    const int d = min(min(x - bx.x, bx.z - 1 - x), min(y - bx.y, bx.w - 1 - y));
                    m[r][q] = border == 0 ? 1.0f : t.feather[c * DCVC_ROI_MAX_BORDER + min(d, border - 1)];
                }
            }
    }

    unsigned acc[3] = {0u, 0u, 0u};  // sse: inside, outside, pixels inside (a wave's and a workgroup's sums fit 32 bits)
    if (x0 < p.W) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + r;
            if (y >= p.H) continue;
            int ka[3][4], kb[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                load_codes(p.a + c * p.a_ps + (int64_t)y * p.a_rs, x0, p.W, p.vec_a, ka[c]);
                if (MODE != FUSE) load_codes(p.b + c * p.b_ps + (int64_t)y * p.b_rs, x0, p.W, p.vec_b, kb[c]);
            }
            if (MODE == RESIDUAL) {
                int v[3][4];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = p.order[j];
                        const int sa = c == 0 ? ka[0][q] : (c == 1 ? ka[1][q] : ka[2][q]);
                        const int sb = c == 0 ? kb[0][q] : (c == 1 ? kb[1][q] : kb[2][q]);
                        v[j][q] = in[r][q] ? min(max(sa - sb + 128, 0), 255) : 0;
                    }
                store_u8(p.u8 + (int64_t)y * p.u8_rs + (int64_t)x0 * p.u8_px, p.u8_cs, p.u8_px, x0, p.W, p.vec_u8, v);
            } else if (MODE == FUSE) {
                int res[3][4];
                load_u8(p.u8 + (int64_t)y * p.u8_rs + (int64_t)x0 * p.u8_px, p.u8_cs, p.u8_px, x0, p.W, p.vec_u8, res);
                float o[3][4];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = p.order[j];  // slot j of the residual belongs to channel c
                        const int base = c == 0 ? ka[0][q] : (c == 1 ? ka[1][q] : ka[2][q]);
                        const float e = (float)res[j][q] - 128.0f;
                        const float s = m[r][q] * e;
                        const float v = s + (float)base;
                        const float f = kUnit8.v[(int)fminf(fmaxf(v, 0.0f), 255.0f)];
                        if (c == 0) o[0][q] = f;
                        else if (c == 1) o[1][q] = f;
                        else o[2][q] = f;
                    }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float *dst = p.out + c * p.out_ps + (int64_t)y * p.out_rs + x0;
                    if (p.vec_out && x0 + 4 <= p.W) {
                        *reinterpret_cast<float4 *>(dst) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (x0 + q < p.W) dst[q] = o[c][q];
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (x0 + q >= p.W) continue;
                    unsigned sq = 0u;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int d = ka[c][q] - kb[c][q];
                        sq += (unsigned)(d * d);
                    }
                    acc[0] += in[r][q] ? sq : 0u;
                    acc[1] += in[r][q] ? 0u : sq;
                    acc[2] += in[r][q] ? 1u : 0u;
                }
            }
        }
    }
    if (MODE == SSE) {  // per wave with shuffles, across waves in LDS, ONE vector atomic per workgroup (three lanes)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned total = wave_sum(acc[c]);
            if (lane == 0) t.part[wave][c] = total;
        }
        __syncthreads();
        if (tid < 3) {
            const unsigned long long total =
                (unsigned long long)t.part[0][tid] + t.part[1][tid] + t.part[2][tid] + t.part[3][tid];
            if (total) atomicAdd(p.sums + tid, total);
        }
    }
}

// The q-scale map (header: "Q-scale map").  One lane per cell of the latent grid; a workgroup first puts the whole list
// into LDS as grown, clipped boxes with their class factor (empty boxes become boxes that touch nothing), then every cell
// walks it.  At 1080p that is 8160 cells in 32 workgroups against at most 1024 boxes.  Like the kernels above it
// addresses nothing through a box.
struct QmapArgs {
    const dcvc_roi_box_t *boxes;
    float *map;
    int32_t H, W, hc, wc, n, grow;
    float f[1 + DCVC_ROI_MAX_CLASSES];
};

__global__ __launch_bounds__(256) void roi_qmap_kernel(const QmapArgs p) {
    __shared__ int4 box[DCVC_ROI_MAX_BOXES];
    __shared__ float fac[DCVC_ROI_MAX_BOXES];
    const int n = min(p.n, DCVC_ROI_MAX_BOXES);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const dcvc_roi_box_t rec = p.boxes[i];
        int4 bx = make_int4(0, 0, 0, 0);  // touches no cell
        if (rec.x2 > rec.x1 && rec.y2 > rec.y1)  // (max / min before the sum: no overflow whatever the record holds)
            bx = make_int4(max(rec.x1, p.grow) - p.grow, max(rec.y1, p.grow) - p.grow, min(rec.x2, p.W - p.grow) + p.grow,
                           min(rec.y2, p.H - p.grow) + p.grow);
        box[i] = bx;
        fac[i] = p.f[1 + (rec.cls & (DCVC_ROI_MAX_CLASSES - 1))];
    }
    __syncthreads();
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= p.hc * p.wc) return;
    const int x0 = (cell % p.wc) * DCVC_ROI_CELL, y0 = (cell / p.wc) * DCVC_ROI_CELL;
    float v = p.f[0];
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const int4 bx = box[i];
        if (bx.x < x0 + DCVC_ROI_CELL && bx.z > x0 && bx.y < y0 + DCVC_ROI_CELL && bx.w > y0) {
            v = any ? fminf(v, fac[i]) : fac[i];
            any = true;
        }
    }
    p.map[cell] = v;
}

bool vec_planes(const float *p, int32_t rs, int64_t ps) { return aligned(p, 16) && rs % 4 == 0 && ps % 4 == 0; }

bool classes_ok(const dcvc_roi_class_t *cls, int32_t n_classes) {
    if (n_classes < 0 || n_classes > DCVC_ROI_MAX_CLASSES || (n_classes > 0 && !cls)) return false;
    for (int32_t c = 0; c < n_classes; ++c)
        if (cls[c].border < 0 || cls[c].border > DCVC_ROI_MAX_BORDER || cls[c].shrink < 0 || cls[c].shrink > DCVC_ROI_MAX_BORDER)
            return false;
    return true;
}

// the 8-bit picture of residual (written) and fuse (read): layout, channel order, and whether 4-byte accesses are aligned
bool u8_ok(const uint8_t *p, int64_t cs, int64_t rs, int32_t px, int32_t o0, int32_t o1, int32_t o2, int32_t H, int32_t W,
           RoiArgs *a) {
    if (!u8_layout_ok(p, cs, rs, px, H, W) || !order_ok(o0, o1, o2)) return false;
    a->u8 = const_cast<uint8_t *>(p), a->u8_cs = cs, a->u8_rs = rs, a->u8_px = px;
    a->order[0] = o0, a->order[1] = o1, a->order[2] = o2;
    a->vec_u8 = aligned(p, 4) && rs % 4 == 0 && (px == 3 || cs % 4 == 0);
    return true;
}

template <int MODE>
int launch(const RoiArgs &a, void *stream) {
    const dim3 block(64, 4), grid((a.W + TILE_W - 1) / TILE_W, (a.H + TILE_H - 1) / TILE_H);
    roi_kernel<MODE><<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

void set_classes(RoiArgs *a, const dcvc_roi_class_t *classes, int32_t n_classes) {
    for (int32_t c = 0; c < n_classes; ++c) a->cls[c] = classes[c];
}

}  // namespace

extern "C" int dcvc_roi_residual(const float *src, int32_t src_row_stride, int64_t src_plane_stride, const float *rec,
                                 int32_t rec_row_stride, int64_t rec_plane_stride, int32_t H, int32_t W,
                                 const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, uint8_t *out,
                                 int64_t out_chan_stride, int64_t out_row_stride, int32_t out_pixel_stride, int32_t order0,
                                 int32_t order1, int32_t order2, void *stream) {
    RoiArgs a{};
    if (!size_ok(H, W) || !planes_ok(src, src_row_stride, src_plane_stride, H, W) ||
        !planes_ok(rec, rec_row_stride, rec_plane_stride, H, W) || !boxes_ok(boxes_host, boxes_dev, n, H, W, DCVC_ROI_MAX_CLASSES) ||
        !u8_ok(out, out_chan_stride, out_row_stride, out_pixel_stride, order0, order1, order2, H, W, &a))
        return DCVC_E_ARG;
    a.a = src, a.a_rs = src_row_stride, a.a_ps = src_plane_stride, a.vec_a = vec_planes(src, src_row_stride, src_plane_stride);
    a.b = rec, a.b_rs = rec_row_stride, a.b_ps = rec_plane_stride, a.vec_b = vec_planes(rec, rec_row_stride, rec_plane_stride);
    a.boxes = boxes_dev, a.n = n, a.H = H, a.W = W;
    return launch<RESIDUAL>(a, stream);
}

extern "C" int dcvc_roi_fuse(const float *base, int32_t base_row_stride, int64_t base_plane_stride, const uint8_t *residual,
                             int64_t res_chan_stride, int64_t res_row_stride, int32_t res_pixel_stride, int32_t order0,
                             int32_t order1, int32_t order2, int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host,
                             const dcvc_roi_box_t *boxes_dev, int32_t n, const dcvc_roi_class_t *classes, int32_t n_classes,
                             float *out, int32_t out_row_stride, int64_t out_plane_stride, void *stream) {
    RoiArgs a{};
    if (!size_ok(H, W) || !planes_ok(base, base_row_stride, base_plane_stride, H, W) ||
        !planes_ok(out, out_row_stride, out_plane_stride, H, W) || !classes_ok(classes, n_classes) ||
        !boxes_ok(boxes_host, boxes_dev, n, H, W, n_classes) ||
        !u8_ok(residual, res_chan_stride, res_row_stride, res_pixel_stride, order0, order1, order2, H, W, &a))
        return DCVC_E_ARG;
    a.a = base, a.a_rs = base_row_stride, a.a_ps = base_plane_stride, a.vec_a = vec_planes(base, base_row_stride, base_plane_stride);
    a.out = out, a.out_rs = out_row_stride, a.out_ps = out_plane_stride, a.vec_out = vec_planes(out, out_row_stride, out_plane_stride);
    a.boxes = boxes_dev, a.n = n, a.H = H, a.W = W;
    set_classes(&a, classes, n_classes);
    return launch<FUSE>(a, stream);
}

extern "C" int dcvc_roi_sse(const float *pa, int32_t a_row_stride, int64_t a_plane_stride, const float *pb, int32_t b_row_stride,
                            int64_t b_plane_stride, int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host,
                            const dcvc_roi_box_t *boxes_dev, int32_t n, const dcvc_roi_class_t *classes, int32_t n_classes,
                            uint64_t *sums, void *stream) {
    if (!size_ok(H, W) || !planes_ok(pa, a_row_stride, a_plane_stride, H, W) || !planes_ok(pb, b_row_stride, b_plane_stride, H, W) ||
        !classes_ok(classes, n_classes) || !boxes_ok(boxes_host, boxes_dev, n, H, W, n_classes) || !sums || !aligned(sums, 8))
        return DCVC_E_ARG;
    RoiArgs a{};
    a.a = pa, a.a_rs = a_row_stride, a.a_ps = a_plane_stride, a.vec_a = vec_planes(pa, a_row_stride, a_plane_stride);
    a.b = pb, a.b_rs = b_row_stride, a.b_ps = b_plane_stride, a.vec_b = vec_planes(pb, b_row_stride, b_plane_stride);
    a.sums = reinterpret_cast<unsigned long long *>(sums);
    a.boxes = boxes_dev, a.n = n, a.H = H, a.W = W;
    set_classes(&a, classes, n_classes);
    return launch<SSE>(a, stream);
}

extern "C" int dcvc_roi_qmap(int32_t H, int32_t W, const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n,
                             int32_t grow, const float *factors, int32_t n_classes, float *map, void *stream) {
    if (!size_ok(H, W) || !factors || !map || grow < 0 || grow > DCVC_ROI_MAX_GROW || n_classes < 0 ||
        n_classes > DCVC_ROI_MAX_CLASSES || !boxes_ok(boxes_host, boxes_dev, n, H, W, n_classes))
        return DCVC_E_ARG;
    QmapArgs a{};
    for (int32_t c = 0; c <= DCVC_ROI_MAX_CLASSES; ++c) {
        const float f = factors[c <= n_classes ? c : 0];  // (a class no validated box names: the background's)
        if (!(f >= 0.1f && f <= 10.0f)) return DCVC_E_ARG;  // (false for a NaN too)
        a.f[c] = f;
    }
    a.boxes = boxes_dev, a.map = map, a.H = H, a.W = W, a.n = n, a.grow = grow;
    a.hc = 4 * ((H + 63) / 64), a.wc = 4 * ((W + 63) / 64);
    const int cells = a.hc * a.wc;  // (at most 2048 * 2048)
    roi_qmap_kernel<<<dim3((cells + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
