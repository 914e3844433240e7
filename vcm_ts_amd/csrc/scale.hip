// scale.hip -- the separable Lanczos-3 resampler of the reduced-resolution base layer (include/dcvc_hip_scale.h, which
// states the arithmetic and its order; this file only arranges it).
//
// One launch per call.  A workgroup is 4 waves and owns a tile of TILE_H = 16 output rows x TILE_W = 64 output columns of
// one plane.  It needs at most ROWS = 16 * 4 + 32 input rows and, of each, at most 64 * 4 + 32 columns (ratios up to 4 to
// 1, at most 32 taps; the entry point refuses tables that need more).  A wave takes every fourth of those rows: it stages
// the row's segment in LDS (16-byte loads where the source's alignment allows, scalar loads guarded by the width
// otherwise), then lane x folds output column x of the row out of it and leaves the fp32 result in h[row][x].  Then a
// lane owns 4 consecutive columns of one output row and folds them vertically out of h with 16-byte LDS reads and one
// 16-byte store (scalar stores guarded by the width where the destination's alignment does not allow it).  The tap rows
// of the tile sit in LDS as int16: the horizontal ones transposed, so that the lanes of a wave read consecutive halves.
// The two __syncthreads() per round of four rows order only a wave's writes and reads of its OWN seg[wave] (and of h, which
// is not read before the loop ends): a wave-level barrier would do.  They are block barriers because nrows is
// block-uniform, which keeps them legal, and (nrows / 4) * 2 of them per tile are nothing beside the tile's traffic.
// Every start read from the device tables is clamped to [0, n_in - T] and every LDS offset to the staged region: whatever
// the device tables hold, only samples of the source and of the destination are touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_roi.h"
#include "dcvc_hip_scale.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_W = DCVC_SCALE_TILE_W, TILE_H = DCVC_SCALE_TILE_H, MAXT = DCVC_SCALE_MAX_TAPS;
constexpr int ROWS = DCVC_SCALE_TILE_ROWS;  // 96 input rows at most
constexpr int SEG = DCVC_SCALE_TILE_COLS;   // 296 staged columns at most: the span, 3 for the aligned start, rounded up
static_assert(ROWS == TILE_H * 4 + MAXT && SEG == TILE_W * 4 + MAXT + 8 && SEG % 4 == 0, "the header states these sizes");
constexpr float UNIT_INV = 1.0f / (float)DCVC_SCALE_UNIT;  // 2^-14: (float) k * UNIT_INV is exact

struct ScaleArgs {
    const float *src;
    float *dst;
    const int32_t *xs, *ys;
    const int16_t *xk, *yk;
    int64_t src_ps, dst_ps;
    int32_t src_rs, dst_rs, H_in, W_in, H_out, W_out, xT, yT, vec_src, vec_dst;
};

struct Tile {
    float h[ROWS][TILE_W];      // the horizontal results: 24 KiB
    float seg[4][SEG];          // one source row segment per wave
    int16_t xk[MAXT][TILE_W];   // horizontal taps, transposed
    int16_t yk[TILE_H][MAXT];   // vertical taps
    int xoff[TILE_W], yoff[TILE_H];  // where a column's / a row's window begins in seg / h
};

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void scale_kernel(const ScaleArgs p) {
    __shared__ __align__(16) Tile t;
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int tw = min(TILE_W, p.W_out - tx0), th = min(TILE_H, p.H_out - ty0);
    const int xT = p.xT, yT = p.yT;
    const float *src = p.src + (int64_t)blockIdx.z * p.src_ps;
    float *dst = p.dst + (int64_t)blockIdx.z * p.dst_ps;

    const int seg0 = clamped(p.xs[tx0], 0, p.W_in - xT) & ~3;
    const int row0 = clamped(p.ys[ty0], 0, p.H_in - yT);
    const int segw = (clamped(clamped(p.xs[tx0 + tw - 1], 0, p.W_in - xT) + xT - seg0, 4, SEG) + 3) & ~3;
    const int nrows = clamped(clamped(p.ys[ty0 + th - 1], 0, p.H_in - yT) + yT - row0, 1, ROWS);

    for (int i = tid; i < MAXT * TILE_W; i += 256) {
        const int tt = i / TILE_W, col = i % TILE_W;
        t.xk[tt][col] = (tt < xT && col < tw) ? p.xk[(tx0 + col) * xT + tt] : (int16_t)0;
    }
    for (int i = tid; i < TILE_H * MAXT; i += 256) {
        const int r = i / MAXT, tt = i % MAXT;
        t.yk[r][tt] = (tt < yT && r < th) ? p.yk[(ty0 + r) * yT + tt] : (int16_t)0;
    }
    if (tid < TILE_W) t.xoff[tid] = tid < tw ? clamped(clamped(p.xs[tx0 + tid], 0, p.W_in - xT) - seg0, 0, SEG - xT) : 0;
    if (tid < TILE_H) t.yoff[tid] = tid < th ? clamped(clamped(p.ys[ty0 + tid], 0, p.H_in - yT) - row0, 0, ROWS - yT) : 0;
    __syncthreads();

    // horizontal: wave w takes input rows row0 + w, row0 + w + 4, ...
    for (int it = 0; it < (nrows + 3) / 4; ++it) {
        const int j = it * 4 + wave, gy = row0 + j;
        const bool live = j < nrows;
        if (live) {
            const float *row = src + (int64_t)gy * p.src_rs;
            for (int c = lane * 4; c < segw; c += 256) {
                const int gx = seg0 + c;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gy < p.H_in) {
                    if (p.vec_src && gx + 4 <= p.W_in) {
                        v = *reinterpret_cast<const float4 *>(row + gx);
                    } else {
                        if (gx < p.W_in) v.x = row[gx];
                        if (gx + 1 < p.W_in) v.y = row[gx + 1];
                        if (gx + 2 < p.W_in) v.z = row[gx + 2];
                        if (gx + 3 < p.W_in) v.w = row[gx + 3];
                    }
                }
                *reinterpret_cast<float4 *>(&t.seg[wave][c]) = v;
            }
        }
        __syncthreads();
        if (live) {
            const int off = t.xoff[lane];
            float acc = 0.0f;
            for (int tt = 0; tt < xT; ++tt) acc = acc + (((float)t.xk[tt][lane] * UNIT_INV) * t.seg[wave][off + tt]);
            t.h[j][lane] = acc;
        }
        __syncthreads();
    }

    // vertical: 16 lanes x 4 columns per output row
    const int r = tid >> 4, xq = (tid & 15) * 4;
    if (r < th && xq < tw) {
        const int off = t.yoff[r];
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int tt = 0; tt < yT; ++tt) {
            const float wf = (float)t.yk[r][tt] * UNIT_INV;
            const float4 h = *reinterpret_cast<const float4 *>(&t.h[off + tt][xq]);
            a0 = a0 + (wf * h.x);
            a1 = a1 + (wf * h.y);
            a2 = a2 + (wf * h.z);
            a3 = a3 + (wf * h.w);
        }
        a0 = fminf(fmaxf(a0, 0.0f), 1.0f);
        a1 = fminf(fmaxf(a1, 0.0f), 1.0f);
        a2 = fminf(fmaxf(a2, 0.0f), 1.0f);
        a3 = fminf(fmaxf(a3, 0.0f), 1.0f);
        const int x = tx0 + xq;
        float *d = dst + (int64_t)(ty0 + r) * p.dst_rs + x;
        if (p.vec_dst && x + 4 <= p.W_out) {
            *reinterpret_cast<float4 *>(d) = make_float4(a0, a1, a2, a3);
        } else {
            if (x + 3 < p.W_out) d[3] = a3;
            if (x + 2 < p.W_out) d[2] = a2;
            if (x + 1 < p.W_out) d[1] = a1;
            d[0] = a0;  // (x < W_out: xq < tw.  Last, or the compiler splits the 16-byte store above to share this one)
        }
    }
}

// The host copy of one axis' table: the header's checks, and that a tile's window fits what the kernel stages (`cap`
// input samples from the start of the tile's first output, aligned down to `align`).
bool axis_ok(const int32_t *start, const int16_t *k, const int32_t *start_dev, const int16_t *k_dev, int32_t T, int32_t n_in,
             int32_t n_out, int tile, int cap, int align) {
    if (!start || !k || !start_dev || !k_dev || T < 1 || T > MAXT || T > n_in) return false;
    for (int32_t i = 0; i < n_out; ++i) {
        if (start[i] < 0 || start[i] > n_in - T || (i > 0 && start[i] < start[i - 1])) return false;
        int32_t sum = 0;
        for (int32_t tt = 0; tt < T; ++tt) sum += k[(int64_t)i * T + tt];
        if (sum != DCVC_SCALE_UNIT) return false;
    }
    for (int32_t i0 = 0; i0 < n_out; i0 += tile) {
        const int32_t last = (i0 + tile < n_out ? i0 + tile : n_out) - 1;
        if (start[last] + T - (start[i0] & ~(align - 1)) > cap) return false;
    }
    return true;
}

bool vec_planes(const float *p, int32_t rs, int64_t ps) { return aligned(p, 16) && rs % 4 == 0 && ps % 4 == 0; }

}  // namespace

extern "C" int dcvc_scale_planes(const float *src, int32_t src_row_stride, int64_t src_plane_stride, float *dst,
                                 int32_t dst_row_stride, int64_t dst_plane_stride, int32_t planes, int32_t H_in, int32_t W_in,
                                 int32_t H_out, int32_t W_out, const int32_t *x_start_host, const int16_t *x_k_host,
                                 const int32_t *x_start_dev, const int16_t *x_k_dev, int32_t x_taps,
                                 const int32_t *y_start_host, const int16_t *y_k_host, const int32_t *y_start_dev,
                                 const int16_t *y_k_dev, int32_t y_taps, void *stream) {
    if (!size_ok(H_in, W_in) || !size_ok(H_out, W_out) || planes < 1 || planes > DCVC_SCALE_MAX_PLANES ||
        !planes_ok(src, src_row_stride, src_plane_stride, H_in, W_in) ||
        !planes_ok(dst, dst_row_stride, dst_plane_stride, H_out, W_out) ||
        !axis_ok(x_start_host, x_k_host, x_start_dev, x_k_dev, x_taps, W_in, W_out, TILE_W, SEG, 4) ||
        !axis_ok(y_start_host, y_k_host, y_start_dev, y_k_dev, y_taps, H_in, H_out, TILE_H, ROWS, 1))
        return DCVC_E_ARG;
    ScaleArgs a{};
    a.src = src, a.src_rs = src_row_stride, a.src_ps = src_plane_stride, a.vec_src = vec_planes(src, src_row_stride, src_plane_stride);
    a.dst = dst, a.dst_rs = dst_row_stride, a.dst_ps = dst_plane_stride, a.vec_dst = vec_planes(dst, dst_row_stride, dst_plane_stride);
    a.xs = x_start_dev, a.xk = x_k_dev, a.xT = x_taps, a.ys = y_start_dev, a.yk = y_k_dev, a.yT = y_taps;
    a.H_in = H_in, a.W_in = W_in, a.H_out = H_out, a.W_out = W_out;
    const dim3 block(64, 4), grid((W_out + TILE_W - 1) / TILE_W, (H_out + TILE_H - 1) / TILE_H, planes);
    scale_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
