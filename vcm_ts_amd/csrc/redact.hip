// redact.hip -- ROI redaction of the picture the codec is handed (include/dcvc_hip_redact.h, which states the arithmetic;
// this file only arranges it).
//
// redact_kernel is one streaming pass bound by memory: per pixel 12 bytes read and 12 written.  A WORKGROUP of 4 waves
// owns a block of 64 x 64 pixels: tile sides are powers of two up to 64 and the grid starts at (0, 0), so a block holds
// whole tiles and the 4 x 4 whole cells of the count grid, which it alone writes -- nothing global is atomic.  A THREAD
// owns 4 x 4 pixels: lane bits 0-3 are the quad column (16 quads = one 256-byte row segment), lane bits 4-5 and the wave
// the quad row.  A cell is 4 x 4 threads: lane bits 2-3 choose its column, the wave its row, so a cell's count is folded
// with four xor-shuffles inside one wave.
//
// Wave 0 first compacts the selected, non-empty boxes whose grown and clipped rectangle meets the block into LDS (16 KB
// for the full list).  A block that none meets is copied straight through: loads, stores, sixteen zero counts.  In a
// touched block a thread folds every kept box into a 16-bit mask of its own pixels (row range x column range, no loop
// over pixels), and for a mosaic forms the sums of its 2 x 2 sub-tiles and of its 4 x 4 pixels in registers.  Tiles of 8
// and more meet in LDS: the 16 x 16 thread sums of each channel are halved level by level (64, 16, 4, 1 entries) up to the
// tile's side, a barrier per level.  Pixels outside the picture are loaded as 0 and code as 0, so a clipped tile's sum is
// that of its n_t pixels.  Integer sums do not depend on order.
//
// A quad is read or written as one 16-byte access when the picture's base and strides allow it and the quad is whole;
// anything else goes element by element.  A pixel outside R is stored from the register it was loaded into: its bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_redact.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

#include "unit8_table.h"

constexpr int BLOCK = 64, WAVES = 4, SIDE = BLOCK / 4, CELLS = BLOCK / DCVC_ROI_CELL;
constexpr int PYR = SIDE * SIDE + 64 + 16 + 4 + 1;  // the sums of 4, 8, 16, 32 and 64 pixels a side
static_assert(DCVC_ROI_CELL == 16 && SIDE == 16 && WAVES * 4 == SIDE && DCVC_REDACT_MAX_TILE == BLOCK, "a thread per 4 x 4 pixels");

struct RedactArgs {
    const float *src;
    float *out;
    const dcvc_roi_box_t *boxes;
    uint16_t *count;
    int64_t sps, ops;
    int32_t srs, ors, H, W, wc, n, class_mask, grow, tile, fill, svec, ovec;
};

// the bits lo .. hi - 1 of a nibble, for the part [lo, hi) of a range that falls into [at, at + 4)
__device__ __forceinline__ unsigned nibble(int lo, int hi, int at) {
    const int a = min(max(lo - at, 0), 4), b = min(max(hi - at, 0), 4);
    return ((1u << b) - 1u) & ~((1u << a) - 1u);
}

// the mean of n pixels' codes with sum S, rounded half up
__device__ __forceinline__ unsigned mean8(unsigned S, int n) { return (2u * S + (unsigned)n) / (2u * (unsigned)n); }

__global__ __launch_bounds__(64 * WAVES) void redact_kernel(const RedactArgs p) {
    __shared__ int4 box[DCVC_ROI_MAX_BOXES];
    __shared__ unsigned pyr[3][PYR];
    __shared__ int kept;
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int qx = lane & (SIDE - 1), ty = wave * 4 + (lane >> 4);
    const int X0 = blockIdx.x * BLOCK, Y0 = blockIdx.y * BLOCK, x0 = X0 + 4 * qx, y0 = Y0 + 4 * ty;

    // ---- the loads of the thread: issued before the list is looked at
    const bool whole = x0 + 4 <= p.W, sv = p.svec && whole, ov = p.ovec && whole;
    float v[3][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool row_in = y0 + i < p.H;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *row = p.src + c * p.sps + (int64_t)(y0 + i) * p.srs + x0;
            if (row_in && sv) {
                const float4 t = *reinterpret_cast<const float4 *>(row);
                v[c][i][0] = t.x, v[c][i][1] = t.y, v[c][i][2] = t.z, v[c][i][3] = t.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[c][i][q] = (row_in && x0 + q < p.W) ? row[q] : 0.0f;
            }
        }
    }

    // ---- wave 0: the selected boxes, grown and clipped, that meet the block
    if (wave == 0) {
        const int bx1 = min(X0 + BLOCK, p.W), by1 = min(Y0 + BLOCK, p.H);
        int count = 0;
        for (int base = 0; base < p.n; base += 64) {
            const int i = base + lane;
            bool keep = false;
            int4 g = make_int4(0, 0, 0, 0);
            if (i < p.n) {
                const dcvc_roi_box_t rec = p.boxes[i];
                g = make_int4(max(rec.x1 - p.grow, 0), max(rec.y1 - p.grow, 0), min(rec.x2 + p.grow, p.W), min(rec.y2 + p.grow, p.H));
                keep = rec.x2 > rec.x1 && rec.y2 > rec.y1 && ((p.class_mask >> (rec.cls & (DCVC_ROI_MAX_CLASSES - 1))) & 1) &&
                       g.x < bx1 && g.z > X0 && g.y < by1 && g.w > Y0;
            }
            const unsigned long long bal = __ballot(keep);
            if (keep) box[count + __popcll(bal & ((1ull << lane) - 1ull))] = g;
            count += __popcll(bal);
        }
        if (lane == 0) kept = count;
    }
    __syncthreads();
    const int nb = kept;  // (uniform across the workgroup)

    // ---- R on the thread's 4 x 4 pixels: bit 4 i + q is pixel (y0 + i, x0 + q)
    unsigned mask = 0;
    for (int b = 0; b < nb; ++b) {
        const int4 g = box[b];  // (every lane reads the same word: a broadcast)
        const unsigned rn = nibble(g.y, g.w, y0);  // (row i of the mask starts at bit 4 i)
        mask |= ((rn | rn << 3 | rn << 6 | rn << 9) & 0x1111u) * nibble(g.x, g.z, x0);
    }

    unsigned mm[3][2][2] = {};
    if (nb > 0 && p.tile > 0) {  // (uniform across the workgroup, as every barrier below)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned s2[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    s2[a][b] = (unsigned)(code8(v[c][2 * a][2 * b]) + code8(v[c][2 * a][2 * b + 1]) + code8(v[c][2 * a + 1][2 * b]) +
                                          code8(v[c][2 * a + 1][2 * b + 1]));
            const unsigned s4 = s2[0][0] + s2[0][1] + s2[1][0] + s2[1][1];
            if (p.tile == 2) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int nt = max(min(2, p.H - (y0 + 2 * a)), 1) * max(min(2, p.W - (x0 + 2 * b)), 1);
                        mm[c][a][b] = mean8(s2[a][b], nt);
                    }
            } else if (p.tile == 4) {
                const int nt = max(min(4, p.H - y0), 1) * max(min(4, p.W - x0), 1);
                mm[c][0][0] = mm[c][0][1] = mm[c][1][0] = mm[c][1][1] = mean8(s4, nt);
            } else {
                pyr[c][ty * SIDE + qx] = s4;
            }
        }
        if (p.tile >= 8) {
            __syncthreads();
            int off = 0, side = SIDE;  // the level read: its first entry and its entries a side
            for (int s = 8; s <= p.tile; s *= 2) {
                const int half = side / 2, to = off + side * side;
                if (tid < 3 * half * half) {
                    const int c = tid / (half * half), r = tid % (half * half), i = r / half, j = r % half;
                    const unsigned *q = pyr[c] + off + 2 * i * side + 2 * j;
                    pyr[c][to + i * half + j] = q[0] + q[1] + q[side] + q[side + 1];
                }
                __syncthreads();
                off = to, side = half;
            }
            const int I = 4 * ty / p.tile, J = 4 * qx / p.tile;
            const int nt = max(min(p.tile, p.H - (Y0 + I * p.tile)), 1) * max(min(p.tile, p.W - (X0 + J * p.tile)), 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) mm[c][0][0] = mm[c][0][1] = mm[c][1][0] = mm[c][1][1] = mean8(pyr[c][off + I * side + J], nt);
        }
    } else if (nb > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) mm[c][0][0] = mm[c][0][1] = mm[c][1][0] = mm[c][1][1] = (unsigned)p.fill;
    }

    // ---- the stores: T[m] inside R, the loaded bits outside
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (mask) {  // (mm is within 0 .. 255 wherever mask is set: nb > 0)
            const float t00 = kUnit8.v[mm[c][0][0] & 255u], t01 = kUnit8.v[mm[c][0][1] & 255u], t10 = kUnit8.v[mm[c][1][0] & 255u],
                        t11 = kUnit8.v[mm[c][1][1] & 255u];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((mask >> (4 * i + q)) & 1u) v[c][i][q] = i < 2 ? (q < 2 ? t00 : t01) : (q < 2 ? t10 : t11);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (y0 + i >= p.H) break;
            float *row = p.out + c * p.ops + (int64_t)(y0 + i) * p.ors + x0;
            if (ov) {
                *reinterpret_cast<float4 *>(row) = make_float4(v[c][i][0], v[c][i][1], v[c][i][2], v[c][i][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) row[q] = v[c][i][q];
            }
        }
    }

    // ---- the counts: a cell is the 16 threads that differ in lane bits 0, 1, 4 and 5
    int cnt = __popc(mask);
    cnt += __shfl_xor(cnt, 1), cnt += __shfl_xor(cnt, 2), cnt += __shfl_xor(cnt, 16), cnt += __shfl_xor(cnt, 32);
    if ((lane & 0x33) == 0) p.count[(int64_t)(blockIdx.y * CELLS + wave) * p.wc + blockIdx.x * CELLS + (lane >> 2)] = (uint16_t)cnt;
}

inline bool mode_ok(int32_t tile, int32_t fill) {
    if (tile == 0) return fill >= 0 && fill <= 255;
    return fill == -1 && tile >= 2 && tile <= DCVC_REDACT_MAX_TILE && (tile & (tile - 1)) == 0;
}

}  // namespace

extern "C" int dcvc_redact(const float *src, int32_t src_rs, int64_t src_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                           int32_t W, const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, int32_t class_mask,
                           int32_t grow, int32_t tile, int32_t fill, uint16_t *count, void *stream) {
    if (!count || !size_ok(H, W) || !planes_ok(src, src_rs, src_ps, H, W) || !planes_ok(out, out_rs, out_ps, H, W) || !aligned(src, 4) ||
        !aligned(out, 4) || !aligned(count, 2) || !boxes_ok(boxes_host, boxes_dev, n, H, W, DCVC_ROI_MAX_CLASSES) || grow < 0 ||
        grow > DCVC_ROI_MAX_GROW || class_mask < 1 || class_mask >= (1 << DCVC_ROI_MAX_CLASSES) || !mode_ok(tile, fill) ||
        extents_overlap(out, out_rs, out_ps, src, src_rs, src_ps, H, W))
        return DCVC_E_ARG;
    RedactArgs a{};
    a.src = src, a.out = out, a.boxes = boxes_dev, a.count = count;
    a.sps = src_ps, a.ops = out_ps, a.srs = src_rs, a.ors = out_rs, a.H = H, a.W = W, a.wc = 4 * ((W + 63) / 64);
    a.n = n, a.class_mask = class_mask, a.grow = grow, a.tile = tile, a.fill = fill;
    a.svec = vec_ok(src, src_rs, src_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    const dim3 block(64, WAVES), grid((W + BLOCK - 1) / BLOCK, (H + BLOCK - 1) / BLOCK);
    redact_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
