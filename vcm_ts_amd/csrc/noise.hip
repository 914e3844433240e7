// noise.hip -- per 16 x 16 cell the absolute luma difference of two consecutive pictures, and the histogram of those cell
// words (include/dcvc_hip_noise.h, which states the arithmetic; this file only arranges it).
//
// noise_cells_kernel is one streaming pass bound by memory: per pixel 12 bytes of picture and 1 byte of the previous
// picture's luma read, 1 byte of this picture's luma written.  It is tiled the way motion_step_kernel is.  A WORKGROUP of 4
// waves owns a strip of 16 rows x 256 columns: the 16 adjacent cells of one cell row, so it alone writes their words and
// nothing global is atomic.  A WAVE takes 4 consecutive rows of the strip, a lane 4 consecutive pixels of each: every
// picture load of a wave reads one row of 1024 contiguous bytes, every luma load 256, and all sixteen loads of a lane (4
// rows x (3 planes + the previous luma)) are issued before the first code is formed.  Lane bits: 0-1 the quad inside the
// cell, 2-5 the cell.  A lane sums its 16 pixels into ONE register, l in the upper half and m in the lower (a cell's sums
// are at most 65280 each, so neither half ever carries), the four lanes of a cell fold with two xor-shuffles, the four
// waves meet in 256 bytes of LDS and sixteen threads store one word each.  Integer sums do not depend on order.
//
// A quad of the picture is read as one 16-byte access when the base and strides allow it; a quad of luma is one 4-byte
// access (y_stride is a multiple of 4 and both planes are 4-byte aligned, so it always is aligned) wherever its four pixels
// lie inside the picture; the quad the right edge cuts is READ whole from yprev all the same (it lies inside the row's
// stride) but WRITTEN byte by byte, so that nothing from column W on is touched.  A row past the picture's last one reads
// the last one again and neither sums nor writes.
//
// noise_hist_kernel.  On a fixed camera most of a picture's cells land in two or three bins: one global atomic per cell
// would serialise on those addresses.  A workgroup counts its share of the words into a histogram of its own in LDS (16 x
// 512 counters, 32 KB) and then adds only its nonzero bins to global memory, one vector atomic per bin.  Inside a wave the
// same contention would serialise the LDS adds, so each add is first AGGREGATED: the lanes that hold the same bin as the
// first active lane are counted with a ballot and that lane adds the count once; the lanes that differ add for
// themselves.  With every cell in one bin a wave does one LDS add per 64 words; with the cells spread out it does what a
// plain LDS atomic per lane does, plus the ballot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_noise.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, ROWS = 4;
static_assert(CELL == 16 && TILE_W == 64 * 4 && ROWS * 4 == CELL, "a lane per quad, a wave per four rows");

struct CellsArgs {
    const float *rgb;
    const uint8_t *yprev;
    uint8_t *ycur;
    uint32_t *cells;
    int64_t ps;
    int32_t rs, H, W, ys, wc, full_h, full_w, pvec;
};

__global__ __launch_bounds__(256) void noise_cells_kernel(const CellsArgs p) {
    __shared__ unsigned part[4][TILE_CELLS];  // (l << 16 | m) of each cell in each wave's four rows
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x0 = blockIdx.x * TILE_W + lane * 4, y0 = blockIdx.y * CELL + wave * ROWS;
    unsigned sum = 0;
    if (x0 < p.W && y0 < p.H) {  // (y0 is uniform across a wave)
        const bool whole = x0 + 4 <= p.W, pv = p.pvec && whole;
        float f[ROWS][3][4];
        unsigned P[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int y = min(y0 + r, p.H - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *row = p.rgb + c * p.ps + (int64_t)y * p.rs + x0;
                if (pv) {
                    const float4 t = *reinterpret_cast<const float4 *>(row);
                    f[r][c][0] = t.x, f[r][c][1] = t.y, f[r][c][2] = t.z, f[r][c][3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) f[r][c][q] = x0 + q < p.W ? row[q] : 0.0f;
                }
            }
            // (x0 + 4 <= the next multiple of 4 from W <= y_stride: the quad lies inside the row)
            P[r] = p.yprev ? *reinterpret_cast<const unsigned *>(p.yprev + (int64_t)y * p.ys + x0) : 0u;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (y0 + r >= p.H) break;  // (uniform across a wave)
            unsigned out = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int Y = luma8(code8(f[r][0][q]), code8(f[r][1][q]), code8(f[r][2][q]));
                const int prev = (int)((P[r] >> (8 * q)) & 0xffu);
                out |= (unsigned)Y << (8 * q);
                sum += ((unsigned)Y << 16) | (unsigned)abs(Y - prev);  // (only a full cell's sum is used: x0 + q < W there)
            }
            uint8_t *yrow = p.ycur + (int64_t)(y0 + r) * p.ys + x0;
            if (whole) {
                *reinterpret_cast<unsigned *>(yrow) = out;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) yrow[q] = (uint8_t)(out >> (8 * q));
            }
        }
    }
    sum += (unsigned)__shfl_xor((int)sum, 1);
    sum += (unsigned)__shfl_xor((int)sum, 2);
    if ((lane & 3) == 0) part[wave][lane >> 2] = sum;
    __syncthreads();
    const int col = blockIdx.x * TILE_CELLS + lane;
    if (wave == 0 && lane < TILE_CELLS && col < p.wc) {
        const unsigned s = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        const bool full = p.yprev && (int)blockIdx.y < p.full_h && col < p.full_w;
        p.cells[(int64_t)blockIdx.y * p.wc + col] = full ? (((s >> 28) << 16) | (s & 0xffffu)) : DCVC_NOISE_NONE;
    }
}

constexpr int HIST_THREADS = 256, HIST_PER_THREAD = 16, HIST_MAX_GROUPS = 256;
static_assert(DCVC_NOISE_COUNTERS % HIST_THREADS == 0, "a thread zeroes and flushes a whole number of counters");

__global__ __launch_bounds__(HIST_THREADS) void noise_hist_kernel(const uint32_t *cells, int64_t n, unsigned *hist) {
    __shared__ unsigned h[DCVC_NOISE_COUNTERS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < DCVC_NOISE_COUNTERS / HIST_THREADS; ++i) h[i * HIST_THREADS + tid] = 0u;
    __syncthreads();

    const int lane = tid & 63;
    const int64_t stride = (int64_t)gridDim.x * HIST_THREADS;
    // (the loop's bound is uniform across a wave: every lane takes part in every ballot, with bin = -1 for no word)
    for (int64_t base = (int64_t)blockIdx.x * HIST_THREADS + (tid - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        const unsigned w = i < n ? cells[i] : DCVC_NOISE_NONE;
        const bool counted = w != DCVC_NOISE_NONE && (w >> 16) < DCVC_NOISE_ROWS;
        const int bin = counted ? (int)(w >> 16) * DCVC_NOISE_COLS + min((int)((w & 0xffffu) >> 4), DCVC_NOISE_COLS - 1) : -1;
        const unsigned long long any = __ballot(counted);
        if (!any) continue;
        // the lanes that hold the first counted lane's bin are counted once, by that lane
        const int first = __ffsll((long long)any) - 1;
        const int lead = __shfl(bin, first);
        const unsigned long long same = __ballot(bin == lead);
        if (counted && bin != lead)
            atomicAdd(&h[bin], 1u);
        else if (lane == first)
            atomicAdd(&h[lead], (unsigned)__popcll(same));
    }
    __syncthreads();

#pragma unroll 4
    for (int i = 0; i < DCVC_NOISE_COUNTERS / HIST_THREADS; ++i) {
        const unsigned v = h[i * HIST_THREADS + tid];
        if (v) atomicAdd(hist + i * HIST_THREADS + tid, v);
    }
}

}  // namespace

extern "C" int dcvc_noise_cells(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, const uint8_t *yprev,
                                uint8_t *ycur, int32_t y_stride, uint32_t *cells, void *stream) {
    if (!ycur || !cells || !size_ok(H, W) || !planes_ok(rgb, row_stride, plane_stride, H, W) || y_stride < W || y_stride % 4 != 0 ||
        !aligned(rgb, 4) || !aligned(ycur, 4) || !aligned(yprev, 4) || !aligned(cells, 4) || ycur == yprev)
        return DCVC_E_ARG;
    CellsArgs a{};
    a.rgb = rgb, a.yprev = yprev, a.ycur = ycur, a.cells = cells, a.ps = plane_stride, a.rs = row_stride, a.H = H, a.W = W;
    a.ys = y_stride, a.wc = 4 * ((W + 63) / 64), a.full_h = H / CELL, a.full_w = W / CELL;
    a.pvec = vec_ok(rgb, row_stride, plane_stride);
    const dim3 block(64, 4), grid(nblk(a.wc, TILE_CELLS), 4 * ((H + 63) / 64));
    noise_cells_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_noise_hist(const uint32_t *cells, int64_t n, uint32_t *hist, void *stream) {
    if (!cells || !hist || n < 0 || n > DCVC_NOISE_MAX_WORDS || !aligned(cells, 4) || !aligned(hist, 4)) return DCVC_E_ARG;
    if (n == 0) return DCVC_OK;
    const unsigned groups = std::min<unsigned>(nblk(n, HIST_THREADS * HIST_PER_THREAD), HIST_MAX_GROUPS);
    noise_hist_kernel<<<dim3(groups), dim3(HIST_THREADS), 0, (hipStream_t)stream>>>(cells, n, reinterpret_cast<unsigned *>(hist));
    RET_LAUNCH();
}
