// scene.hip -- sixteen regional luma histograms of a picture (include/dcvc_hip_scene.h, which states the arithmetic; this
// file only arranges it).
//
// One streaming kernel in the shape of roi.hip: a workgroup is 4 waves and owns a tile of 8 rows x 256 columns, a lane
// owns 4 consecutive pixels of two rows and reads them as 16-byte accesses.  Tiles are laid out PER CELL of the 4 x 4 grid
// (blockIdx.z is the cell): every pixel of a workgroup counts into the same 32 bins, so a workgroup keeps ONE histogram.
// A lane's first column is a multiple of 4 in picture coordinates, so the 16-byte access is aligned whenever the
// picture's rows are; the quads that straddle a cell's left or right edge, and pictures whose rows or pointer do not
// give the alignment, take scalar accesses guarded by the cell's bounds through the same arithmetic.
//
// COUNTER CONTENTION.  In a flat picture every pixel of a cell lands in one bin; a 32-counter LDS histogram would
// serialise all 64 lanes of every add on it.  The workgroup's histogram is therefore REPLICATED BY LANE: counter
// (bin, lane) lives at word bin * 64 + lane, so the 64 lanes of an LDS add always address 64 different words in 64
// different banks (the LDS has 64 banks of 4 bytes), whatever bins they hold: no two lanes of an instruction ever meet,
// and the time of the add does not depend on the picture.  The four waves share the 8 KB table through LDS atomic adds
// (lane l of one wave meets lane l of another only across instructions, where the atomic is what makes it correct).
// At the end each wave folds 8 bins over the 64 replicas with shuffles and one lane per bin adds the workgroup's count
// to global memory: at most 32 integer vector atomics per workgroup, none for a bin the tile did not see.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_scene.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_W = 256, TILE_H = 8, GRID = DCVC_SCENE_GRID, BINS = DCVC_SCENE_BINS;

struct SceneArgs {
    const float *rgb;
    unsigned *hist;
    int64_t ps;
    int32_t rs, H, W, vec;
};

// first row (column) of cell c of a side of n pixels: the smallest y with (4 * y) / n == c
__host__ __device__ __forceinline__ int cell_begin(int c, int n) { return (c * n + GRID - 1) / GRID; }

__global__ __launch_bounds__(256) void scene_hist_kernel(const SceneArgs p) {
    __shared__ unsigned h[BINS * 64];  // counter (bin, lane replica) at bin * 64 + lane
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int cy = blockIdx.z / GRID, cx = blockIdx.z % GRID;
    const int y_lo = cell_begin(cy, p.H), y_hi = cell_begin(cy + 1, p.H);
    const int x_lo = cell_begin(cx, p.W), x_hi = cell_begin(cx + 1, p.W);
    // this tile inside the cell; columns counted from the multiple of 4 at or below the cell's first
    const int x0 = (x_lo & ~3) + blockIdx.x * TILE_W + lane * 4, y0 = y_lo + blockIdx.y * TILE_H + wave * 2;
    if (x_lo >= x_hi || (x_lo & ~3) + (int)blockIdx.x * TILE_W >= x_hi || y_lo + (int)blockIdx.y * TILE_H >= y_hi) return;  // (the whole workgroup)

#pragma unroll
    for (int i = 0; i < BINS * 64 / 256; ++i) h[i * 256 + tid] = 0u;
    __syncthreads();

    if (x0 < x_hi && x0 + 4 > x_lo) {
        const bool whole = p.vec && x0 >= x_lo && x0 + 4 <= x_hi;
        int k[2][3][4];  // every load of the lane's two rows is issued before the first count
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = min(y0 + r, y_hi - 1);  // (a row beyond the cell: read the last one again, count nothing)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *row = p.rgb + c * p.ps + (int64_t)y * p.rs;
                if (whole) {
                    const float4 f = *reinterpret_cast<const float4 *>(row + x0);
                    k[r][c][0] = code8(f.x), k[r][c][1] = code8(f.y), k[r][c][2] = code8(f.z), k[r][c][3] = code8(f.w);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) k[r][c][q] = (x0 + q >= x_lo && x0 + q < x_hi) ? code8(row[x0 + q]) : 0;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (y0 + r >= y_hi || x0 + q < x_lo || x0 + q >= x_hi) continue;
                const int Y = (54 * k[r][0][q] + 183 * k[r][1][q] + 19 * k[r][2][q] + 128) >> 8;
                atomicAdd(&h[(Y >> 3) * 64 + lane], 1u);
            }
    }
    __syncthreads();

    // wave w folds bins 8 w .. 8 w + 7 over the 64 replicas; ONE vector atomic per bin the tile saw
    unsigned *out = p.hist + (cy * GRID + cx) * BINS;
#pragma unroll
    for (int b = 0; b < BINS / 4; ++b) {
        const int bin = wave * (BINS / 4) + b;
        const unsigned total = wave_sum(h[bin * 64 + lane]);
        if (lane == 0 && total) atomicAdd(out + bin, total);
    }
}


}  // namespace

extern "C" int dcvc_scene_hist(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint32_t *hist,
                               void *stream) {
    if (!rgb || !hist || H < 1 || W < 1 || H > DCVC_SCENE_MAX_SIDE || W > DCVC_SCENE_MAX_SIDE || row_stride < W ||
        plane_stride < (int64_t)(H - 1) * row_stride + W || !aligned(rgb, 4) || !aligned(hist, 4))
        return DCVC_E_ARG;
    SceneArgs a{};
    a.rgb = rgb, a.hist = reinterpret_cast<unsigned *>(hist), a.rs = row_stride, a.ps = plane_stride, a.H = H, a.W = W;
    a.vec = aligned(rgb, 16) && row_stride % 4 == 0 && plane_stride % 4 == 0;
    // the largest cell decides the tiles per cell (cells differ by at most one row / column; a left edge that is no
    // multiple of 4 costs up to 3 columns)
    int rows = 0, cols = 0;
    for (int c = 0; c < GRID; ++c) {
        rows = std::max(rows, cell_begin(c + 1, H) - cell_begin(c, H));
        cols = std::max(cols, cell_begin(c + 1, W) - (cell_begin(c, W) & ~3));
    }
    const dim3 block(64, 4), grid((cols + TILE_W - 1) / TILE_W, (rows + TILE_H - 1) / TILE_H, GRID * GRID);
    scene_hist_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
