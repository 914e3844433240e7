// aq.hip -- backward-adaptive quantisation: the activity of every 16 x 16 cell of the reference picture and the q-scale
// map made from it (include/dcvc_hip_aq.h, which states the arithmetic; this file only arranges it).
//
// aq_activity_kernel reads the three planes once and is bound by memory.  Its unit of work is a TILE: the 4 adjacent cells
// of one cell row, 16 rows x 64 columns (Wp is a multiple of 64, so tiles never straddle the picture's edge and no lane
// needs a bound).  ONE WAVE takes a whole tile: 16 lanes to a row, 4 consecutive pixels to a lane, rows r, r + 4, r + 8 and
// r + 12 of the tile for the lanes of row group r -- every load instruction of the wave reads 4 rows of 256 contiguous
// bytes, and all twelve loads of a lane (4 row groups x 3 planes, 192 bytes) are issued before the first code is formed.
// Lane bits: 0-1 the quad inside the cell, 2-3 the cell, 4-5 the row group -- a lane sums its four rows in registers, S1 and
// S2 of a cell then fold with four xor-shuffles (1, 2, 16, 32), and lanes 0, 4, 8, 12 finish one cell each: V, L, the store
// of L.  No LDS and no barrier per tile.  Waves take tiles in the order of their number across the grid (adjacent waves,
// adjacent tiles) and a wave takes TILES_PER_WAVE of them, keeping the sum of its L in a register; at the end the 4 waves
// of a workgroup meet in 16 bytes of LDS and thread 0 adds the workgroup's sum to the picture's with ONE 64-bit integer
// atomic (255 per 1088 x 1920 picture).  The first form of this kernel had a workgroup per tile (a wave per four rows) and so
// 2040 atomics on the one address: 28 us per 1088 x 1920 picture against 7 to 10 for this one (profiles/aq_1080p.txt).
// Integer sums do not depend on order.
// Pictures whose base or strides do not allow 16-byte loads take four 4-byte loads in place of each through the same code.
//
// aq_map_kernel is one thread per cell: a division for the mean, two table reads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_aq.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 4, TILES_PER_WAVE = 2, MIN_K = 10, MAX_K = 1000;
static_assert(CELL == 16 && DCVC_AQ_FTAB == MAX_K - MIN_K + 1 && DCVC_AQ_KTAB == 2 * DCVC_AQ_MAX_L + 1, "dcvc_hip_aq.h");

struct ActivityArgs {
    const float *pic;
    int32_t *L;
    unsigned long long *sum;
    int64_t ps;
    int32_t rs, tiles_x, tiles;
};

__device__ __forceinline__ unsigned fold(unsigned v, int off) { return v + (unsigned)__shfl_xor((int)v, off); }

// L of dcvc_hip_aq.h from V
__device__ __forceinline__ int activity(unsigned V) {
    const unsigned v = V + 1u;
    const int e = 31 - __clz((int)v);
    const unsigned m = (e >= 8 ? v >> (e - 8) : v << (8 - e)) & 255u;
    return 256 * e + (int)m;
}

template <bool VEC>
__global__ __launch_bounds__(256) void aq_activity_kernel(const ActivityArgs p) {
    __shared__ unsigned part[4];  // the sum of L of each wave
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int group = lane >> 4, x_in = (lane & 15) * 4;
    unsigned mine = 0;  // the sum of the L this lane has finished (lanes 0, 4, 8, 12)
    for (int tile = blockIdx.x * 4 + wave; tile < p.tiles; tile += gridDim.x * 4) {  // (uniform across a wave)
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const float *at = p.pic + (int64_t)(ty * CELL + group) * p.rs + tx * (CELL * TILE_CELLS) + x_in;
        float f[4][3][4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *q = at + c * p.ps + (int64_t)(4 * g) * p.rs;
                if (VEC) {
                    const float4 t = *reinterpret_cast<const float4 *>(q);
                    f[g][c][0] = t.x, f[g][c][1] = t.y, f[g][c][2] = t.z, f[g][c][3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) f[g][c][i] = q[i];
                }
            }
        unsigned s1 = 0, s2 = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned Y = (unsigned)luma8(code8(f[g][0][i]), code8(f[g][1][i]), code8(f[g][2][i]));
                s1 += Y, s2 += Y * Y;
            }
        s1 = fold(fold(fold(fold(s1, 1), 2), 16), 32);
        s2 = fold(fold(fold(fold(s2, 1), 2), 16), 32);
        if ((lane & 0x33) == 0) {  // lanes 0, 4, 8, 12: cell lane >> 2 of the tile
            const int L = activity(256u * s2 - s1 * s1);
            p.L[(int64_t)ty * (p.tiles_x * TILE_CELLS) + tx * TILE_CELLS + (lane >> 2)] = L;
            mine += (unsigned)L;
        }
    }
    mine = fold(fold(mine, 4), 8);  // (all 64 lanes: the others hold 0)
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (wave == 0 && lane == 0) {
        const unsigned total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(p.sum, (unsigned long long)total);
    }
}

struct MapArgs {
    const int32_t *L;
    const unsigned long long *sum;
    const uint16_t *ktab;
    const float *ftab, *roi;
    float *map;
    int32_t cells;
};

__global__ __launch_bounds__(256) void aq_map_kernel(const MapArgs p) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= p.cells) return;
    const unsigned long long mean = *p.sum / (unsigned long long)p.cells;
    const int M = mean < DCVC_AQ_MAX_L ? (int)mean : DCVC_AQ_MAX_L;
    const int d = p.L[cell] - M;
    int k = p.ktab[min(max(d + DCVC_AQ_MAX_L, 0), DCVC_AQ_KTAB - 1)];
    if (p.roi) {
        const int k_roi = (int)rintf(100.0f * p.roi[cell]);
        const int64_t both = ((int64_t)k_roi * k + 50) / 100;
        k = both < MIN_K ? MIN_K : both > MAX_K ? MAX_K : (int)both;
    }
    p.map[cell] = p.ftab[min(max(k, MIN_K), MAX_K) - MIN_K];
}

inline bool side_ok(int32_t s) { return s > 0 && s % 64 == 0 && s <= DCVC_ROI_MAX_SIDE; }

}  // namespace

extern "C" int dcvc_aq_activity(const float *pic, int32_t row_stride, int64_t plane_stride, int32_t Hp, int32_t Wp, int32_t *L,
                                uint64_t *sum, void *stream) {
    if (!L || !sum || !side_ok(Hp) || !side_ok(Wp) || !planes_ok(pic, row_stride, plane_stride, Hp, Wp) || !aligned(pic, 4) ||
        !aligned(L, 4) || !aligned(sum, 8))
        return DCVC_E_ARG;
    ActivityArgs a{};
    a.pic = pic, a.L = L, a.sum = reinterpret_cast<unsigned long long *>(sum), a.ps = plane_stride, a.rs = row_stride;
    a.tiles_x = Wp / (CELL * TILE_CELLS), a.tiles = a.tiles_x * (Hp / CELL);
    const dim3 block(64, 4), grid(nblk(a.tiles, 4 * TILES_PER_WAVE));
    if (aligned(pic, 16) && row_stride % 4 == 0 && plane_stride % 4 == 0)
        aq_activity_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(a);
    else
        aq_activity_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_aq_map(const int32_t *L, const uint64_t *sum, int32_t hc, int32_t wc, const uint16_t *ktab, const float *ftab,
                           const float *roi_map, float *map, void *stream) {
    constexpr int MAX_CELLS = DCVC_ROI_MAX_SIDE / CELL;
    if (!L || !sum || !ktab || !ftab || !map || hc <= 0 || wc <= 0 || hc % 4 || wc % 4 || hc > MAX_CELLS || wc > MAX_CELLS ||
        !aligned(sum, 8) || !aligned(L, 4) || !aligned(ftab, 4) || !aligned(roi_map, 4) || !aligned(map, 4) || !aligned(ktab, 2))
        return DCVC_E_ARG;
    MapArgs a{};
    a.L = L, a.sum = reinterpret_cast<const unsigned long long *>(sum), a.ktab = ktab, a.ftab = ftab, a.roi = roi_map;
    a.map = map, a.cells = hc * wc;
    aq_map_kernel<<<nblk(a.cells, 256), 256, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
