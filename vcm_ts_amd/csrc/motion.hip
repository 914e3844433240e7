// motion.hip -- one step of the per-pixel background model and the foreground count of every 16 x 16 cell
// (include/dcvc_hip_motion.h, which states the arithmetic; this file only arranges it).
//
// motion_step_kernel is one streaming pass bound by memory: per pixel 12 bytes of picture read, 2 bytes of model read and
// 2 written.  It is tiled the way aq_activity_kernel is, with bounds, because H and W are the UNPADDED size here.  A
// WORKGROUP of 4 waves owns a strip of 16 rows x 256 columns: the 16 adjacent cells of one cell row, so it alone writes
// their counts and nothing global is atomic.  A WAVE takes 4 consecutive rows of the strip, a lane 4 consecutive pixels
// of each: every load instruction of a wave reads one row of 1024 contiguous bytes, and all sixteen loads of a lane (4
// rows x (3 planes + the model)) are issued before the first code is formed.  Lane bits: 0-1 the quad inside the cell,
// 2-5 the cell.  A lane counts its 16 pixels in a register, the four lanes of a cell fold with two xor-shuffles, the four
// waves meet in 256 bytes of LDS and sixteen threads store one count each.  Integer sums do not depend on order.
//
// A quad is read as one 16-byte access when the picture's base and strides allow it, and the model's quad as one 8-byte
// access when its base and W allow it (W % 4 == 0: then every quad of the picture is whole); anything else goes element
// by element, guarded by the picture's width, through the same arithmetic.  A row past the picture's last one reads the
// last one again and neither counts nor writes -- it belongs to the same lane of the same wave, which reads before it writes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_motion.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, ROWS = 4;
static_assert(CELL == 16 && TILE_W == 64 * 4 && ROWS * 4 == CELL, "a lane per quad, a wave per four rows");

struct MotionArgs {
    const float *rgb;
    uint16_t *bg, *counts;
    int64_t ps;
    int32_t rs, H, W, wc, init, T8, k_bg, k_fg, pvec, bvec;
};

__global__ __launch_bounds__(256) void motion_step_kernel(const MotionArgs p) {
    __shared__ unsigned part[4][TILE_CELLS];  // the count of each cell in each wave's four rows
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x0 = blockIdx.x * TILE_W + lane * 4, y0 = blockIdx.y * CELL + wave * ROWS;
    unsigned cnt = 0;
    if (x0 < p.W && y0 < p.H) {  // (y0 is uniform across a wave)
        const bool whole = x0 + 4 <= p.W, pv = p.pvec && whole, bv = p.bvec && whole;
        float f[ROWS][3][4];
        int B[ROWS][4];
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
            const uint16_t *brow = p.bg + (int64_t)y * p.W + x0;
            if (bv) {
                const uint2 t = *reinterpret_cast<const uint2 *>(brow);
                B[r][0] = t.x & 0xffff, B[r][1] = t.x >> 16, B[r][2] = t.y & 0xffff, B[r][3] = t.y >> 16;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) B[r][q] = x0 + q < p.W ? brow[q] : 0;
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (y0 + r >= p.H) break;  // (uniform across a wave)
            unsigned nb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int Y8 = luma8(code8(f[r][0][q]), code8(f[r][1][q]), code8(f[r][2][q])) << 8;
                const int delta = Y8 - B[r][q], a = abs(delta);
                const bool fg = a > p.T8;
                const int s = a >> (fg ? p.k_fg : p.k_bg);
                nb[q] = (unsigned)(p.init ? Y8 : B[r][q] + (delta < 0 ? -s : s)) & 0xffffu;
                cnt += (!p.init && fg && x0 + q < p.W) ? 1u : 0u;
            }
            uint16_t *brow = p.bg + (int64_t)(y0 + r) * p.W + x0;
            if (bv) {
                *reinterpret_cast<uint2 *>(brow) = make_uint2(nb[0] | nb[1] << 16, nb[2] | nb[3] << 16);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) brow[q] = (uint16_t)nb[q];
            }
        }
    }
    cnt += (unsigned)__shfl_xor((int)cnt, 1);
    cnt += (unsigned)__shfl_xor((int)cnt, 2);
    if ((lane & 3) == 0) part[wave][lane >> 2] = cnt;
    __syncthreads();
    const int col = blockIdx.x * TILE_CELLS + lane;
    if (wave == 0 && lane < TILE_CELLS && col < p.wc)
        p.counts[(int64_t)blockIdx.y * p.wc + col] = (uint16_t)(part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]);
}

}  // namespace

extern "C" int dcvc_motion_step(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint16_t *bg,
                                int32_t init, int32_t T, int32_t k_bg, int32_t k_fg, uint16_t *counts, void *stream) {
    if (!bg || !counts || !size_ok(H, W) || !planes_ok(rgb, row_stride, plane_stride, H, W) || T < 1 || T > DCVC_MOTION_MAX_T ||
        k_bg < 0 || k_bg > DCVC_MOTION_MAX_K || k_fg < 0 || k_fg > DCVC_MOTION_MAX_K || !aligned(rgb, 4) || !aligned(bg, 2) ||
        !aligned(counts, 2))
        return DCVC_E_ARG;
    MotionArgs a{};
    a.rgb = rgb, a.bg = bg, a.counts = counts, a.ps = plane_stride, a.rs = row_stride, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.init = init != 0, a.T8 = T << 8, a.k_bg = k_bg, a.k_fg = k_fg;
    a.pvec = aligned(rgb, 16) && row_stride % 4 == 0 && plane_stride % 4 == 0;
    a.bvec = aligned(bg, 8) && W % 4 == 0;
    const dim3 block(64, 4), grid(nblk(a.wc, TILE_CELLS), 4 * ((H + 63) / 64));
    motion_step_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
