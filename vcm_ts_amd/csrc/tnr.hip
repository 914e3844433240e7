// tnr.hip -- one step of the motion-adaptive temporal noise prefilter (include/dcvc_hip_tnr.h, which states the
// arithmetic; this file only arranges it).
//
// tnr_step_kernel is one streaming pass bound by memory: per pixel 24 bytes of picture read (cur and ref) and 12 written,
// plus the halo's share.  It is tiled the way motion_step_kernel is.  A WORKGROUP of 8 waves owns a strip of 16 rows x
// 256 columns: the 16 adjacent cells of one cell row, so it alone writes their sad / held and nothing global is atomic.
// A WAVE takes 2 consecutive rows of the strip, a lane 4 consecutive pixels of each; the lane keeps those 2 x 4 pixels'
// six floats in registers from the load phase to the blend.  Lane bits: 0-1 the quad inside the cell, 2-5 the cell.
//
// The window needs d on a 2-pixel halo round the strip: 20 rows x 260 columns, so cur and ref are read 20 * 260 /
// (16 * 256) = 1.27 times (30.5 bytes per pixel read, 42.5 moved).  The two rows above and the two below are one more quad
// for the lanes of waves 0-3; the 20 x 4 pixels left and right are one pixel for 80 lanes of waves 4-5.  Every coordinate
// is clamped to the picture BEFORE the load (replicated edges: the clamped pixel's d is the d the window wants), so every
// read is inside the H x W crop, and a strip that sticks out of the picture fills its part of the LDS tile the same way.
// All loads of a lane are issued before the first code is formed.
//
// LDS: d as bytes, 20 rows x 264 (the strip's quads start 4-byte aligned at byte 4; the left halo is bytes 2-3, the right
// one bytes 260-261); the 5-tap horizontal sums of all 20 rows as uint16, 20 x 256; the table, 256 uint16; the cells'
// partial sums of the eight waves: 5280 + 10240 + 512 + 1024 = 17056 bytes.  S is formed separably: each wave sums rows
// w, w + 8, w + 16 horizontally (three words in, two out per lane), then a lane sums five rows vertically for each of its
// own two.  A lane folds its 8 pixels in registers, the four lanes of a cell with two xor-shuffles, the eight waves meet
// in LDS and sixteen threads store one sad and one held each.  Integer sums do not depend on order.
//
// A quad is read or written as one 16-byte access when the picture's base and strides allow it and the quad is whole;
// anything else goes element by element through the same arithmetic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_tnr.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, WAVES = 8, ROWS = 2, HALO = DCVC_TNR_WINDOW / 2;
constexpr int D_ROWS = CELL + 2 * HALO, D_WORDS = TILE_W / 4 + 2, SIDE = 2 * HALO * D_ROWS;
static_assert(CELL == 16 && TILE_W == 64 * 4 && ROWS * WAVES == CELL && HALO == 2, "a lane per quad, a wave per two rows");
static_assert(2 * HALO <= WAVES / 2 && SIDE <= 64 * WAVES / 2, "the halo rows go to waves 0-3, the halo columns to waves 4-7");

struct TnrArgs {
    const float *cur, *ref;
    float *out;
    const uint16_t *wtab;
    uint32_t *sad;
    uint16_t *held;
    int64_t cps, rps, ops;
    int32_t crs, rrs, ors, H, W, wc, P, cvec, rvec, ovec;
};

// the quad at columns x0 .. x0 + 3 of a row, every column clamped to the picture's last one
__device__ __forceinline__ void load_quad(const float *row, int x0, int W, bool vec, float (&f)[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(row + x0);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = row[min(x0 + q, W - 1)];
    }
}

__device__ __forceinline__ unsigned luma_diff(float cr, float cg, float cb, float rr, float rg, float rb) {
    return (unsigned)abs(luma8(code8(cr), code8(cg), code8(cb)) - luma8(code8(rr), code8(rg), code8(rb)));
}

__device__ __forceinline__ unsigned quad_diffs(const float (&c)[3][4], const float (&r)[3][4]) {
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) word |= luma_diff(c[0][q], c[1][q], c[2][q], r[0][q], r[1][q], r[2][q]) << (8 * q);
    return word;
}

__global__ __launch_bounds__(64 * WAVES) void tnr_step_kernel(const TnrArgs p) {
    __shared__ unsigned D[D_ROWS][D_WORDS];           // d, a byte per pixel: row = strip row + 2, byte = strip column + 4
    __shared__ uint2 HS[D_ROWS][TILE_W / 4];          // the horizontal 5-tap sums, four uint16 per quad
    __shared__ uint16_t tab[256];
    __shared__ unsigned part[2][WAVES][TILE_CELLS];   // sad and held of each cell in each wave's two rows
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * CELL, x0 = X0 + lane * 4, y0 = Y0 + wave * ROWS;
    const int col = blockIdx.x * TILE_CELLS + lane;
    const bool writer = wave == 0 && lane < TILE_CELLS && col < p.wc;
    if (X0 >= p.W || Y0 >= p.H) {  // (uniform across the workgroup) a strip of the padding: its cells hold no pixel
        if (writer) p.sad[(int64_t)blockIdx.y * p.wc + col] = 0, p.held[(int64_t)blockIdx.y * p.wc + col] = 0;
        return;
    }
    const bool whole = x0 + 4 <= p.W, cv = p.cvec && whole, rv = p.rvec && whole;

    // ---- every load of the lane: its own 2 x 4 pixels, then its share of the halo
    float c[ROWS][3][4], r[ROWS][3][4], hc[3][4], hr[3][4];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int y = min(y0 + i, p.H - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            load_quad(p.cur + k * p.cps + (int64_t)y * p.crs, x0, p.W, cv, c[i][k]);
            load_quad(p.ref + k * p.rps + (int64_t)y * p.rrs, x0, p.W, rv, r[i][k]);
        }
    }
    const int side = (wave - WAVES / 2) * 64 + lane;  // waves 4-7: which of the 80 pixels left and right of the strip
    int hrow = 0, hbyte = 0;
    if (wave < 2 * HALO) {  // (uniform across a wave) strip rows -2, -1, 16, 17 at the lane's own columns
        const int rel = wave < HALO ? wave - HALO : CELL + wave - HALO;
        const int y = min(max(Y0 + rel, 0), p.H - 1);
        hrow = rel + HALO;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            load_quad(p.cur + k * p.cps + (int64_t)y * p.crs, x0, p.W, cv, hc[k]);
            load_quad(p.ref + k * p.rps + (int64_t)y * p.rrs, x0, p.W, rv, hr[k]);
        }
    } else if (side >= 0 && side < SIDE) {  // strip columns -2, -1, 256, 257 of all 20 rows
        const int rel = side / (2 * HALO) - HALO, k4 = side % (2 * HALO), relx = k4 < HALO ? k4 - HALO : TILE_W + k4 - HALO;
        const int y = min(max(Y0 + rel, 0), p.H - 1), x = min(max(X0 + relx, 0), p.W - 1);
        hrow = rel + HALO, hbyte = relx + 4;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            hc[k][0] = p.cur[k * p.cps + (int64_t)y * p.crs + x];
            hr[k][0] = p.ref[k * p.rps + (int64_t)y * p.rrs + x];
        }
    }
    if (wave * 64 + lane < 256) tab[wave * 64 + lane] = p.wtab[wave * 64 + lane];

    // ---- d of everything loaded, into the tile
    unsigned own[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        own[i] = quad_diffs(c[i], r[i]);
        D[wave * ROWS + i + HALO][1 + lane] = own[i];
    }
    if (wave < 2 * HALO)
        D[hrow][1 + lane] = quad_diffs(hc, hr);
    else if (side >= 0 && side < SIDE)
        reinterpret_cast<uint8_t *>(D[hrow])[hbyte] = (uint8_t)luma_diff(hc[0][0], hc[1][0], hc[2][0], hr[0][0], hr[1][0], hr[2][0]);
    __syncthreads();

    // ---- horizontal: the quad at strip columns 4 l .. 4 l + 3 needs bytes 4 l + 2 .. 4 l + 9 of its row
    for (int row = wave; row < D_ROWS; row += WAVES) {  // (uniform across a wave)
        const unsigned w0 = D[row][lane], w1 = D[row][lane + 1], w2 = D[row][lane + 2];
        const unsigned b2 = (w0 >> 16) & 255, b3 = w0 >> 24, b4 = w1 & 255, b5 = (w1 >> 8) & 255, b6 = (w1 >> 16) & 255,
                       b7 = w1 >> 24, b8 = w2 & 255, b9 = (w2 >> 8) & 255;
        const unsigned mid = b4 + b5 + b6, s0 = b2 + b3 + mid, s1 = b3 + mid + b7, s2 = mid + b7 + b8, s3 = b5 + b6 + b7 + b8 + b9;
        HS[row][lane] = make_uint2(s0 | s1 << 16, s2 | s3 << 16);
    }
    __syncthreads();

    // ---- vertical, the weight, the blend
    const bool ov = p.ovec && whole;
    unsigned sad = 0, held = 0;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (y0 + i >= p.H) break;  // (uniform across a wave)
        unsigned S[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < DCVC_TNR_WINDOW; ++j) {
            const uint2 t = HS[wave * ROWS + i + j][lane];
            S[0] += t.x & 0xffff, S[1] += t.x >> 16, S[2] += t.y & 0xffff, S[3] += t.y >> 16;
        }
        float o[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned d = (own[i] >> (8 * q)) & 255;
            const unsigned w = d > (unsigned)p.P ? 256u : tab[S[q] / 25];
            const bool in = x0 + q < p.W;
            sad += in ? d : 0u;
            held += (in && w < 256u) ? 1u : 0u;
            const float wf = (float)w;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k][q] = w == 256u ? c[i][k][q] : r[i][k][q] + (c[i][k][q] - r[i][k][q]) * wf * 0x1p-8f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float *row = p.out + k * p.ops + (int64_t)(y0 + i) * p.ors + x0;
            if (ov) {
                *reinterpret_cast<float4 *>(row) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) row[q] = o[k][q];
            }
        }
    }
    sad += (unsigned)__shfl_xor((int)sad, 1), held += (unsigned)__shfl_xor((int)held, 1);
    sad += (unsigned)__shfl_xor((int)sad, 2), held += (unsigned)__shfl_xor((int)held, 2);
    if ((lane & 3) == 0) part[0][wave][lane >> 2] = sad, part[1][wave][lane >> 2] = held;
    __syncthreads();
    if (writer) {
        unsigned s = 0, h = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) s += part[0][v][lane], h += part[1][v][lane];
        p.sad[(int64_t)blockIdx.y * p.wc + col] = s;
        p.held[(int64_t)blockIdx.y * p.wc + col] = (uint16_t)h;
    }
}

}  // namespace

extern "C" int dcvc_tnr_step(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps,
                             float *out, int32_t out_rs, int64_t out_ps, int32_t H, int32_t W, const uint16_t *wtab, int32_t P,
                             uint32_t *sad, uint16_t *held, void *stream) {
    if (!wtab || !sad || !held || !size_ok(H, W) || !planes_ok(cur, cur_rs, cur_ps, H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) ||
        !planes_ok(out, out_rs, out_ps, H, W) || P < 0 || P > DCVC_TNR_MAX_P || !aligned(cur, 4) || !aligned(ref, 4) ||
        !aligned(out, 4) || !aligned(sad, 4) || !aligned(wtab, 2) || !aligned(held, 2) ||
        extents_overlap(out, out_rs, out_ps, cur, cur_rs, cur_ps, H, W) || extents_overlap(out, out_rs, out_ps, ref, ref_rs, ref_ps, H, W))
        return DCVC_E_ARG;
    TnrArgs a{};
    a.cur = cur, a.ref = ref, a.out = out, a.wtab = wtab, a.sad = sad, a.held = held;
    a.cps = cur_ps, a.rps = ref_ps, a.ops = out_ps, a.crs = cur_rs, a.rrs = ref_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.P = P;
    a.cvec = vec_ok(cur, cur_rs, cur_ps), a.rvec = vec_ok(ref, ref_rs, ref_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    const dim3 block(64, WAVES), grid(nblk(a.wc, TILE_CELLS), 4 * ((H + 63) / 64));
    tnr_step_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
