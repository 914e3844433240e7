// mesplit.hip -- vectors per 8 x 8 sub-cell for the temporal noise prefilter: every quarter of a cell chooses again among
// the vectors of its cell and the eight around it, and the gather moves the picture sub-cell by sub-cell
// (include/dcvc_hip_mesplit.h, which states the arithmetic; this file only arranges it, and the filters, the luma, the key
// and the two ways of moving a block are mesub_common.h's, shared with mesub.hip).
//
// me_split_kernel: a WORKGROUP of 256 threads owns one 16 x 16 cell, a WAVE one of its four sub-cells (wave w: sub-cell
// (w >> 1, w & 1), lane l its pixel (l >> 3, l & 7)), so a sub-cell's SAD is a sum across one wave and its key never
// leaves it.  Nine lanes fetch the candidates, clamp and scale them and put them in LDS as packed words (vy in the low
// half, vx in the high); every thread then compares the nine words and keeps one bit per FIRST occurrence.  Where a single
// word is left and it is whole (the fixed camera's case) nothing is staged: a thread reads ref's sample under its pixel,
// the wave adds up and lane 0 writes.  Otherwise, per DISTINCT candidate: the 23 x 23 window of ref's luma around the cell
// moved by the whole part (taps -3 .. +4) is formed, every coordinate clamped BEFORE the load and all loads of a thread
// issued before the first code is formed, and kept in LDS as bytes; the horizontal pass makes 23 rows of 16 int16; the
// vertical pass is a thread's own pixel; the wave sums the absolute differences of the pixels that lie in the picture and
// keeps the smaller packed key.  Two barriers a candidate.  Nothing global is atomic, nothing is kept in scratch.
//
// me_compensate_split_kernel: a workgroup of 256 threads per cell.  A cell whose sub-cells (those that hold a pixel) have
// one vector goes down me_compensate_sub_kernel's path for it: the copy of bits by quads, or the staged folds of the whole
// cell.  Any other cell is moved sub-cell by sub-cell by the whole workgroup: 192 lanes copy the bits of a whole vector's
// 8 x 8 x 3 samples, a fractional one stages 15 x 15 x 3 samples and folds them as the cell's path does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_mesplit.h"
#include "kernel_common.h"
#include "mesub_common.h"

namespace {

constexpr int SUB = DCVC_MESPLIT_SUB, NC = 9, SW = CELL + 7, SWP = SW + 1, SPIX = SW * SW, SPER = (SPIX + THREADS - 1) / THREADS;
static_assert(2 * SUB == CELL && SUB * SUB == 64 && SW == SWIN, "a wave per sub-cell; taps -3 .. +4");

struct SplitArgs {
    const float *cur, *ref;
    const int16_t *mv_in;
    int16_t *mv8;
    uint32_t *cost8;
    int64_t cps, rps;
    int32_t crs, rrs, H, W, wc, lambda, unit, rows, cols;
};

__global__ __launch_bounds__(THREADS) void me_split_kernel(const SplitArgs p) {
    __shared__ __align__(4) uint8_t win[SW][SWP];  // Y of ref: row = y - Y0 - iy + 3, byte = x - X0 - ix + 3
    __shared__ int16_t hp[SW][CELL];               // the horizontal pass of every window row
    __shared__ unsigned cand[NC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int X0 = blockIdx.x * CELL, Y0 = blockIdx.y * CELL;
    const int sy = SUB * (wave >> 1), sx = SUB * (wave & 1), yy = sy + (lane >> 3), xx = sx + (lane & 7);  // the thread's pixel in the cell
    const int64_t at = ((int64_t)2 * blockIdx.y + (wave >> 1)) * (2 * p.wc) + 2 * blockIdx.x + (wave & 1);
    const bool holds = Y0 + sy < p.H && X0 + sx < p.W;  // (uniform across the wave) the sub-cell holds a pixel
    if (X0 >= p.W || Y0 >= p.H) {  // (uniform across the workgroup) a cell of the padding holds no pixel
        if (lane == 0) p.mv8[2 * at] = 0, p.mv8[2 * at + 1] = 0, p.cost8[at] = 0;
        return;
    }
    float c[3];
    {
        const int y = min(Y0 + yy, p.H - 1), x = min(X0 + xx, p.W - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = p.cur[k * p.cps + (int64_t)y * p.crs + x];
    }
    if (tid < NC) {  // the candidates: the cells around this one that hold a pixel, clamped and in quarter pixels
        const int ci = min(max((int)blockIdx.y + tid / 3 - 1, 0), p.rows - 1), cj = min(max((int)blockIdx.x + tid % 3 - 1, 0), p.cols - 1);
        const int64_t cell = (int64_t)ci * p.wc + cj;
        const int lim = p.unit == 1 ? DCVC_ME_MAX_R : 4 * DCVC_ME_MAX_R + 3, mul = 4 / p.unit;
        const int vy = mul * min(max((int)p.mv_in[2 * cell], -lim), lim), vx = mul * min(max((int)p.mv_in[2 * cell + 1], -lim), lim);
        cand[tid] = pair16(vy, vx);
    }
    const int yc = (int)luma_of(c);
    const bool inside = Y0 + yy < p.H && X0 + xx < p.W;
    __syncthreads();
    unsigned word[NC], fresh = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) word[k] = cand[k];
#pragma unroll
    for (int k = 0; k < NC; ++k) {  // one bit per first occurrence of a word
        bool first = true;
#pragma unroll
        for (int j = 0; j < k; ++j) first = first && word[j] != word[k];
        fresh |= (unsigned)first << k;
    }
    fresh = __builtin_amdgcn_readfirstlane(fresh);

    if (fresh == 1u && (word[0] & 0x00030003u) == 0) {  // (uniform) nine equal, whole candidates: one unfiltered SAD
        const int w0 = __builtin_amdgcn_readfirstlane((int)word[0]);
        const int vy = (int)(int16_t)(w0 & 0xffff), vx = w0 >> 16;
        const int y = min(max(Y0 + yy + (vy >> 2), 0), p.H - 1), x = min(max(X0 + xx + (vx >> 2), 0), p.W - 1);
        float r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = p.ref[k * p.rps + (int64_t)y * p.rrs + x];
        const unsigned sad = wave_sum(inside ? (unsigned)abs(yc - (int)luma_of(r)) : 0u);
        if (lane == 0) {
            p.mv8[2 * at] = (int16_t)(holds ? vy : 0), p.mv8[2 * at + 1] = (int16_t)(holds ? vx : 0);
            p.cost8[at] = sad;  // (0 where the sub-cell holds no pixel)
        }
        return;
    }

    unsigned long long key = ~0ull;
#pragma unroll 1
    for (int k = 0; k < NC; ++k) {
        if (!((fresh >> k) & 1u)) continue;  // (uniform) met before: the same key
        const int wk = __builtin_amdgcn_readfirstlane((int)cand[k]);
        const int vy = (int)(int16_t)(wk & 0xffff), vx = wk >> 16;
        const int iy = vy >> 2, py = vy & 3, ix = vx >> 2, px = vx & 3;
        // ---- every load of the thread: its share of the window
        float w[SPER][3];
        int wat[SPER];
#pragma unroll
        for (int i = 0; i < SPER; ++i) {
            const int pix = min(i * THREADS + tid, SPIX - 1), wy = pix / SW, wx = pix - wy * SW;
            const int y = min(max(Y0 + iy - LEAD + wy, 0), p.H - 1), x = min(max(X0 + ix - LEAD + wx, 0), p.W - 1);
            wat[i] = wy * SWP + wx;
#pragma unroll
            for (int q = 0; q < 3; ++q) w[i][q] = p.ref[q * p.rps + (int64_t)y * p.rrs + x];
        }
#pragma unroll
        for (int i = 0; i < SPER; ++i) (&win[0][0])[wat[i]] = (uint8_t)luma_of(w[i]);
        __syncthreads();
        // ---- the horizontal pass: 16 positions of every window row
        for (int o = tid; o < SW * CELL; o += THREADS) {
            const int r = o >> 4, x = o & 15;
            int s = 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) s += __mul24(TAP9[3 + px][1 + t], (int)win[r][x + t]);
            hp[r][x] = (int16_t)s;
        }
        __syncthreads();
        // ---- the vertical pass of the thread's pixel and the sub-cell's SAD
        int s = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) s += __mul24(TAP9[3 + py][1 + t], (int)hp[yy + t][xx]);
        const int yi = min(max((s + 2048) >> 12, 0), 255);
        const unsigned sad = wave_sum(inside ? (unsigned)abs(yc - yi) : 0u);
        const unsigned long long cnd = key_of(sad, vy, vx, p.lambda);
        key = cnd < key ? cnd : key;
    }
    if (lane == 0) {
        p.mv8[2 * at] = (int16_t)(holds ? key_vy(key) : 0), p.mv8[2 * at + 1] = (int16_t)(holds ? key_vx(key) : 0);
        p.cost8[at] = holds ? key_sad(key, p.lambda) : 0u;
    }
}

__global__ __launch_bounds__(THREADS) void me_compensate_split_kernel(const SubArgs p) {
    __shared__ float win[3][SWIN][SPITCH];  // ref: row = y - Y0 - iy + 3, column = x - X0 - ix + 3
    __shared__ float hz[3][SWIN][CELL];     // the horizontal pass of every staged row
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * CELL, Y0 = blockIdx.y * CELL;
    if (X0 >= p.W || Y0 >= p.H) return;  // (uniform across the workgroup)
    int vy[4], vx[4];
    bool one = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t at = ((int64_t)2 * blockIdx.y + (q >> 1)) * (2 * p.wc) + 2 * blockIdx.x + (q & 1);
        vy[q] = __builtin_amdgcn_readfirstlane((int)p.mv[2 * at]), vx[q] = __builtin_amdgcn_readfirstlane((int)p.mv[2 * at + 1]);
        const bool holds = Y0 + SUB * (q >> 1) < p.H && X0 + SUB * (q & 1) < p.W;
        one = one && (!holds || (vy[q] == vy[0] && vx[q] == vx[0]));
    }
    if (one) {  // (uniform) one vector for the cell: dcvc_me_compensate_sub's path
        if (((vy[0] | vx[0]) & 3) == 0) move_cell_whole(p, tid, Y0, X0, vy[0] >> 2, vx[0] >> 2);
        else move_block_frac<CELL>(p, tid, Y0, X0, vy[0], vx[0], win, hz, false);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int Ys = Y0 + SUB * (q >> 1), Xs = X0 + SUB * (q & 1);
        if (Ys >= p.H || Xs >= p.W) continue;  // (uniform)
        if (((vy[q] | vx[q]) & 3) != 0) {
            move_block_frac<SUB>(p, tid, Ys, Xs, vy[q], vx[q], win, hz, true);
            continue;
        }
        const int k = tid >> 6, y = Ys + ((tid & 63) >> 3), x = Xs + (tid & 7);  // a whole vector: the bits, a sample a lane
        if (k < 3 && y < p.H && x < p.W) {
            const int fy = min(max(y + (vy[q] >> 2), 0), p.H - 1), fx = min(max(x + (vx[q] >> 2), 0), p.W - 1);
            p.out[k * p.ops + (int64_t)y * p.ors + x] = p.ref[k * p.rps + (int64_t)fy * p.rrs + fx];
        }
    }
}

}  // namespace

extern "C" int dcvc_me_split(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps, int32_t H,
                             int32_t W, int32_t lambda, int32_t unit, const int16_t *mv_in, int16_t *mv8, uint32_t *cost8, void *stream) {
    if (!mv_in || !mv8 || !cost8 || !size_ok(H, W) || !planes_ok(cur, cur_rs, cur_ps, H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) ||
        lambda < 0 || lambda > DCVC_ME_MAX_LAMBDA || (unit != 1 && unit != DCVC_MESUB_UNIT) || !aligned(cur, 4) || !aligned(ref, 4) ||
        !aligned(cost8, 4) || !aligned(mv_in, 2) || !aligned(mv8, 2))
        return DCVC_E_ARG;
    const int32_t wc = 4 * ((W + 63) / 64), hc = 4 * ((H + 63) / 64);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(mv_in), b0 = reinterpret_cast<uintptr_t>(mv8), cells = (uintptr_t)hc * wc;
    if (a0 < b0 + 16 * cells && b0 < a0 + 4 * cells) return DCVC_E_ARG;
    SplitArgs a{};
    a.cur = cur, a.ref = ref, a.mv_in = mv_in, a.mv8 = mv8, a.cost8 = cost8;
    a.cps = cur_ps, a.rps = ref_ps, a.crs = cur_rs, a.rrs = ref_rs, a.H = H, a.W = W, a.wc = wc, a.lambda = lambda, a.unit = unit;
    a.rows = (H + CELL - 1) / CELL, a.cols = (W + CELL - 1) / CELL;
    me_split_kernel<<<dim3(wc, hc), THREADS, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_me_compensate_split(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps,
                                        int32_t H, int32_t W, const int16_t *mv8, void *stream) {
    if (!mv8 || !size_ok(H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) || !planes_ok(out, out_rs, out_ps, H, W) || !aligned(ref, 4) ||
        !aligned(out, 4) || !aligned(mv8, 2) || extents_overlap(out, out_rs, out_ps, ref, ref_rs, ref_ps, H, W))
        return DCVC_E_ARG;
    SubArgs a{};
    a.ref = ref, a.out = out, a.mv = mv8, a.rps = ref_ps, a.ops = out_ps, a.rrs = ref_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.rvec = vec_ok(ref, ref_rs, ref_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    me_compensate_split_kernel<<<dim3((W + CELL - 1) / CELL, (H + CELL - 1) / CELL), THREADS, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
