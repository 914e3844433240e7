// mesub.hip -- quarter-pel motion for the temporal noise prefilter: the refinement of the search's vectors and the
// interpolating gather (include/dcvc_hip_mesub.h, which states the arithmetic; this file only arranges it).
//
// me_refine_kernel: a WORKGROUP of 256 threads owns one 16 x 16 cell, as in me_search_kernel.  With d the cell's whole-pel
// vector, the 49 candidates 4 d + f read ref's luma at whole offsets -4 .. +4 around d only (f < 0 has the whole part d - 1
// and the phase 4 + f), so each f is ONE 9-tap filter over offsets -4 .. +4 with zeros where its phase has no tap.  The
// 24 x 24 window of ref's luma around d (16 pixels and those offsets) is formed once, every coordinate clamped to the
// picture BEFORE the load, all loads of a thread issued before the first code is formed, and kept in LDS as bytes beside
// the 256 bytes of cur's cell (transposed: a column per 16 bytes).  The horizontal pass makes the seven positions fx = -3 .. 3
// of every window row once, four columns an item from three words of the row, int16 in LDS laid out BY COLUMN (7 x 16
// columns of 24 rows, 48 bytes each).  Then an ITEM is a candidate and a column of the cell: the lane reads the column's 24
// horizontal results of its fx (three 16-byte reads: rows 2 i and 2 i + 1 in word i), the taps of its fy in pairs and the
// column of cur (one 16-byte read each), and runs the vertical pass down the column with v_dot2_i32_i16, five an output:
// rows y .. y + 8 lie in the words y / 2 .. y / 2 + 4, against the pairs (t0 t1) .. (t8 0) for an even y and (0 t0) .. (t7 t8)
// for an odd one.  It sums the absolute differences of the pixels that lie in the picture; the 16 lanes of a candidate add
// up with xor-shuffles, the first of them packs (J, |vy| + |vx|, vy + 256, vx + 256) into 19 + 9 + 9 + 9 bits and keeps the
// minimum, which is folded inside the wave and through LDS across the waves as in me_search_kernel.  784 items: three
// rounds of the four waves and a fourth of 16 lanes of the first wave alone.
// Nothing global is atomic, nothing is kept in scratch.
//
// me_compensate_sub_kernel: a workgroup of 256 threads per cell.  A cell whose vector is whole (the common case) is copied
// by 192 lanes, a quad of four pixels of one plane each, the way me_compensate_kernel does it: one 16-byte access where the
// bases, the strides and the vector allow it.  Any other cell stages the 23 x 23 samples around its 16 x 16 pixels (taps
// -3 .. +4) of the three planes in LDS, coordinates clamped before the load, makes the horizontal pass of every staged row
// into LDS and the vertical pass per pixel, a thread a pixel.
//
// The filters, the luma, the packed key and the two ways of moving a block by one vector live in mesub_common.h, which
// mesplit.hip takes them from as well.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_mesub.h"
#include "kernel_common.h"
#include "mesub_common.h"

namespace {

constexpr int WIN = CELL + NT - 1;
constexpr int ITEMS = NF * NF * CELL, ROUNDS = (ITEMS + THREADS - 1) / THREADS;
constexpr int WPIX = WIN * WIN, PER = (WPIX + THREADS - 1) / THREADS;
static_assert(WIN == 24, "offsets -4 .. +4");

struct RefineArgs {
    const float *cur, *ref;
    const int16_t *mv_in;
    int16_t *mvq;
    uint32_t *cost;
    int64_t cps, rps;
    int32_t crs, rrs, H, W, wc, lambda;
};

__global__ __launch_bounds__(THREADS) void me_refine_kernel(const RefineArgs p) {
    __shared__ __align__(16) uint8_t win[WIN][WIN];   // Y of ref: row = y - Y0 - dy + 4, byte = x - X0 - dx + 4
    __shared__ __align__(16) uint8_t cell[CELL][CELL];  // Y of cur, TRANSPOSED: [x][y], a column per uint4
    __shared__ __align__(16) int16_t hp[NF][CELL][WIN];  // the horizontal pass at fx = -3 .. 3, a COLUMN of 24 rows per 48 bytes
    __shared__ int tap[NF][NT];
    __shared__ __align__(16) unsigned tap2[NF][12];  // the taps in pairs: 0 .. 4 for an even first row, 5 .. 9 for an odd one
    __shared__ unsigned long long best[THREADS / 64];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * CELL, Y0 = blockIdx.y * CELL;
    const int64_t at = (int64_t)blockIdx.y * p.wc + blockIdx.x;
    if (X0 >= p.W || Y0 >= p.H) {  // (uniform across the workgroup) a cell of the padding holds no pixel
        if (tid == 0) p.mvq[2 * at] = 0, p.mvq[2 * at + 1] = 0, p.cost[at] = 0;
        return;
    }
    const int dy = min(max((int)p.mv_in[2 * at], -DCVC_ME_MAX_R), DCVC_ME_MAX_R);
    const int dx = min(max((int)p.mv_in[2 * at + 1], -DCVC_ME_MAX_R), DCVC_ME_MAX_R);

    // ---- every load of the thread: its share of the window, then its pixel of the cell
    float w[PER][3], c[3];
    int wat[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int pix = min(i * THREADS + tid, WPIX - 1), wy = pix / WIN, wx = pix - wy * WIN;
        const int y = min(max(Y0 + dy - 4 + wy, 0), p.H - 1), x = min(max(X0 + dx - 4 + wx, 0), p.W - 1);
        wat[i] = pix;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[i][k] = p.ref[k * p.rps + (int64_t)y * p.rrs + x];
    }
    {
        const int y = min(Y0 + tid / CELL, p.H - 1), x = min(X0 + tid % CELL, p.W - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = p.cur[k * p.cps + (int64_t)y * p.crs + x];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) (&win[0][0])[wat[i]] = (uint8_t)luma_of(w[i]);
    cell[tid % CELL][tid / CELL] = (uint8_t)luma_of(c);
    if (tid < NF * NT) (&tap[0][0])[tid] = (&TAP9[0][0])[tid];
    if (tid < NF * 12) {  // rows y .. y + 8 of a column lie in the words y / 2 .. y / 2 + 4: (t0 t1) .. (t8 0), or (0 t0) .. (t7 t8)
        const int f = tid / 12, e = tid - 12 * f, j = e - 5;
        const int *t = TAP9[f];
        unsigned v = 0;
        if (e < 5) v = pair16(t[2 * e], e < 4 ? t[2 * e + 1] : 0);
        else if (e < 10) v = pair16(j > 0 ? t[2 * j - 1] : 0, t[2 * j]);
        tap2[f][e] = v;
    }
    __syncthreads();

    // ---- the horizontal pass: seven positions of every window row, four columns an item from three words of the row
    for (int o = tid; o < NF * WIN * (CELL / 4); o += THREADS) {
        const int f = o / (WIN * (CELL / 4)), rest = o - f * (WIN * (CELL / 4)), r = rest >> 2, xq = rest & 3;
        const unsigned *row = reinterpret_cast<const unsigned *>(win[r]) + xq;
        const unsigned w0 = row[0], w1 = row[1], w2 = row[2];
        int b[12], t[NT];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = (w0 >> (8 * i)) & 255u, b[4 + i] = (w1 >> (8 * i)) & 255u, b[8 + i] = (w2 >> (8 * i)) & 255u;
#pragma unroll
        for (int k = 0; k < NT; ++k) t[k] = tap[f][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < NT; ++k) s += __mul24(t[k], b[j + k]);
            hp[f][4 * xq + j][r] = (int16_t)s;
        }
    }
    __syncthreads();

    // ---- the candidates: the vertical pass and the SAD of a column, the 16 columns of a candidate in 16 lanes
    const int ch = min(CELL, p.H - Y0), cw = min(CELL, p.W - X0);
    unsigned long long key = ~0ull;
#pragma unroll 1
    for (int round = 0; round < ROUNDS; ++round) {
        if (round * THREADS + (tid & ~63) >= ITEMS) break;  // (uniform across the wave: the last round is one wave's)
        const int item = round * THREADS + tid, it = min(item, ITEMS - 1);
        const int cand = it / CELL, x = it % CELL, fyi = cand / NF, fxi = cand - fyi * NF;
        unsigned col[WIN / 2], t[12], cur4[4];  // rows 2 i and 2 i + 1 of the column in word i
        {
            const uint4 *src = reinterpret_cast<const uint4 *>(hp[fxi][x]);
            const uint4 q0 = src[0], q1 = src[1], q2 = src[2];
            col[0] = q0.x, col[1] = q0.y, col[2] = q0.z, col[3] = q0.w, col[4] = q1.x, col[5] = q1.y, col[6] = q1.z, col[7] = q1.w;
            col[8] = q2.x, col[9] = q2.y, col[10] = q2.z, col[11] = q2.w;
            const uint4 *tp = reinterpret_cast<const uint4 *>(tap2[fyi]);
            const uint4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
            t[0] = t0.x, t[1] = t0.y, t[2] = t0.z, t[3] = t0.w, t[4] = t1.x, t[5] = t1.y, t[6] = t1.z, t[7] = t1.w;
            t[8] = t2.x, t[9] = t2.y, t[10] = t2.z, t[11] = t2.w;
            const uint4 cq = *reinterpret_cast<const uint4 *>(cell[x]);
            cur4[0] = cq.x, cur4[1] = cq.y, cur4[2] = cq.z, cur4[3] = cq.w;
        }
        unsigned sad = 0;
#pragma unroll
        for (int y = 0; y < CELL; ++y) {
            int s = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) s = dot2(col[y / 2 + i], t[5 * (y & 1) + i], s);
            const int yi = min(max((s + 2048) >> 12, 0), 255);
            const int diff = abs((int)((cur4[y / 4] >> (8 * (y & 3))) & 255u) - yi);
            sad += (y < ch && x < cw) ? (unsigned)diff : 0u;
        }
#pragma unroll
        for (int off = 8; off; off >>= 1) sad += __shfl_xor(sad, off);  // (the 16 lanes of a candidate are neighbours)
        if (item < ITEMS && x == 0) {
            const unsigned long long cnd = key_of(sad, 4 * dy + fyi - 3, 4 * dx + fxi - 3, p.lambda);
            key = cnd < key ? cnd : key;
        }
    }
    // ---- the minimum: inside the wave, then across the waves
    key = key_min_wave(key);
    if ((tid & 63) == 0) best[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < THREADS / 64; ++v) key = best[v] < key ? best[v] : key;
        p.mvq[2 * at] = (int16_t)key_vy(key);
        p.mvq[2 * at + 1] = (int16_t)key_vx(key);
        p.cost[at] = key_sad(key, p.lambda);
    }
}

__global__ __launch_bounds__(THREADS) void me_compensate_sub_kernel(const SubArgs p) {
    __shared__ float win[3][SWIN][SPITCH];  // ref: row = y - Y0 - iy + 3, column = x - X0 - ix + 3
    __shared__ float hz[3][SWIN][CELL];     // the horizontal pass of every staged row
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * CELL, Y0 = blockIdx.y * CELL;
    if (X0 >= p.W || Y0 >= p.H) return;  // (uniform across the workgroup)
    const int64_t at = (int64_t)blockIdx.y * p.wc + blockIdx.x;
    const int vy = __builtin_amdgcn_readfirstlane((int)p.mv[2 * at]), vx = __builtin_amdgcn_readfirstlane((int)p.mv[2 * at + 1]);
    if (((vy | vx) & 3) == 0) move_cell_whole(p, tid, Y0, X0, vy >> 2, vx >> 2);  // (uniform) a whole vector: the bits
    else move_block_frac<CELL>(p, tid, Y0, X0, vy, vx, win, hz, false);
}

}  // namespace

extern "C" int dcvc_me_refine(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps,
                              int32_t H, int32_t W, int32_t lambda, const int16_t *mv_in, int16_t *mvq, uint32_t *cost, void *stream) {
    if (!mv_in || !mvq || !cost || !size_ok(H, W) || !planes_ok(cur, cur_rs, cur_ps, H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) ||
        lambda < 0 || lambda > DCVC_ME_MAX_LAMBDA || !aligned(cur, 4) || !aligned(ref, 4) || !aligned(cost, 4) || !aligned(mv_in, 2) ||
        !aligned(mvq, 2))
        return DCVC_E_ARG;
    const int32_t wc = 4 * ((W + 63) / 64), hc = 4 * ((H + 63) / 64);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(mv_in), b0 = reinterpret_cast<uintptr_t>(mvq), span = (uintptr_t)4 * hc * wc;
    if (a0 < b0 + span && b0 < a0 + span) return DCVC_E_ARG;
    RefineArgs a{};
    a.cur = cur, a.ref = ref, a.mv_in = mv_in, a.mvq = mvq, a.cost = cost;
    a.cps = cur_ps, a.rps = ref_ps, a.crs = cur_rs, a.rrs = ref_rs, a.H = H, a.W = W, a.wc = wc, a.lambda = lambda;
    me_refine_kernel<<<dim3(wc, hc), THREADS, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_me_compensate_sub(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps,
                                      int32_t H, int32_t W, const int16_t *mvq, void *stream) {
    if (!mvq || !size_ok(H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) || !planes_ok(out, out_rs, out_ps, H, W) || !aligned(ref, 4) ||
        !aligned(out, 4) || !aligned(mvq, 2) || extents_overlap(out, out_rs, out_ps, ref, ref_rs, ref_ps, H, W))
        return DCVC_E_ARG;
    SubArgs a{};
    a.ref = ref, a.out = out, a.mv = mvq, a.rps = ref_ps, a.ops = out_ps, a.rrs = ref_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.rvec = vec_ok(ref, ref_rs, ref_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    me_compensate_sub_kernel<<<dim3((W + CELL - 1) / CELL, (H + CELL - 1) / CELL), THREADS, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
