// me.hip -- block motion search and motion compensation in front of the temporal noise prefilter
// (include/dcvc_hip_me.h, which states the arithmetic; this file only arranges it).
//
// me_search_kernel: a WORKGROUP owns one 16 x 16 cell.  Every luma is formed once: each thread loads its share of the
// (16 + 2R) x (16 + 4 NG) window of ref (NG = ceil((2R + 1) / 4) groups of four dx; the columns past dx = R belong to
// candidates that are thrown away) and of the cell of cur, every coordinate clamped to the picture BEFORE the load, so
// every read is inside the H x W crop; all loads of a thread are issued before the first code is formed; the codes go to
// LDS as bytes (at most 80 rows x 84 bytes of window, 256 bytes of cell).
//
// A LANE takes a candidate group: one dy and the four dx = -R + 4 k .. -R + 4 k + 3, whose windows start at a 4-byte
// boundary of the LDS row.  Per cell row it reads five words of window and the row's four quads of cur (one address for all
// lanes: a broadcast) and issues four v_qsad_pk_u16_u8: the SADs of a quad of cur against the four windows at consecutive
// byte offsets of a 64-bit source, accumulated as four uint16 (a cell's SAD is at most 255 * 256 = 65280).  A cell cut by
// the picture's edge sums its whole quads the same way and its last partial quad with v_alignbyte + v_sad_u8 on masked
// words.  The lane packs (J, |dy| + |dx|, dy + 32, dx + 32) into 17 + 7 + 7 + 7 bits and keeps the minimum; the minimum is
// folded with xor-shuffles inside a wave and through LDS across waves.  The lane that holds (0, 0) stores zero[cell].
// Nothing global is atomic, nothing is kept in scratch.
//
// The groups of a cell number (2R + 1) NG: 85 at R = 8, 297 at R = 16, 1105 at R = 32, so the kernel is instantiated for
// R <= 8 with 128 threads, R <= 16 with 320 and R <= 32 with 256 (the bound fixes the LDS tile and how many pixels a
// thread stages; R itself is a runtime value).
//
// me_compensate_kernel is a streaming gather tiled the way tnr_step_kernel is: a workgroup of 8 waves owns a strip of 16
// rows x 256 columns, a wave 2 rows, a lane 4 consecutive pixels (a quad, inside one cell); six loads, then six stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_me.h"
#include "kernel_common.h"
#include "roi_common.h"

namespace {

constexpr int CELL = DCVC_ROI_CELL, QUADS = CELL / 4, BIAS = DCVC_ME_MAX_R;
static_assert(CELL == 16 && BIAS == 32, "four quads a row; dy + 32 and dx + 32 fit 7 bits");

struct SearchArgs {
    const float *cur, *ref;
    int16_t *mv;
    uint32_t *cost, *zero;
    int64_t cps, rps;
    int32_t crs, rrs, H, W, wc, R, lambda;
};

template <int RMAX>
struct Shape {
    static constexpr int NG = (RMAX + 2) / 2;  // ceil((2 RMAX + 1) / 4)
    static constexpr int WH = CELL + 2 * RMAX, WW = CELL + 4 * NG, PITCH = (WW / 4) | 1;  // (words; odd: rows fall on other banks)
    static constexpr int THREADS = RMAX <= 8 ? 128 : RMAX <= 16 ? 320 : 256;
    static constexpr int PER = (WH * WW + THREADS - 1) / THREADS, CPER = (CELL * CELL + THREADS - 1) / THREADS;
};

__device__ __forceinline__ unsigned luma_of(const float (&v)[3]) { return (unsigned)luma8(code8(v[0]), code8(v[1]), code8(v[2])); }

__device__ __forceinline__ unsigned long long pack64(unsigned lo, unsigned hi) { return (unsigned long long)hi << 32 | lo; }

template <int RMAX>
__global__ __launch_bounds__(Shape<RMAX>::THREADS) void me_search_kernel(const SearchArgs p) {
    using S = Shape<RMAX>;
    __shared__ unsigned win[S::WH * S::PITCH];  // Y of ref, a byte per pixel: row = y - Y0 + R, byte = x - X0 + R
    __shared__ uint4 cell[CELL];                // Y of cur, a byte per pixel, a row per uint4
    __shared__ unsigned long long best[S::THREADS / 64];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * CELL, Y0 = blockIdx.y * CELL;
    const int64_t at = (int64_t)blockIdx.y * p.wc + blockIdx.x;
    if (X0 >= p.W || Y0 >= p.H) {  // (uniform across the workgroup) a cell of the padding holds no pixel
        if (tid == 0) p.mv[2 * at] = 0, p.mv[2 * at + 1] = 0, p.cost[at] = 0, p.zero[at] = 0;
        return;
    }
    const int R = p.R, ng = (R + 2) / 2, ww = CELL + 4 * ng, npix = (CELL + 2 * R) * ww;

    // ---- every load of the thread: its share of the window, then of the cell (a share past the end repeats the last pixel)
    float w[S::PER][3], c[S::CPER][3];
    int wat[S::PER];
#pragma unroll
    for (int i = 0; i < S::PER; ++i) {
        const int pix = min(i * S::THREADS + tid, npix - 1), wy = pix / ww, wx = pix - wy * ww;
        const int y = min(max(Y0 - R + wy, 0), p.H - 1), x = min(max(X0 - R + wx, 0), p.W - 1);
        wat[i] = wy * (4 * S::PITCH) + wx;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[i][k] = p.ref[k * p.rps + (int64_t)y * p.rrs + x];
    }
#pragma unroll
    for (int i = 0; i < S::CPER; ++i) {
        const int pix = min(i * S::THREADS + tid, CELL * CELL - 1);
        const int y = min(Y0 + pix / CELL, p.H - 1), x = min(X0 + pix % CELL, p.W - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i][k] = p.cur[k * p.cps + (int64_t)y * p.crs + x];
    }
    // ---- the codes, as bytes
#pragma unroll
    for (int i = 0; i < S::PER; ++i) reinterpret_cast<uint8_t *>(win)[wat[i]] = (uint8_t)luma_of(w[i]);
#pragma unroll
    for (int i = 0; i < S::CPER; ++i)
        reinterpret_cast<uint8_t *>(cell)[min(i * S::THREADS + tid, CELL * CELL - 1)] = (uint8_t)luma_of(c[i]);
    __syncthreads();

    // ---- the candidates
    const int ch = min(CELL, p.H - Y0), cw = min(CELL, p.W - X0), groups = (2 * R + 1) * ng;
    const int whole = cw >> 2, rest = cw & 3;
    const unsigned mask = (1u << (8 * rest)) - 1u;  // the bytes of the last quad that lie in the picture
    unsigned long long key = ~0ull;
    for (int g = tid; g < groups; g += S::THREADS) {
        const int dyi = g / ng, k = g - dyi * ng;
        const unsigned *row = win + dyi * S::PITCH + k;
        unsigned long long acc = 0;      // four SADs, uint16 each
        unsigned tail[4] = {0, 0, 0, 0};  // what the partial quad adds to them
        if (ch == CELL && cw == CELL) {   // (uniform across the workgroup)
#pragma unroll
            for (int y = 0; y < CELL; ++y) {
                const unsigned *r = row + y * S::PITCH;
                const unsigned r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
                const uint4 q = cell[y];
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r0, r1), q.x, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r1, r2), q.y, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r2, r3), q.z, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r3, r4), q.w, acc);
            }
        } else {
            const unsigned *words = reinterpret_cast<const unsigned *>(cell);
            for (int y = 0; y < ch; ++y) {
                const unsigned *r = row + y * S::PITCH;
                for (int q = 0; q < whole; ++q) acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r[q], r[q + 1]), words[y * QUADS + q], acc);
                if (rest) {
                    const unsigned lo = r[whole], hi = r[whole + 1], cq = words[y * QUADS + whole] & mask;
#pragma unroll
                    for (int i = 0; i < 4; ++i) tail[i] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, i) & mask, cq, tail[i]);
                }
            }
        }
        const int dy = dyi - R, ady = abs(dy);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = 4 * k + i - R;
            if (dx > R) continue;  // (the last group's columns past the search range)
            const unsigned sad = ((unsigned)(acc >> (16 * i)) & 0xffffu) + tail[i], len = (unsigned)(ady + abs(dx));
            const unsigned J = sad + (unsigned)p.lambda * len;
            const unsigned long long cand = (unsigned long long)J << 21 | (unsigned long long)(len << 14 | (unsigned)(dy + BIAS) << 7 | (unsigned)(dx + BIAS));
            key = cand < key ? cand : key;
            if (dy == 0 && dx == 0) p.zero[at] = sad;  // (one lane of the workgroup)
        }
    }
    // ---- the minimum: inside the wave, then across the waves
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
    }
    if ((tid & 63) == 0) best[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < S::THREADS / 64; ++v) key = best[v] < key ? best[v] : key;
        const unsigned len = (unsigned)(key >> 14) & 127u;
        p.mv[2 * at] = (int16_t)((int)((key >> 7) & 127u) - BIAS);
        p.mv[2 * at + 1] = (int16_t)((int)(key & 127u) - BIAS);
        p.cost[at] = (unsigned)(key >> 21) - (unsigned)p.lambda * len;
    }
}

constexpr int TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, WAVES = 8, ROWS = 2;
static_assert(TILE_W == 64 * 4 && ROWS * WAVES == CELL, "a lane per quad, a wave per two rows");

struct CompArgs {
    const float *ref;
    float *out;
    const int16_t *mv;
    int64_t rps, ops;
    int32_t rrs, ors, H, W, wc, rvec, ovec;
};

__global__ __launch_bounds__(64 * WAVES) void me_compensate_kernel(const CompArgs p) {
    const int x0 = blockIdx.x * TILE_W + threadIdx.x * 4, y0 = blockIdx.y * CELL + threadIdx.y * ROWS;
    if (x0 >= p.W || y0 >= p.H) return;  // (no barrier below)
    const int64_t at = (int64_t)blockIdx.y * p.wc + (x0 >> 4);
    const int dy = p.mv[2 * at], dx = p.mv[2 * at + 1], sx = x0 + dx;
    const bool rv = p.rvec && (dx & 3) == 0 && sx >= 0 && sx + 4 <= p.W, ov = p.ovec && x0 + 4 <= p.W;
    float v[ROWS][3][4];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int sy = min(max(min(y0 + i, p.H - 1) + dy, 0), p.H - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *row = p.ref + k * p.rps + (int64_t)sy * p.rrs;
            if (rv) {
                const float4 t = *reinterpret_cast<const float4 *>(row + sx);
                v[i][k][0] = t.x, v[i][k][1] = t.y, v[i][k][2] = t.z, v[i][k][3] = t.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[i][k][q] = row[min(max(sx + q, 0), p.W - 1)];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (y0 + i >= p.H) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float *row = p.out + k * p.ops + (int64_t)(y0 + i) * p.ors + x0;
            if (ov) {
                *reinterpret_cast<float4 *>(row) = make_float4(v[i][k][0], v[i][k][1], v[i][k][2], v[i][k][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) row[q] = v[i][k][q];
            }
        }
    }
}

template <int RMAX>
void launch_search(const SearchArgs &a, hipStream_t stream) {
    const dim3 grid(a.wc, 4 * ((a.H + 63) / 64));
    me_search_kernel<RMAX><<<grid, Shape<RMAX>::THREADS, 0, stream>>>(a);
}

}  // namespace

extern "C" int dcvc_me_search(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref, int32_t ref_rs, int64_t ref_ps,
                              int32_t H, int32_t W, int32_t R, int32_t lambda, int16_t *mv, uint32_t *cost, uint32_t *zero,
                              void *stream) {
    if (!mv || !cost || !zero || !size_ok(H, W) || !planes_ok(cur, cur_rs, cur_ps, H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) ||
        R < 1 || R > DCVC_ME_MAX_R || lambda < 0 || lambda > DCVC_ME_MAX_LAMBDA || !aligned(cur, 4) || !aligned(ref, 4) ||
        !aligned(cost, 4) || !aligned(zero, 4) || !aligned(mv, 2))
        return DCVC_E_ARG;
    SearchArgs a{};
    a.cur = cur, a.ref = ref, a.mv = mv, a.cost = cost, a.zero = zero;
    a.cps = cur_ps, a.rps = ref_ps, a.crs = cur_rs, a.rrs = ref_rs, a.H = H, a.W = W, a.wc = 4 * ((W + 63) / 64), a.R = R, a.lambda = lambda;
    if (R <= 8)
        launch_search<8>(a, (hipStream_t)stream);
    else if (R <= 16)
        launch_search<16>(a, (hipStream_t)stream);
    else
        launch_search<32>(a, (hipStream_t)stream);
    RET_LAUNCH();
}

extern "C" int dcvc_me_compensate(const float *ref, int32_t ref_rs, int64_t ref_ps, float *out, int32_t out_rs, int64_t out_ps,
                                  int32_t H, int32_t W, const int16_t *mv, void *stream) {
    if (!mv || !size_ok(H, W) || !planes_ok(ref, ref_rs, ref_ps, H, W) || !planes_ok(out, out_rs, out_ps, H, W) || !aligned(ref, 4) ||
        !aligned(out, 4) || !aligned(mv, 2) || extents_overlap(out, out_rs, out_ps, ref, ref_rs, ref_ps, H, W))
        return DCVC_E_ARG;
    CompArgs a{};
    a.ref = ref, a.out = out, a.mv = mv, a.rps = ref_ps, a.ops = out_ps, a.rrs = ref_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.rvec = vec_ok(ref, ref_rs, ref_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    const dim3 block(64, WAVES), grid(nblk(a.wc, TILE_CELLS), 4 * ((H + 63) / 64));
    me_compensate_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
