// grain.hip -- film-grain synthesis: the encoder's measurement and the decoder's synthesis (include/dcvc_hip_grain.h, which
// states the arithmetic; this file only arranges it).
//
// Both kernels are streaming passes bound by memory, 24 bytes a pixel each (measure reads src and flt; apply reads in and
// writes out), and both take the strip shape of tnr_step_kernel: a WORKGROUP of 8 waves owns 16 rows x 256 columns, the 16
// adjacent cells of one cell row; a WAVE takes 2 consecutive rows of the strip, a lane 4 consecutive pixels of each.  Lane
// bits: 0-1 the quad inside the cell, 2-5 the cell.  A quad is read or written as one 16-byte access when the picture's
// base and strides allow it and the quad is whole; anything else goes element by element through the same arithmetic.
// Every coordinate is clamped to the picture BEFORE a load, so every read is inside the H x W crop.
//
// grain_measure_kernel: pairs never leave a cell, so there is no halo.  e of the strip goes to LDS as int16 (16 x 256),
// from where a lane takes its right neighbour's first column and the row below its own.  The sums: per bin that any lane
// of the wave holds (a ballot), the lane's 8 pixels are folded in registers and the 64 lanes with wave_sum, lane 0 adds
// the wave's four sums to the workgroup's 32 words in LDS (int32: a strip's sum of e^2 is at most 4096 * 255^2 < 2^28),
// and after a barrier 32 threads issue ONE 64-bit vector atomic add each for the words that gained something.  Integer
// sums: exact, and independent of the order the workgroups arrive in.
//
// grain_apply_kernel: the white field g of the strip plus a one-pixel ring, 18 rows x 258 columns, goes to LDS as int16
// (a row is 264 words: the strip's quads start 8-byte aligned at word 4, the ring's columns are words 3 and 260) -- one
// hash pair per position, not nine.  A lane hashes its own 2 x 4 positions; the ring's 2 * 258 + 2 * 16 = 548 positions
// go round the 512 threads.  After one barrier a lane forms the horizontal sums of its 4 rows x 4 columns and from them
// n of its 2 x 4 pixels.  LDS: 18 * 264 * 2 + 512 = 10016 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_grain.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, WAVES = 8, ROWS = 2;
constexpr int G_ROWS = CELL + 2, G_STRIDE = TILE_W + 8, RING = 2 * (TILE_W + 2) + 2 * CELL;
static_assert(CELL == 16 && TILE_W == 64 * 4 && ROWS * WAVES == CELL, "a lane per quad, a wave per two rows");
static_assert(RING <= 2 * 64 * WAVES, "the ring goes round the threads at most twice");

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

__device__ __forceinline__ int wave_sum_i(int v) { return (int)wave_sum((unsigned)v); }

// ---------------------------------------------------------------------------------------------------------------- measure
struct MeasureArgs {
    const float *src, *flt;
    const uint16_t *held;
    unsigned long long *acc;
    int64_t sps, fps;
    int32_t srs, frs, H, W, wc, svec, fvec;
};

__global__ __launch_bounds__(64 * WAVES) void grain_measure_kernel(const MeasureArgs p) {
    __shared__ int16_t E[CELL + 1][TILE_W + 4];  // e of the strip; row 16 and columns 256 .. 259 are never a pair's partner
    __shared__ int sums[DCVC_GRAIN_WORDS];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * CELL, x0 = X0 + lane * 4, y0 = Y0 + wave * ROWS;
    if (X0 >= p.W || Y0 >= p.H) return;  // (uniform across the workgroup) a strip of the padding
    const int col = blockIdx.x * TILE_CELLS + (lane >> 2);
    // the lane's cell takes part: it holds a pixel, and every pixel it holds was blended
    const int in_h = min(CELL, p.H - Y0), in_w = min(CELL, p.W - col * CELL);
    const bool full = in_w > 0 && (int)p.held[(int64_t)blockIdx.y * p.wc + col] == in_h * in_w;
    if (tid < DCVC_GRAIN_WORDS) sums[tid] = 0;

    const bool whole = x0 + 4 <= p.W, sv = p.svec && whole, fv = p.fvec && whole;
    int e[ROWS][4], bin[ROWS][4];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int y = min(y0 + i, p.H - 1);
        float s[3][4] = {}, f[3][4] = {};
        if (full) {  // (a cell that stays out is not read)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                load_quad(p.src + k * p.sps + (int64_t)y * p.srs, x0, p.W, sv, s[k]);
                load_quad(p.flt + k * p.fps + (int64_t)y * p.frs, x0, p.W, fv, f[k]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = full && x0 + q < p.W && y0 + i < p.H;
            const int yf = in ? luma8(code8(f[0][q]), code8(f[1][q]), code8(f[2][q])) : 0;
            e[i][q] = in ? luma8(code8(s[0][q]), code8(s[1][q]), code8(s[2][q])) - yf : 0;
            bin[i][q] = in ? yf >> 5 : -1;  // (-1: the pixel is in no bin)
            E[wave * ROWS + i][lane * 4 + q] = (int16_t)e[i][q];
        }
    }
    __syncthreads();

    // e * e_right and e * e_below of the lane's pixels; a partner outside the cell or the picture gives no product.  (A
    // partner inside the cell and the picture belongs to the same cell, so it was formed above whenever p was.)
    int pr[ROWS][4], pb[ROWS][4];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int r = wave * ROWS + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cx = lane * 4 + q;
            const bool right = ((cx + 1) & (CELL - 1)) != 0 && x0 + q + 1 < p.W;
            const bool below = r + 1 < CELL && y0 + i + 1 < p.H;
            pr[i][q] = right ? e[i][q] * (q < 3 ? e[i][q + 1] : (int)E[r][cx + 1]) : 0;
            pb[i][q] = below ? e[i][q] * (i + 1 < ROWS ? e[i + 1][q] : (int)E[r + 1][cx]) : 0;
        }
    }

    unsigned present = 0;  // the bins the lane's pixels fall in
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) present |= bin[i][q] >= 0 ? 1u << bin[i][q] : 0u;
    for (int b = 0; b < DCVC_GRAIN_BINS; ++b) {
        if (__ballot((present >> b) & 1u) == 0ull) continue;  // (uniform across a wave)
        int n = 0, s2 = 0, sr = 0, sb = 0;
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool mine = bin[i][q] == b;
                n += mine ? 1 : 0, s2 += mine ? e[i][q] * e[i][q] : 0, sr += mine ? pr[i][q] : 0, sb += mine ? pb[i][q] : 0;
            }
        n = wave_sum_i(n), s2 = wave_sum_i(s2), sr = wave_sum_i(sr), sb = wave_sum_i(sb);
        if (lane == 0) {
            atomicAdd(&sums[4 * b + 0], n), atomicAdd(&sums[4 * b + 1], s2);
            atomicAdd(&sums[4 * b + 2], sr), atomicAdd(&sums[4 * b + 3], sb);
        }
    }
    __syncthreads();
    if (tid < DCVC_GRAIN_WORDS && sums[tid] != 0)  // (two's complement: a negative sum is added as its 64-bit pattern)
        atomicAdd(&p.acc[tid], (unsigned long long)(long long)sums[tid]);
}

// ------------------------------------------------------------------------------------------------------------------ apply
struct ApplyArgs {
    const float *in;
    float *out;
    const uint16_t *stab;
    int64_t ips, ops;
    int32_t irs, ors, H, W, kh, kv, ivec, ovec;
    uint32_t key;
};

__host__ __device__ inline uint32_t fmix(uint32_t h) {
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    return h;
}

__device__ __forceinline__ int bytes_of(uint32_t w) { return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)); }

// g at the picture position (y, x), y >= -1, x >= -1 (a position beyond H or W is hashed like any other and never used)
__device__ __forceinline__ int white(int y, int x, uint32_t key) {
    const uint32_t w0 = fmix((((uint32_t)(y + 1) << 16) | ((uint32_t)(x + 1) & 0xffffu)) ^ key), w1 = fmix(w0 ^ 0x9e3779b9u);
    return bytes_of(w0) + bytes_of(w1) - 1020;
}

__global__ __launch_bounds__(64 * WAVES) void grain_apply_kernel(const ApplyArgs p) {
    __shared__ int16_t G[G_ROWS][G_STRIDE];  // g: row = strip row + 1, word = strip column + 4
    __shared__ uint16_t tab[256];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * CELL, x0 = X0 + lane * 4, y0 = Y0 + wave * ROWS;
    if (X0 >= p.W || Y0 >= p.H) return;  // (uniform across the workgroup) a strip of the padding
    const bool whole = x0 + 4 <= p.W, iv = p.ivec && whole, ov = p.ovec && whole;

    float c[ROWS][3][4];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int y = min(y0 + i, p.H - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) load_quad(p.in + k * p.ips + (int64_t)y * p.irs, x0, p.W, iv, c[i][k]);
    }
    if (tid < 256) tab[tid] = p.stab[tid];

    // ---- the white field: the lane's own positions, then its share of the ring
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) G[wave * ROWS + i + 1][lane * 4 + 4 + q] = (int16_t)white(y0 + i, x0 + q, p.key);
    for (int r = tid; r < RING; r += 64 * WAVES) {
        int ry, rx;  // strip row -1 .. 16, strip column -1 .. 256
        if (r < 2 * (TILE_W + 2))
            ry = r < TILE_W + 2 ? -1 : CELL, rx = (r < TILE_W + 2 ? r : r - (TILE_W + 2)) - 1;
        else
            ry = (r - 2 * (TILE_W + 2)) >> 1, rx = (r & 1) ? TILE_W : -1;
        G[ry + 1][rx + 4] = (int16_t)white(Y0 + ry, X0 + rx, p.key);
    }
    __syncthreads();

    // ---- the shape: horizontal sums of rows -1 .. 2 of the lane's two, then the vertical taps
    int hs[ROWS + 2][4];
#pragma unroll
    for (int j = 0; j < ROWS + 2; ++j) {
        const int16_t *row = &G[wave * ROWS + j][lane * 4 + 3];  // (strip row 2 wave + j - 1; word 3 is strip column 4 lane - 1)
        int g[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) g[m] = row[m];
#pragma unroll
        for (int q = 0; q < 4; ++q) hs[j][q] = p.kh * (g[q] + g[q + 2]) + DCVC_GRAIN_CENTRE * g[q + 1];
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (y0 + i >= p.H) break;  // (uniform across a wave)
        float o[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = p.kv * (hs[i][q] + hs[i + 2][q]) + DCVC_GRAIN_CENTRE * hs[i + 1][q];
            const int s = tab[luma8(code8(c[i][0][q]), code8(c[i][1][q]), code8(c[i][2][q]))];
            const long long D = ((long long)n * s + (1ll << (DCVC_GRAIN_SHIFT - 1))) >> DCVC_GRAIN_SHIFT;
            const float d = (float)(int)D * (1.0f / 4080.0f);
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k][q] = s == 0 ? c[i][k][q] : fminf(fmaxf(c[i][k][q] + d, 0.0f), 1.0f);
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
}

}  // namespace

extern "C" int dcvc_grain_measure(const float *src, int32_t src_rs, int64_t src_ps, const float *flt, int32_t flt_rs, int64_t flt_ps,
                                  int32_t H, int32_t W, const uint16_t *held, int64_t *acc, void *stream) {
    if (!held || !acc || !size_ok(H, W) || !planes_ok(src, src_rs, src_ps, H, W) || !planes_ok(flt, flt_rs, flt_ps, H, W) ||
        !aligned(src, 4) || !aligned(flt, 4) || !aligned(held, 2) || !aligned(acc, 8))
        return DCVC_E_ARG;
    MeasureArgs a{};
    a.src = src, a.flt = flt, a.held = held, a.acc = reinterpret_cast<unsigned long long *>(acc);
    a.sps = src_ps, a.fps = flt_ps, a.srs = src_rs, a.frs = flt_rs, a.H = H, a.W = W, a.wc = 4 * ((W + 63) / 64);
    a.svec = vec_ok(src, src_rs, src_ps), a.fvec = vec_ok(flt, flt_rs, flt_ps);
    const dim3 block(64, WAVES), grid(nblk(W, TILE_W), nblk(H, CELL));
    grain_measure_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_grain_apply(const float *in, int32_t in_rs, int64_t in_ps, float *out, int32_t out_rs, int64_t out_ps, int32_t H,
                                int32_t W, int32_t t, int32_t kh, int32_t kv, const uint16_t *stab, void *stream) {
    if (!stab || !size_ok(H, W) || !planes_ok(in, in_rs, in_ps, H, W) || !planes_ok(out, out_rs, out_ps, H, W) || !aligned(in, 4) ||
        !aligned(out, 4) || !aligned(stab, 2) || kh < -DCVC_GRAIN_MAX_TAP || kh > DCVC_GRAIN_MAX_TAP || kv < -DCVC_GRAIN_MAX_TAP ||
        kv > DCVC_GRAIN_MAX_TAP || t < 0 || extents_overlap(out, out_rs, out_ps, in, in_rs, in_ps, H, W))
        return DCVC_E_ARG;
    ApplyArgs a{};
    a.in = in, a.out = out, a.stab = stab, a.ips = in_ps, a.ops = out_ps, a.irs = in_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.kh = kh, a.kv = kv, a.key = fmix((uint32_t)t ^ 0x9e3779b9u);
    a.ivec = vec_ok(in, in_rs, in_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    const dim3 block(64, WAVES), grid(nblk(W, TILE_W), nblk(H, CELL));
    grain_apply_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
