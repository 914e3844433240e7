// mesub_common.h -- what mesub.hip and mesplit.hip share: the interpolation filters of include/dcvc_hip_mesub.h in their
// integer and fp32 forms, the luma of a sample, the packed key of a candidate and its minimum across a workgroup, and the two
// ways a block of pixels is moved by ONE quarter-pel vector (a copy of bits, or the fp32 folds through LDS).  Written once:
// the arithmetic of both files is this.
#ifndef DCVC_MESUB_COMMON_H
#define DCVC_MESUB_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip_mesub.h"
#include "roi_common.h"

#pragma clang fp contract(off)  // (the fp32 folds are part of the interface: every product and every sum rounded)

namespace {

constexpr int CELL = DCVC_ROI_CELL, THREADS = 256, NF = 7, NT = 9, BIAS = 256;
static_assert(CELL == 16 && THREADS == CELL * CELL && DCVC_MESUB_UNIT == 4, "a thread per pixel; quarter pixels");
static_assert(4 * DCVC_ME_MAX_R + 3 < BIAS, "vy + 256 and vx + 256 fit 9 bits");

// the filter of f = -3 .. 3 over the whole offsets -4 .. +4 around d; row 3 + p, entries 1 .. 8, is the filter of the
// phase p over the offsets -3 .. +4
__constant__ int TAP9[NF][NT] = {{-1, 4, -10, 58, 17, -5, 1, 0, 0}, {-1, 4, -11, 40, 40, -11, 4, -1, 0}, {0, 1, -5, 17, 58, -10, 4, -1, 0},
                                 {0, 0, 0, 0, 64, 0, 0, 0, 0},
                                 {0, -1, 4, -10, 58, 17, -5, 1, 0}, {0, -1, 4, -11, 40, 40, -11, 4, -1}, {0, 0, 1, -5, 17, 58, -10, 4, -1}};

__device__ __forceinline__ unsigned luma_of(const float (&v)[3]) { return (unsigned)luma8(code8(v[0]), code8(v[1]), code8(v[2])); }

typedef short short2v __attribute__((ext_vector_type(2)));

// the sum of two int16 products on top of acc: one v_dot2_i32_i16
__device__ __forceinline__ int dot2(unsigned a, unsigned b, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), acc, false);
}

__device__ __forceinline__ unsigned pair16(int lo, int hi) { return ((unsigned)lo & 0xffffu) | (unsigned)hi << 16; }

// (J, |vy| + |vx|, vy + 256, vx + 256) in 19 + 9 + 9 + 9 bits: unsigned order is the key's order
__device__ __forceinline__ unsigned long long key_of(unsigned sad, int vy, int vx, int lambda) {
    const unsigned len = (unsigned)(abs(vy) + abs(vx)), J = 4u * sad + (unsigned)lambda * len;
    return (unsigned long long)J << 27 | (unsigned long long)(len << 18 | (unsigned)(vy + BIAS) << 9 | (unsigned)(vx + BIAS));
}
__device__ __forceinline__ int key_vy(unsigned long long key) { return (int)((key >> 9) & 511u) - BIAS; }
__device__ __forceinline__ int key_vx(unsigned long long key) { return (int)(key & 511u) - BIAS; }
__device__ __forceinline__ unsigned key_sad(unsigned long long key, int lambda) {
    return ((unsigned)(key >> 27) - (unsigned)lambda * ((unsigned)(key >> 18) & 511u)) >> 2;
}
// the smallest key of a wave, in every lane
__device__ __forceinline__ unsigned long long key_min_wave(unsigned long long key) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
    }
    return key;
}

// the filters of the phases 1 .. 3 as (first offset, taps, tap / 64): phase 0 is the identity and has no row here
__constant__ int FIRST[4] = {0, -3, -3, -2}, COUNT[4] = {1, 7, 8, 7};
__constant__ float TAPF[4][8] = {{1.0f, 0, 0, 0, 0, 0, 0, 0},
                                 {-1 / 64.0f, 4 / 64.0f, -10 / 64.0f, 58 / 64.0f, 17 / 64.0f, -5 / 64.0f, 1 / 64.0f, 0},
                                 {-1 / 64.0f, 4 / 64.0f, -11 / 64.0f, 40 / 64.0f, 40 / 64.0f, -11 / 64.0f, 4 / 64.0f, -1 / 64.0f},
                                 {1 / 64.0f, -5 / 64.0f, 17 / 64.0f, 58 / 64.0f, -10 / 64.0f, 4 / 64.0f, -1 / 64.0f, 0}};
constexpr int SWIN = CELL + 7, SPITCH = SWIN + 1, LEAD = 3;  // samples at offsets -3 .. +4 around the 16 pixels

struct SubArgs {
    const float *ref;
    float *out;
    const int16_t *mv;
    int64_t rps, ops;
    int32_t rrs, ors, H, W, wc, rvec, ovec;
};

// The cell at (Y0, X0) moved by a WHOLE vector (iy, ix) pixels: the bits, a quad of four pixels of one plane a lane (192 of
// the 256), one 16-byte access where the bases, the strides and the vector allow it.
__device__ __forceinline__ void move_cell_whole(const SubArgs &p, int tid, int Y0, int X0, int iy, int ix) {
    const int k = tid >> 6, y = Y0 + ((tid & 63) >> 2), x0 = X0 + 4 * (tid & 3);
    if (k >= 3 || y >= p.H || x0 >= p.W) return;
    const int sy = min(max(y + iy, 0), p.H - 1), sx = x0 + ix;
    const bool rv = p.rvec && (ix & 3) == 0 && sx >= 0 && sx + 4 <= p.W, ov = p.ovec && x0 + 4 <= p.W;
    const float *src = p.ref + k * p.rps + (int64_t)sy * p.rrs;
    float *dst = p.out + k * p.ops + (int64_t)y * p.ors + x0;
    float v[4];
    if (rv) {
        const float4 t = *reinterpret_cast<const float4 *>(src + sx);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = src[min(max(sx + q, 0), p.W - 1)];
    }
    if (ov) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x0 + q < p.W) dst[q] = v[q];
    }
}

// The N x N block at (Y0, X0) moved by a vector with a fractional component, by the WHOLE workgroup (every thread comes
// here: three barriers).  The (N + 7)^2 samples around the block (taps -3 .. +4) of the three planes are staged in LDS,
// coordinates clamped before the load, the horizontal pass of every staged row goes into LDS and the vertical pass is per
// pixel, a thread a pixel.  The last barrier lets the next call stage again.
template <int N>
__device__ __forceinline__ void move_block_frac(const SubArgs &p, int tid, int Y0, int X0, int vy, int vx, float (&win)[3][SWIN][SPITCH],
                                                float (&hz)[3][SWIN][CELL], bool again) {
    constexpr int WN = N + 7;
    const int iy = vy >> 2, py = vy & 3, ix = vx >> 2, px = vx & 3;
    // ---- the samples around the block, coordinates clamped before the load
    for (int o = tid; o < 3 * WN * WN; o += THREADS) {
        const int k = o / (WN * WN), rest = o - k * (WN * WN), r = rest / WN, cc = rest - r * WN;
        const int y = min(max(Y0 + iy - LEAD + r, 0), p.H - 1), x = min(max(X0 + ix - LEAD + cc, 0), p.W - 1);
        win[k][r][cc] = p.ref[k * p.rps + (int64_t)y * p.rrs + x];
    }
    __syncthreads();
    // ---- horizontal: the identity at phase 0, else the fold in increasing offset
    const int hfirst = LEAD + FIRST[px], hn = COUNT[px];
    for (int o = tid; o < 3 * WN * N; o += THREADS) {
        const int k = o / (WN * N), rest = o - k * (WN * N), r = rest / N, x = rest % N;
        const float *s = &win[k][r][x + hfirst];
        float a = s[0];
        if (px != 0) {
            a = TAPF[px][0] * s[0];
            for (int j = 1; j < hn; ++j) a = a + TAPF[px][j] * s[j];
        }
        hz[k][r][x] = a;
    }
    __syncthreads();
    // ---- vertical, a thread a pixel
    const int yy = tid / N, xx = tid % N;
    if (tid < N * N && Y0 + yy < p.H && X0 + xx < p.W) {
        const int vfirst = LEAD + FIRST[py], vn = COUNT[py];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float a = hz[k][yy + vfirst][xx];
            if (py != 0) {
                a = TAPF[py][0] * a;
                for (int j = 1; j < vn; ++j) a = a + TAPF[py][j] * hz[k][yy + vfirst + j][xx];
            }
            a = fminf(fmaxf(a, 0.0f), 1.0f);
            p.out[k * p.ops + (int64_t)(Y0 + yy) * p.ors + X0 + xx] = a == 0.0f ? 0.0f : a;  // (a zero of either sign is +0)
        }
    }
    if (again) __syncthreads();
}

}  // namespace
#endif
