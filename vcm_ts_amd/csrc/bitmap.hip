// bitmap.hip -- per-cell bit maps (include/dcvc_hip_bits.h): the code length of every symbol the rANS coder is about to
// write, looked up in a host-built integer cost array and summed per latent position; and the sums of those maps over
// labelled regions of the 16-pixel cell grid.  Integers only: no logarithm, no float, no order of summation.
//
// These are small launches (a 1080p picture has 68 x 120 cells and ~0.8 M symbols) where latency counts, not bandwidth:
// the planes are (n, k, y, x), so the 64 lanes of a wave read 64 consecutive positions of one channel plane (coalesced),
// the four waves of a workgroup take every fourth channel, and LDS adds the four partial sums.  No atomics on memory.
// The ladder sweep (further down) is the one kernel here that divides: two fp32 divisions per element and candidate,
// integers after them, one 64-bit integer atomic per workgroup and candidate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip_bits.h"
#include "kernel_common.h"

namespace {

constexpr int CELLS = 64;   // positions per workgroup (one per lane of a wave)
constexpr int SLICES = 4;   // channel slices per workgroup (one wave each)

struct Table {
    const int32_t *cost, *sizes, *offsets;
    int32_t n_rows, stride;
};

// cost of one symbol in 2^-16 bit; a row that cannot be addressed costs 0 and sets `bad`
// (__host__ too, like position_cost and region_term below: plain integer code that a host program can step through)
__host__ __device__ inline int32_t symbol_cost(const Table &t, int32_t row, int32_t sym, int &bad) {
    if ((uint32_t)row >= (uint32_t)t.n_rows) {
        bad = 1;
        return 0;
    }
    const int32_t size = t.sizes[row];
    if (size < 2 || size > t.stride) {
        bad = 1;
        return 0;
    }
    const int32_t sentinel = size - 2;
    const int64_t v = (int64_t)sym - t.offsets[row];
    const int32_t *c = t.cost + (size_t)row * t.stride;
    if (v >= 0 && v < sentinel) return c[v];
    const uint32_t raw = v < 0 ? (uint32_t)(-2 * v - 1) : (uint32_t)(2 * (v - sentinel));
    const int32_t nib = raw ? (32 - __builtin_clz(raw) + 3) >> 2 : 0;
    return c[sentinel] + 4 * DCVC_BITS_UNIT * (1 + nib);
}

// planes of sample n at position pos, channels k0, k0 + step, ...: the sum of their symbols' costs
__host__ __device__ inline int32_t position_cost(const int32_t *__restrict__ sym0, const int32_t *__restrict__ idx0,
                                                 const int32_t *__restrict__ sym1, const int32_t *__restrict__ idx1,
                                                 const Table &t, int P, int HW, size_t n, int pos, int k0, int step, int &bad) {
    int32_t acc = 0;
    for (int k = k0; k < P; k += step) {
        const size_t i = (n * P + k) * HW + pos;
        acc += symbol_cost(t, idx0 ? idx0[i] : k, sym0[i], bad);
        if (sym1) acc += symbol_cost(t, idx1[i], sym1[i], bad);
    }
    return acc;
}

// grid (ceil(HW / CELLS), N), block (CELLS, SLICES).  planes: P channel planes of HW entries per sample in each of
// sym0 / sym1 (sym1 absent for the factorised kind); idx NULL: the row is the channel.
__global__ __launch_bounds__(CELLS * SLICES) void bits_map_kernel(const int32_t *__restrict__ sym0,
                                                                   const int32_t *__restrict__ idx0,
                                                                   const int32_t *__restrict__ sym1,
                                                                   const int32_t *__restrict__ idx1, const Table t,
                                                                   int32_t *__restrict__ map, int P, int HW,
                                                                   int32_t *__restrict__ status) {
    __shared__ int32_t part[SLICES][CELLS];
    const int lane = threadIdx.x, slice = threadIdx.y;
    const int pos = blockIdx.x * CELLS + lane;
    const size_t n = blockIdx.y;
    int bad = 0;
    part[slice][lane] = pos < HW ? position_cost(sym0, idx0, sym1, idx1, t, P, HW, n, pos, slice, SLICES, bad) : 0;
    __syncthreads();
    if (slice == 0 && pos < HW) {
        int32_t s = part[0][lane];
#pragma unroll
        for (int j = 1; j < SLICES; ++j) s += part[j][lane];
        map[n * HW + pos] = s;
    }
    if (bad) atomicOr(status, DCVC_BITS_BAD_INDEX);
}

struct Maps {
    const int32_t *m[4];  // mv_z, mv_y, z, y
};

// what cell p = (i, j) of sample n adds to component c of its label, in 2^-20 bit: 16 x a y-type map's entry, or the
// entry of the z-type element that covers the cell
__host__ __device__ inline long long region_term(const Maps &maps, int c, size_t n, int p, int hc, int wc) {
    if (c & 1) return 16ll * maps.m[c][n * hc * wc + p];
    const int i = p / wc, j = p - i * wc, zw = wc >> 2;
    return (long long)maps.m[c][n * (hc >> 2) * zw + (i >> 2) * zw + (j >> 2)];
}

// one workgroup per sample; the K * 4 sums live in LDS (64-bit integer adds: exact, any order)
__global__ __launch_bounds__(256) void bits_regions_kernel(const Maps maps, const uint8_t *__restrict__ labels, int K,
                                                           int64_t *__restrict__ sums, int hc, int wc,
                                                           int32_t *__restrict__ status) {
    __shared__ unsigned long long acc[DCVC_BITS_MAX_LABELS * 4];
    const int t = threadIdx.x;
    const size_t n = blockIdx.x;
    if (t < DCVC_BITS_MAX_LABELS * 4) acc[t] = 0ull;
    __syncthreads();
    const int cells = hc * wc;
    int bad = 0;
    for (int p = t; p < cells; p += 256) {
        const int label = labels[n * cells + p];
        if (label >= K) {
            bad = 1;
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!maps.m[c]) continue;
            const long long v = region_term(maps, c, n, p, hc, wc);
            if (v) atomicAdd(&acc[label * 4 + c], (unsigned long long)v);  // (two's complement: the signed add)
        }
    }
    __syncthreads();
    if (t < K * 4) sums[n * K * 4 + t] = (int64_t)acc[t];
    if (bad) atomicOr(status, DCVC_BITS_BAD_LABEL);
}

// ---- the ladder sweep ------------------------------------------------------------------------------------------------
// What the symbols of a scale-coded latent would cost if the quantisation step were f times as large and the prior
// rescaled with it, for up to DCVC_BITS_MAX_LADDER factors at once.  The planes are dense NHWC, so consecutive lanes
// read consecutive elements; each lane keeps one int32 sum per factor over its SWEEP_ITEMS elements (a symbol costs
// less than 2^22 units, so a wave's sum stays below 2^31), the wave adds them by shuffles, the four waves meet in LDS
// and the workgroup makes ONE 64-bit integer add per factor to est (zeroed by the entry point; integer adds have no
// order).  Two correctly rounded fp32 divisions per element and factor; everything after them is integer.
constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_ITEMS = 4;
constexpr int SWEEP_WAVES = SWEEP_THREADS / 64;

struct Factors {
    float f[DCVC_BITS_MAX_LADDER];
};

// grid (ceil(per / (SWEEP_THREADS * SWEEP_ITEMS)), N), block SWEEP_THREADS; per = H * W * C elements per sample
__global__ __launch_bounds__(SWEEP_THREADS) void bits_sweep_kernel(const float *__restrict__ res,
                                                                   const float *__restrict__ sc,
                                                                   const float *__restrict__ edges_g, const Factors fac,
                                                                   const int K, const Table t,
                                                                   unsigned long long *__restrict__ est, const int64_t per,
                                                                   int32_t *__restrict__ status) {
    __shared__ float edges[256];
    __shared__ int32_t part[SWEEP_WAVES][DCVC_BITS_MAX_LADDER];
    const int tid = threadIdx.x;
    edges[tid] = edges_g[tid];
    __syncthreads();
    const size_t n = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * (SWEEP_THREADS * SWEEP_ITEMS) + tid;
    int32_t acc[DCVC_BITS_MAX_LADDER];
#pragma unroll
    for (int k = 0; k < DCVC_BITS_MAX_LADDER; ++k) acc[k] = 0;
    int bad_index = 0, bad_value = 0;
#pragma unroll
    for (int j = 0; j < SWEEP_ITEMS; ++j) {
        const int64_t i = base + (int64_t)j * SWEEP_THREADS;
        if (i >= per) break;
        const float r = res[n * per + i], s = sc[n * per + i];
        // not finite (a NaN compares false), or a symbol that is no int32 for one of the factors: the element costs
        // nothing for EVERY factor, so that the sums stay comparable with each other
        bool ok = fabsf(r) <= 3.402823466e38f && fabsf(s) <= 3.402823466e38f;
        float q[DCVC_BITS_MAX_LADDER];
#pragma unroll
        for (int k = 0; k < DCVC_BITS_MAX_LADDER; ++k) {
            q[k] = k < K ? r / fac.f[k] : 0.f;
            ok = ok && fabsf(q[k]) < 2147483648.f;
        }
        if (!ok) {
            bad_value = 1;
            continue;
        }
#pragma unroll
        for (int k = 0; k < DCVC_BITS_MAX_LADDER; ++k)
            if (k < K) acc[k] += symbol_cost(t, scale_index(s / fac.f[k], edges), (int32_t)rintf(q[k]), bad_index);
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < DCVC_BITS_MAX_LADDER; ++k) {
        int32_t v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (tid < K) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < SWEEP_WAVES; ++w) v += part[w][tid];
        if (v) atomicAdd(&est[n * K + tid], (unsigned long long)v);  // (costs are >= 0; est[n][k] was zeroed)
    }
    if (bad_index | bad_value)
        atomicOr(status, (bad_index ? DCVC_BITS_BAD_INDEX : 0) | (bad_value ? DCVC_BITS_BAD_VALUE : 0));
}

bool map_args_ok(const void *cost, int32_t n_rows, int32_t stride, const void *sizes, const void *offsets, const void *map,
                 int32_t N, int32_t H, int32_t W, const void *status) {
    return cost && sizes && offsets && map && status && n_rows >= 1 && n_rows <= DCVC_BITS_MAX_ROWS && stride >= 2 &&
           N >= 1 && N <= DCVC_BITS_MAX_N && H >= 1 && H <= DCVC_BITS_MAX_SIDE && W >= 1 && W <= DCVC_BITS_MAX_SIDE;
}

}  // namespace

extern "C" int dcvc_bits_map_scale(const int32_t *sym0, const int32_t *idx0, const int32_t *sym1, const int32_t *idx1,
                                   const int32_t *cost, int32_t n_rows, int32_t stride, const int32_t *sizes,
                                   const int32_t *offsets, int32_t *map, int32_t N, int32_t C, int32_t H, int32_t W,
                                   int32_t *status, void *stream) {
    if (!sym0 || !idx0 || !sym1 || !idx1 || !map_args_ok(cost, n_rows, stride, sizes, offsets, map, N, H, W, status) ||
        C < 2 || (C & 1) || C > DCVC_BITS_MAX_C)
        return DCVC_E_ARG;
    const Table t{cost, sizes, offsets, n_rows, stride};
    const int HW = H * W;
    bits_map_kernel<<<dim3(nblk(HW, CELLS), N), dim3(CELLS, SLICES), 0, (hipStream_t)stream>>>(sym0, idx0, sym1, idx1, t, map,
                                                                                              C / 2, HW, status);
    RET_LAUNCH();
}

extern "C" int dcvc_bits_map_factorized(const int32_t *sym, const int32_t *cost, int32_t n_rows, int32_t stride,
                                        const int32_t *sizes, const int32_t *offsets, int32_t *map, int32_t N, int32_t C,
                                        int32_t H, int32_t W, int32_t *status, void *stream) {
    if (!sym || !map_args_ok(cost, n_rows, stride, sizes, offsets, map, N, H, W, status) || C < 1 || C > DCVC_BITS_MAX_C ||
        C > n_rows)
        return DCVC_E_ARG;
    const Table t{cost, sizes, offsets, n_rows, stride};
    const int HW = H * W;
    bits_map_kernel<<<dim3(nblk(HW, CELLS), N), dim3(CELLS, SLICES), 0, (hipStream_t)stream>>>(sym, nullptr, nullptr, nullptr,
                                                                                              t, map, C, HW, status);
    RET_LAUNCH();
}

extern "C" int dcvc_bits_regions(const int32_t *const *maps, const uint8_t *labels, int32_t K, int64_t *sums, int32_t N,
                                 int32_t hc, int32_t wc, int32_t *status, void *stream) {
    if (!maps || !labels || !sums || !status || ((uintptr_t)sums & 7) || K < 1 || K > DCVC_BITS_MAX_LABELS || N < 1 ||
        N > DCVC_BITS_MAX_N || hc < 4 || hc > DCVC_BITS_MAX_SIDE || (hc & 3) || wc < 4 || wc > DCVC_BITS_MAX_SIDE || (wc & 3))
        return DCVC_E_ARG;
    if (!maps[0] && !maps[1] && !maps[2] && !maps[3]) return DCVC_E_ARG;
    const Maps m{{maps[0], maps[1], maps[2], maps[3]}};
    bits_regions_kernel<<<dim3(N), dim3(256), 0, (hipStream_t)stream>>>(m, labels, K, sums, hc, wc, status);
    RET_LAUNCH();
}

extern "C" int dcvc_bits_sweep_scale(const float *y_res, const float *scales_hat, const float *idx_edges,
                                     const float *factors, int32_t K, const int32_t *cost, int32_t n_rows, int32_t stride,
                                     const int32_t *sizes, const int32_t *offsets, int64_t *est, int32_t N, int32_t C,
                                     int32_t H, int32_t W, int32_t *status, void *stream) {
    if (!y_res || !scales_hat || !idx_edges || !factors || !map_args_ok(cost, n_rows, stride, sizes, offsets, est, N, H, W, status) ||
        ((uintptr_t)est & 7) || K < 1 || K > DCVC_BITS_MAX_LADDER || C < 2 || (C & 1) || C > DCVC_BITS_MAX_C)
        return DCVC_E_ARG;
    Factors fac{};
    for (int k = 0; k < K; ++k) {
        if (!(factors[k] >= 0.1f && factors[k] <= 10.f)) return DCVC_E_ARG;  // (a NaN compares false)
        fac.f[k] = factors[k];
    }
    const Table t{cost, sizes, offsets, n_rows, stride};
    const int64_t per = (int64_t)H * W * C;
    if (hipMemsetAsync(est, 0, sizeof(int64_t) * (size_t)N * K, (hipStream_t)stream) != hipSuccess) return DCVC_E_LAUNCH;
    bits_sweep_kernel<<<dim3(nblk(per, SWEEP_THREADS * SWEEP_ITEMS), N), dim3(SWEEP_THREADS), 0, (hipStream_t)stream>>>(
        y_res, scales_hat, idx_edges, fac, K, t, (unsigned long long *)est, per, status);
    RET_LAUNCH();
}
