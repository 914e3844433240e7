// deint.hip -- one output picture of the motion-adaptive deinterlacer (include/dcvc_hip_deint.h, which states the
// arithmetic; this file only arranges it).
//
// deint_kernel is one streaming pass bound by memory, one launch for the three planes.  A WORKGROUP owns one band of
// DCVC_DEINT_BAND = 8 luma rows and the 4 rows of each chroma plane that go with them, over the whole width, so it alone
// writes the band's word of `moved` and nothing global is atomic.  A LANE owns one 16-byte column strip of one plane (16
// samples at 8 bits, 8 at 10 bits): the strips of Y, then of U, then of V are dealt to the lanes in order (1920 x 1080 at 8
// bits: 120 + 60 + 60 strips, one workgroup of 256 lanes per band; wider pictures take up to 512 lanes and then more than
// one strip a lane).  Consecutive lanes read and write consecutive 16 bytes of a row.
//
// The rule is vertical only, so there is no LDS in the data path (64 bytes of it add the waves' counts up).  The lane
// holds its band's whole window in registers, rows kept PACKED as they were loaded: for the band's 4 missing rows r (2 in a
// chroma plane) the 7 field rows cur[r-3 .. r+3] (5), the 5 (3) rows r-1, r+1 of prev and of next, the missing rows of cur and
// of the other frame: 25 (15) loads of 16 bytes, ALL issued before the arithmetic, so the band costs one round of memory
// latency; then the rule runs down the window and stores two rows a step, the interpolated one and the copied one, which is
// already there.  So per band of a plane every row is loaded once, not once per missing row; what is loaded more than once is
// the window's reach into the neighbouring bands.  (A first form walked the band with a five-row sliding window and loaded a
// step at a time, five dependent rounds of latency with one wave a SIMD to hide them behind: 10.3 us from cache and 12.3 us from
// HBM at 1080p and 8 bits where this one takes 9.6 and 11.4, profiles/deint_1080p.txt.)
//
// What it moves, in samples per luma pixel (bytes at 8 bits, twice that at 10): the minimum is 3.75 read (cur once, one
// neighbour frame in full, the other by half) and 1.5 written.  The lanes ISSUE loads of 25 rows per 8 luma rows (11 of cur,
// 5 + 5 of the field-parity rows of prev and next, 4 of the other frame) and 15 per 4 chroma rows: 3.125 + 2 * 0.25 * 3.75 =
// 5.0 samples per pixel; the 1.25 beyond the minimum are rows that the band above or below loads as well and come from the
// cache.  1.5 are written, each once.
//
// A strip is read or written as one 16-byte access when the plane's bases (of the three frames; of the output) and
// strides allow it and the strip is whole; anything else goes sample by sample through the same arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_deint.h"
#include "kernel_common.h"

namespace {

constexpr int BAND = DCVC_DEINT_BAND, MAX_LANES = 512;
static_assert(BAND % 4 == 0, "a band holds whole row pairs of the chroma planes");

struct DeintArgs {
    const void *prev[3], *cur[3], *next[3];  // Y, U, V
    void *out[3];
    uint32_t *moved;
    int32_t prev_s[2], cur_s[2], next_s[2], out_s[2];  // luma, chroma row strides in samples
    int32_t H, W, parity, second, max_code, ivec[3], ovec[3];
};

// sample q of a packed strip (q is a constant after unrolling)
template <typename S>
__device__ __forceinline__ int get(const uint4 &v, int q) {
    constexpr int PER = 4 / (int)sizeof(S), BITS = 8 * (int)sizeof(S);
    const int w = q / PER;
    const unsigned word = w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w;
    return (int)((word >> (BITS * (q % PER))) & ((1u << BITS) - 1u));
}

struct Packer {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    template <typename S>
    __device__ __forceinline__ void put(int q, unsigned s) {
        constexpr int PER = 4 / (int)sizeof(S), BITS = 8 * (int)sizeof(S);
        w[q / PER] |= s << (BITS * (q % PER));
    }
    __device__ __forceinline__ uint4 strip() const { return make_uint4(w[0], w[1], w[2], w[3]); }
};

// the strip at columns x0 .. x0 + N - 1 of a row; columns beyond the plane read as 0 (and are never stored or counted)
template <typename S>
__device__ __forceinline__ uint4 load_strip(const S *row, int x0, int PW, bool vec) {
    constexpr int N = 16 / (int)sizeof(S);
    if (vec) return *reinterpret_cast<const uint4 *>(row + x0);
    Packer p;
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (x0 + q < PW) p.put<S>(q, (unsigned)row[x0 + q]);
    return p.strip();
}

template <typename S>
__device__ __forceinline__ void store_strip(S *row, int x0, int PW, bool vec, const uint4 &v) {
    constexpr int N = 16 / (int)sizeof(S);
    if (vec) {
        *reinterpret_cast<uint4 *>(row + x0) = v;
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (x0 + q < PW) row[x0 + q] = (S)get<S>(v, q);
    }
}

// a row index outside the plane -> the nearest row inside it that has the index's parity (PH is even)
__device__ __forceinline__ int field_row(int q, int PH) { return q < 0 ? (q & 1) : q > PH - 1 ? PH - 2 + (q & 1) : q; }

// Rows R0 .. R1 - 1 (R0 and R1 even, at most BAND of them) of one plane at the lane's strip.  oth: the frame other than cur
// that holds a field next to this one (prev for the earlier field, next for the later).  The band's whole window is loaded
// first -- with K missing rows: K + 3 field rows of cur, K + 1 of prev and of next, the K missing rows of cur and of oth --
// then the rule runs down the window.  -> the strip's missing samples with diff > 0
template <typename S>
__device__ __forceinline__ unsigned walk(const S *__restrict__ cur, int cs, const S *__restrict__ prev, int ps, const S *__restrict__ next,
                                         int ns, const S *__restrict__ oth, int os, S *__restrict__ out, int outs, int PH, int PW, int R0,
                                         int R1, int x0, int p, int max_code, bool iv, bool ov) {
    constexpr int N = 16 / (int)sizeof(S), KMAX = BAND / 2;
    const auto ld = [&](const S *plane, int stride, int row) { return load_strip<S>(plane + (size_t)row * stride, x0, PW, iv); };
    const int r0 = R0 + 1 - p, K = (R1 - R0) / 2;
    // ---- every load of the band: w[j] = cur[r0 - 3 + 2 j], pp[j] / nn[j] = prev / next [r0 - 1 + 2 j], m[k] / o[k] = cur / oth [r0 + 2 k]
    uint4 w[KMAX + 3], pp[KMAX + 1], nn[KMAX + 1], m[KMAX], o[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX + 3; ++j)
        if (j < K + 3) w[j] = ld(cur, cs, field_row(r0 - 3 + 2 * j, PH));
#pragma unroll
    for (int j = 0; j < KMAX + 1; ++j)
        if (j < K + 1) pp[j] = ld(prev, ps, field_row(r0 - 1 + 2 * j, PH)), nn[j] = ld(next, ns, field_row(r0 - 1 + 2 * j, PH));
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) m[k] = ld(cur, cs, r0 + 2 * k), o[k] = ld(oth, os, r0 + 2 * k);
    // ---- the rule, a missing row and a sample at a time
    unsigned count = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k >= K) break;
        const int r = r0 + 2 * k;
        Packer res;
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int c = get<S>(w[k + 1], q), e = get<S>(w[k + 2], q), c3 = get<S>(w[k], q), e3 = get<S>(w[k + 3], q);
            const int a = get<S>(m[k], q), b = get<S>(o[k], q);
            const int d = (a + b) >> 1, td0 = abs(a - b);
            const int td1 = (abs(get<S>(pp[k], q) - c) + abs(get<S>(pp[k + 1], q) - e)) >> 1;
            const int td2 = (abs(get<S>(nn[k], q) - c) + abs(get<S>(nn[k + 1], q) - e)) >> 1;
            const int diff = max(td0 >> 1, max(td1, td2));
            const int pred = min(max((9 * (c + e) - (c3 + e3) + 8) >> 4, 0), max_code);
            res.put<S>(q, (unsigned)min(max(pred, d - diff), d + diff));
            count += (diff > 0 && x0 + q < PW) ? 1u : 0u;
        }
        store_strip<S>(out + (size_t)r * outs, x0, PW, ov, res.strip());
        if (p == 0)  // the field's own row beside it: r - 1 (top field) or r + 1, inside the band either way
            store_strip<S>(out + (size_t)(r - 1) * outs, x0, PW, ov, w[k + 1]);
        else
            store_strip<S>(out + (size_t)(r + 1) * outs, x0, PW, ov, w[k + 2]);
    }
    return count;
}

template <typename S>
__global__ __launch_bounds__(MAX_LANES) void deint_kernel(const DeintArgs a) {
    constexpr int N = 16 / (int)sizeof(S);
    __shared__ unsigned part[MAX_LANES / 64];
    const int band = blockIdx.x, ls = (a.W + N - 1) / N, cs = (a.W / 2 + N - 1) / N;
    unsigned count = 0;
    for (int s = threadIdx.x; s < ls + 2 * cs; s += blockDim.x) {
        const int pl = s < ls ? 0 : s < ls + cs ? 1 : 2, strip = s - (pl == 0 ? 0 : pl == 1 ? ls : ls + cs), c = pl != 0;
        const int PH = c ? a.H / 2 : a.H, PW = c ? a.W / 2 : a.W, rows = c ? BAND / 2 : BAND;
        const int R0 = band * rows, R1 = min(R0 + rows, PH), x0 = strip * N;
        const bool whole = x0 + N <= PW;
        const S *cur = static_cast<const S *>(a.cur[pl]), *prev = static_cast<const S *>(a.prev[pl]);
        const S *next = static_cast<const S *>(a.next[pl]);
        const unsigned n = walk<S>(cur, a.cur_s[c], prev, a.prev_s[c], next, a.next_s[c], a.second ? next : prev,
                                   a.second ? a.next_s[c] : a.prev_s[c], static_cast<S *>(a.out[pl]), a.out_s[c], PH, PW, R0, R1, x0,
                                   a.parity, a.max_code, a.ivec[pl] && whole, a.ovec[pl] && whole);
        count += pl == 0 ? n : 0u;
    }
    count = wave_sum(count);  // (every lane of every wave is here: the block is whole waves)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
        for (int w = 0; w < (int)blockDim.x / 64; ++w) total += part[w];
        a.moved[band] = total;
    }
}

bool aligned(const void *p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

struct Extent {
    uintptr_t lo, hi;
};
Extent extent_of(const void *p, int rows, int width, int stride, size_t sb) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + ((size_t)(rows - 1) * stride + width) * sb};
}
bool overlap(const Extent &a, const Extent &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int dcvc_deinterlace420(const void *prev_y, const void *prev_u, const void *prev_v, int32_t prev_ys, int32_t prev_cs,
                                   const void *cur_y, const void *cur_u, const void *cur_v, int32_t cur_ys, int32_t cur_cs,
                                   const void *next_y, const void *next_u, const void *next_v, int32_t next_ys, int32_t next_cs,
                                   int32_t H, int32_t W, int32_t bit_depth, int32_t parity, int32_t second, void *out_y, void *out_u,
                                   void *out_v, int32_t out_ys, int32_t out_cs, uint32_t *moved, int32_t n_moved, void *stream) {
    const void *in[9] = {prev_y, prev_u, prev_v, cur_y, cur_u, cur_v, next_y, next_u, next_v};
    void *out[3] = {out_y, out_u, out_v};
    const int32_t in_s[9] = {prev_ys, prev_cs, prev_cs, cur_ys, cur_cs, cur_cs, next_ys, next_cs, next_cs};
    const int32_t out_s[3] = {out_ys, out_cs, out_cs};
    for (const void *p : in)
        if (!p) return DCVC_E_ARG;
    if (!out_y || !out_u || !out_v || !moved) return DCVC_E_ARG;
    if (H <= 0 || W <= 0 || H % 4 != 0 || W % 2 != 0 || H > DCVC_COLOR_MAX_SIDE || W > DCVC_COLOR_MAX_SIDE) return DCVC_E_ARG;
    if ((bit_depth != 8 && bit_depth != 10) || (parity != 0 && parity != 1) || (second != 0 && second != 1)) return DCVC_E_ARG;
    if (n_moved != (H + BAND - 1) / BAND || !aligned(moved, 4)) return DCVC_E_ARG;
    const size_t sb = bit_depth == 8 ? 1 : 2;
    Extent ie[9], oe[3];
    for (int k = 0; k < 9; ++k) {
        const int rows = k % 3 ? H / 2 : H, width = k % 3 ? W / 2 : W;
        if (in_s[k] < width || !aligned(in[k], sb)) return DCVC_E_ARG;
        ie[k] = extent_of(in[k], rows, width, in_s[k], sb);
    }
    for (int k = 0; k < 3; ++k) {
        const int rows = k ? H / 2 : H, width = k ? W / 2 : W;
        if (out_s[k] < width || !aligned(out[k], sb)) return DCVC_E_ARG;
        oe[k] = extent_of(out[k], rows, width, out_s[k], sb);
    }
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 9; ++j)
            if (overlap(oe[k], ie[j])) return DCVC_E_ARG;
        for (int j = 0; j < k; ++j)
            if (overlap(oe[k], oe[j])) return DCVC_E_ARG;
    }
    DeintArgs a{};
    for (int k = 0; k < 3; ++k) {
        a.prev[k] = in[k], a.cur[k] = in[3 + k], a.next[k] = in[6 + k], a.out[k] = out[k];
        a.ivec[k] = a.ovec[k] = 1;
        for (int f = 0; f < 3; ++f) a.ivec[k] &= aligned(in[3 * f + k], 16) && ((size_t)in_s[3 * f + k] * sb) % 16 == 0;
        a.ovec[k] = aligned(out[k], 16) && ((size_t)out_s[k] * sb) % 16 == 0;
    }
    a.prev_s[0] = prev_ys, a.prev_s[1] = prev_cs, a.cur_s[0] = cur_ys, a.cur_s[1] = cur_cs;
    a.next_s[0] = next_ys, a.next_s[1] = next_cs, a.out_s[0] = out_ys, a.out_s[1] = out_cs;
    a.moved = moved, a.H = H, a.W = W, a.parity = parity, a.second = second, a.max_code = (1 << bit_depth) - 1;
    const int n = 16 / (int)sb, strips = (W + n - 1) / n + 2 * ((W / 2 + n - 1) / n);
    const dim3 block(min(MAX_LANES, round_up(strips, 64))), grid(n_moved);
    if (sb == 1)
        deint_kernel<uint8_t><<<grid, block, 0, (hipStream_t)stream>>>(a);
    else
        deint_kernel<uint16_t><<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
