// mepyr.hip -- the hierarchical motion search in front of the temporal noise prefilter (include/dcvc_hip_mepyr.h, which
// states the arithmetic; this file only arranges it).
//
// me_pyramid_kernel is a streaming kernel tiled the way tnr_step_kernel is: a workgroup of 8 waves owns a strip of 16 rows x
// 256 columns of the picture, a wave 2 rows, a lane 4 consecutive pixels.  Six loads (16 bytes each where the picture's base
// and strides allow it), then the luma of the quad as one word to LDS and to y0.  The strip's origin is a multiple of 4 in
// both directions, so the 8 x 128 pixels of level 1 and the 4 x 64 of level 2 below it are reduced from LDS alone: a thread
// per word of four pixels, every index clamped to the part of the strip that lies in the picture (the edge replication of
// the header).  Bytes are stored as words; a word cut by the level's right edge goes byte by byte.
//
// me_coarse_kernel has the shape of me_search_kernel (me.hip) with rows of 8 bytes: a WORKGROUP owns one cell, the support
// (8 x 8, cut by the level on any side) and its window of ref are staged in LDS as bytes, every coordinate clamped BEFORE the
// load; a LANE takes one dy and four consecutive dx whose windows start at a 4-byte boundary of the LDS row and issues two
// v_qsad_pk_u16_u8 a row, a cut support its whole quads the same way and its partial quad with v_alignbyte + v_sad_u8 on
// masked words.  The minimum of the packed key is folded with xor-shuffles inside a wave and through LDS across waves.
//
// me_descend_kernel: a WAVE owns one cell, a workgroup four cells of a row.  The candidates clamp(2 p + e) all lie within
// 2 E of clamp(2 p - E), so ONE window of (B + 2 E) rows serves them (B = 16, E = 2 at level 0; B = 8, E = 1 at level 1);
// the block of ref at (0, 0) is staged below it.  A lane takes one candidate and one part of the rows (26 candidates x 2
// parts, or 10 x 4), reads the window at its byte offset with v_alignbyte and sums with v_sad_u8 on words masked to the
// cell's width; the parts are added and the key's minimum is folded with xor-shuffles.  Nothing passes between waves.
//
// The key is (J, |dy| + |dx|, dy + 128, dx + 128) in 17 + 9 + 9 + 9 bits: +-128 needs 9 bits a component, so me.hip's 7-bit
// packing does not carry over.  Nothing global is atomic, nothing is kept in scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_mepyr.h"
#include "kernel_common.h"
#include "roi_common.h"

namespace {

constexpr int BIAS = DCVC_MEPYR_MAX_R;
static_assert(BIAS == 128 && DCVC_ROI_CELL == 16, "dy + 128 and dx + 128 fit 9 bits, a length of 256 too");

__device__ __forceinline__ unsigned long long pack_key(unsigned J, int dy, int dx) {
    const unsigned len = (unsigned)(abs(dy) + abs(dx));
    return (unsigned long long)J << 27 | (unsigned long long)(len << 18 | (unsigned)(dy + BIAS) << 9 | (unsigned)(dx + BIAS));
}
__device__ __forceinline__ int key_dy(unsigned long long k) { return (int)((k >> 9) & 511u) - BIAS; }
__device__ __forceinline__ int key_dx(unsigned long long k) { return (int)(k & 511u) - BIAS; }
__device__ __forceinline__ unsigned key_len(unsigned long long k) { return (unsigned)(k >> 18) & 511u; }

__device__ __forceinline__ unsigned long long wave_min(unsigned long long key) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
    }
    return key;
}

__device__ __forceinline__ unsigned long long pack64(unsigned lo, unsigned hi) { return (unsigned long long)hi << 32 | lo; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------------------------- pyramid
constexpr int PT_W = 256, PT_H = 16, WAVES = 8, ROWS = 2;
static_assert(PT_W == 64 * 4 && ROWS * WAVES == PT_H, "a lane per quad, a wave per two rows");

struct PyrArgs {
    const float *pic;
    uint8_t *y0, *y1, *y2;
    int64_t ps;
    int32_t rs, H, W, s0, s1, s2, levels, vec;
};

// four pixels of a level as one word: a word store where the quad lies in the level, bytes where the level's edge cuts it
__device__ __forceinline__ void store_quad(uint8_t *row, int x, int width, unsigned word) {
    if (x + 4 <= width) {
        *reinterpret_cast<unsigned *>(row + x) = word;
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (x + q < width) row[x + q] = (uint8_t)(word >> (8 * q));
    }
}

// the word of four pixels (r, 4 c .. 4 c + 3) of the next level from a strip of `pitch` bytes a row, of which h rows and w
// columns lie in the level above
__device__ __forceinline__ unsigned reduce_quad(const uint8_t *strip, int pitch, int r, int c, int h, int w) {
    const uint8_t *a = strip + min(2 * r, h - 1) * pitch, *b = strip + min(2 * r + 1, h - 1) * pitch;
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int xa = min(2 * (4 * c + q), w - 1), xb = min(2 * (4 * c + q) + 1, w - 1);
        word |= (((unsigned)a[xa] + a[xb] + b[xa] + b[xb] + 2u) >> 2) << (8 * q);
    }
    return word;
}

__global__ __launch_bounds__(64 * WAVES) void me_pyramid_kernel(const PyrArgs p) {
    __shared__ unsigned l0[PT_H * PT_W / 4];  // Y of the strip, a byte per pixel
    __shared__ unsigned l1[PT_H * PT_W / 16];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    const int X0 = blockIdx.x * PT_W, Y0 = blockIdx.y * PT_H, x0 = X0 + lane * 4;
    if (x0 < p.W) {
        const bool vec = p.vec && x0 + 4 <= p.W;
        float v[ROWS][3][4];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = min(Y0 + wave * ROWS + i, p.H - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float *row = p.pic + k * p.ps + (int64_t)y * p.rs;
                if (vec) {
                    const float4 t = *reinterpret_cast<const float4 *>(row + x0);
                    v[i][k][0] = t.x, v[i][k][1] = t.y, v[i][k][2] = t.z, v[i][k][3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[i][k][q] = row[min(x0 + q, p.W - 1)];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = Y0 + wave * ROWS + i;
            unsigned word = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) word |= (unsigned)luma8(code8(v[i][0][q]), code8(v[i][1][q]), code8(v[i][2][q])) << (8 * q);
            l0[(wave * ROWS + i) * (PT_W / 4) + lane] = word;  // (a row past the picture repeats the last one and is never read)
            if (y < p.H) store_quad(p.y0 + (int64_t)y * p.s0, x0, p.W, word);
        }
    }
    __syncthreads();
    const int H1 = (p.H + 1) >> 1, W1 = (p.W + 1) >> 1;
    if (tid < PT_H * PT_W / 16) {  // level 1: 8 rows x 32 words
        const int r = tid >> 5, c = tid & 31, y = (Y0 >> 1) + r, x = (X0 >> 1) + 4 * c;
        const unsigned word = reduce_quad(reinterpret_cast<const uint8_t *>(l0), PT_W, r, c, min(PT_H, p.H - Y0), min(PT_W, p.W - X0));
        l1[tid] = word;
        if (y < H1 && x < W1) store_quad(p.y1 + (int64_t)y * p.s1, x, W1, word);
    }
    __syncthreads();
    if (p.levels == 2 && tid < PT_H * PT_W / 64) {  // level 2: 4 rows x 16 words
        const int H2 = (H1 + 1) >> 1, W2 = (W1 + 1) >> 1;
        const int r = tid >> 4, c = tid & 15, y = (Y0 >> 2) + r, x = (X0 >> 2) + 4 * c;
        const unsigned word =
            reduce_quad(reinterpret_cast<const uint8_t *>(l1), PT_W / 2, r, c, min(PT_H / 2, H1 - (Y0 >> 1)), min(PT_W / 2, W1 - (X0 >> 1)));
        if (y < H2 && x < W2) store_quad(p.y2 + (int64_t)y * p.s2, x, W2, word);
    }
}

// ----------------------------------------------------------------------------------------------------------------- coarse
constexpr int SUP = 8, SQUADS = SUP / 4;  // the support's side; its quads a row

struct CoarseArgs {
    const uint8_t *cur, *ref;
    int16_t *mv;
    int32_t cs, rs, HL, WL, H, W, wc, R, lambda, mul, step, lead;  // the support of cell i starts at step * i - lead
};

template <int RMAX>
struct Shape {
    static constexpr int NG = (RMAX + 2) / 2;  // ceil((2 RMAX + 1) / 4)
    static constexpr int WH = SUP + 2 * RMAX, WW = SUP + 4 * NG, PITCH = (WW / 4) | 1;  // (words; odd: rows fall on other banks)
    static constexpr int THREADS = RMAX <= 8 ? 128 : RMAX <= 16 ? 320 : 256;
    static constexpr int PER = (WH * WW + THREADS - 1) / THREADS;
};

template <int RMAX>
__global__ __launch_bounds__(Shape<RMAX>::THREADS) void me_coarse_kernel(const CoarseArgs p) {
    using S = Shape<RMAX>;
    __shared__ unsigned win[S::WH * S::PITCH];  // Y_L of ref, a byte per pixel: row = y - sy0 + R, byte = x - sx0 + R
    __shared__ uint2 sup[SUP];                  // Y_L of cur over the support, a row per uint2
    __shared__ unsigned long long best[S::THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t at = (int64_t)blockIdx.y * p.wc + blockIdx.x;
    if ((int)blockIdx.x * DCVC_ROI_CELL >= p.W || (int)blockIdx.y * DCVC_ROI_CELL >= p.H) {  // (uniform) a cell without a pixel
        if (tid == 0) p.mv[2 * at] = 0, p.mv[2 * at + 1] = 0;
        return;
    }
    // the support, intersected with the level: never empty for a cell that holds a pixel
    const int sy0 = max((int)blockIdx.y * p.step - p.lead, 0), sx0 = max((int)blockIdx.x * p.step - p.lead, 0);
    const int sh = min((int)blockIdx.y * p.step - p.lead + SUP, p.HL) - sy0, sw = min((int)blockIdx.x * p.step - p.lead + SUP, p.WL) - sx0;
    const int R = p.R, ng = (R + 2) / 2, ww = SUP + 4 * ng, npix = (SUP + 2 * R) * ww;

    // ---- every load of the thread: its share of the window, then of the support (a share past the end repeats the last pixel)
    uint8_t w[S::PER];
    int wat[S::PER];
#pragma unroll
    for (int i = 0; i < S::PER; ++i) {
        const int pix = min(i * S::THREADS + tid, npix - 1), wy = pix / ww, wx = pix - wy * ww;
        const int y = clampi(sy0 - R + wy, 0, p.HL - 1), x = clampi(sx0 - R + wx, 0, p.WL - 1);
        wat[i] = wy * (4 * S::PITCH) + wx;
        w[i] = p.ref[(int64_t)y * p.rs + x];
    }
    const int cpix = min(tid, SUP * SUP - 1);
    const uint8_t c = p.cur[(int64_t)min(sy0 + cpix / SUP, p.HL - 1) * p.cs + min(sx0 + cpix % SUP, p.WL - 1)];
#pragma unroll
    for (int i = 0; i < S::PER; ++i) reinterpret_cast<uint8_t *>(win)[wat[i]] = w[i];
    if (tid < SUP * SUP) reinterpret_cast<uint8_t *>(sup)[tid] = c;
    __syncthreads();

    // ---- the candidates
    const int groups = (2 * R + 1) * ng, whole = sw >> 2, rest = sw & 3;
    const unsigned mask = (1u << (8 * rest)) - 1u;  // the bytes of the last quad that lie in the support
    unsigned long long key = ~0ull;
    for (int g = tid; g < groups; g += S::THREADS) {
        const int dyi = g / ng, k = g - dyi * ng;
        const unsigned *row = win + dyi * S::PITCH + k;
        unsigned long long acc = 0;      // four SADs, uint16 each
        unsigned tail[4] = {0, 0, 0, 0};  // what the partial quad adds to them
        if (sh == SUP && sw == SUP) {     // (uniform across the workgroup)
#pragma unroll
            for (int y = 0; y < SUP; ++y) {
                const unsigned *r = row + y * S::PITCH;
                const unsigned r0 = r[0], r1 = r[1], r2 = r[2];
                const uint2 q = sup[y];
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r0, r1), q.x, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r1, r2), q.y, acc);
            }
        } else {
            const unsigned *words = reinterpret_cast<const unsigned *>(sup);
            for (int y = 0; y < sh; ++y) {
                const unsigned *r = row + y * S::PITCH;
                for (int q = 0; q < whole; ++q) acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r[q], r[q + 1]), words[y * SQUADS + q], acc);
                if (rest) {
                    const unsigned lo = r[whole], hi = r[whole + 1], cq = words[y * SQUADS + whole] & mask;
#pragma unroll
                    for (int i = 0; i < 4; ++i) tail[i] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, i) & mask, cq, tail[i]);
                }
            }
        }
        const int dy = dyi - R;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = 4 * k + i - R;
            if (dx > R) continue;  // (the last group's columns past the search range)
            const unsigned sad = ((unsigned)(acc >> (16 * i)) & 0xffffu) + tail[i];
            const unsigned long long cand = pack_key((unsigned)p.mul * sad + (unsigned)p.lambda * (unsigned)(abs(dy) + abs(dx)), dy, dx);
            key = cand < key ? cand : key;
        }
    }
    // ---- the minimum: inside the wave, then across the waves
    key = wave_min(key);
    if ((tid & 63) == 0) best[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < S::THREADS / 64; ++v) key = best[v] < key ? best[v] : key;
        p.mv[2 * at] = (int16_t)key_dy(key);
        p.mv[2 * at + 1] = (int16_t)key_dx(key);
    }
}

template <int RMAX>
void launch_coarse(const CoarseArgs &a, hipStream_t stream) {
    const dim3 grid(a.wc, 4 * ((a.H + 63) / 64));
    me_coarse_kernel<RMAX><<<grid, Shape<RMAX>::THREADS, 0, stream>>>(a);
}

// ---------------------------------------------------------------------------------------------------------------- descent
constexpr int DCELLS = 4;  // cells (waves) a workgroup

struct DescArgs {
    const uint8_t *cur, *ref;
    const int16_t *mv_in;
    int16_t *mv;
    uint32_t *cost, *zero;
    int32_t cs, rs, HL, WL, H, W, wc, R, lambda, mul;
};

template <int B, int E>
__global__ __launch_bounds__(64 * DCELLS) void me_descend_kernel(const DescArgs p) {
    constexpr int SPAN = B + 2 * E, QUADS = B / 4, PITCH = QUADS + 2, SIDE = 2 * E + 1, NC = SIDE * SIDE + 1;
    constexpr int CL = NC <= 16 ? 16 : 32, PARTS = 64 / CL, RPP = B / PARTS;
    static_assert(NC <= CL && RPP * PARTS == B && 4 * PITCH >= SPAN + 4, "a lane per candidate and part; the window's rows hold an aligned read past the span");
    __shared__ unsigned win[DCELLS][(SPAN + B) * PITCH];  // Y of ref: SPAN rows of the window, then B rows of the block at (0, 0)
    __shared__ unsigned blk[DCELLS][B * QUADS];           // Y of cur over the cell
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.y, j = blockIdx.x * DCELLS + wave;
    const int64_t at = (int64_t)i * p.wc + j;
    const bool live = DCVC_ROI_CELL * i < p.H && DCVC_ROI_CELL * j < p.W;  // (uniform across the wave)
    const int Y0 = B * i, X0 = B * j, R = p.R;
    int py = 0, px = 0, by = 0, bx = 0;
    if (live) {
        py = p.mv_in[2 * at], px = p.mv_in[2 * at + 1];
        by = clampi(2 * py - E, -R, R), bx = clampi(2 * px - E, -R, R);  // every candidate lies within [by, by + 2 E] x [bx, bx + 2 E]
        uint8_t *wb = reinterpret_cast<uint8_t *>(win[wave]), *cb = reinterpret_cast<uint8_t *>(blk[wave]);
        constexpr int NW = (SPAN + B) * 4 * PITCH, NB = B * B;
        uint8_t w[(NW + 63) / 64], c[(NB + 63) / 64];
#pragma unroll
        for (int k = 0; k < (NW + 63) / 64; ++k) {  // every coordinate clamped before the load
            const int idx = min(k * 64 + lane, NW - 1), wy = idx / (4 * PITCH), wx = idx - wy * (4 * PITCH);
            const int oy = wy < SPAN ? by + wy : wy - SPAN, ox = wy < SPAN ? bx + wx : wx;
            w[k] = p.ref[(int64_t)clampi(Y0 + oy, 0, p.HL - 1) * p.rs + clampi(X0 + ox, 0, p.WL - 1)];
        }
#pragma unroll
        for (int k = 0; k < (NB + 63) / 64; ++k) {
            const int idx = k * 64 + lane;
            c[k] = p.cur[(int64_t)min(Y0 + idx / B, p.HL - 1) * p.cs + min(X0 + idx % B, p.WL - 1)];
        }
#pragma unroll
        for (int k = 0; k < (NW + 63) / 64; ++k) wb[min(k * 64 + lane, NW - 1)] = w[k];
#pragma unroll
        for (int k = 0; k < (NB + 63) / 64; ++k) cb[k * 64 + lane] = c[k];
    }
    __syncthreads();
    if (!live) {
        if (lane == 0) {
            p.mv[2 * at] = 0, p.mv[2 * at + 1] = 0;
            if (p.cost) p.cost[at] = 0, p.zero[at] = 0;
        }
        return;
    }
    const int cand = lane % CL, part = lane / CL;
    const int ch = min(B, p.HL - Y0), cw = min(B, p.WL - X0);
    int dy = 0, dx = 0, oy = SPAN, ox = 0;  // (the last candidate: (0, 0), whose block lies below the window)
    if (cand < NC - 1) {
        dy = clampi(2 * py + cand / SIDE - E, -R, R), dx = clampi(2 * px + cand % SIDE - E, -R, R);
        oy = dy - by, ox = dx - bx;
    }
    unsigned sad = 0;
    if (cand < NC) {
        const unsigned *rows = win[wave] + oy * PITCH, *cur = blk[wave];
#pragma unroll
        for (int r = part * RPP; r < part * RPP + RPP; ++r) {
            if (r >= ch) break;
#pragma unroll
            for (int q = 0; q < QUADS; ++q) {
                const int left = cw - 4 * q;  // the bytes of this quad that lie in the cell
                if (left <= 0) break;
                const unsigned mask = left >= 4 ? ~0u : (1u << (8 * left)) - 1u;
                const int o = ox + 4 * q;
                const unsigned *wp = rows + r * PITCH + (o >> 2);
                sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(wp[1], wp[0], (unsigned)(o & 3)) & mask, cur[r * QUADS + q] & mask, sad);
            }
        }
    }
#pragma unroll
    for (int off = CL; off < 64; off <<= 1) sad += (unsigned)__shfl_xor((int)sad, off);  // the parts of a candidate
    const unsigned len = (unsigned)(abs(dy) + abs(dx));
    unsigned long long key = cand < NC ? pack_key((unsigned)p.mul * sad + (unsigned)p.lambda * len, dy, dx) : ~0ull;
    if (lane == NC - 1 && p.zero) p.zero[at] = sad;
    key = wave_min(key);
    if (lane == 0) {
        p.mv[2 * at] = (int16_t)key_dy(key);
        p.mv[2 * at + 1] = (int16_t)key_dx(key);
        if (p.cost) p.cost[at] = ((unsigned)(key >> 27) - (unsigned)p.lambda * key_len(key)) / (unsigned)p.mul;
    }
}

// ------------------------------------------------------------------------------------------------------------ entry points
inline bool range_ok(int32_t R, int32_t levels, int32_t lambda) {
    return levels >= 1 && levels <= DCVC_MEPYR_MAX_LEVELS && R >= 2 * levels && R <= 64 * levels && lambda >= 0 && lambda <= DCVC_ME_MAX_LAMBDA;
}

inline int32_t level_side(int32_t v, int32_t level) { return level == 0 ? v : level == 1 ? (v + 1) / 2 : ((v + 1) / 2 + 1) / 2; }

inline bool plane_ok(const uint8_t *p, int32_t s, int32_t H, int32_t W, int32_t level) {
    return p && s >= level_side(W, level) && s % 4 == 0 && aligned(p, 4);
}

struct Extent {
    uintptr_t lo, hi;
};
inline Extent plane_extent(const uint8_t *p, int32_t s, int32_t H, int32_t W, int32_t level) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + (uintptr_t)(level_side(H, level) - 1) * (uintptr_t)s + (uintptr_t)level_side(W, level)};
}
inline bool overlap(const Extent &a, const Extent &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int dcvc_me_pyramid(const float *pic, int32_t rs, int64_t ps, int32_t H, int32_t W, int32_t levels, uint8_t *y0, int32_t s0,
                               uint8_t *y1, int32_t s1, uint8_t *y2, int32_t s2, void *stream) {
    if (!size_ok(H, W) || !planes_ok(pic, rs, ps, H, W) || levels < 1 || levels > DCVC_MEPYR_MAX_LEVELS || !aligned(pic, 4) ||
        !plane_ok(y0, s0, H, W, 0) || !plane_ok(y1, s1, H, W, 1) || (levels == 2 && !plane_ok(y2, s2, H, W, 2)))
        return DCVC_E_ARG;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(pic);
    // (unsigned: a plane stride near 2^63 wraps instead of overflowing, and such a picture overlaps nothing real)
    const Extent e[4] = {{p0, p0 + 4 * (2 * (uintptr_t)ps + (uintptr_t)(H - 1) * (uintptr_t)rs + (uintptr_t)W)}, plane_extent(y0, s0, H, W, 0),
                         plane_extent(y1, s1, H, W, 1), levels == 2 ? plane_extent(y2, s2, H, W, 2) : Extent{0, 0}};
    for (int a = 1; a <= levels + 1; ++a)
        for (int b = 0; b < a; ++b)
            if (overlap(e[a], e[b])) return DCVC_E_ARG;
    PyrArgs a{};
    a.pic = pic, a.y0 = y0, a.y1 = y1, a.y2 = levels == 2 ? y2 : nullptr, a.ps = ps, a.rs = rs, a.H = H, a.W = W;
    a.s0 = s0, a.s1 = s1, a.s2 = s2, a.levels = levels, a.vec = vec_ok(pic, rs, ps);
    const dim3 block(64, WAVES), grid(nblk(W, PT_W), nblk(H, PT_H));
    me_pyramid_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_me_coarse(const uint8_t *cur, int32_t cur_s, const uint8_t *ref, int32_t ref_s, int32_t H, int32_t W, int32_t R,
                              int32_t levels, int32_t lambda, int16_t *mv, void *stream) {
    if (!mv || !size_ok(H, W) || !range_ok(R, levels, lambda) || !plane_ok(cur, cur_s, H, W, levels) || !plane_ok(ref, ref_s, H, W, levels) ||
        !aligned(mv, 2))
        return DCVC_E_ARG;
    CoarseArgs a{};
    a.cur = cur, a.ref = ref, a.mv = mv, a.cs = cur_s, a.rs = ref_s, a.HL = level_side(H, levels), a.WL = level_side(W, levels);
    a.H = H, a.W = W, a.wc = 4 * ((W + 63) / 64), a.R = levels == 1 ? (R + 1) / 2 : (R + 3) / 4, a.lambda = lambda;
    a.mul = levels == 1 ? 2 : 1, a.step = levels == 1 ? 8 : 4, a.lead = levels == 1 ? 0 : 2;
    if (a.R <= 8)
        launch_coarse<8>(a, (hipStream_t)stream);
    else if (a.R <= 16)
        launch_coarse<16>(a, (hipStream_t)stream);
    else
        launch_coarse<32>(a, (hipStream_t)stream);
    RET_LAUNCH();
}

extern "C" int dcvc_me_descend(const uint8_t *cur, int32_t cur_s, const uint8_t *ref, int32_t ref_s, int32_t H, int32_t W, int32_t R,
                               int32_t levels, int32_t level, int32_t lambda, const int16_t *mv_in, int16_t *mv, uint32_t *cost,
                               uint32_t *zero, void *stream) {
    if (!mv_in || !mv || !size_ok(H, W) || !range_ok(R, levels, lambda) || level < 0 || level >= levels ||
        !plane_ok(cur, cur_s, H, W, level) || !plane_ok(ref, ref_s, H, W, level) || !aligned(mv_in, 2) || !aligned(mv, 2) ||
        (const int16_t *)mv == mv_in || (level == 0 && (!cost || !zero || !aligned(cost, 4) || !aligned(zero, 4))))
        return DCVC_E_ARG;
    DescArgs a{};
    a.cur = cur, a.ref = ref, a.mv_in = mv_in, a.mv = mv, a.cost = level == 0 ? cost : nullptr, a.zero = level == 0 ? zero : nullptr;
    a.cs = cur_s, a.rs = ref_s, a.HL = level_side(H, level), a.WL = level_side(W, level), a.H = H, a.W = W, a.wc = 4 * ((W + 63) / 64);
    a.R = level == 0 ? R : (R + 1) / 2, a.lambda = lambda, a.mul = level == 0 ? 1 : 2;
    const dim3 grid(a.wc / DCELLS, 4 * ((H + 63) / 64));
    if (level == 0)
        me_descend_kernel<16, 2><<<grid, 64 * DCELLS, 0, (hipStream_t)stream>>>(a);
    else
        me_descend_kernel<8, 1><<<grid, 64 * DCELLS, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}
