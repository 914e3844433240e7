// shake.hip -- one whole-pixel vector per picture against an anchor picture: the anchor's luma as a byte plane, a 2-D search
// on a sparse sample of every 64 x 64 tile, and the median vote over the tiles (include/dcvc_hip_shake.h, which states the
// arithmetic; this file only arranges it).
//
// shake_plane_kernel is noise_cells_kernel (noise.hip) without the previous plane and the cells: a workgroup of 4 waves owns
// 16 rows x 256 columns, a wave 4 rows, a lane 4 consecutive pixels of each; all twelve loads of a lane are issued before
// the first code is formed; a quad of luma is one 4-byte store (y_stride is a multiple of 4 and the plane is 4-byte
// aligned) wherever its four pixels lie inside the picture, else byte by byte, so that nothing from column W on is touched.
//
// shake_tiles_kernel: a WORKGROUP of 4 waves owns one tile and its five words.  Every luma is formed once: a thread
// converts one quad of one of the sixteen sampled rows of cur (rows 64 a + 4 i; a tile lies wholly inside the picture, so
// nothing is clamped) into one word of LDS, and the threads copy the anchor's (61 + 2R) x (64 + 4 NG) window (NG = ceil((2R +
// 1) / 4) groups of four dx; the columns past dx = R belong to candidates that are thrown away), every coordinate clamped to
// the picture BEFORE the load, into LDS as bytes: at most 93 rows of 100 bytes.
//
// The work is dealt in UNITS of (a candidate group, four sampled rows): a group is one dy and the four dx = -R + 4 k ..
// -R + 4 k + 3, whose windows start at a 4-byte boundary of the LDS row, exactly as in me.hip.  Per row a lane reads
// seventeen words of window and the row's sixteen quads of cur (one address for the lanes of a row quarter: a broadcast)
// and issues sixteen v_qsad_pk_u16_u8, four SADs as four uint16.  Four rows of 64 pixels are at most 65280, so the packed
// accumulator cannot carry; after them the four sums are ADDED to a table of 32-bit SADs in LDS (integer adds: no order).
// At R = 16 that is 1188 units on 256 threads where whole candidates would be 297 on 256.  After a barrier the threads walk
// the (2R + 1)^2 candidates of the table: the smallest packed key (SAD, |dy| + |dx|, dy + 16, dx + 16) in 18 + 6 + 7 + 7
// bits, and the largest SAD; both are folded with xor-shuffles inside a wave and through LDS across waves.  Nothing global is
// atomic, nothing is kept in scratch.
//
// shake_vote_kernel is ONE workgroup: the voting tiles' dy and dx are counted into 2R + 1 bins each in LDS, one thread walks
// the bins to the two lower medians, a second pass over the records counts the tiles that agree, one thread writes the
// record and all of them fill the vector field.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_shake.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------------ the plane
constexpr int STRIP_W = 256, STRIP_H = 16, ROWS = 4;
static_assert(STRIP_W == 64 * 4 && ROWS * 4 == STRIP_H, "a lane per quad, a wave per four rows");

struct PlaneArgs {
    const float *rgb;
    uint8_t *y;
    int64_t ps;
    int32_t rs, H, W, ys, pvec;
};

__global__ __launch_bounds__(256) void shake_plane_kernel(const PlaneArgs p) {
    const int x0 = blockIdx.x * STRIP_W + threadIdx.x * 4, y0 = blockIdx.y * STRIP_H + threadIdx.y * ROWS;
    if (x0 >= p.W || y0 >= p.H) return;  // (no barrier below)
    const bool whole = x0 + 4 <= p.W, pv = p.pvec && whole;
    float f[ROWS][3][4];
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
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (y0 + r >= p.H) break;  // (uniform across a wave)
        unsigned out = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) out |= (unsigned)luma8(code8(f[r][0][q]), code8(f[r][1][q]), code8(f[r][2][q])) << (8 * q);
        uint8_t *yrow = p.y + (int64_t)(y0 + r) * p.ys + x0;
        if (whole) {
            *reinterpret_cast<unsigned *>(yrow) = out;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x0 + q < p.W) yrow[q] = (uint8_t)(out >> (8 * q));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the tiles
constexpr int TILE = DCVC_SHAKE_TILE, SROWS = DCVC_SHAKE_ROWS, STEP = TILE / SROWS, QUADS = TILE / 4, RMAX = DCVC_SHAKE_MAX_R;
constexpr int NGMAX = (RMAX + 2) / 2;                       // ceil((2 RMAX + 1) / 4)
constexpr int WHMAX = TILE - STEP + 1 + 2 * RMAX;           // 93 rows of window
constexpr int PITCH = (QUADS + NGMAX) | 1;                  // (words; odd: rows fall on other banks)
constexpr int TABLE = (2 * RMAX + 1) * 4 * NGMAX;           // 32-bit SADs, 4 NG a row
constexpr int THREADS = 256, PARTS = 4, PART_ROWS = SROWS / PARTS, BIAS = RMAX;
static_assert(TILE == 64 && SROWS == 16 && STEP == 4 && THREADS == SROWS * QUADS, "a thread per quad of the sampled rows");
static_assert(PITCH >= QUADS + NGMAX && PITCH == 25, "the widest row: sixteen quads and NG more words");
static_assert(PART_ROWS * TILE * 255 <= 65535, "four rows cannot carry out of a uint16 sum");
static_assert(SROWS * TILE * 255 < (1 << 18) && 2 * RMAX < 64 && 2 * BIAS < 128, "the key's fields");

struct TilesArgs {
    const float *rgb;
    const uint8_t *anchor;
    int32_t *tiles;
    int64_t ps;
    int32_t rs, H, W, ys, tw, R, pvec;
};

__device__ __forceinline__ unsigned long long pack64(unsigned lo, unsigned hi) { return (unsigned long long)hi << 32 | lo; }

__global__ __launch_bounds__(THREADS) void shake_tiles_kernel(const TilesArgs p) {
    __shared__ unsigned win[WHMAX * PITCH];  // the anchor: row = y - Y0 + R, byte = x - X0 + R
    __shared__ uint4 cur[SROWS][QUADS / 4];  // Y of cur's sampled rows, a byte per pixel
    __shared__ unsigned sad[TABLE];          // SAD of candidate (dy, dx) at (dy + R) * 4 ng + dx + R
    __shared__ unsigned long long best[THREADS / 64];
    __shared__ unsigned most[THREADS / 64];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * TILE, Y0 = blockIdx.y * TILE;
    const int R = p.R, ng = (R + 2) / 2, ww = TILE + 4 * ng, wh = TILE - STEP + 1 + 2 * R, side = 2 * R + 1;

    // ---- this thread's quad of cur: all loads first
    float c[3][4];
    {
        const int i = tid / QUADS, q = tid % QUADS;
        const float *at = p.rgb + (int64_t)(Y0 + STEP * i) * p.rs + X0 + 4 * q;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (p.pvec) {
                const float4 t = *reinterpret_cast<const float4 *>(at + k * p.ps);
                c[k][0] = t.x, c[k][1] = t.y, c[k][2] = t.z, c[k][3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) c[k][e] = at[k * p.ps + e];
            }
        }
    }
    // ---- the window, byte by byte, every coordinate clamped before the load; the table starts at zero
    const int npix = wh * ww;
#pragma unroll 4
    for (int pix = tid; pix < npix; pix += THREADS) {
        const int wy = pix / ww, wx = pix - wy * ww;
        const int y = min(max(Y0 - R + wy, 0), p.H - 1), x = min(max(X0 - R + wx, 0), p.W - 1);
        reinterpret_cast<uint8_t *>(win)[wy * (4 * PITCH) + wx] = p.anchor[(int64_t)y * p.ys + x];
    }
    for (int i = tid; i < side * 4 * ng; i += THREADS) sad[i] = 0u;
    {
        unsigned word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= (unsigned)luma8(code8(c[0][e]), code8(c[1][e]), code8(c[2][e])) << (8 * e);
        reinterpret_cast<unsigned *>(cur)[tid] = word;
    }
    __syncthreads();

    // ---- the units: (four sampled rows, a candidate group)
    const int groups = side * ng, units = groups * PARTS;
    for (int u = tid; u < units; u += THREADS) {
        const int part = u / groups, g = u - part * groups, dyi = g / ng, k = g - dyi * ng;
        unsigned long long acc = 0;  // four SADs, uint16 each
#pragma unroll
        for (int r = 0; r < PART_ROWS; ++r) {
            const int i = part * PART_ROWS + r;
            const unsigned *row = win + (STEP * i + dyi) * PITCH + k;
            unsigned w[QUADS + 1];
#pragma unroll
            for (int j = 0; j <= QUADS; ++j) w[j] = row[j];
#pragma unroll
            for (int j4 = 0; j4 < QUADS / 4; ++j4) {
                const uint4 q = cur[i][j4];
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w[4 * j4], w[4 * j4 + 1]), q.x, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w[4 * j4 + 1], w[4 * j4 + 2]), q.y, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w[4 * j4 + 2], w[4 * j4 + 3]), q.z, acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(w[4 * j4 + 3], w[4 * j4 + 4]), q.w, acc);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(&sad[dyi * (4 * ng) + 4 * k + e], (unsigned)(acc >> (16 * e)) & 0xffffu);
    }
    __syncthreads();

    // ---- the smallest key and the largest SAD
    unsigned long long key = ~0ull;
    unsigned top = 0;
    for (int cand = tid; cand < side * side; cand += THREADS) {
        const int dyi = cand / side, dxi = cand - dyi * side, dy = dyi - R, dx = dxi - R;
        const unsigned s = sad[dyi * (4 * ng) + dxi], len = (unsigned)(abs(dy) + abs(dx));
        const unsigned long long k64 = (unsigned long long)s << 20 | (unsigned long long)(len << 14 | (unsigned)(dy + BIAS) << 7 | (unsigned)(dx + BIAS));
        key = k64 < key ? k64 : key;
        top = max(top, s);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
        top = max(top, (unsigned)__shfl_xor((int)top, off));
    }
    if ((tid & 63) == 0) best[tid >> 6] = key, most[tid >> 6] = top;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < THREADS / 64; ++v) key = best[v] < key ? best[v] : key, top = max(top, most[v]);
        int32_t *out = p.tiles + (int64_t)DCVC_SHAKE_WORDS * ((int64_t)blockIdx.y * p.tw + blockIdx.x);
        out[0] = (int)((key >> 7) & 127u) - BIAS;
        out[1] = (int)(key & 127u) - BIAS;
        out[2] = (int)(key >> 20);
        out[3] = (int)top;
        out[4] = (int)sad[R * (4 * ng) + R];
    }
}

// ------------------------------------------------------------------------------------------------------------- the vote
constexpr int VOTE_THREADS = 1024, BINS = 2 * RMAX + 1;

__device__ __forceinline__ bool votes(const int32_t *t, int R) {
    return abs(t[0]) <= R && abs(t[1]) <= R && t[3] > 0 && 2 * (int64_t)t[2] <= (int64_t)t[3];
}

__device__ __forceinline__ int lower_median(const int *bins, int n, int R) {
    int run = 0;
    for (int b = 0; b < 2 * R + 1; ++b) {
        run += bins[b];
        if (run > (n - 1) / 2) return b - R;
    }
    return 0;
}

__global__ __launch_bounds__(VOTE_THREADS) void shake_vote_kernel(const int32_t *tiles, int n_tiles, int R, int min_votes, int cells,
                                                                  int32_t *record, int16_t *mv) {
    __shared__ int hy[BINS], hx[BINS], found[4];  // found: my, mx, n, agree
    const int tid = threadIdx.x;
    if (tid < BINS) hy[tid] = 0, hx[tid] = 0;
    if (tid < 4) found[tid] = 0;
    __syncthreads();
    for (int t = tid; t < n_tiles; t += VOTE_THREADS) {
        const int32_t *rec = tiles + (int64_t)DCVC_SHAKE_WORDS * t;
        if (votes(rec, R)) atomicAdd(&hy[rec[0] + R], 1), atomicAdd(&hx[rec[1] + R], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int b = 0; b < 2 * R + 1; ++b) n += hy[b];
        found[2] = n;
        if (n > 0) found[0] = lower_median(hy, n, R), found[1] = lower_median(hx, n, R);
    }
    __syncthreads();
    const int my = found[0], mx = found[1], n = found[2];
    int same = 0;
    for (int t = tid; t < n_tiles; t += VOTE_THREADS) {
        const int32_t *rec = tiles + (int64_t)DCVC_SHAKE_WORDS * t;
        same += votes(rec, R) && rec[0] == my && rec[1] == mx;
    }
    if (same) atomicAdd(&found[3], same);
    __syncthreads();
    const int status = (n < min_votes ? DCVC_SHAKE_FEW : 0) | (abs(my) == R || abs(mx) == R ? DCVC_SHAKE_EDGE : 0);
    const int dy = status ? 0 : my, dx = status ? 0 : mx;
    if (tid == 0) {
        record[0] = dy, record[1] = dx, record[2] = n, record[3] = found[3];
        record[4] = n_tiles, record[5] = status, record[6] = my, record[7] = mx;
    }
    for (int c = tid; c < cells; c += VOTE_THREADS) mv[2 * c] = (int16_t)-dy, mv[2 * c + 1] = (int16_t)-dx;
}

inline bool plane_ok(const void *y, int32_t ys, int32_t W) { return y && ys >= W && ys % 4 == 0 && aligned(y, 4); }

}  // namespace

extern "C" int dcvc_shake_plane(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint8_t *y,
                                int32_t y_stride, void *stream) {
    if (!size_ok(H, W) || !planes_ok(rgb, row_stride, plane_stride, H, W) || !plane_ok(y, y_stride, W) || !aligned(rgb, 4))
        return DCVC_E_ARG;
    PlaneArgs a{};
    a.rgb = rgb, a.y = y, a.ps = plane_stride, a.rs = row_stride, a.H = H, a.W = W, a.ys = y_stride;
    a.pvec = vec_ok(rgb, row_stride, plane_stride);
    const dim3 block(64, 4), grid(nblk(W, STRIP_W), nblk(H, STRIP_H));
    shake_plane_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_shake_tiles(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W,
                                const uint8_t *anchor, int32_t y_stride, int32_t R, int32_t *tiles, void *stream) {
    if (!tiles || !size_ok(H, W) || !planes_ok(rgb, row_stride, plane_stride, H, W) || !plane_ok(anchor, y_stride, W) || R < 1 ||
        R > DCVC_SHAKE_MAX_R || !aligned(rgb, 4) || !aligned(tiles, 4))
        return DCVC_E_ARG;
    const int th = H / TILE, tw = W / TILE;
    if (th * tw == 0) return DCVC_OK;
    TilesArgs a{};
    a.rgb = rgb, a.anchor = anchor, a.tiles = tiles, a.ps = plane_stride, a.rs = row_stride, a.H = H, a.W = W, a.ys = y_stride;
    a.tw = tw, a.R = R, a.pvec = vec_ok(rgb, row_stride, plane_stride);
    shake_tiles_kernel<<<dim3(tw, th), dim3(THREADS), 0, (hipStream_t)stream>>>(a);
    RET_LAUNCH();
}

extern "C" int dcvc_shake_vote(const int32_t *tiles, int32_t n_tiles, int32_t R, int32_t min_votes, int32_t H, int32_t W,
                               int32_t *record, int16_t *mv, void *stream) {
    if (!tiles || !record || !mv || n_tiles < 0 || n_tiles > DCVC_SHAKE_MAX_TILES || R < 1 || R > DCVC_SHAKE_MAX_R || min_votes < 1 ||
        min_votes > DCVC_SHAKE_MAX_TILES || !size_ok(H, W) || !aligned(tiles, 4) || !aligned(record, 4) || !aligned(mv, 2))
        return DCVC_E_ARG;
    const int cells = 4 * ((H + 63) / 64) * 4 * ((W + 63) / 64);
    shake_vote_kernel<<<dim3(1), dim3(VOTE_THREADS), 0, (hipStream_t)stream>>>(tiles, n_tiles, R, min_votes, cells, record, mv);
    RET_LAUNCH();
}
