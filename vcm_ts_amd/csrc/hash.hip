// hash.hip -- the CRC-32 of a picture on the device (include/dcvc_hip_hash.h, which defines the byte strings and states the
// algebra; this file only arranges it).
//
// The byte string M is extended IN FRONT, virtually, by zero bytes to a whole number of blocks: a CRC register that starts
// from 0 stays 0 over zero bytes, so crc0 of the extended string is crc0(M), every chunk has the same length, every
// workgroup the same shape, and the last chunk ends exactly on the last byte -- there is no tail case anywhere.  A lane
// whose chunk begins before M feeds zeros (or, for whole words, nothing) until M begins.
//
// Launch 1 (one workgroup of 4 waves per block of 256 chunks): a lane walks its chunk of 192 bytes -- 48 fp32 words, or
// 64 pixels whose twelve codes per four pixels are packed into three words -- through slicing-by-4 tables in LDS (4 KB,
// computed by the workgroup itself: entry (k, t) is byte t followed by k zero bytes).  Loads are issued in batches ahead
// of the table walk.  The 64 lanes of a wave are then combined by a shuffle tree (level k: the left half times
// x^(8 * 192 * 2^k), xor the right half), the four waves by Horner through LDS, and ONE lane stores the block's partial
// with a vector store.  The multipliers are pure functions of the constants and arrive as kernel arguments.
//
// Launch 2 (one wave): lane j folds its run of partials by Horner (the run count is extended in front by zero partials,
// the same trick), the shuffle tree combines the lanes, and lane 0 applies the init and xorout terms and stores the word.
// No flags, no counters, no atomics: the kernel boundary is the synchronisation, and the value is a pure function of M.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crc_common.h"
#include "dcvc_hip.h"
#include "dcvc_hip_hash.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

extern "C" {
const int32_t dcvc_hash_chunk_bytes = DCVC_HASH_CHUNK_BYTES;
const int32_t dcvc_hash_block_bytes = DCVC_HASH_BLOCK_BYTES;
const int32_t dcvc_hash_scratch_bytes = DCVC_HASH_SCRATCH_BYTES;
}

namespace {

constexpr int CHUNK = DCVC_HASH_CHUNK_BYTES, LANES = 256, WAVE = 64, LEVELS = 6;
constexpr int CHUNK_WORDS = CHUNK / 4, CHUNK_PIXELS = CHUNK / 3, BATCH = 8;
static_assert(CHUNK % 12 == 0 && DCVC_HASH_BLOCK_BYTES == LANES * CHUNK, "a chunk starts on a pixel and on a word");
static_assert(CHUNK_WORDS % BATCH == 0 && CHUNK_PIXELS % 4 == 0 && (1 << LEVELS) == WAVE, "batches and the wave tree");

struct HashArgs {
    const float *src;
    uint32_t *partial;
    int64_t ps, front;  // front: the virtual zero units (words or pixels) before M
    int32_t rs, H, W;
    uint32_t xlane[LEVELS], xwave;  // x^(8 * CHUNK * 2^k); x^(8 * CHUNK * 64)
};

struct FoldArgs {
    const uint32_t *partial;
    uint32_t *out;
    int32_t per_lane, front;  // front: the virtual zero partials before the first
    uint32_t xblock, xlane[LEVELS], init;  // x^(8 * BLOCK); x^(8 * BLOCK * per_lane * 2^k); 0xFFFFFFFF * x^(8 |M|)
};

// entry (k, t): the register after byte t and k zero bytes
__device__ __forceinline__ void make_tables(uint32_t *T, int tid) {
    uint32_t r = (uint32_t)tid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int b = 0; b < 8; ++b) r = (r >> 1) ^ (POLY & (0u - (r & 1u)));
        T[k * 256 + tid] = r;
    }
}

// four bytes more: the first byte of M is the word's lowest
__device__ __forceinline__ uint32_t word_step(const uint32_t *T, uint32_t crc, uint32_t w) {
    crc ^= w;
    return T[3 * 256 + (crc & 255u)] ^ T[2 * 256 + ((crc >> 8) & 255u)] ^ T[256 + ((crc >> 16) & 255u)] ^ T[crc >> 24];
}

// lane l holds crc0 of piece l of 64 consecutive pieces, each `x[0]` = x^(8 |piece|): lane 0 returns crc0 of all of them
__device__ __forceinline__ uint32_t wave_combine(uint32_t crc, const uint32_t *x) {
#pragma unroll
    for (int k = 0; k < LEVELS; ++k) {
        const uint32_t right = (uint32_t)__shfl_down((int)crc, 1 << k);
        crc = mulmod(crc, x[k]) ^ right;  // (valid in the lanes that are multiples of 2^(k+1); lane 0 reads only those)
    }
    return crc;
}

__device__ __forceinline__ void block_store(uint32_t crc, const HashArgs &p, uint32_t *waves, int tid) {
    crc = wave_combine(crc, p.xlane);
    if ((tid & (WAVE - 1)) == 0) waves[tid / WAVE] = crc;
    __syncthreads();
    if (tid == 0) {
        uint32_t r = waves[0];
#pragma unroll
        for (int w = 1; w < LANES / WAVE; ++w) r = mulmod(r, p.xwave) ^ waves[w];
        p.partial[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(256) void hash_f32_kernel(const HashArgs p) {
    __shared__ uint32_t T[4 * 256], waves[LANES / WAVE];
    const int tid = threadIdx.x;
    make_tables(T, tid);
    __syncthreads();
    // element e of M (order c, y, x) is word e; this lane's chunk is the words e0 .. e0 + 47, those below 0 virtual
    const int64_t e0 = ((int64_t)blockIdx.x * LANES + tid) * CHUNK_WORDS - p.front;
    uint32_t crc = 0;
    if (e0 + CHUNK_WORDS > 0) {
        const int64_t s = e0 < 0 ? 0 : e0, HW = (int64_t)p.H * p.W;
        int64_t c = s / HW;
        const int64_t r = s - c * HW;
        int y = (int)(r / p.W), x = (int)(r - (int64_t)y * p.W);
        const float *row = p.src + c * p.ps + (int64_t)y * p.rs;
        for (int b = 0; b < CHUNK_WORDS; b += BATCH) {
            uint32_t w[BATCH];
#pragma unroll
            for (int j = 0; j < BATCH; ++j) {
                const bool real = e0 + b + j >= 0;
                w[j] = real ? __float_as_uint(row[x]) : 0u;  // (a virtual word: the lane still stands on M's first)
                if (real && ++x == p.W) {  // (after M's last word the row is computed and never read)
                    x = 0;
                    if (++y == p.H) y = 0, ++c;
                    row = p.src + c * p.ps + (int64_t)y * p.rs;
                }
            }
#pragma unroll
            for (int j = 0; j < BATCH; ++j) crc = word_step(T, crc, w[j]);
        }
    }
    block_store(crc, p, waves, tid);
}

__global__ __launch_bounds__(256) void hash_pixels_kernel(const HashArgs p) {
    __shared__ uint32_t T[4 * 256], waves[LANES / WAVE];
    const int tid = threadIdx.x;
    make_tables(T, tid);
    __syncthreads();
    // pixel q of M (row-major) is the bytes 3 q .. 3 q + 2; this lane's chunk is the pixels q0 .. q0 + 63
    const int64_t q0 = ((int64_t)blockIdx.x * LANES + tid) * CHUNK_PIXELS - p.front;
    uint32_t crc = 0;
    if (q0 + CHUNK_PIXELS > 0) {
        const int64_t s = q0 < 0 ? 0 : q0;
        int y = (int)(s / p.W), x = (int)(s - (int64_t)y * p.W);
        const float *row = p.src + (int64_t)y * p.rs;
        for (int b = 0; b < CHUNK_PIXELS; b += 4) {
            uint32_t k[4][3];  // twelve codes: the loads of four pixels are issued before the table walk
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool real = q0 + b + j >= 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) k[j][c] = real ? (uint32_t)code8(row[c * p.ps + x]) : 0u;
                if (real && ++x == p.W) x = 0, ++y, row += p.rs;  // (after M's last pixel: computed, never read)
            }
            crc = word_step(T, crc, k[0][0] | k[0][1] << 8 | k[0][2] << 16 | k[1][0] << 24);
            crc = word_step(T, crc, k[1][1] | k[1][2] << 8 | k[2][0] << 16 | k[2][1] << 24);
            crc = word_step(T, crc, k[2][2] | k[3][0] << 8 | k[3][1] << 16 | k[3][2] << 24);
        }
    }
    block_store(crc, p, waves, tid);
}

__global__ __launch_bounds__(64) void hash_fold_kernel(const FoldArgs p) {
    const int lane = threadIdx.x;
    uint32_t crc = 0;
    for (int s = 0; s < p.per_lane; ++s) {
        const int q = lane * p.per_lane + s - p.front;
        crc = mulmod(crc, p.xblock) ^ (q >= 0 ? p.partial[q] : 0u);
    }
    crc = wave_combine(crc, p.xlane);
    if (lane == 0) *p.out = crc ^ p.init ^ 0xFFFFFFFFu;
}

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// both launches of a digest over `bytes` bytes in units (words or pixels) of `unit` bytes
template <typename K>
int launch(K kernel, HashArgs a, int64_t bytes, int unit, uint32_t *out, uint32_t *scratch, void *stream) {
    constexpr int64_t BLOCK = DCVC_HASH_BLOCK_BYTES;
    const int64_t blocks = (bytes + BLOCK - 1) / BLOCK;
    a.partial = scratch;
    a.front = (blocks * BLOCK - bytes) / unit;
    uint32_t x = x8n(CHUNK);
    for (int k = 0; k < LEVELS; ++k, x = mulmod(x, x)) a.xlane[k] = x;
    a.xwave = x;  // x^(8 * CHUNK * 64)
    kernel<<<dim3((unsigned)blocks), dim3(LANES), 0, (hipStream_t)stream>>>(a);
    if (hipGetLastError() != hipSuccess) return DCVC_E_LAUNCH;
    FoldArgs f{};
    f.partial = scratch, f.out = out;
    f.per_lane = (int32_t)((blocks + WAVE - 1) / WAVE);
    f.front = (int32_t)((int64_t)f.per_lane * WAVE - blocks);
    f.xblock = x8n(BLOCK);
    x = x8n((uint64_t)BLOCK * f.per_lane);
    for (int k = 0; k < LEVELS; ++k, x = mulmod(x, x)) f.xlane[k] = x;
    f.init = mulmod(0xFFFFFFFFu, x8n((uint64_t)bytes));
    hash_fold_kernel<<<dim3(1), dim3(WAVE), 0, (hipStream_t)stream>>>(f);
    RET_LAUNCH();
}

bool bad_plane(const float *src, int32_t rs, int64_t ps, int32_t H, int32_t W, const uint32_t *out, const uint32_t *scratch) {
    return !src || !out || !scratch || H < 1 || W < 1 || H > DCVC_HASH_MAX_SIDE || W > DCVC_HASH_MAX_SIDE || rs < W ||
           ps < (int64_t)(H - 1) * rs + W || !aligned4(src) || !aligned4(out) || !aligned4(scratch);
}

}  // namespace

extern "C" int dcvc_hash_pixels(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint32_t *out,
                                uint32_t *scratch, void *stream) {
    if (bad_plane(rgb, row_stride, plane_stride, H, W, out, scratch) || 3 * (int64_t)H * W >= ((int64_t)1 << 32))
        return DCVC_E_ARG;
    HashArgs a{};
    a.src = rgb, a.rs = row_stride, a.ps = plane_stride, a.H = H, a.W = W;
    return launch(hash_pixels_kernel, a, 3 * (int64_t)H * W, 3, out, scratch, stream);
}

extern "C" int dcvc_hash_f32(const float *src, int32_t row_stride, int64_t plane_stride, int32_t C, int32_t H, int32_t W,
                             uint32_t *out, uint32_t *scratch, void *stream) {
    if (bad_plane(src, row_stride, plane_stride, H, W, out, scratch) || C < 1 || C > DCVC_HASH_MAX_SIDE ||
        4 * (int64_t)C * H * W >= ((int64_t)1 << 32))
        return DCVC_E_ARG;
    HashArgs a{};
    a.src = src, a.rs = row_stride, a.ps = plane_stride, a.H = H, a.W = W;
    return launch(hash_f32_kernel, a, 4 * (int64_t)C * H * W, 4, out, scratch, stream);
}
