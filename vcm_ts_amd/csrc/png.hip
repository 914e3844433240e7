// png.hip -- a picture on the device as a finished .png file (include/dcvc_hip_png.h, which defines every byte; this file
// only arranges it; the tables' check is png_check.cpp).
//
// Launch A (one workgroup of 4 waves per band).  LDS holds the band's string (24 KB), the image of its chunk from "IDAT"
// on (24 KB; before the string exists, the band's unfiltered codes), a histogram that later becomes the chosen preset's
// codes, the segments' bit counts and a CRC table: 52 KB, three workgroups to a CU.
//   1. codes: every lane converts pixels of the band's rows into the image buffer (coalesced loads along x).
//   2. filters: ONE WAVE PER ROW -- the five costs by wave reductions, the choice, the filtered row into the string.  The
//      row above the band's first row is converted from the source again (never staged).  No workgroup barrier inside.
//   3. tokens: one wave per segment, one lane per byte.  With E = the ballot of "equals the byte before", a lane's run of
//      set bits is found with two bit scans; the run's first lane owns the match, every lane outside a run of >= 3 a
//      literal.  Symbols are counted with LDS adds.
//   4. prices: 8 lanes per preset dot the histogram with the lengths; one lane picks the coding.
//   5. bits: segments' totals, a scan of them by one wave, then every token is ORed into the image at its offset (LDS ORs
//      join the boundary words); the header's words likewise.  A stored band is copied instead.
//   6. CRC-32 by the algebra of dcvc_hip_hash.h: 256 equal pieces of the zero-extended chunk, a shuffle tree, Horner over
//      the waves.  Adler partials in 64-bit sums.  Then the slot is written with word stores.
// Launch B (bands + 1 workgroups): workgroup b sums the sizes in front of band b and copies its chunk with word stores
// where the file's words are whole and byte stores at both ends; the last workgroup sums everything, combines Adler and
// writes prefix, trailer and size.  The kernel boundary is the only synchronisation between workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "crc_common.h"
#include "dcvc_hip.h"
#include "dcvc_hip_png.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256, WAVE = 64, WAVES = LANES / WAVE, LEVELS = 6;
constexpr int NSYM = DCVC_PNG_SYMBOLS, SEG = DCVC_PNG_SEG, MAX_SEGS = DCVC_PNG_BAND_MAX / SEG;
constexpr int SLOT_WORDS = DCVC_PNG_SLOT_BYTES / 4, META_WORDS = 4, IMG_WORDS = SLOT_WORDS - META_WORDS;
constexpr uint32_t ADLER = 65521u, IDAT = 0x54414449u;  // "IDAT" as the little-endian word of its bytes
static_assert(SEG == WAVE && DCVC_PNG_BAND_MAX % SEG == 0 && DCVC_PNG_SLOT_BYTES % 4 == 0, "a lane per byte of a segment");
static_assert(4 * IMG_WORDS >= 8 + 5 + DCVC_PNG_BAND_MAX, "a stored band's chunk from its type on fits the image");
static_assert(DCVC_PNG_PRESET_WORDS == NSYM + 1 + DCVC_PNG_HEADER_WORDS + 1 && DCVC_PNG_HEADER_WORDS <= LANES, "the preset's layout");

struct BandArgs {
    const float *src;
    const uint32_t *tables;
    uint32_t *staging;
    int64_t ps;
    int32_t rs, H, W, R, K;
};

struct PackArgs {
    const uint32_t *staging;
    uint8_t *file;
    uint32_t *size_word;
    int64_t capacity;
    int32_t H, W, R, bands;
};

// the five filtered bytes of x with a = left, b = above, c = above left
__device__ __forceinline__ void filter5(int x, int a, int b, int c, int *f) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x, f[1] = (x - a) & 255, f[2] = (x - b) & 255, f[3] = (x - ((a + b) >> 1)) & 255, f[4] = (x - paeth) & 255;
}

// The token a lane owns, of the segment whose "equals the byte before" bits are E: its symbol (-1: none -- the lane is
// beyond the string or inside a match another lane owns), and the bits that follow the symbol's code: `extra` holds the
// length's extra bits and, above them, the distance code 0; ebits counts both.
__device__ __forceinline__ int token(unsigned long long E, int lane, bool valid, int byte, int &extra, int &ebits) {
    extra = 0, ebits = 0;
    if (!valid) return -1;
    if (!((E >> lane) & 1ull)) return byte;
    const unsigned long long below = ~E & ((1ull << lane) - 1ull);  // (bit 0 of E is never set: below != 0)
    const int start = 64 - __builtin_clzll(below), L = __builtin_ctzll(~(E >> start));
    if (L < 3) return byte;
    if (lane != start) return -1;
    if (L <= 10) {
        ebits = 1;
        return 254 + L;
    }
    const int e = L <= 18 ? 1 : L <= 34 ? 2 : 3, base = 3 + (4 << e);
    extra = (L - base) & ((1 << e) - 1), ebits = e + 1;
    return 261 + 4 * e + ((L - base) >> e);
}

// the segment's byte of this lane and the segment's E
__device__ __forceinline__ unsigned long long segment(const uint8_t *str, int n, int s, int lane, bool &valid, int &byte) {
    const int pos = s * SEG + lane;
    valid = pos < n;
    byte = valid ? str[pos] : 0;
    const int prev = __shfl_up(byte, 1);
    return __ballot(valid && lane > 0 && byte == prev);
}

__device__ __forceinline__ void or_bits(uint32_t *img, uint32_t at, unsigned long long v) {
    v <<= (at & 31u);
    if ((uint32_t)v) atomicOr(&img[at >> 5], (uint32_t)v);
    if ((uint32_t)(v >> 32)) atomicOr(&img[(at >> 5) + 1], (uint32_t)(v >> 32));
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}

// the sum of v over the workgroup, in every lane; red: WAVES words of LDS, free again on return
__device__ __forceinline__ unsigned long long block_sum64(unsigned long long v, unsigned long long *red, int tid) {
    v = wave_sum64(v);
    __syncthreads();
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = v;
    __syncthreads();
    unsigned long long r = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) r += red[w];
    return r;
}

__global__ __launch_bounds__(LANES) void png_band_kernel(const BandArgs p) {
    __shared__ uint32_t str_w[DCVC_PNG_BAND_MAX / 4], img[IMG_WORDS], hist[NSYM + 2], segbits[MAX_SEGS + 1], T[256];
    __shared__ uint32_t price[DCVC_PNG_MAX_PRESETS], pick[2], wcrc[WAVES];
    __shared__ unsigned long long red[WAVES];
    uint8_t *const str = reinterpret_cast<uint8_t *>(str_w), *const img8 = reinterpret_cast<uint8_t *>(img);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int W = p.W, rb = 3 * W, y0 = (int)blockIdx.x * p.R, rows = min(p.R, p.H - y0), n = rows * (rb + 1);
    const int nseg = (n + SEG - 1) / SEG;

    {  // the CRC table (the register after byte t), an empty histogram, and the band's codes
        uint32_t r = (uint32_t)tid;
#pragma unroll
        for (int b = 0; b < 8; ++b) r = (r >> 1) ^ (POLY & (0u - (r & 1u)));
        T[tid] = r;
        for (int s = tid; s < NSYM + 2; s += LANES) hist[s] = 0;
        for (int q = tid; q < rows * W; q += LANES) {
            const int y = q / W, x = q - y * W;
            const float *px = p.src + (int64_t)(y0 + y) * p.rs + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) img8[3 * q + c] = (uint8_t)code8(px[c * p.ps]);
        }
    }
    __syncthreads();

    for (int r = wave; r < rows; r += WAVES) {  // a wave filters a row
        const uint8_t *cur = img8 + r * rb;
        const bool top = y0 + r == 0, staged = r > 0;
        const float *above = p.src + (int64_t)(y0 + r - 1) * p.rs;  // (read only where the row above is neither absent nor staged)
        auto up = [&](int i) -> int {
            if (top) return 0;
            if (staged) return cur[i - rb];
            const int x = i / 3;
            return code8(above[(i - 3 * x) * p.ps + x]);
        };
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        int f[5];
        for (int i = lane; i < rb; i += WAVE) {
            filter5(cur[i], i >= 3 ? cur[i - 3] : 0, up(i), i >= 3 ? up(i - 3) : 0, f);
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += (uint32_t)min(f[t], 256 - f[t]);
        }
        int best = 0;
        uint32_t least = wave_sum(cost[0]);
#pragma unroll
        for (int t = 1; t < 5; ++t) {
            const uint32_t c = wave_sum(cost[t]);
            if (c < least) least = c, best = t;
        }
        uint8_t *out = str + r * (rb + 1);
        if (lane == 0) out[0] = (uint8_t)best;
        for (int i = lane; i < rb; i += WAVE) {
            filter5(cur[i], i >= 3 ? cur[i - 3] : 0, up(i), i >= 3 ? up(i - 3) : 0, f);
            out[1 + i] = (uint8_t)f[best];
        }
    }
    __syncthreads();

    for (int s = wave; s < nseg; s += WAVES) {  // the symbols' counts
        bool valid;
        int byte, extra, ebits;
        const unsigned long long E = segment(str, n, s, lane, valid, byte);
        const int sym = token(E, lane, valid, byte, extra, ebits);
        if (sym >= 0) atomicAdd(&hist[sym], 1u);
    }
    __syncthreads();

    {  // the presets' prices in bytes: 8 lanes each
        const int k = tid >> 3, j = tid & 7;
        const uint32_t *t = p.tables + (k < p.K ? k : 0) * DCVC_PNG_PRESET_WORDS;
        uint32_t bits = 0;
        for (int s = j; s < NSYM; s += 8) {
            const uint32_t h = hist[s];
            if (h) bits += h * ((t[s] >> 16) + (s < 265 ? 0u : (uint32_t)(s - 261) >> 2) + (s > 256 ? 1u : 0u));
        }
        bits += (uint32_t)__shfl_xor((int)bits, 1);
        bits += (uint32_t)__shfl_xor((int)bits, 2);
        bits += (uint32_t)__shfl_xor((int)bits, 4);
        if (j == 0 && k < p.K) {
            const uint32_t D = 3u + t[NSYM] + bits + (t[256] >> 16);
            price[k] = (D & 7u) ? (D + 3u + 7u) / 8u + 4u : D / 8u;
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t best = 5u + (uint32_t)n, which = 0xFFFFFFFFu;  // stored, unless a preset takes fewer bytes
        for (int k = 0; k < p.K; ++k)
            if (price[k] < best) best = price[k], which = (uint32_t)k;
        pick[0] = which, pick[1] = best;
    }
    __syncthreads();
    const uint32_t which = pick[0], bytes = pick[1];

    if (which == 0xFFFFFFFFu) {
        for (int i = tid; i < n; i += LANES) img8[9 + i] = str[i];
        if (tid == 0) {
            img[0] = IDAT;
            img8[4] = 0, img8[5] = (uint8_t)n, img8[6] = (uint8_t)(n >> 8), img8[7] = (uint8_t)~n, img8[8] = (uint8_t)(~n >> 8);
        }
    } else {
        const uint32_t *t = p.tables + which * DCVC_PNG_PRESET_WORDS;
        uint32_t *codes = hist;  // (the counts have been priced)
        for (int s = tid; s < NSYM; s += LANES) codes[s] = t[s];
        for (int i = tid; i < (int)(8u + bytes + 3u) / 4; i += LANES) img[i] = i ? 0u : IDAT;
        __syncthreads();
        for (int s = wave; s < nseg; s += WAVES) {  // the segments' bits
            bool valid;
            int byte, extra, ebits;
            const unsigned long long E = segment(str, n, s, lane, valid, byte);
            const int sym = token(E, lane, valid, byte, extra, ebits);
            const uint32_t total = wave_sum(sym >= 0 ? (codes[sym] >> 16) + (uint32_t)ebits : 0u);
            if (lane == 0) segbits[s] = total;
        }
        __syncthreads();
        if (wave == 0) {  // segbits[s]: the bits in front of segment s; segbits[nseg]: all
            const int per = (nseg + WAVE - 1) / WAVE, s0 = lane * per;
            uint32_t mine = 0;
            for (int s = s0; s < min(s0 + per, nseg); ++s) mine += segbits[s];
            uint32_t incl = mine;
#pragma unroll
            for (int k = 0; k < LEVELS; ++k) {
                const uint32_t left = (uint32_t)__shfl_up((int)incl, 1 << k);
                if (lane >= (1 << k)) incl += left;
            }
            uint32_t at = incl - mine;
            for (int s = s0; s < min(s0 + per, nseg); ++s) {
                const uint32_t b = segbits[s];
                segbits[s] = at, at += b;
            }
            if (lane == WAVE - 1) segbits[nseg] = incl;
        }
        __syncthreads();
        const uint32_t hbits = t[NSYM], first = 32u + 3u + hbits;  // (the data begins behind the chunk's type)
        if (tid == 0) or_bits(img, 32u, 4ull);                    // BFINAL = 0, BTYPE = 10
        if (tid < DCVC_PNG_HEADER_WORDS && 32u * tid < hbits) or_bits(img, 35u + 32u * tid, t[NSYM + 1 + tid]);
        for (int s = wave; s < nseg; s += WAVES) {
            bool valid;
            int byte, extra, ebits;
            const unsigned long long E = segment(str, n, s, lane, valid, byte);
            const int sym = token(E, lane, valid, byte, extra, ebits);
            const uint32_t c = sym >= 0 ? codes[sym] : 0u, len = c >> 16, mine = sym >= 0 ? len + (uint32_t)ebits : 0u;
            uint32_t incl = mine;
#pragma unroll
            for (int k = 0; k < LEVELS; ++k) {
                const uint32_t left = (uint32_t)__shfl_up((int)incl, 1 << k);
                if (lane >= (1 << k)) incl += left;
            }
            if (sym >= 0) or_bits(img, first + segbits[s] + incl - mine, (unsigned long long)(c & 0xFFFFu) | (unsigned long long)extra << len);
        }
        if (tid == 0) {  // the end of the block and, off a byte boundary, the empty stored block
            const uint32_t at = first + segbits[nseg], D = at + (codes[256] >> 16) - 32u;
            or_bits(img, at, codes[256] & 0xFFFFu);
            if (D & 7u) or_bits(img, 32u + 8u * (bytes - 2u), 0xFFFFull);
        }
    }
    __syncthreads();

    {  // the chunk's CRC-32 over type and data, and the Adler partials of the string
        const uint32_t m = 4u + bytes, c = (m + LANES - 1) / LANES, front = LANES * c - m;
        uint32_t crc = 0;
        for (uint32_t v = tid * c; v < (tid + 1) * c; ++v) crc = T[(crc ^ (v >= front ? img8[v - front] : 0u)) & 255u] ^ (crc >> 8);
        uint32_t x = x8n(c);
#pragma unroll 1
        for (int k = 0; k < LEVELS; ++k) {
            const uint32_t right = (uint32_t)__shfl_down((int)crc, 1 << k);
            crc = mulmod(crc, x) ^ right;
            x = mulmod(x, x);
        }
        if (lane == 0) wcrc[wave] = crc;
        unsigned long long a = 0, b = 0;
        for (int i = tid; i < n; i += LANES) a += str[i], b += (unsigned long long)(n - i) * str[i];
        a = block_sum64(a, red, tid);  // (its barriers also publish wcrc)
        b = block_sum64(b, red, tid);
        if (tid == 0) {
            uint32_t r = wcrc[0];
#pragma unroll 1
            for (int w = 1; w < WAVES; ++w) r = mulmod(r, x) ^ wcrc[w];  // x: x^(8 * 64 c)
            r ^= mulmod(0xFFFFFFFFu, x8n(m)) ^ 0xFFFFFFFFu;
            img8[m] = (uint8_t)(r >> 24), img8[m + 1] = (uint8_t)(r >> 16), img8[m + 2] = (uint8_t)(r >> 8), img8[m + 3] = (uint8_t)r;
            uint32_t *meta = p.staging + (int64_t)blockIdx.x * SLOT_WORDS;
            meta[0] = bytes, meta[1] = (uint32_t)(a % ADLER), meta[2] = (uint32_t)(b % ADLER), meta[3] = (uint32_t)n;
        }
    }
    __syncthreads();
    uint32_t *slot = p.staging + (int64_t)blockIdx.x * SLOT_WORDS + META_WORDS;
    for (int i = tid; i < (int)(8u + bytes + 3u) / 4; i += LANES) slot[i] = img[i];
}

// zlib's crc32 of n bytes, one bit at a time (the prefix and the trailer: a few dozen bytes, once per picture)
__device__ uint32_t crc_bytes(const uint8_t *b, int n) {
    uint32_t crc = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) {
        crc ^= b[i];
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (POLY & (0u - (crc & 1u)));
    }
    return ~crc;
}

__device__ __forceinline__ void put_be32(uint8_t *b, uint32_t v) { b[0] = (uint8_t)(v >> 24), b[1] = (uint8_t)(v >> 16), b[2] = (uint8_t)(v >> 8), b[3] = (uint8_t)v; }

// a chunk of n data bytes already at b + 8: its length, type and CRC around them
__device__ void close_chunk(uint8_t *b, const char *type, int n) {
    put_be32(b, (uint32_t)n);
    for (int i = 0; i < 4; ++i) b[4 + i] = (uint8_t)type[i];
    put_be32(b + 8 + n, crc_bytes(b + 4, 4 + n));
}

__global__ __launch_bounds__(LANES) void png_pack_kernel(const PackArgs p) {
    __shared__ unsigned long long red[WAVES];
    __shared__ uint8_t head[DCVC_PNG_PREFIX_BYTES + 1], tail[DCVC_PNG_TRAILER_BYTES + 3];
    const int tid = threadIdx.x, b = (int)blockIdx.x, in_front = min(b, p.bands);
    const bool last = b == p.bands;
    const unsigned long long rowlen = 3ull * (unsigned long long)p.W + 1ull, N = (unsigned long long)p.H * rowlen;
    unsigned long long size = 0, s1 = 0, s2 = 0;
    for (int j = tid; j < in_front; j += LANES) {
        const uint32_t *meta = p.staging + (int64_t)j * SLOT_WORDS;
        size += 12ull + meta[0];
        if (last) {
            const unsigned long long after = N - (unsigned long long)min((int64_t)(j + 1) * p.R, (int64_t)p.H) * rowlen;
            s1 += meta[1], s2 += (meta[2] + (after % ADLER) * meta[1]) % ADLER;
        }
    }
    const unsigned long long at = DCVC_PNG_PREFIX_BYTES + block_sum64(size, red, tid);
    if (!last) {
        const uint32_t *slot = p.staging + (int64_t)b * SLOT_WORDS, len = 8u + slot[0];
        if ((int64_t)(at + 4ull + len) + DCVC_PNG_TRAILER_BYTES > p.capacity) return;  // (cannot happen within the bound; nothing is written past it)
        if (tid < 4) p.file[at + tid] = (uint8_t)(slot[0] >> (24 - 8 * tid));
        const unsigned long long d = at + 4ull, end = d + len;
        for (unsigned long long a = (d & ~3ull) + 4ull * tid; a < end; a += 4ull * LANES) {
            if (a >= d && a + 4ull <= end) {  // a whole word of the file: from one or two words of the slot
                const uint32_t s = (uint32_t)(a - d), sh = 8u * (s & 3u), w = slot[META_WORDS + (s >> 2)];
                *reinterpret_cast<uint32_t *>(p.file + a) = sh ? (w >> sh) | (slot[META_WORDS + (s >> 2) + 1] << (32u - sh)) : w;
            } else {
                for (unsigned long long g = a < d ? d : a; g < a + 4ull && g < end; ++g) {
                    const uint32_t s = (uint32_t)(g - d);
                    p.file[g] = (uint8_t)(slot[META_WORDS + (s >> 2)] >> (8u * (s & 3u)));
                }
            }
        }
        return;
    }
    s1 = block_sum64(s1, red, tid);
    s2 = block_sum64(s2, red, tid);
    const bool fits = (int64_t)at + DCVC_PNG_TRAILER_BYTES <= p.capacity;
    if (tid == 0) {
        const uint8_t sig[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
        for (int i = 0; i < 8; ++i) head[i] = sig[i];
        put_be32(head + 16, (uint32_t)p.W), put_be32(head + 20, (uint32_t)p.H);
        head[24] = 8, head[25] = 2, head[26] = 0, head[27] = 0, head[28] = 0;
        close_chunk(head + 8, "IHDR", 13);
        head[41] = 0x78, head[42] = 0x01;
        close_chunk(head + 33, "IDAT", 2);
        tail[8] = 1, tail[9] = 0, tail[10] = 0, tail[11] = 0xFF, tail[12] = 0xFF;
        put_be32(tail + 13, (uint32_t)((N + s2) % ADLER) << 16 | (uint32_t)((1ull + s1) % ADLER));
        close_chunk(tail, "IDAT", 9);
        close_chunk(tail + 21, "IEND", 0);
        *p.size_word = fits ? (uint32_t)(at + DCVC_PNG_TRAILER_BYTES) : 0u;
    }
    __syncthreads();
    if (fits && tid < DCVC_PNG_PREFIX_BYTES) p.file[tid] = head[tid];
    if (fits && tid < DCVC_PNG_TRAILER_BYTES) p.file[at + tid] = tail[tid];
}

// the tables the last call passed and the check accepted: the same presets with every picture cost a comparison
std::mutex accepted_lock;
std::vector<uint32_t> accepted;

bool tables_ok(const uint32_t *host, int32_t K) {
    const size_t words = (size_t)K * DCVC_PNG_PRESET_WORDS;
    std::lock_guard<std::mutex> hold(accepted_lock);
    if (accepted.size() == words && memcmp(accepted.data(), host, 4 * words) == 0) return true;
    if (dcvc_png_tables_check(host, K) != DCVC_OK) return false;
    accepted.assign(host, host + words);
    return true;
}

}  // namespace

extern "C" int dcvc_png_encode(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, int32_t R,
                               const uint32_t *tables_host, const uint32_t *tables_dev, int32_t K, uint8_t *staging, uint8_t *file,
                               int64_t capacity, uint32_t *size_word, void *stream) {
    if (!rgb || !tables_host || !tables_dev || !staging || !file || !size_word || !aligned(rgb, 4) || !aligned(tables_host, 4) ||
        !aligned(tables_dev, 4) || !aligned(staging, 4) || !aligned(file, 4) || !aligned(size_word, 4))
        return DCVC_E_ARG;
    const int64_t most = dcvc_png_bound(H, W, R);  // (-1: H, W or R out of range)
    if (most < 0 || row_stride < W || plane_stride < (int64_t)(H - 1) * row_stride + W || capacity < most) return DCVC_E_ARG;
    if (K < 1 || K > DCVC_PNG_MAX_PRESETS || !tables_ok(tables_host, K)) return DCVC_E_ARG;
    const int32_t bands = (H + R - 1) / R;
    BandArgs a{};
    a.src = rgb, a.tables = tables_dev, a.staging = reinterpret_cast<uint32_t *>(staging), a.ps = plane_stride;
    a.rs = row_stride, a.H = H, a.W = W, a.R = R, a.K = K;
    png_band_kernel<<<dim3((unsigned)bands), dim3(LANES), 0, (hipStream_t)stream>>>(a);
    if (hipGetLastError() != hipSuccess) return DCVC_E_LAUNCH;
    PackArgs b{};
    b.staging = a.staging, b.file = file, b.size_word = size_word, b.capacity = capacity, b.H = H, b.W = W, b.R = R, b.bands = bands;
    png_pack_kernel<<<dim3((unsigned)bands + 1u), dim3(LANES), 0, (hipStream_t)stream>>>(b);
    RET_LAUNCH();
}
