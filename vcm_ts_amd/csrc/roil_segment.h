// roil_segment.h -- the per-sample decode of one segment of the ROI residual layer (include/dcvc_hip_roil.h, "Segment")
// over a BOUNDED word array: the decode kernel calls it per lane on the cell's segment in LDS, the host fuzz program
// (tests/fuzz/roil_fuzz.cpp) runs the same code under sanitizers.  Word j holds bytes 4 j .. 4 j + 3 of the segment,
// little-endian, so bit b of the segment is bit (b & 31) of word (b >> 5).  Nothing here reads beyond n_words words.
#ifndef DCVC_ROIL_SEGMENT_H
#define DCVC_ROIL_SEGMENT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define ROIL_HD __host__ __device__ inline
#else
#define ROIL_HD inline
#endif

constexpr int ROIL_MAX_N = 256;      // samples of a segment: the pixels of a cell
constexpr int ROIL_SEG_WORDS = 64;   // 256 bytes, the longest segment

// is L a possible length of a segment of n samples in `mode`?
ROIL_HD bool roil_length_ok(int n, int mode, int L) {
    if (n < 1 || n > ROIL_MAX_N || mode < 0 || mode > 9 || L < 0 || L > n) return false;
    if (mode == 9) return L == 0;
    if (mode == 8) return L == n;
    return 8 * L >= n * (mode + 1);  // at least the low parts and one bit per sample
}

// the position of the j-th (from 0) set bit among bits [lo, hi) of the array, or -1
ROIL_HD int roil_select(const uint32_t *w, int n_words, int lo, int hi, int j) {
    if (hi > 32 * n_words) hi = 32 * n_words;
    if (j < 0 || lo < 0 || lo >= hi) return -1;
    int wi = lo >> 5;
    const int last = (hi - 1) >> 5;
    uint32_t cur = w[wi] & (~0u << (lo & 31));
    for (;;) {
        if (wi == last && (hi & 31)) cur &= (1u << (hi & 31)) - 1u;
        const int c = __builtin_popcount(cur);
        if (j < c) {
            while (j-- > 0) cur &= cur - 1u;
            return wi * 32 + __builtin_ctz(cur);
        }
        j -= c;
        if (wi == last) return -1;
        cur = w[++wi];
    }
}

// u of sample i (0 <= i < n) of a segment of n samples in `mode` and of L bytes, roil_length_ok(n, mode, L); -1 where the
// payload does not hold it: fewer than i + 1 set bits in the unary section, or u > 255
ROIL_HD int roil_sample(const uint32_t *w, int n_words, int n, int mode, int L, int i) {
    if (i < 0 || i >= n || !roil_length_ok(n, mode, L) || 8 * L > 32 * n_words) return -1;
    if (mode == 9) return 0;
    if (mode == 8) return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
    int low = 0;
    if (mode > 0) {
        const int b = i * mode, j = b >> 5;  // (b + mode <= n * mode <= 8 L: word j exists)
        uint64_t two = w[j];
        if (j + 1 < n_words) two |= (uint64_t)w[j + 1] << 32;
        low = (int)((two >> (b & 31)) & ((1u << mode) - 1u));
    }
    const int lo = n * mode, hi = 8 * L;
    const int prev = i == 0 ? lo - 1 : roil_select(w, n_words, lo, hi, i - 1);
    if (i > 0 && prev < 0) return -1;
    const int at = roil_select(w, n_words, prev + 1, hi, 0);
    if (at < 0) return -1;
    const int gap = at - prev - 1;
    if (gap > (255 >> mode)) return -1;
    return (gap << mode) | low;
}

// r' of a decoded u (include/dcvc_hip_roil.h, "Samples")
ROIL_HD int roil_reconstruct(int u, int step) {
    const int q = (u & 1) ? -((u + 1) >> 1) : (u >> 1);
    const int v = 128 + q * step;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

#endif
