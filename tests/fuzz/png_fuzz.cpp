// png_fuzz.cpp -- memory-safety fuzz of the host half of the PNG writer: dcvc_png_tables_check and dcvc_png_bound of
// vcm_ts_amd/csrc/png_check.cpp, built with AddressSanitizer + UBSan by tests/test_pngdev_host.py.
//
// Per round: K presets are written by the serial builder below (test code, from the header's text: 226 symbols of length 8
// and 60 of length 9 in a random arrangement, a header without repeat codes under a three-symbol code-length code); they
// must pass.  Then words are mutated -- bits flipped in the codes, in the header's count and in its bits, words replaced by
// random ones -- and every mutant must be accepted or refused with a status.  The tables are handed over in EXACTLY sized
// heap arrays, so a read beyond K * DCVC_PNG_PRESET_WORDS words is a sanitizer report.
//
//   png_fuzz ROUNDS SEED
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "dcvc_hip.h"
#include "dcvc_hip_png.h"

static uint32_t reversed(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int j = 0; j < bits; ++j) r |= ((v >> j) & 1u) << (bits - 1 - j);
    return r;
}

struct Writer {
    uint32_t *w;
    uint32_t n;
    void put(uint32_t v, int bits) {
        for (int j = 0; j < bits; ++j, ++n) w[n >> 5] |= ((v >> j) & 1u) << (n & 31);
    }
};

static void build(uint32_t *p, std::mt19937 &rng) {
    memset(p, 0, 4 * DCVC_PNG_PRESET_WORDS);
    std::vector<int> len(DCVC_PNG_SYMBOLS, 8);
    std::fill(len.begin(), len.begin() + 60, 9);
    std::shuffle(len.begin(), len.end(), rng);
    uint32_t next8 = 0, next9 = 226u << 1;  // canonical: the 8-bit codes first, the 9-bit ones behind them
    for (int s = 0; s < DCVC_PNG_SYMBOLS; ++s) p[s] = (uint32_t)len[s] << 16 | reversed(len[s] == 8 ? next8++ : next9++, len[s]);
    Writer h{p + DCVC_PNG_SYMBOLS + 1, 0};
    h.put(DCVC_PNG_SYMBOLS - 257, 5), h.put(0, 5), h.put(18 - 4, 4);  // the order's 18th entry is symbol 1
    const int order[18] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1};
    for (int s : order) h.put(s == 8 ? 1 : (s == 9 || s == 1) ? 2 : 0, 3);
    // the code-length code: symbol 8 is `0`, symbol 1 is `10`, symbol 9 is `11` (most significant bit first)
    for (int s = 0; s <= DCVC_PNG_SYMBOLS; ++s) {
        const int v = s < DCVC_PNG_SYMBOLS ? len[s] : 1;
        if (v == 8) h.put(0, 1);
        else h.put(reversed(v == 1 ? 2 : 3, 2), 2);
    }
    p[DCVC_PNG_SYMBOLS] = h.n;
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto below = [&](int n) { return (int)(rng() % (unsigned)n); };
    long accepted = 0, refused = 0;
    for (int round = 0; round < rounds; ++round) {
        const int K = 1 + below(DCVC_PNG_MAX_PRESETS), words = K * DCVC_PNG_PRESET_WORDS;
        std::vector<uint32_t> t(words);
        for (int k = 0; k < K; ++k) build(t.data() + k * DCVC_PNG_PRESET_WORDS, rng);
        if (dcvc_png_tables_check(t.data(), K) != DCVC_OK) return 2;
        if (dcvc_png_tables_check(t.data(), 0) != DCVC_E_ARG || dcvc_png_tables_check(nullptr, K) != DCVC_E_ARG) return 3;
        ++accepted;
        for (int m = 0; m < 40; ++m) {
            uint32_t *exact = (uint32_t *)malloc(4 * (size_t)words);  // exactly sized: the check must stay inside it
            memcpy(exact, t.data(), 4 * (size_t)words);
            uint32_t *p = exact + below(K) * DCVC_PNG_PRESET_WORDS;
            const int kind = below(5);
            if (kind == 0) p[below(DCVC_PNG_SYMBOLS)] ^= 1u << below(32);
            else if (kind == 1) p[DCVC_PNG_SYMBOLS] = below(2) ? (uint32_t)rng() : p[DCVC_PNG_SYMBOLS] + (uint32_t)below(64) - 32u;
            else if (kind == 2) p[DCVC_PNG_SYMBOLS + 1 + below(DCVC_PNG_HEADER_WORDS)] ^= 1u << below(32);
            else if (kind == 3) p[below(DCVC_PNG_PRESET_WORDS)] = (uint32_t)rng();
            else for (int j = 0; j < DCVC_PNG_HEADER_WORDS; ++j) p[DCVC_PNG_SYMBOLS + 1 + j] = (uint32_t)rng(), p[DCVC_PNG_SYMBOLS] = 32u * (uint32_t)below(DCVC_PNG_HEADER_WORDS + 1);
            const int rc = dcvc_png_tables_check(exact, K);
            free(exact);
            if (rc == DCVC_OK) ++accepted;
            else if (rc == DCVC_E_ARG) ++refused;
            else return 4;
        }
        const int32_t H = (int32_t)rng(), W = (int32_t)rng(), R = (int32_t)rng();
        const int64_t b = dcvc_png_bound(H >> below(32), W >> below(32), R >> below(32));
        if (b < -1 || b == 0) return 5;
    }
    printf("png_fuzz: %d rounds, %ld table sets accepted, %ld refused with a status\n", rounds, accepted, refused);
    return 0;
}
