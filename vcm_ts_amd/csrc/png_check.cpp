// png_check.cpp -- the host half of the PNG writer (include/dcvc_hip_png.h): the size bound and the check of the preset
// tables, which decodes every preset's block header the way an inflater would.  Plain C++ without HIP, so that a
// stand-alone program can hold it under host sanitizers.
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_png.h"

namespace {

constexpr int NSYM = DCVC_PNG_SYMBOLS, NLEN = NSYM + 1;  // the lengths a header carries: 286 and one distance code
constexpr int ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Bits {  // the header's bits, read from bit 0 up; past the end is an error that sticks
    const uint32_t *w;
    uint32_t n, at;
    bool bad;
    uint32_t take(int k) {
        if (at + k > n) {
            bad = true;
            return 0;
        }
        const uint64_t two = w[at >> 5] | (uint64_t)((at >> 5) + 1 < DCVC_PNG_HEADER_WORDS ? w[(at >> 5) + 1] : 0u) << 32;
        const uint32_t v = (uint32_t)(two >> (at & 31)) & ((1u << k) - 1u);
        at += k;
        return v;
    }
};

// canonical codes of `n` lengths (0: unused) within `maxbits`, NOT reversed; false unless the code is complete
bool canonical(const uint8_t *len, int n, int maxbits, uint16_t *code) {
    uint32_t count[16] = {0}, next[16] = {0}, kraft = 0;
    for (int s = 0; s < n; ++s) {
        if (len[s] > maxbits) return false;
        if (len[s]) ++count[len[s]], kraft += 1u << (maxbits - len[s]);
    }
    if (kraft != 1u << maxbits) return false;
    for (int b = 1, c = 0; b <= maxbits; ++b) next[b] = c = (c + count[b - 1]) << 1;
    for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)next[len[s]]++ : 0;
    return true;
}

uint32_t reversed(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int j = 0; j < bits; ++j) r |= ((v >> j) & 1u) << (bits - 1 - j);
    return r;
}

bool preset_ok(const uint32_t *p) {
    uint8_t len[NSYM];
    uint16_t code[NSYM];
    for (int s = 0; s < NSYM; ++s) {
        if (p[s] >> 20 || (p[s] >> 16) < 1 || (p[s] >> 16) > 15) return false;
        len[s] = (uint8_t)(p[s] >> 16);
    }
    if (!canonical(len, NSYM, 15, code)) return false;
    for (int s = 0; s < NSYM; ++s)
        if ((p[s] & 0xFFFFu) != reversed(code[s], len[s])) return false;
    const uint32_t hbits = p[NSYM];
    if (hbits > 32u * DCVC_PNG_HEADER_WORDS || p[DCVC_PNG_PRESET_WORDS - 1]) return false;
    const uint32_t *h = p + NSYM + 1;
    for (uint32_t j = hbits >> 5; j < DCVC_PNG_HEADER_WORDS; ++j)
        if (j == hbits >> 5 ? h[j] >> (hbits & 31) : h[j]) return false;
    Bits in{h, hbits, 0, false};
    if (in.take(5) != NSYM - 257 || in.take(5) != 0) return false;
    const int ncl = (int)in.take(4) + 4;
    uint8_t cl[19] = {0};
    uint16_t clcode[19];
    for (int j = 0; j < ncl; ++j) cl[ORDER[j]] = (uint8_t)in.take(3);
    if (in.bad || !canonical(cl, 19, 7, clcode)) return false;
    // the code-length code's symbols by (length, symbol), and how many there are of every length: the canonical decoder
    int sorted[19], count[8] = {0}, filled = 0;
    for (int b = 1; b <= 7; ++b)
        for (int s = 0; s < 19; ++s)
            if (cl[s] == b) sorted[filled++] = s, ++count[b];
    int got = 0, prev = -1;
    while (got < NLEN) {
        int sym = -1;
        for (int b = 1, acc = 0, first = 0, index = 0; b <= 7 && sym < 0; ++b) {  // bits arrive most significant first
            acc |= (int)in.take(1);
            if (acc - count[b] < first) sym = sorted[index + (acc - first)];
            index += count[b], first = (first + count[b]) << 1, acc <<= 1;
        }
        if (in.bad || sym < 0) return false;
        int value = sym, times = 1;
        if (sym == 16) {
            if (prev < 0) return false;
            value = prev, times = 3 + (int)in.take(2);
        } else if (sym == 17) {
            value = 0, times = 3 + (int)in.take(3);
        } else if (sym == 18) {
            value = 0, times = 11 + (int)in.take(7);
        }
        if (in.bad || got + times > NLEN) return false;
        for (; times; --times, ++got)
            if (value != (got < NSYM ? len[got] : 1)) return false;
        prev = value;
    }
    return in.at == hbits;
}

}  // namespace

extern "C" int64_t dcvc_png_bound(int32_t H, int32_t W, int32_t R) {
    if (H < 1 || H > DCVC_PNG_MAX_H || W < 1 || W > DCVC_PNG_MAX_W || R < 1 || (int64_t)R * (3 * W + 1) > DCVC_PNG_BAND_MAX) return -1;
    return 80 + (int64_t)H * (3 * W + 1) + 17 * (int64_t)((H + R - 1) / R);
}

extern "C" int dcvc_png_tables_check(const uint32_t *tables_host, int32_t K) {
    if (!tables_host || (reinterpret_cast<uintptr_t>(tables_host) & 3) || K < 1 || K > DCVC_PNG_MAX_PRESETS) return DCVC_E_ARG;
    for (int32_t k = 0; k < K; ++k)
        if (!preset_ok(tables_host + (int64_t)k * DCVC_PNG_PRESET_WORDS)) return DCVC_E_ARG;
    return DCVC_OK;
}
