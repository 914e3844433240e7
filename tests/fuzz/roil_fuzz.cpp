// roil_fuzz.cpp -- memory-safety fuzz of the host half of the ROI residual layer: the record validation of
// vcm_ts_amd/csrc/roil_check.cpp (dcvc_roil_check, dcvc_roil_cells) and the per-sample segment decoder the decode kernel
// runs per lane (vcm_ts_amd/csrc/roil_segment.h), built with AddressSanitizer + UBSan by tests/test_roil_host.py.
//
// Per round: random boxes in a small picture give the counts n_a; a record is written for random samples by the serial
// encoder below (test code, the format's text); it must pass the check and decode to its samples.  Then the record is
// mutated -- truncated, extended, bit-flipped in header, table or payload, payload zeroed -- and each mutant must either
// be refused, or decode with every sample within 0 .. 255 or reported undecodable.  Segments are handed to the decoder in
// EXACTLY sized heap arrays, so a read beyond n_words words is a sanitizer report.
//
//   roil_fuzz ROUNDS SEED
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "dcvc_hip.h"
#include "dcvc_hip_roil.h"
#include "roil_segment.h"

typedef std::vector<uint8_t> Bytes;

static void put_bit(Bytes &b, int at) {
    if ((size_t)(at >> 3) >= b.size()) b.resize((at >> 3) + 1, 0);
    b[at >> 3] |= (uint8_t)(1u << (at & 7));
}

static int encode_segment(const std::vector<int> &u, Bytes *out) {
    const int n = (int)u.size();
    int best = 8, fewest = 8 * n;
    bool zero = true;
    for (int v : u) zero = zero && v == 0;
    for (int m = 7; m >= 0; --m) {
        int bits = n * (m + 1);
        for (int v : u) bits += v >> m;
        if (bits <= fewest) best = m, fewest = bits;
    }
    out->clear();
    if (zero) return 9;
    out->assign((fewest + 7) / 8, 0);
    if (best == 8) {
        for (int i = 0; i < n; ++i) (*out)[i] = (uint8_t)u[i];
        return 8;
    }
    int at = n * best;
    for (int i = 0; i < n; ++i) {
        for (int t = 0; t < best; ++t)
            if ((u[i] >> t) & 1) put_bit(*out, i * best + t);
        at += u[i] >> best;
        put_bit(*out, at++);
    }
    if (at != fewest) abort();
    return best;
}

// decodes every sample of a record that passed the check; returns the number of samples reported undecodable, -1 if a
// sample left 0 .. 255
static long decode_all(const Bytes &rec, const std::vector<int32_t> &counts, std::vector<int> *samples) {
    const int A = (int)counts.size();
    size_t at = DCVC_ROIL_HEADER + 6 * (size_t)A;
    long undecodable = 0;
    if (samples) samples->clear();
    for (int s = 0; s < 3 * A; ++s) {
        const unsigned e = rec[DCVC_ROIL_HEADER + 2 * s] | (rec[DCVC_ROIL_HEADER + 2 * s + 1] << 8);
        const int mode = (int)(e >> 12), L = (int)(e & 0xfffu), n = counts[s / 3];
        const int n_words = (L + 3) / 4;
        uint32_t *w = new uint32_t[n_words > 0 ? n_words : 1]();  // exactly sized: a read beyond it is reported
        for (int b = 0; b < L; ++b) w[b >> 2] |= (uint32_t)rec[at + b] << (8 * (b & 3));
        for (int i = 0; i < n; ++i) {
            const int u = roil_sample(w, n_words, n, mode, L, i);
            if (u < 0)
                ++undecodable;
            else if (u > 255 || roil_reconstruct(u, rec[3]) < 0 || roil_reconstruct(u, rec[3]) > 255)
                return -1;
            if (samples) samples->push_back(u);
        }
        if (roil_sample(w, n_words, n, mode, L, n) != -1 || roil_sample(w, n_words, n, mode, L, -1) != -1) return -1;
        delete[] w;
        at += L;
    }
    return undecodable;
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    auto below = [&](int n) { return (int)(rng() % (unsigned)n); };
    long accepted = 0, refused = 0, undecodable = 0;
    for (int round = 0; round < rounds; ++round) {
        const int H = 1 + below(50), W = 1 + below(70), nb = below(6);
        std::vector<dcvc_roi_box_t> boxes(nb);
        for (auto &b : boxes) b = {below(W + 1), below(H + 1), below(W + 1), below(H + 1), below(4)};
        const int A = dcvc_roil_cells(H, W, boxes.data(), nb, nullptr, nullptr, 0);
        if (A < 0) return 2;
        std::vector<int32_t> cells(A), counts(A);
        if (A && dcvc_roil_cells(H, W, boxes.data(), nb, cells.data(), counts.data(), A) != A) return 2;
        if (A && dcvc_roil_cells(H, W, boxes.data(), nb, cells.data(), counts.data(), A - 1) != DCVC_E_ARG) return 2;
        // a record of random samples, every cell with a spread of its own
        const int step = 1 + below(64);
        Bytes rec = {'R', 'L', DCVC_ROIL_VERSION, (uint8_t)step, (uint8_t)A, (uint8_t)(A >> 8), (uint8_t)(A >> 16), (uint8_t)(A >> 24)};
        Bytes table, payload, seg;
        std::vector<int> all;
        for (int s = 0; s < 3 * A; ++s) {
            if (counts[s / 3] < 1 || counts[s / 3] > 256) return 2;
            std::vector<int> u(counts[s / 3]);
            const int spread = below(10);
            for (int &v : u) v = spread == 0 ? 0 : (spread == 9 ? below(256) : below(1 << spread) & below(256));
            const int mode = encode_segment(u, &seg);
            if ((int)seg.size() > (int)u.size()) return 3;  // L <= n
            const unsigned e = (unsigned)seg.size() | ((unsigned)mode << 12);
            table.push_back((uint8_t)e), table.push_back((uint8_t)(e >> 8));
            payload.insert(payload.end(), seg.begin(), seg.end());
            all.insert(all.end(), u.begin(), u.end());
        }
        rec.insert(rec.end(), table.begin(), table.end());
        rec.insert(rec.end(), payload.begin(), payload.end());
        std::vector<int> got;
        if (dcvc_roil_check(rec.data(), (int64_t)rec.size(), counts.data(), A) != DCVC_OK) return 4;
        if (decode_all(rec, counts, &got) != 0 || got != all) return 5;
        ++accepted;
        for (int k = 0; k < 24; ++k) {
            Bytes m = rec;
            const int kind = below(6);
            if (kind == 0) m.resize(below((int)m.size() + 1));
            else if (kind == 1) m.resize(m.size() + 1 + below(9), (uint8_t)below(256));
            else if (kind == 2) m[below(8)] ^= (uint8_t)(1u << below(8));
            else if (kind == 3 && A) m[DCVC_ROIL_HEADER + below(6 * A)] ^= (uint8_t)(1u << below(8));
            else if (kind == 4 && payload.size()) m[DCVC_ROIL_HEADER + 6 * A + below((int)payload.size())] ^= (uint8_t)(1u << below(8));
            else if (kind == 5) std::fill(m.begin() + DCVC_ROIL_HEADER + 6 * A, m.end(), 0);  // valid table, no set bits
            uint8_t *exact = (uint8_t *)malloc(m.size() ? m.size() : 1);  // exactly sized: the check must stay inside `size`
            memcpy(exact, m.data(), m.size());
            const int rc = dcvc_roil_check(exact, (int64_t)m.size(), counts.data(), A);
            free(exact);
            if (rc != DCVC_OK) {
                ++refused;
                continue;
            }
            const long bad = decode_all(m, counts, nullptr);
            if (bad < 0) return 6;
            undecodable += bad;
            ++accepted;
        }
    }
    printf("roil_fuzz: %d rounds, %ld records decoded, %ld refused with a status, %ld samples reported undecodable\n", rounds,
           accepted, refused, undecodable);
    return 0;
}
