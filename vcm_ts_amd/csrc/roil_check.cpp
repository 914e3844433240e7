// roil_check.cpp -- the host half of the ROI residual layer (include/dcvc_hip_roil.h): the active cells of a box list and
// the validation of a picture record against them.  Plain C++ without HIP: part of libdcvc_hip.so, and compiled on its own
// with sanitizers by the fuzz program (tests/fuzz/roil_fuzz.cpp).
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dcvc_hip.h"
#include "dcvc_hip_roil.h"
#include "roil_segment.h"

extern "C" int dcvc_roil_cells(int32_t H, int32_t W, const dcvc_roi_box_t *boxes, int32_t n, int32_t *cells, int32_t *counts,
                               int32_t capacity) {
    if (H <= 0 || W <= 0 || H > DCVC_ROI_MAX_SIDE || W > DCVC_ROI_MAX_SIDE || n < 0 || n > DCVC_ROI_MAX_BOXES ||
        (n > 0 && !boxes) || (cells == nullptr) != (counts == nullptr))
        return DCVC_E_ARG;
    for (int32_t i = 0; i < n; ++i) {
        const dcvc_roi_box_t &b = boxes[i];
        if (b.x1 < 0 || b.x1 > W || b.x2 < 0 || b.x2 > W || b.y1 < 0 || b.y1 > H || b.y2 < 0 || b.y2 > H || b.cls < 0 ||
            b.cls >= DCVC_ROI_MAX_CLASSES)
            return DCVC_E_ARG;
    }
    const int hc = (H + DCVC_ROI_CELL - 1) / DCVC_ROI_CELL, wc = (W + DCVC_ROI_CELL - 1) / DCVC_ROI_CELL;
    std::vector<int32_t> slot((size_t)hc * wc, -1);  // cell -> its row masks, in order of first touch
    std::vector<uint16_t> rows;                      // 16 row masks per touched cell: bit x of row y = pixel in the mask
    for (int32_t i = 0; i < n; ++i) {
        const dcvc_roi_box_t &b = boxes[i];
        if (b.x2 <= b.x1 || b.y2 <= b.y1) continue;
        for (int cy = b.y1 / DCVC_ROI_CELL; cy <= (b.y2 - 1) / DCVC_ROI_CELL; ++cy)
            for (int cx = b.x1 / DCVC_ROI_CELL; cx <= (b.x2 - 1) / DCVC_ROI_CELL; ++cx) {
                int32_t &s = slot[(size_t)cy * wc + cx];
                if (s < 0) {
                    s = (int32_t)(rows.size() / DCVC_ROI_CELL);
                    rows.resize(rows.size() + DCVC_ROI_CELL, 0);
                }
                const int x0 = cx * DCVC_ROI_CELL, y0 = cy * DCVC_ROI_CELL;
                const int xa = b.x1 > x0 ? b.x1 - x0 : 0, xb = b.x2 < x0 + DCVC_ROI_CELL ? b.x2 - x0 : DCVC_ROI_CELL;
                const int ya = b.y1 > y0 ? b.y1 - y0 : 0, yb = b.y2 < y0 + DCVC_ROI_CELL ? b.y2 - y0 : DCVC_ROI_CELL;
                const uint16_t bits = (uint16_t)(((1u << xb) - 1u) & ~((1u << xa) - 1u));
                for (int y = ya; y < yb; ++y) rows[(size_t)s * DCVC_ROI_CELL + y] |= bits;
            }
    }
    const int64_t A = (int64_t)(rows.size() / DCVC_ROI_CELL);
    if (!cells) return (int)A;
    if (capacity < A) return DCVC_E_ARG;
    int32_t a = 0;
    for (size_t c = 0; c < slot.size(); ++c) {
        if (slot[c] < 0) continue;
        int count = 0;
        for (int y = 0; y < DCVC_ROI_CELL; ++y) count += __builtin_popcount(rows[(size_t)slot[c] * DCVC_ROI_CELL + y]);
        cells[a] = (int32_t)c;
        counts[a++] = count;
    }
    return (int)A;
}

extern "C" int dcvc_roil_check(const uint8_t *record, int64_t size, const int32_t *counts, int32_t A) {
    if (!record || size < 0 || A < 0 || (A > 0 && !counts)) return DCVC_E_ARG;
    if (size < DCVC_ROIL_HEADER) return DCVC_ROIL_E_TRUNCATED;
    if (record[0] != 'R' || record[1] != 'L') return DCVC_ROIL_E_MAGIC;
    if (record[2] != DCVC_ROIL_VERSION) return DCVC_ROIL_E_VERSION;
    if (record[3] < 1 || record[3] > DCVC_ROIL_MAX_STEP) return DCVC_ROIL_E_STEP;
    const uint32_t have = (uint32_t)record[4] | ((uint32_t)record[5] << 8) | ((uint32_t)record[6] << 16) | ((uint32_t)record[7] << 24);
    if (have != (uint32_t)A) return DCVC_ROIL_E_CELLS;
    const int64_t table = DCVC_ROIL_HEADER + 6 * (int64_t)A;
    if (size < table) return DCVC_ROIL_E_TRUNCATED;
    int64_t total = table;
    for (int64_t s = 0; s < 3 * (int64_t)A; ++s) {
        const unsigned entry = (unsigned)record[DCVC_ROIL_HEADER + 2 * s] | ((unsigned)record[DCVC_ROIL_HEADER + 2 * s + 1] << 8);
        const int mode = (int)(entry >> 12), L = (int)(entry & 0xfffu);
        if (mode > 9) return DCVC_ROIL_E_MODE;
        if (!roil_length_ok(counts[s / 3], mode, L)) return DCVC_ROIL_E_LENGTH;
        total += L;
    }
    if (size < total) return DCVC_ROIL_E_TRUNCATED;
    if (size > total) return DCVC_ROIL_E_TRAILING;
    return DCVC_OK;
}
