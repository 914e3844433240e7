// roil.hip -- the ROI residual layer as a bitstream (include/dcvc_hip_roil.h, which states the arithmetic and the format;
// this file only arranges them).
//
// Encode and decode give an ACTIVE 16 x 16 cell to one workgroup of 4 waves, a pixel to a lane: lane t owns pixel
// (t >> 4, t & 15) of the cell, so lane order is the raster order the format takes samples in.  The first wave culls the
// picture's box list against the cell into LDS (roi_common.h), every lane then knows whether its pixel is in the mask,
// and a ballot with a prefix popcount gives it its RANK among the cell's n samples.
//   encode   u for three channels; n and sum(u >> m), m = 0 .. 7, reduced with wave shuffles (two 16-bit sums to a
//            register: a sum is at most 256 * 255), then across the waves in LDS; every lane picks the three modes from
//            the totals; a scan of (u >> m) + 1 gives the lane the place of ITS one bit of the unary section; the
//            segment is assembled in zeroed LDS with atomic ORs (low part: one or two, unary: ONE bit); the header
//            entries go to the record, the 768 bytes to the cell's slot of the staging buffer.
//   pack     a workgroup per 256 segments: sums the lengths before its chunk, scans its own, and a wave copies a segment
//            behind the header byte by byte across its lanes.  The first writes the 8-byte header, the last the size.
//   decode   the three header entries are held against roil_length_ok and the record's size BY THE KERNEL too (the entry
//            point did so on the host copy), the segments are copied to LDS, and every lane selects its sample
//            (roil_segment.h: the same code the host fuzz program runs).  A fill launch zeroes the picture first.
// The kernels address nothing through a box and bound everything they take from the table and the record: whatever the
// device copies hold, only pixels of the H x W picture, the record's `size` bytes, the A slots and the record's
// capacity are touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "dcvc_hip.h"
#include "dcvc_hip_roil.h"
#include "kernel_common.h"
#include "roi_common.h"
#include "roil_segment.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL = DCVC_ROI_CELL;
constexpr int SLOT_WORDS = DCVC_ROIL_SLOT / 4;

struct CellList {  // the culled boxes of a cell
    int4 box[DCVC_ROI_MAX_BOXES];
    uint8_t cls[DCVC_ROI_MAX_BOXES];
    int count;
    int wave_n[4];
};

// (in the mask?, rank among the cell's samples, n) of this lane's pixel (x, y); all four waves call it
__device__ __forceinline__ bool cell_mask(CellList &t, const dcvc_roi_box_t *boxes, int n_boxes, int cx0, int cy0, int x, int y,
                                          int W, int H, int lane, int wave, int *rank, int *n) {
    if (wave == 0) {
        const int count = roi_cull(boxes, n_boxes, lane, cx0, cy0, cx0 + CELL, cy0 + CELL, t.box, t.cls, [](int) { return 0; });
        if (lane == 0) t.count = count;
    }
    __syncthreads();
    bool in = false;
    if (x < W && y < H) {
        const int count = t.count;
        for (int j = 0; j < count; ++j) {
            const int4 bx = t.box[j];
            in = in || (x >= bx.x && x < bx.z && y >= bx.y && y < bx.w);
        }
    }
    const unsigned long long bal = __ballot(in);
    if (lane == 0) t.wave_n[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = t.wave_n[w];
        before += w < wave ? c : 0;
        total += c;
    }
    *rank = before, *n = total;
    return in;
}

__device__ __forceinline__ unsigned wave_scan(unsigned v, int lane) {  // inclusive
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)v, off);
        v += lane >= off ? o : 0u;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------------------ encode
struct EncArgs {
    const float *a, *b;  // source, reconstruction
    const dcvc_roi_box_t *boxes;
    const int2 *table;
    uint32_t *staging;
    uint8_t *record;
    int64_t a_ps, b_ps;
    int32_t a_rs, b_rs, H, W, n, wc, cells, step;
};

struct EncTile {
    CellList list;
    unsigned seg[3][ROIL_SEG_WORDS];
    unsigned sums[4][12];  // per wave: channel c, pair k -> sum(u >> 2k) | sum(u >> (2k + 1)) << 16
    unsigned scan[4][3];   // per wave: the wave's total of the unary lengths
};

__global__ __launch_bounds__(256) void roil_encode_kernel(const EncArgs p) {
    __shared__ EncTile t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = blockIdx.x;
    uint16_t *entries = reinterpret_cast<uint16_t *>(p.record + DCVC_ROIL_HEADER) + 3 * (int64_t)a;
    const int cell = p.table[a].x;
    if (cell < 0 || cell >= p.cells) {  // (no validated table names such a cell) an empty slot, nothing read
        if (tid < 3) entries[tid] = (uint16_t)(9u << 12);
        return;
    }
    const int cx0 = (cell % p.wc) * CELL, cy0 = (cell / p.wc) * CELL, x = cx0 + (tid & 15), y = cy0 + (tid >> 4);
    if (tid < 3 * ROIL_SEG_WORDS) (&t.seg[0][0])[tid] = 0u;
    int rank, n;
    const bool in = cell_mask(t.list, p.boxes, p.n, cx0, cy0, x, y, p.W, p.H, lane, wave, &rank, &n);

    int u[3] = {0, 0, 0};
    if (in) {
        const int half = p.step >> 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sa = code8(p.a[c * p.a_ps + (int64_t)y * p.a_rs + x]), sb = code8(p.b[c * p.b_ps + (int64_t)y * p.b_rs + x]);
            const int e = min(max(sa - sb + 128, 0), 255) - 128;
            const int mag = ((e < 0 ? -e : e) + half) / p.step;
            u[c] = e < 0 && mag > 0 ? 2 * mag - 1 : 2 * mag;  // q = -mag -> -2 q - 1; q >= 0 -> 2 q
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned s = wave_sum((unsigned)(u[c] >> (2 * k)) | ((unsigned)(u[c] >> (2 * k + 1)) << 16));
            if (lane == 0) t.sums[wave][c * 4 + k] = s;
        }
    __syncthreads();
    int mode[3], bits[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int best = 8, fewest = 8 * n;
        unsigned s0 = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const unsigned s = t.sums[0][c * 4 + k] + t.sums[1][c * 4 + k] + t.sums[2][c * 4 + k] + t.sums[3][c * 4 + k];
            const int hi = n * (2 * k + 2) + (int)(s >> 16), lo = n * (2 * k + 1) + (int)(s & 0xffffu);
            if (hi <= fewest) best = 2 * k + 1, fewest = hi;  // (descending, <=: the smallest mode among equals)
            if (lo <= fewest) best = 2 * k, fewest = lo;
            s0 = s & 0xffffu;
        }
        if (s0 == 0u) best = 9, fewest = 0;  // every u is 0 (also a cell the device's list leaves without samples)
        mode[c] = best, bits[c] = fewest;
    }
    // the place of this lane's one bit: n * m + (the unary lengths of the samples before it) + (u >> m)
    unsigned len[3], incl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        len[c] = in && mode[c] < 8 ? (unsigned)(u[c] >> mode[c]) + 1u : 0u;
        incl[c] = wave_scan(len[c], lane);
        if (lane == 63) t.scan[wave][c] = incl[c];
    }
    __syncthreads();
    if (in) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int m = mode[c];
            unsigned *seg = t.seg[c];
            if (m < 8) {
                unsigned before = incl[c] - len[c];
#pragma unroll
                for (int w = 0; w < 3; ++w) before += w < wave ? t.scan[w][c] : 0u;
                if (m > 0) {
                    const unsigned low = (unsigned)u[c] & ((1u << m) - 1u);
                    const int b = rank * m, sh = b & 31;
                    atomicOr(&seg[b >> 5], low << sh);
                    if (sh + m > 32) atomicOr(&seg[(b >> 5) + 1], low >> (32 - sh));
                }
                const int at = n * m + (int)before + (u[c] >> m);  // (< bits <= 8 n <= 2048)
                atomicOr(&seg[at >> 5], 1u << (at & 31));
            } else if (m == 8) {
                atomicOr(&seg[rank >> 2], (unsigned)u[c] << (8 * (rank & 3)));
            }
        }
    }
    __syncthreads();
    if (tid < 3) {
        const int c = tid;
        const int L = ((c == 0 ? bits[0] : (c == 1 ? bits[1] : bits[2])) + 7) >> 3;
        const int m = c == 0 ? mode[0] : (c == 1 ? mode[1] : mode[2]);
        entries[c] = (uint16_t)((unsigned)L | ((unsigned)m << 12));
    }
    if (tid < SLOT_WORDS) p.staging[(int64_t)a * SLOT_WORDS + tid] = (&t.seg[0][0])[tid];
}

// -------------------------------------------------------------------------------------------------------------- pack
struct PackArgs {
    const uint8_t *staging;
    uint8_t *record;
    uint32_t *size_word;
    int32_t A, step;
};

__global__ __launch_bounds__(256) void roil_pack_kernel(const PackArgs p) {
    __shared__ unsigned part[4], tot[4], at[256], len[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n_seg = 3 * (int64_t)p.A, first = (int64_t)blockIdx.x * 256;
    const uint16_t *entries = reinterpret_cast<const uint16_t *>(p.record + DCVC_ROIL_HEADER);
    unsigned before = 0u;  // the bytes of the segments before this chunk
    for (int64_t i = tid; i < first; i += 256) before += min((unsigned)entries[i] & 0xfffu, 256u);
    before = wave_sum(before);
    const unsigned L = first + tid < n_seg ? min((unsigned)entries[first + tid] & 0xfffu, 256u) : 0u;
    const unsigned incl = wave_scan(L, lane);
    if (lane == 63) tot[wave] = incl;
    if (lane == 0) part[wave] = before;
    __syncthreads();
    unsigned base = DCVC_ROIL_HEADER + 6u * (unsigned)p.A + part[0] + part[1] + part[2] + part[3];
    const unsigned chunk = tot[0] + tot[1] + tot[2] + tot[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) base += w < wave ? tot[w] : 0u;
    at[tid] = base + incl - L, len[tid] = L;
    __syncthreads();
    for (int j = 0; j < 64; ++j) {  // a wave copies its 64 segments one after the other, a byte per lane and round
        const int s = wave * 64 + j;
        if (first + s >= n_seg) break;
        const unsigned bytes = len[s];
        const uint8_t *src = p.staging + ((first + s) / 3) * DCVC_ROIL_SLOT + ((first + s) % 3) * 256;
        uint8_t *dst = p.record + at[s];
        for (unsigned b = lane; b < bytes; b += 64) dst[b] = src[b];
    }
    if (blockIdx.x == 0 && tid == 0) {
        *reinterpret_cast<uint32_t *>(p.record) = (uint32_t)'R' | ((uint32_t)'L' << 8) | ((uint32_t)DCVC_ROIL_VERSION << 16) | ((uint32_t)p.step << 24);
        *reinterpret_cast<uint32_t *>(p.record + 4) = (uint32_t)p.A;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0)
        *p.size_word = DCVC_ROIL_HEADER + 6u * (unsigned)p.A + part[0] + part[1] + part[2] + part[3] + chunk;
}

// ------------------------------------------------------------------------------------------------------------ decode
struct DecArgs {
    const uint8_t *record;
    const dcvc_roi_box_t *boxes;
    const int2 *table;
    uint8_t *out;
    uint32_t *status;
    int64_t size, cs, rs;
    int32_t px, H, W, n, wc, cells, A, vec, step;
    int32_t order[3];
};

struct DecTile {
    CellList list;
    unsigned seg[3][ROIL_SEG_WORDS];
};

// zeroes the picture: a lane owns 4 consecutive bytes of one row (planar: rows of W bytes in 3 H rows; interleaved: rows
// of 3 W bytes)
__global__ __launch_bounds__(256) void roil_zero_kernel(const DecArgs p) {
    const int row = blockIdx.x, row_bytes = p.px == 1 ? p.W : 3 * p.W;
    const int b0 = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (b0 >= row_bytes) return;
    uint8_t *at = p.out + (p.px == 1 ? (row / p.H) * p.cs + (int64_t)(row % p.H) * p.rs : (int64_t)row * p.rs) + b0;
    if (p.vec && b0 + 4 <= row_bytes) {
        *reinterpret_cast<uint32_t *>(at) = 0u;
    } else {
        for (int b = 0; b < 4 && b0 + b < row_bytes; ++b) at[b] = 0;
    }
}

__global__ __launch_bounds__(256) void roil_decode_kernel(const DecArgs p) {
    __shared__ DecTile t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = blockIdx.x;
    const int2 entry = p.table[a];
    const int cell = entry.x;
    const int64_t table_end = DCVC_ROIL_HEADER + 6 * (int64_t)p.A;
    if (cell < 0 || cell >= p.cells || table_end > p.size) {  // (no validated call gets here) nothing read, nothing written
        if (tid == 0) atomicOr(p.status, DCVC_ROIL_BAD_STREAM);
        return;
    }
    const int cx0 = (cell % p.wc) * CELL, cy0 = (cell / p.wc) * CELL, x = cx0 + (tid & 15), y = cy0 + (tid >> 4);
    if (tid < 3 * ROIL_SEG_WORDS) (&t.seg[0][0])[tid] = 0u;
    int rank, n;
    const bool in = cell_mask(t.list, p.boxes, p.n, cx0, cy0, x, y, p.W, p.H, lane, wave, &rank, &n);  // (syncs: seg is zero)

    // the three entries, held against what a segment of n samples can be and against the record's size
    const uint16_t *entries = reinterpret_cast<const uint16_t *>(p.record + DCVC_ROIL_HEADER) + 3 * (int64_t)a;
    int mode[3], L[3];
    int64_t off = entry.y;
    bool bad = off < table_end;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned e = entries[c];
        mode[c] = (int)(e >> 12), L[c] = (int)(e & 0xfffu);
        if (bad || !roil_length_ok(n, mode[c], L[c]) || off + L[c] > p.size) bad = true, mode[c] = 9, L[c] = 0;
        uint8_t *dst = reinterpret_cast<uint8_t *>(t.seg[c]);
        for (int b = tid; b < L[c]; b += 256) dst[b] = p.record[off + b];
        off += L[c];
    }
    __syncthreads();
    if (x < p.W && y < p.H) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = p.order[j];
            int v = 0;
            if (in) {
                const unsigned *seg = c == 0 ? t.seg[0] : (c == 1 ? t.seg[1] : t.seg[2]);
                const int m = c == 0 ? mode[0] : (c == 1 ? mode[1] : mode[2]), len = c == 0 ? L[0] : (c == 1 ? L[1] : L[2]);
                int u = roil_sample(seg, ROIL_SEG_WORDS, n, m, len, rank);
                if (u < 0) bad = true, u = 0;
                v = roil_reconstruct(u, p.step);
            }
            p.out[j * p.cs + (int64_t)y * p.rs + (int64_t)x * p.px] = (uint8_t)v;
        }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(p.status, DCVC_ROIL_BAD_STREAM);
}

// the active cells of the validated host list, or -1
int active_cells(int32_t H, int32_t W, const dcvc_roi_box_t *boxes, int32_t n, std::vector<int32_t> *counts) {
    const int A = dcvc_roil_cells(H, W, boxes, n, nullptr, nullptr, 0);
    if (A <= 0 || !counts) return A;
    std::vector<int32_t> cells((size_t)A);
    counts->resize((size_t)A);
    return dcvc_roil_cells(H, W, boxes, n, cells.data(), counts->data(), A);
}

}  // namespace

extern "C" int dcvc_roil_encode(const float *src, int32_t src_row_stride, int64_t src_plane_stride, const float *rec,
                                int32_t rec_row_stride, int64_t rec_plane_stride, int32_t H, int32_t W,
                                const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n, int32_t step,
                                const int32_t *table_dev, int32_t A, uint8_t *staging, uint8_t *record, int64_t capacity,
                                uint32_t *size_word, void *stream) {
    if (!size_ok(H, W) || !planes_ok(src, src_row_stride, src_plane_stride, H, W) ||
        !planes_ok(rec, rec_row_stride, rec_plane_stride, H, W) || !boxes_ok(boxes_host, boxes_dev, n, H, W, DCVC_ROI_MAX_CLASSES) ||
        step < 1 || step > DCVC_ROIL_MAX_STEP || A < 0 || !record || !aligned(record, 4) || !size_word || !aligned(size_word, 4) ||
        capacity < DCVC_ROIL_HEADER + (int64_t)DCVC_ROIL_CELL_MAX * A ||
        (A > 0 && (!table_dev || !aligned(table_dev, 8) || !staging || !aligned(staging, 4))))
        return DCVC_E_ARG;
    if (active_cells(H, W, boxes_host, n, nullptr) != A) return DCVC_E_ARG;
    if (A > 0) {
        EncArgs e{};
        e.a = src, e.a_rs = src_row_stride, e.a_ps = src_plane_stride, e.b = rec, e.b_rs = rec_row_stride, e.b_ps = rec_plane_stride;
        e.boxes = boxes_dev, e.table = reinterpret_cast<const int2 *>(table_dev), e.staging = reinterpret_cast<uint32_t *>(staging);
        e.record = record, e.H = H, e.W = W, e.n = n, e.step = step;
        e.wc = (W + CELL - 1) / CELL, e.cells = e.wc * ((H + CELL - 1) / CELL);
        roil_encode_kernel<<<dim3((unsigned)A), dim3(256), 0, (hipStream_t)stream>>>(e);
        if (hipGetLastError() != hipSuccess) return DCVC_E_LAUNCH;
    }
    PackArgs k{};
    k.staging = staging, k.record = record, k.size_word = size_word, k.A = A, k.step = step;
    const unsigned chunks = A > 0 ? nblk(3 * (int64_t)A, 256) : 1u;
    roil_pack_kernel<<<dim3(chunks), dim3(256), 0, (hipStream_t)stream>>>(k);
    RET_LAUNCH();
}

extern "C" int dcvc_roil_decode(const uint8_t *record_host, const uint8_t *record_dev, int64_t size, int32_t H, int32_t W,
                                const dcvc_roi_box_t *boxes_host, const dcvc_roi_box_t *boxes_dev, int32_t n,
                                const int32_t *table_dev, uint8_t *out, int64_t out_chan_stride, int64_t out_row_stride,
                                int32_t out_pixel_stride, int32_t order0, int32_t order1, int32_t order2, uint32_t *status,
                                void *stream) {
    if (!size_ok(H, W) || !record_host || !record_dev || !aligned(record_dev, 2) || size < DCVC_ROIL_HEADER ||
        !boxes_ok(boxes_host, boxes_dev, n, H, W, DCVC_ROI_MAX_CLASSES) ||
        !u8_layout_ok(out, out_chan_stride, out_row_stride, out_pixel_stride, H, W) || !order_ok(order0, order1, order2) || !status ||
        !aligned(status, 4))
        return DCVC_E_ARG;
    std::vector<int32_t> counts;
    const int A = active_cells(H, W, boxes_host, n, &counts);
    if (A < 0 || (A > 0 && (!table_dev || !aligned(table_dev, 8)))) return DCVC_E_ARG;
    const int rc = dcvc_roil_check(record_host, size, counts.data(), A);
    if (rc != DCVC_OK) return rc;
    DecArgs d{};
    d.record = record_dev, d.boxes = boxes_dev, d.table = reinterpret_cast<const int2 *>(table_dev), d.out = out, d.status = status;
    d.size = size, d.cs = out_chan_stride, d.rs = out_row_stride, d.px = out_pixel_stride, d.H = H, d.W = W, d.n = n, d.A = A, d.step = record_host[3];
    d.wc = (W + CELL - 1) / CELL, d.cells = d.wc * ((H + CELL - 1) / CELL);
    d.order[0] = order0, d.order[1] = order1, d.order[2] = order2;
    d.vec = aligned(out, 4) && out_row_stride % 4 == 0 && (out_pixel_stride == 3 || out_chan_stride % 4 == 0);
    const int rows = out_pixel_stride == 1 ? 3 * H : H, row_bytes = out_pixel_stride == 1 ? W : 3 * W;
    roil_zero_kernel<<<dim3((unsigned)rows, nblk(row_bytes, 1024)), dim3(256), 0, (hipStream_t)stream>>>(d);
    if (hipGetLastError() != hipSuccess) return DCVC_E_LAUNCH;
    if (A > 0) roil_decode_kernel<<<dim3((unsigned)A), dim3(256), 0, (hipStream_t)stream>>>(d);
    RET_LAUNCH();
}
