// color.hip -- 4:2:0 Y'CbCr sample planes <-> planar fp32 RGB (include/dcvc_hip_color.h, which states the arithmetic and
// its order; this file only arranges it).
//
// Both kernels are streaming kernels: a lane owns a block of 2 luma rows x 4 luma columns, i.e. one chroma row and two
// chroma columns, so chroma is fetched (or produced) once per block.  A wave is 64 such blocks side by side: its luma
// loads are 256 (512) contiguous bytes per row, its fp32 accesses 1 KB contiguous per row and plane (16 bytes a lane).
// A workgroup is 4 waves stacked: 8 rows x 256 columns.  Vector accesses need aligned rows; a picture whose width or
// pointers do not provide that, and the last block of a row whose width is not a multiple of 4, take scalar accesses
// guarded by the width -- the arithmetic is the same code.  No LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_color.h"
#include "kernel_common.h"

#pragma clang fp contract(off)

namespace {

#include "unit8_table.h"

struct ToRgb {
    const void *y, *u, *v;
    float *rgb;
    dcvc_color_coeffs_t cc;
    int64_t plane_stride;
    int32_t H, W, y_stride, c_stride, out_H, out_W, row_stride, quantize8, vec_in, vec_out;
};

struct FromRgb {
    const float *rgb;
    void *y, *u, *v;
    const void *src_y, *src_u, *src_v;
    unsigned long long *sse;
    dcvc_color_coeffs_t cc;
    int64_t plane_stride;
    int32_t H, W, row_stride, y_stride, c_stride, src_y_stride, src_c_stride, vec_in, vec_out;
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// four consecutive samples as one 4- or 8-byte access
__device__ __forceinline__ void load4(const uint8_t *p, int s[4]) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
    s[0] = w & 255u, s[1] = (w >> 8) & 255u, s[2] = (w >> 16) & 255u, s[3] = w >> 24;
}
__device__ __forceinline__ void load4(const uint16_t *p, int s[4]) {
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    s[0] = w.x & 65535u, s[1] = w.x >> 16, s[2] = w.y & 65535u, s[3] = w.y >> 16;
}
__device__ __forceinline__ void store4(uint8_t *p, const int s[4]) {
    *reinterpret_cast<uint32_t *>(p) = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}
__device__ __forceinline__ void store4(uint16_t *p, const int s[4]) {
    *reinterpret_cast<uint2 *>(p) = make_uint2((uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16));
}

// The chroma of one lane's block, in sixteenths: out[r][q] for luma row y0 + r, luma column x0 + q.
template <typename S>
__device__ __forceinline__ void upsample_chroma(const S *c, int stride, int CH, int CW, int j, int i0, int siting, int out[2][4]) {
    const int rows[3] = {max(j - 1, 0), j, min(j + 1, CH - 1)};
    const int cols[4] = {max(i0 - 1, 0), i0, min(i0 + 1, CW - 1), min(i0 + 2, CW - 1)};
    int s[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[a][k] = (int)c[(size_t)rows[a] * stride + cols[k]];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 3 * s[1][k] + s[r == 0 ? 0 : 2][k];
        if (siting == DCVC_SITING_CENTER) {
            out[r][0] = 3 * v[1] + v[0], out[r][1] = 3 * v[1] + v[2], out[r][2] = 3 * v[2] + v[1], out[r][3] = 3 * v[2] + v[3];
        } else {
            out[r][0] = 4 * v[1], out[r][1] = 2 * v[1] + 2 * v[2], out[r][2] = 4 * v[2], out[r][3] = 2 * v[2] + 2 * v[3];
        }
    }
}

template <typename S>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const ToRgb p) {
    const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
    const int x0 = bx * 4, y0 = by * 2;
    if (x0 >= p.out_W || y0 >= p.out_H) return;
    float px[3][2][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) px[c][r][q] = 0.0f;  // the padding right of W and below H

    if (x0 < p.W && y0 < p.H) {  // (H is even: row y0 + 1 exists with row y0)
        const dcvc_color_coeffs_t &k = p.cc;
        int cu[2][4], cv[2][4];
        upsample_chroma(static_cast<const S *>(p.u), p.c_stride, p.H / 2, p.W / 2, by, bx * 2, k.siting, cu);
        upsample_chroma(static_cast<const S *>(p.v), p.c_stride, p.H / 2, p.W / 2, by, bx * 2, k.siting, cv);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const S *row = static_cast<const S *>(p.y) + (size_t)(y0 + r) * p.y_stride + x0;
            int ys[4];
            if (p.vec_in && x0 + 4 <= p.W) {
                load4(row, ys);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) ys[q] = x0 + q < p.W ? (int)row[q] : 0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (x0 + q >= p.W) continue;
                const float yp = ((float)ys[q] - k.y_off) * k.y_scale;
                const float cb = ((float)cu[r][q] * 0.0625f - k.c_off) * k.c_scale;
                const float cr = ((float)cv[r][q] * 0.0625f - k.c_off) * k.c_scale;
                float rgb[3] = {clamp01(yp + k.crr * cr), clamp01((yp - k.cgb * cb) - k.cgr * cr), clamp01(yp + k.cbb * cb)};
                if (p.quantize8) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[c] = kUnit8.v[(int)rintf(255.0f * rgb[c])];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c][r][q] = rgb[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (y0 + r >= p.out_H) continue;
            float *dst = p.rgb + (size_t)c * p.plane_stride + (size_t)(y0 + r) * p.row_stride + x0;
            if (p.vec_out && x0 + 4 <= p.out_W) {
                *reinterpret_cast<float4 *>(dst) = make_float4(px[c][r][0], px[c][r][1], px[c][r][2], px[c][r][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.out_W) dst[q] = px[c][r][q];
            }
        }
}

__device__ __forceinline__ int to_code(float v, float range, float off, int max_code) {
    return (int)fminf(fmaxf(rintf(v * range + off), 0.0f), (float)max_code);
}

template <typename S>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const FromRgb p) {
    const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y;
    const int x0 = bx * 4, y0 = by * 2;
    unsigned sq[3] = {0u, 0u, 0u};  // this lane's squared differences (at most 8 * 1023^2: a wave's sum fits 32 bits)
    if (x0 < p.W && y0 < p.H) {
        const dcvc_color_coeffs_t &k = p.cc;
        // column slot 0 is the left neighbour x0 - 1 (clamped at 0), slots 1..4 are x0 .. x0 + 3
        float cb[2][5], cr[2][5];
        int ys[2][4];
        const int xl = max(x0 - 1, 0);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float in[3][5];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *row = p.rgb + (size_t)c * p.plane_stride + (size_t)(y0 + r) * p.row_stride;
                in[c][0] = k.siting == DCVC_SITING_LEFT ? row[xl] : 0.0f;
                if (p.vec_in && x0 + 4 <= p.W) {
                    const float4 f = *reinterpret_cast<const float4 *>(row + x0);
                    in[c][1] = f.x, in[c][2] = f.y, in[c][3] = f.z, in[c][4] = f.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) in[c][1 + q] = x0 + q < p.W ? row[x0 + q] : 0.0f;
                }
            }
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const float R = clamp01(in[0][s]), G = clamp01(in[1][s]), B = clamp01(in[2][s]);
                const float yp = (k.kr * R + k.kg * G) + k.kb * B;
                cb[r][s] = (B - yp) * k.icb;
                cr[r][s] = (R - yp) * k.icr;
                if (s > 0) ys[r][s - 1] = to_code(yp, k.y_range, k.y_off, k.max_code);
            }
            S *dst = static_cast<S *>(p.y) + (size_t)(y0 + r) * p.y_stride + x0;
            if (p.vec_out && x0 + 4 <= p.W) {
                store4(dst, ys[r]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) dst[q] = (S)ys[r][q];
            }
            if (p.sse) {
                const S *src = static_cast<const S *>(p.src_y) + (size_t)(y0 + r) * p.src_y_stride + x0;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) {
                        const int d = ys[r][q] - (int)src[q];
                        sq[0] += (unsigned)(d * d);
                    }
            }
        }
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            if (x0 + 2 * ci >= p.W) continue;  // (W is even: column x0 + 2 ci + 1 exists with column x0 + 2 ci)
            const int m = 1 + 2 * ci;
            float fu, fv;
            if (k.siting == DCVC_SITING_CENTER) {
                fu = ((cb[0][m] + cb[0][m + 1]) + (cb[1][m] + cb[1][m + 1])) * 0.25f;
                fv = ((cr[0][m] + cr[0][m + 1]) + (cr[1][m] + cr[1][m + 1])) * 0.25f;
            } else {
                const float ul = cb[0][m - 1] + cb[1][m - 1], um = cb[0][m] + cb[1][m], ur = cb[0][m + 1] + cb[1][m + 1];
                const float vl = cr[0][m - 1] + cr[1][m - 1], vm = cr[0][m] + cr[1][m], vr = cr[0][m + 1] + cr[1][m + 1];
                fu = ((ul + ur) + (um + um)) * 0.125f;
                fv = ((vl + vr) + (vm + vm)) * 0.125f;
            }
            const int su = to_code(fu, k.c_range, k.c_off, k.max_code), sv = to_code(fv, k.c_range, k.c_off, k.max_code);
            const size_t at = (size_t)by * p.c_stride + bx * 2 + ci;
            static_cast<S *>(p.u)[at] = (S)su;
            static_cast<S *>(p.v)[at] = (S)sv;
            if (p.sse) {
                const size_t sat = (size_t)by * p.src_c_stride + bx * 2 + ci;
                const int du = su - (int)static_cast<const S *>(p.src_u)[sat], dv = sv - (int)static_cast<const S *>(p.src_v)[sat];
                sq[1] += (unsigned)(du * du);
                sq[2] += (unsigned)(dv * dv);
            }
        }
    }
    if (p.sse) {  // (uniform: every lane of the wave takes part in the shuffles, idle blocks with zeros)
        // One vector atomic per wave and plane.  Measured 161 us at 1080x1920 (12240 adds onto three integers in one cache
        // line, the likely cause) against 7.5 us without sums: 0.7 % of a picture's time, paid only with a report; summing
        // per workgroup first is the next step (profiles/yuv_io_1080p.txt).
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned total = wave_sum(sq[c]);
            if (threadIdx.x == 0 && total) atomicAdd(p.sse + c, (unsigned long long)total);
        }
    }
}

bool aligned(const void *p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

bool coeffs_ok(const dcvc_color_coeffs_t *cc) {
    return cc && (cc->bit_depth == 8 || cc->bit_depth == 10) && cc->max_code == (1 << cc->bit_depth) - 1 &&
           (cc->siting == DCVC_SITING_LEFT || cc->siting == DCVC_SITING_CENTER);
}

bool size_ok(int32_t H, int32_t W) {
    return H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && H <= DCVC_COLOR_MAX_SIDE && W <= DCVC_COLOR_MAX_SIDE;
}

}  // namespace

extern "C" int dcvc_color_coeffs(int32_t matrix, int32_t range, int32_t bit_depth, int32_t siting, dcvc_color_coeffs_t *out) {
    if (!out || (matrix != DCVC_MATRIX_BT709 && matrix != DCVC_MATRIX_BT601) ||
        (range != DCVC_RANGE_LIMITED && range != DCVC_RANGE_FULL) || (bit_depth != 8 && bit_depth != 10) ||
        (siting != DCVC_SITING_LEFT && siting != DCVC_SITING_CENTER))
        return DCVC_E_ARG;
    const double kr = matrix == DCVC_MATRIX_BT709 ? 0.2126 : 0.299, kb = matrix == DCVC_MATRIX_BT709 ? 0.0722 : 0.114;
    const double kg = (1.0 - kr) - kb;
    const double s = (double)(1 << (bit_depth - 8)), mx = (double)((1 << bit_depth) - 1);
    const double y_off = range == DCVC_RANGE_LIMITED ? 16.0 * s : 0.0, c_off = 128.0 * s;
    const double y_range = range == DCVC_RANGE_LIMITED ? 219.0 * s : mx, c_range = range == DCVC_RANGE_LIMITED ? 224.0 * s : mx;
    out->y_off = (float)y_off, out->c_off = (float)c_off;
    out->y_scale = (float)(1.0 / y_range), out->c_scale = (float)(1.0 / c_range);
    out->crr = (float)(2.0 * (1.0 - kr));
    out->cgb = (float)(2.0 * kb * (1.0 - kb) / kg);
    out->cgr = (float)(2.0 * kr * (1.0 - kr) / kg);
    out->cbb = (float)(2.0 * (1.0 - kb));
    out->kr = (float)kr, out->kg = (float)kg, out->kb = (float)kb;
    out->icb = (float)(1.0 / (2.0 * (1.0 - kb))), out->icr = (float)(1.0 / (2.0 * (1.0 - kr)));
    out->y_range = (float)y_range, out->c_range = (float)c_range;
    out->max_code = (1 << bit_depth) - 1;
    out->bit_depth = bit_depth, out->siting = siting, out->matrix = matrix, out->range = range;
    return DCVC_OK;
}

extern "C" int dcvc_yuv420_to_rgb(const void *y, const void *u, const void *v, int32_t H, int32_t W, int32_t y_stride,
                                  int32_t c_stride, const dcvc_color_coeffs_t *cc, float *rgb, int32_t out_H, int32_t out_W,
                                  int32_t out_row_stride, int64_t out_plane_stride, int32_t quantize8, void *stream) {
    if (!y || !u || !v || !rgb || !coeffs_ok(cc) || !size_ok(H, W)) return DCVC_E_ARG;
    if (out_H < H || out_W < W || out_H > DCVC_COLOR_MAX_SIDE || out_W > DCVC_COLOR_MAX_SIDE || y_stride < W ||
        c_stride < W / 2 || out_row_stride < out_W || out_plane_stride < (int64_t)(out_H - 1) * out_row_stride + out_W)
        return DCVC_E_ARG;
    const size_t sb = cc->bit_depth == 8 ? 1 : 2;
    ToRgb p{};
    p.y = y, p.u = u, p.v = v, p.rgb = rgb, p.cc = *cc, p.plane_stride = out_plane_stride;
    p.H = H, p.W = W, p.y_stride = y_stride, p.c_stride = c_stride, p.out_H = out_H, p.out_W = out_W;
    p.row_stride = out_row_stride, p.quantize8 = quantize8 != 0;
    p.vec_in = aligned(y, 4 * sb) && y_stride % 4 == 0;
    p.vec_out = aligned(rgb, 16) && out_row_stride % 4 == 0 && out_plane_stride % 4 == 0;
    const dim3 block(64, 4), grid((out_W + 255) / 256, (out_H + 7) / 8);
    if (sb == 1)
        yuv420_to_rgb_kernel<uint8_t><<<grid, block, 0, (hipStream_t)stream>>>(p);
    else
        yuv420_to_rgb_kernel<uint16_t><<<grid, block, 0, (hipStream_t)stream>>>(p);
    RET_LAUNCH();
}

extern "C" int dcvc_rgb_to_yuv420(const float *rgb, int32_t H, int32_t W, int32_t row_stride, int64_t plane_stride,
                                  const dcvc_color_coeffs_t *cc, void *y, void *u, void *v, int32_t y_stride, int32_t c_stride,
                                  const void *src_y, const void *src_u, const void *src_v, int32_t src_y_stride,
                                  int32_t src_c_stride, uint64_t *sse, void *stream) {
    if (!rgb || !y || !u || !v || !coeffs_ok(cc) || !size_ok(H, W)) return DCVC_E_ARG;
    if (row_stride < W || plane_stride < (int64_t)(H - 1) * row_stride + W || y_stride < W || c_stride < W / 2) return DCVC_E_ARG;
    const int n_src = (src_y != nullptr) + (src_u != nullptr) + (src_v != nullptr) + (sse != nullptr);
    if (n_src != 0 && n_src != 4) return DCVC_E_ARG;
    if (n_src && (src_y_stride < W || src_c_stride < W / 2 || !aligned(sse, 8))) return DCVC_E_ARG;
    const size_t sb = cc->bit_depth == 8 ? 1 : 2;
    if (sb == 2 && !(aligned(y, 2) && aligned(u, 2) && aligned(v, 2) && (!n_src || (aligned(src_y, 2) && aligned(src_u, 2) && aligned(src_v, 2)))))
        return DCVC_E_ARG;
    FromRgb p{};
    p.rgb = rgb, p.y = y, p.u = u, p.v = v, p.src_y = src_y, p.src_u = src_u, p.src_v = src_v;
    p.sse = reinterpret_cast<unsigned long long *>(sse), p.cc = *cc, p.plane_stride = plane_stride;
    p.H = H, p.W = W, p.row_stride = row_stride, p.y_stride = y_stride, p.c_stride = c_stride;
    p.src_y_stride = src_y_stride, p.src_c_stride = src_c_stride;
    p.vec_in = aligned(rgb, 16) && row_stride % 4 == 0 && plane_stride % 4 == 0;
    p.vec_out = aligned(y, 4 * sb) && y_stride % 4 == 0;
    const dim3 block(64, 4), grid((W + 255) / 256, (H + 7) / 8);
    if (sb == 1)
        rgb_to_yuv420_kernel<uint8_t><<<grid, block, 0, (hipStream_t)stream>>>(p);
    else
        rgb_to_yuv420_kernel<uint16_t><<<grid, block, 0, (hipStream_t)stream>>>(p);
    RET_LAUNCH();
}
