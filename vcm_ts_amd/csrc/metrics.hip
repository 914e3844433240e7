// metrics.hip -- MS-SSIM (pytorch_msssim.ms_ssim 1.0 semantics) and its gradient on planar fp32 pictures; the squared
// error for PSNR comes out of the same loads.  Definition and C ABI: include/dcvc_hip_metrics.h; DESIGN.md 4d.
//
//   level_kernel<0>   one 32x32 tile of a level's SSIM maps per workgroup: the 42x42 input tile (10-pixel halo) of X and
//                     Y is staged once in LDS, five products (x, d = x - y, xx, yy, dd) are filtered row-wise into LDS and
//                     column-wise into registers, the cs / ssim maps are reduced in the workgroup in a fixed order and
//                     ONE partial sum per (plane, tile) is written -- no atomics.
//   level_kernel<1>   the same code up to the maps, then the three gradient maps a = dL/dmu1, b = dL/dE[xx],
//                     c = dL/dE[xy] are written instead of the sums.
//   gradT_kernel      dL/dX = G^T a + 2 X G^T b + Y G^T c ("full" transposed separable filter out of LDS) plus the
//                     avg-pool transpose of the coarser level's gradient.
//   pool_kernel       avg_pool2d(2, 2, padding = (H%2, W%2)), zeros counted, of X and Y in one launch.
//   finish_kernel     per sample: the partial sums in a fixed order (fp64), relu, the weighted product, the mean over the
//                     channels; with an upstream gradient also the per-(level, plane) map coefficients.
//
// All of it is bound by HBM / L2 traffic and launch latency (66 MB at 3x1080x1920); nothing here is MFMA work.
// Contraction is off for the file and the fused operations are written out, so both instantiations of level_kernel
// compute s1, s2 and var(x - y) -- differences of nearly equal numbers -- with exactly the same operations.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_metrics.h"
#include "kernel_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TAPS = 11, HALO = TAPS - 1, TILE = 32, IN = TILE + HALO, LEVELS = DCVC_MS_SSIM_LEVELS, THREADS = 256;
constexpr int MAX_SIDE = 32768, MAX_PLANES = 65535;
const double LEVEL_WEIGHTS[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

struct Window {
    float g[TAPS];
};

struct LevelArgs {
    const float *x, *y;
    int64_t x_ps, y_ps;
    int x_rs, y_rs, H, W, clamp;
    float C1, C2;
    float *part;      // MODE 0: (planes, tiles, 2) sums of cs_map and ssim_map
    float *sse_part;  // MODE 0, optional: (planes, tiles) sums of (x - y)^2 over the pixels a tile owns
    const float *coef;  // MODE 1: per plane, dL/d(map pixel) of the map this level keeps
    float *maps;        // MODE 1: (3, planes, H-10, W-10)
    int last, planes;
    Window w;
};

// fixed-order sum over the workgroup: a shuffle tree inside each wave, then the four wave sums in order by thread 0
__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void level_kernel(const LevelArgs a) {
    __shared__ float sx[IN][IN + 1], sy[IN][IN + 1];
    __shared__ float rb[5][IN][TILE + 1];
    __shared__ float red[3][4];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const int Ho = a.H - HALO, Wo = a.W - HALO;
    const float *xp = a.x + (int64_t)plane * a.x_ps, *yp = a.y + (int64_t)plane * a.y_ps;
    // every input pixel belongs to exactly one tile for the squared error: the tile's own 32x32, and for the last tile
    // row / column also the halo (which reaches the picture's edge there)
    const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
    float sse = 0.0f;
    for (int i = tid; i < IN * IN; i += THREADS) {
        const int r = i / IN, c = i - r * IN, gy = y0 + r, gx = x0 + c;
        float vx = 0.0f, vy = 0.0f;
        if (gy < a.H && gx < a.W) {
            vx = xp[(int64_t)gy * a.x_rs + gx];
            vy = yp[(int64_t)gy * a.y_rs + gx];
            if (a.clamp) vx = fminf(fmaxf(vx, 0.0f), 1.0f);
            if (MODE == 0 && (r < TILE || lasty) && (c < TILE || lastx)) {
                const float d = vx - vy;
                sse = fmaf(d, d, sse);
            }
        }
        sx[r][c] = vx;
        sy[r][c] = vy;
    }
    __syncthreads();
    for (int i = tid; i < IN * TILE; i += THREADS) {
        const int r = i / TILE, c = i - r * TILE;
        float m1 = 0.0f, md = 0.0f, xx = 0.0f, yy = 0.0f, dd = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float g = a.w.g[k], x = sx[r][c + k], y = sy[r][c + k], d = x - y;
            m1 = fmaf(g, x, m1);
            md = fmaf(g, d, md);
            xx = fmaf(g, x * x, xx);
            yy = fmaf(g, y * y, yy);
            dd = fmaf(g, d * d, dd);
        }
        rb[0][r][c] = m1;
        rb[1][r][c] = md;
        rb[2][r][c] = xx;
        rb[3][r][c] = yy;
        rb[4][r][c] = dd;
    }
    __syncthreads();
    float acc_cs = 0.0f, acc_ssim = 0.0f;
    const float coef = MODE == 1 ? a.coef[plane] : 0.0f;
    for (int i = tid; i < TILE * TILE; i += THREADS) {
        const int r = i / TILE, c = i - r * TILE, oy = y0 + r, ox = x0 + c;
        if (oy >= Ho || ox >= Wo) continue;
        float m1 = 0.0f, md = 0.0f, xx = 0.0f, yy = 0.0f, dd = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float g = a.w.g[k];
            m1 = fmaf(g, rb[0][r + k][c], m1);
            md = fmaf(g, rb[1][r + k][c], md);
            xx = fmaf(g, rb[2][r + k][c], xx);
            yy = fmaf(g, rb[3][r + k][c], yy);
            dd = fmaf(g, rb[4][r + k][c], dd);
        }
        // s1 + s2 - 2 s12 is the windowed variance of the DIFFERENCE x - y; taken from d directly it is a small number
        // computed from small numbers, where 2 s12 - (s1 + s2) would cancel three window sums of size ~mean^2:
        // cs = (2 s12 + C2) / (s1 + s2 + C2) = 1 - var(d) / (s1 + s2 + C2)
        const float m2 = m1 - md;
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s1 = xx - m11, s2 = yy - m22, vd = dd - md * md;
        const float D = (s1 + s2) + a.C2;
        const float cs = 1.0f - vd / D;
        const float lden = (m11 + m22) + a.C1;
        const float lum = (2.0f * m12 + a.C1) / lden;
        if (MODE == 0) {
            acc_cs += cs;
            acc_ssim += lum * cs;
        } else {
            // levels 0..3 keep mean(cs_map), level 4 keeps mean(lum * cs_map)
            const float g_cs = a.last ? coef * lum : coef;
            const float g_s12 = 2.0f * g_cs / D, g_s1 = -(g_cs * cs) / D;
            float ga = -2.0f * g_s1 * m1 - g_s12 * m2;
            if (a.last) ga += coef * cs * (2.0f * m2 - 2.0f * lum * m1) / lden;
            const int64_t map = (int64_t)Ho * Wo, o = (int64_t)plane * map + (int64_t)oy * Wo + ox;
            a.maps[o] = ga;
            a.maps[(int64_t)a.planes * map + o] = g_s1;
            a.maps[2 * (int64_t)a.planes * map + o] = g_s12;
        }
    }
    if (MODE == 0) {
        const float t_cs = block_sum(acc_cs, red[0]), t_ssim = block_sum(acc_ssim, red[1]);
        const float t_sse = a.sse_part ? block_sum(sse, red[2]) : 0.0f;
        if (tid == 0) {
            const int64_t tile = ((int64_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            a.part[2 * tile] = t_cs;
            a.part[2 * tile + 1] = t_ssim;
            if (a.sse_part) a.sse_part[tile] = t_sse;
        }
    }
}

struct GradArgs {
    const float *maps;  // (3, planes, H-10, W-10)
    const float *x, *y;
    int64_t x_ps, y_ps;
    int x_rs, y_rs, H, W, planes;
    const float *coarse;  // gradient of the next level's X (planes, Hc, Wc), or NULL at the last level
    int Hc, Wc, py, px;
    float *gx;  // (planes, H, W) dense
    Window w;
};

__global__ __launch_bounds__(THREADS) void gradT_kernel(const GradArgs a) {
    __shared__ float s[3][IN][IN + 1];
    __shared__ float t[3][IN][TILE + 1];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const int Ho = a.H - HALO, Wo = a.W - HALO;
    const int64_t map = (int64_t)Ho * Wo;
    for (int i = tid; i < 3 * IN * IN; i += THREADS) {
        const int q = i / (IN * IN), j = i - q * (IN * IN), r = j / IN, c = j - r * IN;
        const int my = y0 - HALO + r, mx = x0 - HALO + c;
        float v = 0.0f;
        if (my >= 0 && my < Ho && mx >= 0 && mx < Wo) v = a.maps[((int64_t)q * a.planes + plane) * map + (int64_t)my * Wo + mx];
        s[q][r][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < 3 * IN * TILE; i += THREADS) {
        const int q = i / (IN * TILE), j = i - q * (IN * TILE), r = j / TILE, c = j - r * TILE;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) acc = fmaf(a.w.g[k], s[q][r][c + HALO - k], acc);
        t[q][r][c] = acc;
    }
    __syncthreads();
    const float *xp = a.x + (int64_t)plane * a.x_ps, *yp = a.y + (int64_t)plane * a.y_ps;
    for (int i = tid; i < TILE * TILE; i += THREADS) {
        const int r = i / TILE, c = i - r * TILE, gy = y0 + r, gx = x0 + c;
        if (gy >= a.H || gx >= a.W) continue;
        float A = 0.0f, B = 0.0f, Cc = 0.0f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float g = a.w.g[k];
            A = fmaf(g, t[0][r + HALO - k][c], A);
            B = fmaf(g, t[1][r + HALO - k][c], B);
            Cc = fmaf(g, t[2][r + HALO - k][c], Cc);
        }
        const float x = xp[(int64_t)gy * a.x_rs + gx], y = yp[(int64_t)gy * a.y_rs + gx];
        float v = (A + 2.0f * x * B) + y * Cc;
        // avg_pool2d transposed: a quarter of the pooled pixel this one went into (padded positions got nothing)
        if (a.coarse) v += 0.25f * a.coarse[((int64_t)plane * a.Hc + ((gy + a.py) >> 1)) * a.Wc + ((gx + a.px) >> 1)];
        a.gx[((int64_t)plane * a.H + gy) * a.W + gx] = v;
    }
}

struct PoolArgs {
    const float *in[2];
    int64_t in_ps[2];
    int in_rs[2], clamp[2];
    float *out[2];  // (planes, Ho, Wo) dense
    int H, W, Ho, Wo, py, px;
};

__global__ __launch_bounds__(THREADS) void pool_kernel(const PoolArgs a) {
    const int which = blockIdx.z, plane = blockIdx.y;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.Ho * a.Wo) return;
    const int oy = i / a.Wo, ox = i - oy * a.Wo;
    const float *p = a.in[which] + (int64_t)plane * a.in_ps[which];
    const int rs = a.in_rs[which], clamp = a.clamp[which];
    float v[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int yy = 2 * oy - a.py + (d >> 1), xx = 2 * ox - a.px + (d & 1);
        float t = 0.0f;
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
            t = p[(int64_t)yy * rs + xx];
            if (clamp) t = fminf(fmaxf(t, 0.0f), 1.0f);
        }
        v[d] = t;
    }
    a.out[which][(int64_t)plane * a.Ho * a.Wo + i] = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25f;
}

struct FinishArgs {
    const float *part[LEVELS];
    int tiles[LEVELS];
    double inv_count[LEVELS], weight[LEVELS];
    const float *sse_part;
    int C, planes;
    float *out_ms, *out_levels, *out_sse;
    const float *g_ms;
    float *coef;  // (LEVELS, planes)
};

// sum of p[0], p[stride], ... (n terms) in fp64: thread-strided partial sums, then a fixed tree over the workgroup
__device__ double strided_sum(const float *p, int n, int stride, double *red) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) acc += (double)p[(int64_t)i * stride];
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const FinishArgs a) {
    __shared__ double red[THREADS];
    const int n = blockIdx.x;
    double ms_sum = 0.0, sse = 0.0;
    for (int c = 0; c < a.C; ++c) {
        const int plane = n * a.C + c;
        double kept[LEVELS], ms = 1.0;
        for (int l = 0; l < LEVELS; ++l) {
            const int which = l == LEVELS - 1 ? 1 : 0;
            const double mean = strided_sum(a.part[l] + 2 * (int64_t)plane * a.tiles[l] + which, a.tiles[l], 2, red) * a.inv_count[l];
            kept[l] = mean > 0.0 ? mean : 0.0;
            ms *= pow(kept[l], a.weight[l]);
        }
        if (a.sse_part) sse += strided_sum(a.sse_part + (int64_t)plane * a.tiles[0], a.tiles[0], 1, red);
        ms_sum += ms;
        if (threadIdx.x == 0) {
            for (int l = 0; l < LEVELS; ++l) {
                if (a.out_levels) a.out_levels[l * a.planes + plane] = (float)kept[l];
                if (a.g_ms)
                    a.coef[l * a.planes + plane] =
                        kept[l] > 0.0 ? (float)((double)a.g_ms[n] / a.C * a.weight[l] * ms / kept[l] * a.inv_count[l]) : 0.0f;
            }
        }
    }
    if (threadIdx.x == 0) {
        a.out_ms[n] = (float)(ms_sum / a.C);
        if (a.out_sse) a.out_sse[n] = (float)sse;
    }
}

// ------------------------------------------------------------------------------------------------- host side
inline int64_t r4(int64_t n) { return (n + 3) / 4 * 4; }

struct Plan {
    int H[LEVELS], W[LEVELS], tx[LEVELS], ty[LEVELS];
    int64_t px[LEVELS], py[LEVELS];  // pyramid planes of X and Y (levels 1..4), float offsets into the workspace
    int64_t part[LEVELS], sse_part, levels, coef, ms, maps, g[LEVELS], total;
};

bool shape_ok(int N, int C, int H, int W) {
    return N >= 1 && C >= 1 && (int64_t)N * C <= MAX_PLANES && H >= DCVC_MS_SSIM_MIN_SIDE && W >= DCVC_MS_SSIM_MIN_SIDE &&
           H <= MAX_SIDE && W <= MAX_SIDE;
}

Plan make_plan(int N, int C, int H, int W, bool want_grad) {
    Plan p{};
    const int64_t planes = (int64_t)N * C;
    int64_t off = 0;
    auto take = [&](int64_t n) {
        const int64_t at = off;
        off += r4(n);
        return at;
    };
    for (int l = 0; l < LEVELS; ++l) {
        p.H[l] = l ? (p.H[l - 1] + 2 * (p.H[l - 1] % 2) - 2) / 2 + 1 : H;
        p.W[l] = l ? (p.W[l - 1] + 2 * (p.W[l - 1] % 2) - 2) / 2 + 1 : W;
        p.tx[l] = (p.W[l] - HALO + TILE - 1) / TILE;
        p.ty[l] = (p.H[l] - HALO + TILE - 1) / TILE;
        if (l) {
            p.px[l] = take(planes * p.H[l] * p.W[l]);
            p.py[l] = take(planes * p.H[l] * p.W[l]);
        }
        p.part[l] = take(2 * planes * p.tx[l] * p.ty[l]);
    }
    p.sse_part = take(planes * p.tx[0] * p.ty[0]);
    p.levels = take(LEVELS * planes);
    p.coef = take(LEVELS * planes);
    p.ms = take(N);
    if (want_grad) {
        p.maps = take(3 * planes * (H - HALO) * (W - HALO));
        for (int l = 1; l < LEVELS; ++l) p.g[l] = take(planes * p.H[l] * p.W[l]);
    }
    p.total = off;
    return p;
}

Window make_window() {
    double g[TAPS], sum = 0.0;
    for (int k = 0; k < TAPS; ++k) sum += g[k] = exp(-(double)((k - TAPS / 2) * (k - TAPS / 2)) / (2.0 * 1.5 * 1.5));
    Window w;
    for (int k = 0; k < TAPS; ++k) w.g[k] = (float)(g[k] / sum);
    return w;
}

struct Operands {
    const float *x, *y;
    int N, C, H, W, x_rs, y_rs;
    int64_t x_ps, y_ps;
    float data_range;
    int clamp;
};

bool operands_ok(const Operands &o, const void *workspace) {
    if (!o.x || !o.y || !workspace || !shape_ok(o.N, o.C, o.H, o.W)) return false;
    if (o.x_rs < o.W || o.y_rs < o.W) return false;
    const int64_t need_x = (int64_t)(o.H - 1) * o.x_rs + o.W, need_y = (int64_t)(o.H - 1) * o.y_rs + o.W;
    if (o.x_ps < need_x || o.y_ps < need_y) return false;
    if (!(o.data_range > 0.0f) || !isfinite(o.data_range)) return false;
    return ((uintptr_t)workspace & 15) == 0;
}

// pyramid + per-level sums + finish; leaves the pyramid, kept values and (with g_ms) the map coefficients in the workspace
int run_forward(const Operands &o, const Plan &p, float *ws, const Window &w, float *out_ms, float *out_levels,
                float *out_sse, const float *g_ms, hipStream_t st) {
    const int planes = o.N * o.C;
    const float C1 = (0.01f * o.data_range) * (0.01f * o.data_range), C2 = (0.03f * o.data_range) * (0.03f * o.data_range);
    FinishArgs f{};
    for (int l = 0; l < LEVELS; ++l) {
        LevelArgs a{};
        a.x = l ? ws + p.px[l] : o.x;
        a.y = l ? ws + p.py[l] : o.y;
        a.x_rs = l ? p.W[l] : o.x_rs;
        a.y_rs = l ? p.W[l] : o.y_rs;
        a.x_ps = l ? (int64_t)p.H[l] * p.W[l] : o.x_ps;
        a.y_ps = l ? (int64_t)p.H[l] * p.W[l] : o.y_ps;
        a.H = p.H[l];
        a.W = p.W[l];
        a.clamp = l ? 0 : o.clamp;
        a.C1 = C1;
        a.C2 = C2;
        a.part = ws + p.part[l];
        a.sse_part = (l == 0 && out_sse) ? ws + p.sse_part : nullptr;
        a.planes = planes;
        a.w = w;
        hipLaunchKernelGGL(level_kernel<0>, dim3(p.tx[l], p.ty[l], planes), dim3(THREADS), 0, st, a);
        if (l + 1 < LEVELS) {
            PoolArgs q{};
            q.in[0] = a.x, q.in[1] = a.y;
            q.in_ps[0] = a.x_ps, q.in_ps[1] = a.y_ps;
            q.in_rs[0] = a.x_rs, q.in_rs[1] = a.y_rs;
            q.clamp[0] = a.clamp, q.clamp[1] = 0;
            q.out[0] = ws + p.px[l + 1], q.out[1] = ws + p.py[l + 1];
            q.H = p.H[l], q.W = p.W[l], q.Ho = p.H[l + 1], q.Wo = p.W[l + 1];
            q.py = p.H[l] % 2, q.px = p.W[l] % 2;
            const unsigned blocks = (unsigned)(((int64_t)q.Ho * q.Wo + THREADS - 1) / THREADS);
            hipLaunchKernelGGL(pool_kernel, dim3(blocks, planes, 2), dim3(THREADS), 0, st, q);
        }
        f.part[l] = ws + p.part[l];
        f.tiles[l] = p.tx[l] * p.ty[l];
        f.inv_count[l] = 1.0 / ((double)(p.H[l] - HALO) * (double)(p.W[l] - HALO));
        f.weight[l] = LEVEL_WEIGHTS[l];
    }
    f.sse_part = out_sse ? ws + p.sse_part : nullptr;
    f.C = o.C;
    f.planes = planes;
    f.out_ms = out_ms ? out_ms : ws + p.ms;
    f.out_levels = out_levels ? out_levels : ws + p.levels;
    f.out_sse = out_sse;
    f.g_ms = g_ms;
    f.coef = ws + p.coef;
    hipLaunchKernelGGL(finish_kernel, dim3(o.N), dim3(THREADS), 0, st, f);
    RET_LAUNCH();
}

}  // namespace

extern "C" {

int64_t dcvc_ms_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t want_grad) {
    if (!shape_ok(N, C, H, W)) return 0;
    return make_plan(N, C, H, W, want_grad != 0).total * (int64_t)sizeof(float);
}

int dcvc_ms_ssim(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t x_row_stride,
                 int64_t x_plane_stride, int32_t y_row_stride, int64_t y_plane_stride, float data_range,
                 int32_t clamp01_x, void *workspace, float *out_ms, float *out_levels, float *out_sse, void *stream) {
    const Operands o{x, y, N, C, H, W, x_row_stride, y_row_stride, x_plane_stride, y_plane_stride, data_range, clamp01_x != 0};
    if (!operands_ok(o, workspace) || !out_ms) return DCVC_E_ARG;
    const Plan p = make_plan(N, C, H, W, false);
    return run_forward(o, p, (float *)workspace, make_window(), out_ms, out_levels, out_sse, nullptr, (hipStream_t)stream);
}

int dcvc_ms_ssim_grad(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t x_row_stride,
                      int64_t x_plane_stride, int32_t y_row_stride, int64_t y_plane_stride, float data_range,
                      int32_t clamp01_x, void *workspace, const float *g_ms, float *gx, void *stream) {
    const Operands o{x, y, N, C, H, W, x_row_stride, y_row_stride, x_plane_stride, y_plane_stride, data_range, 0};
    if (!operands_ok(o, workspace) || !g_ms || !gx || clamp01_x) return DCVC_E_ARG;
    const Plan p = make_plan(N, C, H, W, true);
    float *ws = (float *)workspace;
    const Window w = make_window();
    hipStream_t st = (hipStream_t)stream;
    const int rc = run_forward(o, p, ws, w, nullptr, nullptr, nullptr, g_ms, st);
    if (rc != DCVC_OK) return rc;
    const int planes = N * C;
    const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
    for (int l = LEVELS - 1; l >= 0; --l) {  // coarse to fine: a level's gradient needs the pooled one below it
        LevelArgs a{};
        a.x = l ? ws + p.px[l] : x;
        a.y = l ? ws + p.py[l] : y;
        a.x_rs = l ? p.W[l] : x_row_stride;
        a.y_rs = l ? p.W[l] : y_row_stride;
        a.x_ps = l ? (int64_t)p.H[l] * p.W[l] : x_plane_stride;
        a.y_ps = l ? (int64_t)p.H[l] * p.W[l] : y_plane_stride;
        a.H = p.H[l];
        a.W = p.W[l];
        a.C1 = C1;
        a.C2 = C2;
        a.coef = ws + p.coef + (int64_t)l * planes;
        a.maps = ws + p.maps;
        a.last = l == LEVELS - 1;
        a.planes = planes;
        a.w = w;
        hipLaunchKernelGGL(level_kernel<1>, dim3(p.tx[l], p.ty[l], planes), dim3(THREADS), 0, st, a);
        GradArgs g{};
        g.maps = a.maps;
        g.x = a.x, g.y = a.y, g.x_ps = a.x_ps, g.y_ps = a.y_ps, g.x_rs = a.x_rs, g.y_rs = a.y_rs;
        g.H = a.H, g.W = a.W, g.planes = planes;
        g.coarse = a.last ? nullptr : ws + p.g[l + 1];
        g.Hc = a.last ? 0 : p.H[l + 1];
        g.Wc = a.last ? 0 : p.W[l + 1];
        g.py = p.H[l] % 2, g.px = p.W[l] % 2;
        g.gx = l ? ws + p.g[l] : gx;
        g.w = w;
        hipLaunchKernelGGL(gradT_kernel, dim3((g.W + TILE - 1) / TILE, (g.H + TILE - 1) / TILE, planes), dim3(THREADS), 0, st, g);
    }
    RET_LAUNCH();
}

}  // extern "C"
