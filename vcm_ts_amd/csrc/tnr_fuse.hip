// tnr_fuse.hip -- the temporal noise prefilter on an I picture: one pass that blends a picture with up to four references
// (include/dcvc_hip_tnr_fuse.h, which states the arithmetic; this file only arranges it).
//
// tnr_fuse_kernel<N> takes tnr_step_kernel's geometry (csrc/tnr.hip): a WORKGROUP of 8 waves owns a strip of 16 rows x 256
// columns, so it alone writes the strip's sad / held and nothing global is atomic; a WAVE takes 2 consecutive rows, a lane
// 4 consecutive pixels of each.  Lane bits: 0-1 the quad inside the cell, 2-5 the cell.  The halo is shared out as there:
// the two rows above and the two below are one more quad for the lanes of waves 0-3, the 20 x 4 pixels left and right one
// pixel for 80 lanes of waves 4-5; every coordinate is clamped to the picture BEFORE the load.
//
// cur is read ONCE: the lane keeps its 2 x 4 pixels' three floats for the blend and, of everything it loaded of cur, the
// luma codes packed four to a word (two words of its own pixels, one of its halo share).  Every reference has an LDS tile
// of its own, so the workgroup moves through three phases with two barriers whatever N is: every load of every reference
// and d_j as bytes into tile j (20 rows x 264); the 5-tap horizontal sums of the 20 rows of every tile as uint16; five of
// them summed vertically per pixel, the weight, and u_j = 256 - w_j kept as a byte per pixel (two words per reference),
// then the blend in increasing j.
//
// The blend needs every reference's 2 x 4 x 3 floats again.  KEEP = true holds all N in registers from the first load,
// 24 N + 24 floats per lane (212 VGPRs at N = 4: one workgroup per CU); KEEP = false reads them a second time (a hit in
// L2, the strip was loaded moments ago).  FUSE_KEEP below is the one built: keeping is faster by x0.74 .. x0.82 at every
// N, from cache and from HBM (DESIGN.md 4y has the two side by side).
//
// LDS: N x (5280 (d) + 10240 (horizontal sums)) + 512 (wtab) + 4084 (rtab) + 1024 (the cells' partial sums) = 21152 bytes
// at N = 1, 67712 at N = 4.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcvc_hip.h"
#include "dcvc_hip_tnr_fuse.h"
#include "kernel_common.h"
#include "roi_common.h"

#pragma clang fp contract(off)

#ifndef FUSE_KEEP
#define FUSE_KEEP 1
#endif

namespace {

constexpr int CELL = DCVC_ROI_CELL, TILE_CELLS = 16, TILE_W = CELL * TILE_CELLS, WAVES = 8, ROWS = 2, HALO = DCVC_TNR_WINDOW / 2;
constexpr int D_ROWS = CELL + 2 * HALO, D_WORDS = TILE_W / 4 + 2, SIDE = 2 * HALO * D_ROWS, MAX_REFS = DCVC_TNR_FUSE_MAX_REFS;
static_assert(CELL == 16 && TILE_W == 64 * 4 && ROWS * WAVES == CELL && HALO == 2, "a lane per quad, a wave per two rows");
static_assert(2 * HALO <= WAVES / 2 && SIDE <= 64 * WAVES / 2, "the halo rows go to waves 0-3, the halo columns to waves 4-7");
static_assert(DCVC_TNR_FUSE_RCP <= 2 * 64 * WAVES, "rtab is staged in two rounds");

struct FuseArgs {
    const float *cur, *ref[MAX_REFS];
    float *out;
    const uint16_t *wtab;
    const float *rtab;
    uint32_t *sad;
    uint16_t *held;
    int64_t cps, rps, ops;
    int32_t crs, rrs, ors, H, W, wc, P, cvec, rvec[MAX_REFS], ovec;
};

// the quad at columns x0 .. x0 + 3 of a row, every column clamped to the picture's last one
__device__ __forceinline__ void load_quad(const float *row, int x0, int W, bool vec, float (&f)[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(row + x0);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] = row[min(x0 + q, W - 1)];
    }
}

// the luma codes of a quad, a byte each
__device__ __forceinline__ unsigned quad_luma(const float (&c)[3][4]) {
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) word |= (unsigned)luma8(code8(c[0][q]), code8(c[1][q]), code8(c[2][q])) << (8 * q);
    return word;
}

// |a - b| byte by byte
__device__ __forceinline__ unsigned quad_diffs(unsigned a, unsigned b) {
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) word |= (unsigned)abs((int)((a >> (8 * q)) & 255) - (int)((b >> (8 * q)) & 255)) << (8 * q);
    return word;
}

template <int N, bool KEEP>
__global__ __launch_bounds__(64 * WAVES) void tnr_fuse_kernel(const FuseArgs p) {
    __shared__ unsigned D[N][D_ROWS][D_WORDS];        // d_j, a byte per pixel: row = strip row + 2, byte = strip column + 4
    __shared__ uint2 HS[N][D_ROWS][TILE_W / 4];       // the horizontal 5-tap sums of d_j, four uint16 per quad
    __shared__ uint16_t tab[256];
    __shared__ float rcp[DCVC_TNR_FUSE_RCP];
    __shared__ unsigned part[2][WAVES][TILE_CELLS];   // sad and held of each cell in each wave's two rows
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * CELL, x0 = X0 + lane * 4, y0 = Y0 + wave * ROWS;
    const int col = blockIdx.x * TILE_CELLS + lane;
    const bool writer = wave == 0 && lane < TILE_CELLS && col < p.wc;
    if (X0 >= p.W || Y0 >= p.H) {  // (uniform across the workgroup) a strip of the padding: its cells hold no pixel
        if (writer) p.sad[(int64_t)blockIdx.y * p.wc + col] = 0, p.held[(int64_t)blockIdx.y * p.wc + col] = 0;
        return;
    }
    const bool whole = x0 + 4 <= p.W, cv = p.cvec && whole;

    // ---- where the lane's share of the halo lies (the same pixels of cur and of every reference)
    const int side = (wave - WAVES / 2) * 64 + lane;  // waves 4-7: which of the 80 pixels left and right of the strip
    const bool halo_row = wave < 2 * HALO, halo_px = !halo_row && side >= 0 && side < SIDE;  // (uniform across a wave; per lane)
    int hrow = 0, hbyte = 0, hy = 0, hx = 0;
    if (halo_row) {  // strip rows -2, -1, 16, 17 at the lane's own columns
        const int rel = wave < HALO ? wave - HALO : CELL + wave - HALO;
        hy = min(max(Y0 + rel, 0), p.H - 1), hrow = rel + HALO;
    } else if (halo_px) {  // strip columns -2, -1, 256, 257 of all 20 rows
        const int rel = side / (2 * HALO) - HALO, k4 = side % (2 * HALO), relx = k4 < HALO ? k4 - HALO : TILE_W + k4 - HALO;
        hy = min(max(Y0 + rel, 0), p.H - 1), hx = min(max(X0 + relx, 0), p.W - 1);
        hrow = rel + HALO, hbyte = relx + 4;
    }
    int yrow[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) yrow[i] = min(y0 + i, p.H - 1);

    // ---- cur, once: the floats of the lane's own pixels and the luma of everything
    float c[ROWS][3][4];
    unsigned ycur[ROWS], yhalo = 0;
    {
        float h[3][4] = {};
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) load_quad(p.cur + k * p.cps + (int64_t)yrow[i] * p.crs, x0, p.W, cv, c[i][k]);
        if (halo_row) {
#pragma unroll
            for (int k = 0; k < 3; ++k) load_quad(p.cur + k * p.cps + (int64_t)hy * p.crs, x0, p.W, cv, h[k]);
        } else if (halo_px) {
#pragma unroll
            for (int k = 0; k < 3; ++k) h[k][0] = p.cur[k * p.cps + (int64_t)hy * p.crs + hx];
        }
        for (int e = wave * 64 + lane; e < DCVC_TNR_FUSE_RCP; e += 64 * WAVES) rcp[e] = p.rtab[e];
        if (wave * 64 + lane < 256) tab[wave * 64 + lane] = p.wtab[wave * 64 + lane];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) ycur[i] = quad_luma(c[i]);
        yhalo = quad_luma(h);
    }

    // ---- every load of the lane from every reference, then d_j into reference j's tile
    float kept[KEEP ? N : 1][ROWS][3][4];
    unsigned own[N][ROWS];  // d_j of the lane's 2 x 4 pixels, a byte each
    {
        float once[KEEP ? 1 : N][ROWS][3][4], h[N][3][4] = {};
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float *ref = p.ref[j];
            const bool rv = p.rvec[j] && whole;
            float(&r)[ROWS][3][4] = KEEP ? kept[KEEP ? j : 0] : once[KEEP ? 0 : j];
#pragma unroll
            for (int i = 0; i < ROWS; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) load_quad(ref + k * p.rps + (int64_t)yrow[i] * p.rrs, x0, p.W, rv, r[i][k]);
            if (halo_row) {
#pragma unroll
                for (int k = 0; k < 3; ++k) load_quad(ref + k * p.rps + (int64_t)hy * p.rrs, x0, p.W, rv, h[j][k]);
            } else if (halo_px) {
#pragma unroll
                for (int k = 0; k < 3; ++k) h[j][k][0] = ref[k * p.rps + (int64_t)hy * p.rrs + hx];
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float(&r)[ROWS][3][4] = KEEP ? kept[KEEP ? j : 0] : once[KEEP ? 0 : j];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                own[j][i] = quad_diffs(ycur[i], quad_luma(r[i]));
                D[j][wave * ROWS + i + HALO][1 + lane] = own[j][i];
            }
            const unsigned dh = quad_diffs(yhalo, quad_luma(h[j]));
            if (halo_row)
                D[j][hrow][1 + lane] = dh;
            else if (halo_px)
                reinterpret_cast<uint8_t *>(D[j][hrow])[hbyte] = (uint8_t)(dh & 255);
        }
    }
    __syncthreads();

    // ---- horizontal: the quad at strip columns 4 l .. 4 l + 3 needs bytes 4 l + 2 .. 4 l + 9 of its row
#pragma unroll
    for (int j = 0; j < N; ++j)
        for (int row = wave; row < D_ROWS; row += WAVES) {  // (uniform across a wave)
            const unsigned w0 = D[j][row][lane], w1 = D[j][row][lane + 1], w2 = D[j][row][lane + 2];
            const unsigned b2 = (w0 >> 16) & 255, b3 = w0 >> 24, b4 = w1 & 255, b5 = (w1 >> 8) & 255, b6 = (w1 >> 16) & 255,
                           b7 = w1 >> 24, b8 = w2 & 255, b9 = (w2 >> 8) & 255;
            const unsigned mid = b4 + b5 + b6, s0 = b2 + b3 + mid, s1 = b3 + mid + b7, s2 = mid + b7 + b8, s3 = b5 + b6 + b7 + b8 + b9;
            HS[j][row][lane] = make_uint2(s0 | s1 << 16, s2 | s3 << 16);
        }
    __syncthreads();

    // ---- vertical and the weight
    unsigned u[N][ROWS];  // 256 - w_j of the lane's 2 x 4 pixels, a byte each
    unsigned sad = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            unsigned S[4] = {0, 0, 0, 0}, word = 0;
#pragma unroll
            for (int v = 0; v < DCVC_TNR_WINDOW; ++v) {
                const uint2 t = HS[j][wave * ROWS + i + v][lane];
                S[0] += t.x & 0xffff, S[1] += t.x >> 16, S[2] += t.y & 0xffff, S[3] += t.y >> 16;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned d = (own[j][i] >> (8 * q)) & 255;
                const unsigned w = d > (unsigned)p.P ? 256u : tab[S[q] / 25];
                word |= (256u - w) << (8 * q);
                if (j == 0) sad += (y0 + i < p.H && x0 + q < p.W) ? d : 0u;
            }
            u[j][i] = word;
        }

    // ---- the blend
    const bool ov = p.ovec && whole;
    unsigned held = 0;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        if (y0 + i >= p.H) break;  // (uniform across a wave; no barrier lies inside the loop)
        float acc[3][4] = {};
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float once[3][4];
            if (!KEEP) {
                const bool rv = p.rvec[j] && whole;
#pragma unroll
                for (int k = 0; k < 3; ++k) load_quad(p.ref[j] + k * p.rps + (int64_t)(y0 + i) * p.rrs, x0, p.W, rv, once[k]);
            }
            float(&r)[3][4] = KEEP ? kept[KEEP ? j : 0][i] : once;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned uj = (u[j][i] >> (8 * q)) & 255;
                const float uf = (float)uj;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float t = (r[k][q] - c[i][k][q]) * uf;
                    acc[k][q] = uj > 0 ? acc[k][q] + t : acc[k][q];
                }
            }
        }
        float o[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned U = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) U += (u[j][i] >> (8 * q)) & 255;
            held += (x0 + q < p.W && U > 0) ? 1u : 0u;
            const float rU = rcp[U];
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k][q] = U == 0 ? c[i][k][q] : c[i][k][q] + acc[k][q] * rU;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float *row = p.out + k * p.ops + (int64_t)(y0 + i) * p.ors + x0;
            if (ov) {
                *reinterpret_cast<float4 *>(row) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < p.W) row[q] = o[k][q];
            }
        }
    }
    sad += (unsigned)__shfl_xor((int)sad, 1), held += (unsigned)__shfl_xor((int)held, 1);
    sad += (unsigned)__shfl_xor((int)sad, 2), held += (unsigned)__shfl_xor((int)held, 2);
    if ((lane & 3) == 0) part[0][wave][lane >> 2] = sad, part[1][wave][lane >> 2] = held;
    __syncthreads();
    if (writer) {
        unsigned s = 0, h = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) s += part[0][v][lane], h += part[1][v][lane];
        p.sad[(int64_t)blockIdx.y * p.wc + col] = s;
        p.held[(int64_t)blockIdx.y * p.wc + col] = (uint16_t)h;
    }
}

}  // namespace

extern "C" int dcvc_tnr_fuse(const float *cur, int32_t cur_rs, int64_t cur_ps, const float *ref0, const float *ref1, const float *ref2,
                             const float *ref3, int32_t ref_rs, int64_t ref_ps, int32_t n, float *out, int32_t out_rs, int64_t out_ps,
                             int32_t H, int32_t W, const uint16_t *wtab, const float *rtab, int32_t P, uint32_t *sad, uint16_t *held,
                             void *stream) {
    const float *refs[MAX_REFS] = {ref0, ref1, ref2, ref3};
    if (!wtab || !rtab || !sad || !held || n < 1 || n > MAX_REFS || !size_ok(H, W) || !planes_ok(cur, cur_rs, cur_ps, H, W) ||
        !planes_ok(out, out_rs, out_ps, H, W) || P < 0 || P > DCVC_TNR_MAX_P || !aligned(cur, 4) || !aligned(out, 4) ||
        !aligned(sad, 4) || !aligned(rtab, 4) || !aligned(wtab, 2) || !aligned(held, 2) ||
        extents_overlap(out, out_rs, out_ps, cur, cur_rs, cur_ps, H, W))
        return DCVC_E_ARG;
    for (int j = 0; j < n; ++j)
        if (!planes_ok(refs[j], ref_rs, ref_ps, H, W) || !aligned(refs[j], 4) ||
            extents_overlap(out, out_rs, out_ps, refs[j], ref_rs, ref_ps, H, W))
            return DCVC_E_ARG;
    FuseArgs a{};
    a.cur = cur, a.out = out, a.wtab = wtab, a.rtab = rtab, a.sad = sad, a.held = held;
    a.cps = cur_ps, a.rps = ref_ps, a.ops = out_ps, a.crs = cur_rs, a.rrs = ref_rs, a.ors = out_rs, a.H = H, a.W = W;
    a.wc = 4 * ((W + 63) / 64), a.P = P;
    a.cvec = vec_ok(cur, cur_rs, cur_ps), a.ovec = vec_ok(out, out_rs, out_ps);
    for (int j = 0; j < n; ++j) a.ref[j] = refs[j], a.rvec[j] = vec_ok(refs[j], ref_rs, ref_ps);
    const dim3 block(64, WAVES), grid(nblk(a.wc, TILE_CELLS), 4 * ((H + 63) / 64));
    constexpr bool KEEP = FUSE_KEEP != 0;
    const hipStream_t s = (hipStream_t)stream;
    switch (n) {
    case 1: tnr_fuse_kernel<1, KEEP><<<grid, block, 0, s>>>(a); break;
    case 2: tnr_fuse_kernel<2, KEEP><<<grid, block, 0, s>>>(a); break;
    case 3: tnr_fuse_kernel<3, KEEP><<<grid, block, 0, s>>>(a); break;
    default: tnr_fuse_kernel<4, KEEP><<<grid, block, 0, s>>>(a); break;
    }
    RET_LAUNCH();
}
