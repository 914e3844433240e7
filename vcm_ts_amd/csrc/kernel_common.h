// kernel_common.h -- what more than one translation unit of libdcvc_hip.so has to agree on, defined once: launch
// helpers, the split-fp16 number format, the packed-weight layout that conv_mfma.hip reads and that both its host packer
// and the device packer (backward.hip) write, and the entry-point code the three convolution kernels share.
// Internal: not installed, not part of the C ABI (include/*.h).  Every unit is compiled on its own and nothing here is
// exported, hence the unnamed namespace.
#ifndef DCVC_KERNEL_COMMON_H
#define DCVC_KERNEL_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcvc_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

namespace {

#define RET_LAUNCH() return hipGetLastError() == hipSuccess ? DCVC_OK : DCVC_E_LAUNCH
inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// a tensor whose rows can be addressed 16 bytes (4 channels) at a time; an absent one qualifies
inline bool aligned16(const void *p, int cs) { return p == nullptr || ((((uintptr_t)p) & 15) == 0 && (cs & 3) == 0); }

// ---- split-fp16 mode ("fp16x3", DCVC_PREC_FP16X3) ---------------------------------------------------------------------
// Every fp32 operand v is carried as hi = fp16(v * 2^s) and lo = fp16(v * 2^s - hi); x*w ~= xh*wh + xh*wl + xl*wh on the
// fp16 MFMAs with fp32 accumulation (products of fp16 are exact in fp32; the dropped xl*wl is <= 2^-22 |x w|).
// gfx950's MFMA honours fp16 subnormals (tools/probes/mfma_f16_subnormal.hip), so lo needs no separate scale:
// representation error <= max(2^-22 |v|, 2^-25 / 2^s).  The power-of-two pre-scales keep typical activations / weights in
// fp16's normal range and are undone exactly in the epilogue.
constexpr float ACT_SCALE = 8.f;   // activations: |x| < 8188 representable
constexpr float WGT_SCALE = 64.f;  // weights:     |w| < 1023 representable
constexpr float F16_MAX = 65504.f;
constexpr float ACT_LIMIT = F16_MAX / ACT_SCALE;  // an output beyond it would be clamped by a split-fp16 consumer

__device__ __forceinline__ float act(float v, float slope) { return v > 0.f ? v : v * slope; }

// the sum of v over the 64 lanes of a wave, in every lane (roi.hip, roil.hip, scene.hip, color.hip)
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
    return v;
}

// ---- CDF row of a scale ------------------------------------------------------------------------------------------------
// The number of bin edges <= s among edges[0 .. 254] (256 entries, the last one +inf and never read), by bisection; the
// dual-prior kernels (entropy_kernels.hip, where the edges are explained) and the ladder sweep (bitmap.hip) share it, so
// that a swept scale lands in the row the coder would use.  A NaN compares false everywhere -> 0.
__device__ __forceinline__ int32_t scale_index(float s, const float *edges) {
    int lo = 0;  // invariant: edges[0..lo) <= s
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1)
        if (edges[lo + step - 1] <= s) lo += step;
    return lo;
}

// ---- packed weights ---------------------------------------------------------------------------------------------------
// A weight enters a split-fp16 layout as sv = w * WGT_SCALE clamped to +-F16_MAX, then split_f16(sv).  The CLAMP is each
// packer's own line, because three policies exist on purpose:
//   dcvc_conv_pack_weights (host, also packs fp32)       clamps silently, a NaN stays a NaN
//   the paired, k32 and small host packers               return DCVC_E_RANGE with the clamped buffer; a NaN becomes -F16_MAX
//   pack_body (device, backward.hip)                     fminf / fmaxf, nothing reported: a kernel returns no status, and a
//                                                        device status word would cost every training step a read-back
struct SplitF16 {
    _Float16 hi, lo;
};
__host__ __device__ inline SplitF16 split_f16(float sv) {  // sv: already scaled and clamped
    const _Float16 hi = (_Float16)sv;
    return {hi, (_Float16)(sv - (float)hi)};
}

// nn.PixelShuffle(2) rides on the convolution's store: output channel n is packed at position
// n' = (n % 4) * (Cout / 4) + n / 4, so that the four sub-pixel planes are contiguous channel ranges
__host__ __device__ inline int ps_packed_channel(int n, int Cq) { return (n & 3) * Cq + (n >> 2); }
__host__ __device__ inline int ps_source_channel(int np, int Cq) { return (np % Cq) * 4 + np / Cq; }

// The layout conv_mfma.hip consumes: K chunks of MFMA_KC input channels (a chunk never straddles a segment), T taps per
// chunk, Cout padded to cp.  Channel cc = 4 kq + j = 8 h + jj of its chunk:
//   fp32 form    wpack[chunk][tap][kq][n'][j]                               as floats
//   fp16 form    rows [chunk][tap][hi h0, hi h1, lo h0, lo h1][n'][jj]      as fp16, 8 per (row, n')
// (h and jj are named before the sum on purpose: the device packer's code object is compared byte for byte across
// refactors, and the order of these operations is what the compiler's schedule follows)
constexpr int MFMA_KC = 16;
__host__ __device__ inline size_t mfma_wpack_f32(int cg, int T, int t, int cc, int cp, int np) {
    const int kq = cc >> 2, j = cc & 3;
    return ((((size_t)cg * T + t) * 4 + kq) * cp + np) * 4 + j;
}
__host__ __device__ inline size_t mfma_wpack_f16(int cg, int T, int t, int cc, int cp, int np, int lo) {
    const int h = cc >> 3, jj = cc & 7;
    return ((((size_t)cg * T + t) * 4 + 2 * lo + h) * cp + np) * 8 + jj;
}

// ---- entry points of the three convolution kernels ---------------------------------------------------------------------
// what dcvc_conv2d, dcvc_conv2d_k32 and dcvc_conv2d_small all demand: the pointers, positive sizes, and per input segment a 16-byte
// aligned base and a channel stride that is a multiple of 4 and covers the channels
inline bool conv_args_ok(const dcvc_conv_args *a) {
    if (!a || a->nseg < 1 || a->nseg > DCVC_MAX_SEG || !a->out || !a->wpack || !a->bpack) return false;
    if (a->N <= 0 || a->Hin <= 0 || a->Win <= 0 || a->Cout <= 0) return false;  // an empty grid is no launch
    for (int s = 0; s < a->nseg; ++s)
        if (!a->seg[s].ptr || (a->seg[s].cs & 3) || a->seg[s].cs < round_up(a->seg[s].C, 4) || ((uintptr_t)a->seg[s].ptr & 15))
            return false;
    return true;
}

// the 16-byte epilogue: every output / residual row is addressable in groups of 4 (final) channels
inline bool vec_epilogue_ok(const dcvc_conv_args *a) {
    const int cfin = a->pixel_shuffle ? a->Cout / 4 : a->Cout;
    return cfin % 4 == 0 && aligned16(a->out, a->out_cs) && aligned16(a->res, a->res_cs) && aligned16(a->res2, a->res2_cs) &&
           aligned16(a->res_gate, 0);
}

// dcvc_conv_args -> the members that ConvK, K32 and SmallK all have, matched by name (picture sizes are named per kernel)
template <class K>
inline void copy_conv_args(K &k, const dcvc_conv_args *a) {
    for (int s = 0; s < a->nseg; ++s) {
        k.seg_ptr[s] = a->seg[s].ptr;
        k.seg_C[s] = a->seg[s].C;
        k.seg_cs[s] = a->seg[s].cs;
    }
    k.nseg = a->nseg;
    k.in_act = a->in_act;
    k.in_slope = a->in_slope;
    k.wpack = (decltype(k.wpack))a->wpack;
    k.bpack = a->bpack;
    k.Cout = a->Cout;
    k.out = a->out;
    k.out_cs = a->out_cs;
    k.out_act = a->out_act;
    k.out_slope = a->out_slope;
    k.res = a->res;
    k.res_cs = a->res_cs;
    k.status = a->status;
}

// ... and those that only ConvK and K32 have: the full epilogue and banded launches
template <class K>
inline void copy_conv_args_full(K &k, const dcvc_conv_args *a) {
    copy_conv_args(k, a);
    k.Cout_pad = a->Cout_pad;
    k.ps = a->pixel_shuffle;
    k.res_gate = a->res_gate;
    k.res2 = a->res2;
    k.res2_cs = a->res2_cs;
    k.chan_partial = a->chan_partial;
    k.ty0 = a->tile_rows > 0 ? a->tile_row0 : 0;
    k.band_rows = a->tile_rows > 0 ? a->tile_rows : 0;
}

}  // namespace

#endif
