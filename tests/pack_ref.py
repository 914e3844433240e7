"""numpy restatement of the four host weight packings of include/dcvc_hip.h and of their bias packing, written from the
layout comments of the headers and kernels (conv_mfma.hip, conv_k32.hip, conv_small.hip).  It never calls the library:
tests/test_pack_host.py compares the library's bytes with these.

All packers take w as nn.Conv2d stores it, (Cout, Cin, ks, ks) fp32, and walk the input channels segment by segment
(the channel order of the torch.cat a layer replaces).  Split-fp16 form of a weight: sv = 64 w clamped to +-65504,
hi = fp16(sv), lo = fp16(sv - hi).  Every function returns (wpack, bpack, status) with wpack as the raw buffer in its
natural element type (float32 for the fp32 layout, float16 otherwise)."""
import numpy as np

OK, E_ARG, E_RANGE = 0, -1, -3
FP32, FP16X3 = 0, 1
WGT_SCALE = np.float32(64.0)
F16_MAX = np.float32(65504.0)


def round_up(v, m):
    return (v + m - 1) // m * m


def clamp_silent(sv):
    """The plain packer: out-of-range values are clamped without a word, a NaN stays a NaN."""
    return np.where(sv > F16_MAX, F16_MAX, np.where(sv < -F16_MAX, -F16_MAX, sv)).astype(np.float32)


def clamp_report(sv):
    """The other three: anything that is not |sv| <= 65504 (a NaN included) is reported and becomes +-65504, a NaN
    -65504.  Returns (clamped values, whether any was)."""
    bad = ~(np.abs(sv) <= F16_MAX)
    return np.where(bad, np.where(sv > 0, F16_MAX, -F16_MAX), sv).astype(np.float32), bool(bad.any())


def split(sv):
    with np.errstate(invalid="ignore"):
        hi = sv.astype(np.float16)
        lo = (sv - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def shuffled(n, Cout, pixel_shuffle):
    """Packed position of output channel n: with PixelShuffle(2) the four sub-pixel planes are contiguous ranges."""
    return (n % 4) * (Cout // 4) + n // 4 if pixel_shuffle else n


def chunks_of(seg_C, kc):
    """(chunk index, first source channel, channels in the chunk) of every K chunk; a chunk never straddles a segment."""
    out, cin0 = [], 0
    for C in seg_C:
        for c0 in range(0, C, kc):
            out.append((len(out), cin0 + c0, min(kc, C - c0)))
        cin0 += C
    return out


def bias(b, Cout, length, pixel_shuffle=0):
    bp = np.zeros(length, np.float32)
    if b is not None:
        for n in range(Cout):
            bp[shuffled(n, Cout, pixel_shuffle)] = b[n]
    return bp


def plain_size(Cout, ks, seg_C):
    cp = round_up(Cout, 32)
    return len(chunks_of(seg_C, 16)) * ks * ks * 4 * cp * 4, cp


def plain(w, b, seg_C, pixel_shuffle, precision):
    """dcvc_conv_pack_weights.  fp32: wpack[chunk][tap][kq][n'][j] = w[n][16 chunk + 4 kq + j][tap].
    fp16x3: rows [chunk][tap][hi h0, hi h1, lo h0, lo h1][n'][8 fp16], channel 16 chunk + 8 h + jj."""
    Cout, Cin, ks = w.shape[0], w.shape[1], w.shape[2]
    T = ks * ks
    total, cp = plain_size(Cout, ks, seg_C)
    wf = w.reshape(Cout, Cin, T)
    pos = [shuffled(n, Cout, pixel_shuffle) for n in range(Cout)]
    if precision == FP32:
        out = np.zeros((total // (T * 4 * cp * 4), T, 4, cp, 4), np.float32)
        for cg, cin, cn in chunks_of(seg_C, 16):
            for c in range(cn):
                out[cg, :, c // 4, pos, c % 4] = wf[:, cin + c, :]
    else:
        hi, lo = split(clamp_silent(wf * WGT_SCALE))
        out = np.zeros((total // (T * 4 * cp * 4), T, 4, cp, 8), np.float16)
        for cg, cin, cn in chunks_of(seg_C, 16):
            for c in range(cn):
                out[cg, :, c // 8, pos, c % 8] = hi[:, cin + c, :]
                out[cg, :, 2 + c // 8, pos, c % 8] = lo[:, cin + c, :]
    return out.reshape(-1), bias(b, Cout, cp, pixel_shuffle), OK


def paired_size(Cout):
    cp = round_up(Cout, 32)
    return 7 * 4 * 4 * cp * 4, cp


def paired(w, b):
    """dcvc_conv_pack_weights_paired (7x7, Cin <= 8): K step (ky, j) holds tap (ky, 2j) in channel half 0 and tap
    (ky, 2j + 1) in half 1 -- nothing for kx = 7.  Rows [ky * 4 + j][hi h0, hi h1, lo h0, lo h1][n][8 fp16]."""
    Cout, Cin = w.shape[0], w.shape[1]
    cp = paired_size(Cout)[1]
    sv, clamped = clamp_report(w * WGT_SCALE)
    hi, lo = split(sv)
    out = np.zeros((7, 4, 4, cp, 8), np.float16)
    for kx in range(7):
        out[:, kx // 2, kx % 2, :Cout, :Cin] = hi[:, :, :, kx].transpose(2, 0, 1)
        out[:, kx // 2, 2 + kx % 2, :Cout, :Cin] = lo[:, :, :, kx].transpose(2, 0, 1)
    return out.reshape(-1), bias(b, Cout, cp), E_RANGE if clamped else OK


def small_size(ks, seg_C):
    return len(chunks_of(seg_C, 16)) * ks * ks * 1024


def small(w, b, seg_C):
    """dcvc_conv_small_pack_weights (Cout <= 16): [chunk][tap][hi k0-7, hi k8-15, lo k0-7, lo k8-15][16 channels][8 fp16];
    bpack is 16 floats."""
    Cout, Cin, ks = w.shape[0], w.shape[1], w.shape[2]
    T = ks * ks
    sv, clamped = clamp_report(w.reshape(Cout, Cin, T) * WGT_SCALE)
    hi, lo = split(sv)
    out = np.zeros((small_size(ks, seg_C) // (T * 1024), T, 4, 16, 8), np.float16)
    for cg, cin, cn in chunks_of(seg_C, 16):
        for c in range(cn):
            out[cg, :, c // 8, :Cout, c % 8] = hi[:, cin + c, :].T
            out[cg, :, 2 + c // 8, :Cout, c % 8] = lo[:, cin + c, :].T
    return out.reshape(-1), bias(b, Cout, 16), E_RANGE if clamped else OK


def k32_size(Cout, ks, seg_C):
    cp = round_up(Cout, 32)
    return len(chunks_of(seg_C, 32)) * ks * ks * 8 * cp * 16, cp


def k32(w, b, seg_C, pixel_shuffle):
    """dcvc_conv_k32_pack_weights (segments are multiples of 32): 16-byte entries
    [chunk][tap][hi, lo][kq 0..3][n'] = 8 fp16 of channels 32 chunk + 8 kq + j."""
    Cout, Cin, ks = w.shape[0], w.shape[1], w.shape[2]
    T = ks * ks
    nbytes, cp = k32_size(Cout, ks, seg_C)
    sv, clamped = clamp_report(w.reshape(Cout, Cin, T) * WGT_SCALE)
    hi, lo = split(sv)
    pos = [shuffled(n, Cout, pixel_shuffle) for n in range(Cout)]
    out = np.zeros((nbytes // (T * 8 * cp * 16), T, 2, 4, cp, 8), np.float16)
    for c in range(Cin):
        out[c // 32, :, 0, (c % 32) // 8, pos, c % 8] = hi[:, c, :]
        out[c // 32, :, 1, (c % 32) // 8, pos, c % 8] = lo[:, c, :]
    return out.reshape(-1), bias(b, Cout, cp, pixel_shuffle), E_RANGE if clamped else OK
