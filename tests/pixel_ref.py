"""The arithmetic that every picture kernel shares (vcm_ts_amd/csrc/roi_common.h: code8, luma8, the cell grid), restated
once in numpy.  The *_ref.py restatements import it and re-export the names their tests use."""
import numpy as np

F32 = np.float32


def code(v):
    """(int) rint(255.0f * clamp01(v)): one float32 multiply, round-half-to-even; clamp01 = fminf(fmaxf(v, 0), 1), so a
    NaN codes as 0.  int64."""
    v = np.asarray(v, dtype=F32)
    c = np.minimum(np.maximum(np.where(np.isnan(v), F32(0), v), F32(0)), F32(1))
    return np.rint(F32(255.0) * c).astype(np.int64)


def luma_of_codes(r, g, b):
    """Y of three planes of 8-bit codes."""
    return (54 * r + 183 * g + 19 * b + 128) >> 8


def luma(pic):
    """Y of a (3, H, W) float32 picture, int64."""
    return luma_of_codes(code(pic[0]), code(pic[1]), code(pic[2]))


def grid(H, W):
    """(hc, wc): the 16 x 16 cells of the picture padded to multiples of 64."""
    return 4 * ((H + 63) // 64), 4 * ((W + 63) // 64)
