"""A numpy / Python-int restatement of include/dcvc_hip_grain.h and of grain.params / grain.table, written from their text
(not from the kernels or the module): the sums of the measurement, the counter-hashed white field, the 3-tap shape, the
scale and the float32 add operation by operation -- and the held arrays, tables and pictures the grain tests share.
Integer work is int64 (the hash: uint64 masked to 32 bits)."""
import math

import numpy as np

from tests import tnr_ref as T
from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as G.luma, ...)

F32 = np.float32
CELL, BINS, WORDS, MAX_TAP, CENTRE, SHIFT, WHITE_VAR = 16, 8, 32, 24, 64, 24, 43690
SIZES = T.SIZES
TAPS = [(0, 0), (24, -24), (-24, 24), (7, 3)]
TIMES = [0, 1, 2 ** 31 - 1]
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------- measure
def full_counts(H, W):
    """(hc, wc) int64: the number of a cell's pixels inside the picture."""
    return T.cell_sums(np.ones((H, W), dtype=np.int64))


def measure(src, flt, held, acc=None):
    """acc (32 int64) after one dcvc_grain_measure: held is the (hc, wc) array of the filter's cells."""
    H, W = src.shape[1:]
    acc = np.zeros(WORDS, dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64)
    ys, yf = luma(src), luma(flt)
    e, b = ys - yf, yf >> 5
    want = full_counts(H, W)
    takes = (np.asarray(held, dtype=np.int64).reshape(want.shape) == want) & (want > 0)
    part = np.repeat(np.repeat(takes, CELL, axis=0), CELL, axis=1)[:H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    right = np.zeros((H, W), dtype=np.int64)
    right[:, :-1] = e[:, :-1] * e[:, 1:]
    right[(xx + 1) % CELL == 0] = 0  # (the partner is in the next cell; the picture's last column has none)
    below = np.zeros((H, W), dtype=np.int64)
    below[:-1] = e[:-1] * e[1:]
    below[(yy + 1) % CELL == 0] = 0
    for k, v in enumerate((np.ones((H, W), dtype=np.int64), e * e, right, below)):
        for n in range(BINS):
            acc[4 * n + k] += int(v[part & (b == n)].sum())
    return acc


def held_cases(H, W):
    """name -> (hc, wc) host-written held arrays: every cell full; none full (one short everywhere, and zero where that
    is negative); a checkerboard of full cells; all full but the last cell that holds a pixel, which is one short."""
    full = full_counts(H, W)
    ii, jj = np.mgrid[0:full.shape[0], 0:full.shape[1]]
    edge = full.copy()
    edge[(H - 1) // CELL, (W - 1) // CELL] -= 1
    return {"full": full, "none": np.maximum(full - 1, 0) * (full > 1), "checker": np.where((ii + jj) % 2 == 0, full, 0), "edge": edge}


# --------------------------------------------------------------------------------------------------------------- apply
def fmix(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def byte_sum(w):
    return ((w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + (w >> 24)).astype(np.int64)


def white(t, H, W):
    """g on y = -1 .. H, x = -1 .. W: (H + 2, W + 2) int64, element [y + 1, x + 1]."""
    key = fmix(np.uint64(t) ^ np.uint64(0x9E3779B9))
    yy, xx = np.mgrid[0:H + 2, 0:W + 2].astype(np.uint64)
    w0 = fmix(((yy << 16) | xx) ^ key)
    w1 = fmix(w0 ^ np.uint64(0x9E3779B9))
    return byte_sum(w0) + byte_sum(w1) - 1020


def shaped(g, kh, kv):
    """n on the picture from g on the picture and its ring."""
    H, W = g.shape[0] - 2, g.shape[1] - 2
    th, tv = (kh, CENTRE, kh), (kv, CENTRE, kv)
    return sum(tv[dy] * th[dx] * g[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def apply(pic, t, kh, kv, stab):
    """out (3, H, W) float32 of one dcvc_grain_apply."""
    pic = np.asarray(pic, dtype=F32)
    H, W = pic.shape[1:]
    n = shaped(white(t, H, W), kh, kv)
    s = np.asarray(stab, dtype=np.int64)[luma(pic)]
    D = (n * s + (1 << (SHIFT - 1))) >> SHIFT  # (numpy's >> on int64 is arithmetic)
    assert np.abs(n).max() < 2 ** 24 and np.abs(D).max() <= 49980
    d = D.astype(F32) * (F32(1.0) / F32(4080.0))
    v = pic + d[None]
    assert d.dtype == F32 and v.dtype == F32
    with np.errstate(invalid="ignore"):
        v = np.fmin(np.fmax(v, F32(0.0)), F32(1.0))  # (fmaxf / fminf: the other operand for a NaN)
    return np.where((s == 0)[None], pic, v)


# ---------------------------------------------------------------------------------------------------------- the record
def tap(cross, square):
    """The k in -24 .. 24 whose 128 k / (4096 + 2 k^2) is nearest cross / square (exact fractions); ties to the smaller |k|."""
    from fractions import Fraction

    if square <= 0:
        return 0
    return min(range(-MAX_TAP, MAX_TAP + 1),
               key=lambda k: (abs(Fraction(cross, square) - Fraction(2 * CENTRE * k, CENTRE * CENTRE + 2 * k * k)), abs(k), k))


def params(acc, min_samples):
    acc = [int(v) for v in acc]
    counts = [acc[4 * b] for b in range(BINS)]
    good = [b for b in range(BINS) if counts[b] >= min_samples and counts[b] > 0]
    if not good:
        return {"points": [0] * BINS, "kh": 0, "kv": 0, "counts": counts}
    points = []
    for b in range(BINS):
        n = min(good, key=lambda m: (abs(m - b), m))
        points.append(math.isqrt(256 * acc[4 * n + 1] // counts[n]))
    sq = sum(acc[4 * b + 1] for b in good)
    return {"points": points, "kh": tap(sum(acc[4 * b + 2] for b in good), sq), "kv": tap(sum(acc[4 * b + 3] for b in good), sq),
            "counts": counts}


def table(points, kh, kv, percent=100):
    den = 32 * 100 * math.isqrt(WHITE_VAR * (CENTRE ** 2 + 2 * kh * kh) * (CENTRE ** 2 + 2 * kv * kv))
    out = []
    for y in range(256):
        if y <= 16:
            s32 = 32 * points[0]
        elif y >= 240:
            s32 = 32 * points[7]
        else:
            b, f = (y - 16) // 32, (y - 16) % 32
            s32 = points[b] * (32 - f) + points[b + 1] * f
        out.append(min(65535, (s32 * percent * 2 ** SHIFT + den // 2) // den))
    return np.array(out, dtype=np.uint16)


def record(pics, tnr, intra, min_samples):
    """{first picture of a GOP: params} of a stream coded with the filter tnr = (T, floor, P), and the filtered pictures."""
    run, gops, acc, first = T.run(pics, tnr, intra), {}, None, None
    for t in range(len(pics)):
        if t in intra:
            if first is not None:
                gops[first] = params(acc, min_samples)
            first, acc = t, np.zeros(WORDS, dtype=np.int64)
        else:
            acc = measure(np.asarray(pics[t], dtype=F32), run[t][0], run[t][2], acc)
    gops[first] = params(acc, min_samples)
    return gops, run


def grained(pics, gops, intra, percent=100):
    """What GrainSynth shows of the pictures `pics` (a list of (3, H, W) float32), by the record `gops`."""
    out, first = [], None
    for t, pic in enumerate(pics):
        if t in intra:
            first = t
            out.append(np.asarray(pic, dtype=F32))
            continue
        rec = gops[first]
        tab = table(rec["points"], rec["kh"], rec["kv"], percent)
        out.append(apply(pic, t, rec["kh"], rec["kv"], tab) if tab.any() else np.asarray(pic, dtype=F32))
    return out


# ------------------------------------------------------------------------------------------------------------ pictures
def ramp(H, W):
    """A grey picture whose luma visits every code 0 .. 255 that H * W pixels allow, in order."""
    v = (np.arange(H * W, dtype=np.int64) * 255 // max(H * W - 1, 1)) if H * W >= 256 else np.arange(H * W, dtype=np.int64) * (255 // max(H * W - 1, 1))
    pic = np.broadcast_to((v.reshape(H, W).astype(F32) / F32(255.0)).astype(F32), (3, H, W)).copy()
    assert np.array_equal(luma(pic), v.reshape(H, W))
    return pic


def stabs():
    """name -> 256 uint16: a table that rises with the code, the maximum everywhere, zero everywhere, zero at even codes."""
    y = np.arange(256, dtype=np.int64)
    return {"rising": (40 + 9 * y).astype(np.uint16), "max": np.full(256, 65535, np.uint16), "zero": np.zeros(256, np.uint16),
            "even-zero": np.where(y % 2 == 0, 0, 3000 + 100 * y).astype(np.uint16)}
