"""include/dcvc_hip_noise.h restated in numpy (luma, cell_words, hist_add), the estimator of vcm_ts_amd/noise.py restated
independently in a few lines (estimate, auto_threshold -- the module's own are imported by the tests only to be compared
with these), and the clip the tests measure: a smooth static coloured ground in luma 64 .. 190, a textured object that moves (3, 7)
pixels a picture, and independent Gaussian noise of `s` codes on each of R, G and B from a fixed seed, rounded to 8-bit
samples.  The luma noise of one picture is then sigma_Y = s sqrt(54^2 + 183^2 + 19^2) / 256 = 0.749 s, and the mean
absolute luma difference of two pictures sqrt(2) sigma_Y sqrt(2 / pi)."""
import math

import numpy as np

from tests.pixel_ref import code, grid, luma  # noqa: F401 (re-exported)

F32 = np.float32
NONE = 0xFFFFFFFF
ROWS, COLS = 16, 512
MAX_T = 64  # (tnr.MAX_T)

# dcvc_noise_cells: one full cell; no full cell; one full cell beside partial ones; more cells; two sizes that cross a
# 256-column strip with full and partial cells
SIZES = [(16, 16), (15, 40), (17, 33), (64, 96), (100, 260), (48, 516)]


# ------------------------------------------------------------------------------------------------------ the header
def cell_words(pic, yprev):
    """(ycur (H, W) int64, words (hc, wc) int64 holding uint32 values) of a (3, H, W) float32 picture against the previous
    picture's luma plane (None: the first picture, every word NONE)."""
    ycur = luma(pic)
    H, W = ycur.shape
    hc, wc = grid(H, W)
    words = np.full((hc, wc), NONE, dtype=np.int64)
    if yprev is not None:
        fh, fw = H // 16, W // 16
        d = np.abs(ycur - yprev)[:16 * fh, :16 * fw].reshape(fh, 16, fw, 16)
        y = ycur[:16 * fh, :16 * fw].reshape(fh, 16, fw, 16)
        m, l = d.sum(axis=(1, 3)), y.sum(axis=(1, 3))
        words[:fh, :fw] = ((l >> 12) << 16) | m
    return ycur, words


def hist_add(hist, words):
    """ADDS the words (any shape) into hist, a (16, 512) int64 array, in place; returns it."""
    w = np.asarray(words, dtype=np.int64).reshape(-1)
    w = w[(w != NONE) & ((w >> 16) <= ROWS - 1)]
    np.add.at(hist, (w >> 16, np.minimum((w & 0xFFFF) >> 4, COLS - 1)), 1)
    return hist


def run(pics):
    """[(ycur, words)] of a sequence, picture by picture."""
    out, prev = [], None
    for p in pics:
        out.append(cell_words(p, prev))
        prev = out[-1][0]
    return out


def histogram(pics):
    hist = np.zeros((ROWS, COLS), dtype=np.int64)
    for _, words in run(pics):
        hist_add(hist, words)
    return hist


# --------------------------------------------------------------------------------------------------- the estimator
def _quartile(counts, min_cells):
    """counts: 512 integers, column 0 already zero -> the lower quartile's bin centre in 1/32 code, or None."""
    n = int(counts.sum())
    if n < min_cells or n == 0:
        return None
    c = int(np.searchsorted(np.cumsum(counts), (n - 1) // 4, side="right"))  # the first column whose cumulative count exceeds the rank
    return None if c == COLS - 1 else 2 * c + 1


def estimate(hist, min_cells=1024, pairs=None):
    """What noise.estimate(...).to_json() must say."""
    hist = np.asarray(hist, dtype=np.int64)
    mid = hist[1:ROWS - 1].copy()
    still = int(mid[:, 0].sum())
    mid[:, 0] = 0
    mad32 = _quartile(mid.sum(axis=0), min_cells)
    by_luma = [None] + [_quartile(r, min_cells) for r in mid] + [None]
    return {"mad32": mad32, "sigma_milli": None if mad32 is None else int(round(mad32 / 32.0 * math.sqrt(math.pi) / 2.0 * 1000.0)),
            "cells": int(mid.sum()), "still": still, "clipped": int(hist[0].sum() + hist[ROWS - 1].sum()), "pairs": pairs,
            "by_luma": by_luma, "min_cells": min_cells}


def auto_threshold(mad32, scale):
    s100 = int(round(scale * 100.0))
    return min(max(-((-s100 * mad32) // 3200), 1), MAX_T)


def record(pics, scale=3.0, min_cells=1024, pixel=None):
    """What noise.json holds for the pictures: the estimate, the scale, and the resolved threshold and pixel."""
    est = estimate(histogram(pics), min_cells, len(pics) - 1)
    T = auto_threshold(est["mad32"], scale)
    return dict(est, scale=scale, threshold=T, pixel=min(255, 3 * T) if pixel is None else pixel)


# -------------------------------------------------------------------------------------------------------- the clip
SIGMA_Y = math.sqrt(54 ** 2 + 183 ** 2 + 19 ** 2) / 256.0  # of one picture's luma, per code of s


def expected_mad(s):
    """The Gaussian mean absolute luma difference of two noisy pictures, in codes."""
    return math.sqrt(2.0) * SIGMA_Y * s * math.sqrt(2.0 / math.pi)


def clip(H=128, W=192, n=6, s=2.0, obj=(40, 48), seed=7, codes=(0, 256), grey=False):
    """(n, 3, H, W) float32 of exact 8-bit samples.  obj: the (height, width) of the moving object, None for none; it
    starts at (8, 10) and moves (3, 7) pixels a picture, cut at the picture's edge; its texture is uniformly random codes
    within `codes`, the same in every picture.  s = 0: no noise.

    The ground's luma rises smoothly from 64 to 190 along the diagonal.  It is COLOURED -- R and B leave the luma by up to
    15 and 20 codes across the picture and G makes up for them, so that the luma is exactly that ramp -- because the luma's
    weights add up to 256: where R = G = B the sum 54 r + 183 g + 19 b of the ground's codes is a multiple of 256, the luma
    of a grey pixel has no fractional part of its own, and the rounding of Y acts on the noise undithered.  grey=True gives
    that ground (R = G = B = the ramp): a monochrome camera's picture, which measures HIGHER at small noise levels."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    v, u = yy / max(H - 1, 1), xx / max(W - 1, 1)
    ramp = 64.0 + 126.0 * (0.5 * v + 0.5 * u)
    ground = np.repeat(ramp[None], 3, axis=0)
    if not grey:
        dr, db = 30.0 * (u - 0.5), 40.0 * (v - 0.5)
        ground = np.stack([ramp + dr, ramp - (54.0 * dr + 19.0 * db) / 183.0, ramp + db])
    texture = np.random.default_rng(seed + 1000).integers(*codes, size=(3,) + tuple(obj)).astype(np.float64) if obj is not None else None
    out = np.empty((n, 3, H, W), dtype=F32)
    for t in range(n):
        pic = ground.copy()
        if obj is not None:
            y0, x0 = 8 + 3 * t, 10 + 7 * t
            h, w = min(obj[0], H - y0), min(obj[1], W - x0)
            pic[:, y0:y0 + h, x0:x0 + w] = texture[:, :h, :w]
        if s:
            pic = pic + g.normal(0.0, s, size=pic.shape)
        out[t] = np.clip(np.rint(pic), 0, 255).astype(np.int64).astype(F32) / F32(255.0)  # (through integers: no -0.0)
    return out
