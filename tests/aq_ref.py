"""A numpy restatement of include/dcvc_hip_aq.h, written from its text (not from the kernel): the 8-bit code and luma of a
float picture, the activity L of every 16x16 cell, the picture mean, the two host-built tables and the q-scale map -- and
the pictures the backward-adaptive quantisation tests share."""
import numpy as np

from tests.pixel_ref import code, luma  # noqa: F401 (the tests use them as R.code, R.luma)

F32 = np.float32
CELL, MAX_L = 16, 7935
SIZES = [(64, 64), (64, 128), (128, 192), (192, 64)]  # (Hp, Wp)


def variance256(Y):
    """V = 256 S2 - S1^2 per cell of an (Hp, Wp) integer luma plane -> (hc, wc) int64."""
    Hp, Wp = Y.shape
    assert Hp % 64 == 0 and Wp % 64 == 0
    cells = Y.astype(np.int64).reshape(Hp // CELL, CELL, Wp // CELL, CELL)
    s1, s2 = cells.sum(axis=(1, 3)), (cells * cells).sum(axis=(1, 3))
    return 256 * s2 - s1 * s1


def log_activity(V):
    """L = 256 e + m of v = V + 1, with Python integers: e the position of the leading one, m the 8 bits below it."""
    out = np.empty(np.shape(V), dtype=np.int64)
    flat = out.reshape(-1)
    for i, V_i in enumerate(np.asarray(V, dtype=np.int64).reshape(-1).tolist()):
        v = V_i + 1
        e = v.bit_length() - 1
        m = ((v >> (e - 8)) if e >= 8 else (v << (8 - e))) & 255
        flat[i] = 256 * e + m
    return out


def activity(pic):
    """(L as (hc, wc) int64, the sum of L as a Python integer) of a (3, Hp, Wp) float32 picture."""
    L = log_activity(variance256(luma(pic)))
    return L, int(L.sum())


def ktab(A, lo=10, hi=1000):
    """k(d), d = -7935 .. 7935, as uint16; float64 on the host."""
    d = np.arange(-MAX_L, MAX_L + 1).astype(np.float64)
    return np.clip(np.rint(100.0 * np.exp2(A * d / (100.0 * 256.0 * 6.0))), lo, hi).astype(np.uint16)


def ftab():
    return np.array([F32(k) / F32(100.0) for k in range(10, 1001)], dtype=F32)


def q_map(L, total, A, lo=10, hi=1000, roi=None):
    """The (hc, wc) float32 map from L and the sum of L (which need not be L.sum(): the kernel takes what it is given)."""
    kt, ft = ktab(A, lo, hi), ftab()
    M = int(total) // L.size
    k = kt[(L - M) + MAX_L].astype(np.int64)
    if roi is not None:
        k_roi = np.rint(F32(100.0) * np.asarray(roi, dtype=F32).reshape(L.shape)).astype(np.int64)
        k = np.clip((k_roi * k + 50) // 100, 10, 1000)
    return ft[k - 10]


def picture_map(pic, A, lo=10, hi=1000, roi=None):
    """q_map of a picture's own activity: what aq.AqMaps.map returns for a (1, 3, Hp, Wp) reference picture."""
    L, total = activity(np.asarray(pic, dtype=F32).reshape((3,) + tuple(np.shape(pic)[-2:])))
    return q_map(L, total, A, lo, hi, roi)


def pictures(Hp, Wp):
    """name -> (3, Hp, Wp) float32 pictures: random 8-bit codes / 255, values outside [0, 1] (and a NaN), all 0, all 255,
    a checkerboard of 0 and 255 (the largest V in every cell), cells that are each flat, one busy cell among flat ones
    (d at both ends of the table)."""
    g = np.random.default_rng(100 * Hp + Wp)
    codes = g.integers(0, 256, (3, Hp, Wp))
    wild = (g.standard_normal((3, Hp, Wp)) * 0.8 + 0.5).astype(F32)
    wild[0, 3, 5], wild[2, Hp - 1, Wp - 1] = np.nan, np.inf
    yy, xx = np.mgrid[0:Hp, 0:Wp]
    checker = np.broadcast_to(((yy + xx) & 1).astype(F32), (3, Hp, Wp)).copy()
    flat_cells = np.repeat(np.repeat(g.integers(0, 256, (3, Hp // CELL, Wp // CELL)), CELL, axis=1), CELL, axis=2)
    lone = np.full((3, Hp, Wp), F32(0.5), dtype=F32)
    lone[:, 16:32, 32:48] = checker[:, 16:32, 32:48]
    smooth = np.broadcast_to((xx / F32(Wp)).astype(F32), (3, Hp, Wp)).copy()
    smooth[:, : Hp // 2] = (codes[:, : Hp // 2] / 255.0).astype(F32)
    return {"random": codes.astype(F32) / F32(255.0), "wild": wild, "zeros": np.zeros((3, Hp, Wp), F32),
            "ones": np.ones((3, Hp, Wp), F32), "checker": checker, "flat-cells": flat_cells.astype(F32) / F32(255.0),
            "lone-busy": lone, "half-smooth": smooth}
