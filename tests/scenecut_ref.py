"""A numpy restatement of include/dcvc_hip_scene.h written from its formulas (not from the kernel), of the distance of
vcm_ts_amd/scenecut.py and of its `plan` rule, plus the pictures the scene-cut tests share.

Everything is integer arithmetic after one float32 multiply per sample, so comparisons need no tolerance.
"""
import numpy as np

from tests.pixel_ref import code, luma_of_codes as luma  # noqa: F401 (the tests use them as R.code, R.luma)

from vcm_ts_amd.synthetic import frames

GRID, BINS = 4, 32


def hist(rgb):
    """(512,) int64: rgb is a (3, H, W) float32 picture."""
    k = code(rgb)
    _, H, W = k.shape
    bins = luma(k[0], k[1], k[2]) >> 3
    cy = (4 * np.arange(H)) // H
    cx = (4 * np.arange(W)) // W
    index = (cy[:, None] * GRID + cx[None, :]) * BINS + bins
    return np.bincount(index.reshape(-1), minlength=GRID * GRID * BINS).astype(np.int64)


def cell_pixels(H, W):
    """(16,) pixels per cell, counted pixel by pixel"""
    cy = (4 * np.arange(H)) // H
    cx = (4 * np.arange(W)) // W
    return np.bincount((cy[:, None] * GRID + cx[None, :]).reshape(-1), minlength=GRID * GRID)


def distance(h0, h1, H, W):
    return float(np.abs(np.asarray(h1, np.int64) - np.asarray(h0, np.int64)).sum()) / (2.0 * H * W)


def distances(pictures):
    """float64 d, d[0] = 0, d[t] the distance of pictures t - 1 and t"""
    H, W = pictures[0].shape[1:]
    hs = [hist(p) for p in pictures]
    return np.array([0.0] + [distance(a, b, H, W) for a, b in zip(hs, hs[1:])])


def plan(d, gop, threshold, min_gop=1):
    out, last = [0], 0
    for t in range(1, len(d)):
        since = t - last
        if since >= gop:
            out.append(t)
            last = t
        elif threshold is not None and d[t] > threshold and since >= min_gop:
            out.append(t)
            last = t
    return out


# ------------------------------------------------------------------------------------------------------- test pictures
def scene_a(seed, n, h, w):
    """bright: every luma code is 127 or above"""
    return (np.float32(0.5) + np.float32(0.5) * frames(seed, n, h, w)).astype(np.float32)


def scene_b(seed, n, h, w):
    """dark: every luma code is 90 or below"""
    return (np.float32(0.35) * frames(seed, n, h, w)).astype(np.float32)


def cut_clip(h, w, n_a=5, n_b=11, seed=31):
    """n_a frames of scene A, then n_b of scene B, as 8-bit (n, h, w, 3) pictures (what a PNG or a Y4M is written from)"""
    clip = np.concatenate([scene_a(seed, n_a, h, w), scene_b(seed + 1, n_b, h, w)])
    return code(clip).astype(np.uint8).transpose(0, 2, 3, 1)


def wide_picture(seed, H, W):
    """values over [-0.5, 1.5]: both clamps act"""
    g = np.random.default_rng(seed)
    return g.uniform(-0.5, 1.5, (3, H, W)).astype(np.float32)


def content_pictures(H, W):
    """a constant picture (one counter per cell takes everything), a two-valued checkerboard, a horizontal ramp"""
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.where((yy + xx) % 2 == 0, np.float32(0.2), np.float32(0.8)).astype(np.float32)
    ramp = (xx / max(W - 1, 1)).astype(np.float32)
    return {"constant": np.full((3, H, W), 0.4, np.float32), "checkerboard": np.stack([board] * 3),
            "ramp": np.stack([ramp, ramp[:, ::-1], ramp])}
