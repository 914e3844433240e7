"""A numpy restatement of include/dcvc_hip_roi.h written from its formulas (not from the kernels), and the box lists and
pictures the ROI tests share.  The feather mask exists twice: `feather_mask_literal` is the reference's procedure (box
after box, slice assignment of a gradient mask built ring by ring), `feather_mask` the header's closed form."""
import numpy as np

from tests.pixel_ref import code  # noqa: F401 (the tests use it as R.code)

F32 = np.float32
T = np.arange(256).astype(F32) / F32(255.0)  # the host quotients k / 255


def feather_table(border):
    return (1.0 - np.linspace(0.9, 0.0, border)).astype(F32)


def _nonempty(boxes):
    return [tuple(int(v) for v in b) for b in np.asarray(boxes).reshape(-1, 5) if b[2] > b[0] and b[3] > b[1]]


def binary_mask(boxes, H, W, shrinks=None):
    """1 where any non-empty box holds the pixel; shrinks: per class, [y1 + p : y2 - p, x1 + p : x2 - p] (a box that
    shrinks to nothing is empty)."""
    mask = np.zeros((H, W), dtype=bool)
    for x1, y1, x2, y2, c in _nonempty(boxes):
        p = shrinks[c] if shrinks is not None else 0
        if x2 - p > x1 + p and y2 - p > y1 + p:
            mask[y1 + p:y2 - p, x1 + p:x2 - p] = True
    return mask


def gradient_mask(w, h, border):
    """create_gradient_mask"""
    if border == 0:
        return np.ones((h, w), dtype=F32)
    mask = np.zeros((h, w), dtype=F32)
    for i, x in enumerate(np.linspace(0.9, 0.0, border)):
        mask[i:h - i, i:w - i] = 1 - x  # (i > h makes h - i negative, but a slice that starts beyond h is empty anyway)
    return mask


def feather_mask_literal(boxes, borders, H, W):
    mask = np.zeros((H, W), dtype=F32)
    for x1, y1, x2, y2, c in _nonempty(boxes):
        mask[y1:y2, x1:x2] = gradient_mask(x2 - x1, y2 - y1, borders[c])
    return mask


def feather_mask(boxes, borders, H, W):
    """closed form: the last box that holds the pixel, feather[min(d, border - 1)]"""
    mask = np.zeros((H, W), dtype=F32)
    ys, xs = np.mgrid[0:H, 0:W]
    for x1, y1, x2, y2, c in _nonempty(boxes):
        inside = (xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)
        border = borders[c]
        if border == 0:
            mask[inside] = F32(1.0)
            continue
        d = np.minimum(np.minimum(xs - x1, x2 - 1 - xs), np.minimum(ys - y1, y2 - 1 - ys))
        table = feather_table(border)
        mask[inside] = table[np.minimum(d, border - 1)[inside]]
    return mask


def residual(src, rec, boxes):
    """(3, H, W) uint8 in channel order R, G, B"""
    H, W = src.shape[1:]
    r = np.clip(code(src) - code(rec) + 128, 0, 255)
    return np.where(binary_mask(boxes, H, W)[None], r, 0).astype(np.uint8)


def fuse(base, res, boxes, borders):
    """base (3, H, W) float32, res (3, H, W) uint8 in R, G, B order -> (3, H, W) float32"""
    H, W = base.shape[1:]
    m = feather_mask(boxes, borders, H, W)[None]
    e = res.astype(F32) - F32(128.0)
    b = code(base).astype(F32)
    s = (m * e).astype(F32)       # one rounded multiply
    v = (s + b).astype(F32)       # one rounded add
    k = np.minimum(np.maximum(v, F32(0.0)), F32(255.0)).astype(np.int64)  # truncation toward zero
    return T[k]


def sse(a, b, boxes, shrinks):
    H, W = a.shape[1:]
    mask = binary_mask(boxes, H, W, shrinks)
    d2 = ((code(a) - code(b)) ** 2).sum(0)
    return [int(d2[mask].sum()), int(d2[~mask].sum()), int(mask.sum())]


def psnr(sums, H, W, divisors):
    s_in, s_out, n_in = (np.float64(v) for v in sums)
    total = np.float64(3 * H * W)
    d_in, d_out = (3 * n_in, total - 3 * n_in) if divisors == "samples" else (n_in, total - n_in)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = lambda s, n: float(10.0 * np.log10(255.0 ** 2 / (s / n)))
        return f(s_in + s_out, total), f(s_out, d_out), f(s_in, d_in)


def fma_sensitive(m, e, b):
    """True where truncating the exact m * e + b rounded once (a fused multiply-add) gives another code than the
    header's multiply-then-add.  float64 holds the product of two float32 exactly, and the sum of it with a small
    integer to more bits than float32 keeps."""
    m, e, b = (np.asarray(v, dtype=F32) for v in (m, e, b))
    two = ((m * e).astype(F32) + b).astype(F32)
    one = (m.astype(np.float64) * e.astype(np.float64) + b.astype(np.float64)).astype(F32)
    trunc = lambda v: np.minimum(np.maximum(v, F32(0.0)), F32(255.0)).astype(np.int64)
    return trunc(two) != trunc(one)


# ------------------------------------------------------------------------------------------------ shared cases
SIZES = [(37, 131), (38, 518), (64, 64), (1, 1)]
BORDERS = (10, 3, 0, 1)     # classes 0..3
SHRINKS = {"shrink0": (0, 0, 0, 0), "shrink3": (3, 3, 3, 3), "emptying": (30, 2, 64, 7)}


def pictures(seed, H, W):
    """(src, rec): float32 (3, H, W); src on the 8-bit grid, rec off it and reaching beyond [0, 1]"""
    rng = np.random.default_rng(seed)
    src = T[rng.integers(0, 256, (3, H, W))]
    rec = (src + rng.normal(0.0, 0.08, (3, H, W))).astype(F32)
    rec[:, :: 7, :: 5] = F32(1.3)
    rec[:, 1:: 11, 2:: 3] = F32(-0.2)
    return src, rec


def residual_picture(seed, H, W):
    """(3, H, W) uint8 with every value near the extremes often enough to reach the clip of fuse"""
    rng = np.random.default_rng(seed + 1000)
    r = rng.integers(0, 256, (3, H, W))
    r[:, ::3, ::4] = rng.choice([0, 1, 254, 255], size=r[:, ::3, ::4].shape)
    return r.astype(np.uint8)


def box_lists(H, W):
    """{name: (n, 5) int32}: the lists of tests/test_gpu_roi.py for one picture size"""
    rng = np.random.default_rng(H * 100003 + W)
    c = lambda v, hi: int(min(max(v, 0), hi))
    out = {"none": np.zeros((0, 5), np.int32), "whole": np.array([[0, 0, W, H, 0]], np.int32)}
    # edges at every x residue mod 4 and on tile boundaries (columns 256, 512; rows 8, 16)
    edges = []
    for k in range(8):
        edges.append([c(k, W), c(k % 3, H), c(k + 9 + k, W), c(5 + k, H), k % 4])
    for x in (252, 255, 256, 257, 510, 512, 513):
        edges.append([c(x, W), c(6, H), c(x + 3, W), c(10, H), 1])
        edges.append([c(x - 20, W), c(8, H), c(x, W), c(16, H), 2])
    out["edges"] = np.array(edges, np.int32)
    out["touching"] = np.array([[c(W - 5, W), c(H - 7, H), W, H, 0], [0, c(H - 2, H), c(9, W), H, 1], [c(W - 1, W), 0, W, c(3, H), 3]], np.int32)
    out["empty"] = np.array([[c(5, W), c(5, H), c(5, W), c(9, H), 0], [c(9, W), c(9, H), c(3, W), c(3, H), 1], [0, 0, c(4, W), 0, 2], [c(2, W), c(1, H), c(30, W), c(20, H), 1]], np.int32)
    over = np.array([[c(2, W), c(2, H), c(40, W), c(30, H), 0], [c(20, W), c(10, H), c(60, W), c(36, H), 1],
                     [c(30, W), c(0, H), c(50, W), c(25, H), 2], [c(10, W), c(15, H), c(45, W), c(33, H), 3]], np.int32)
    out["overlap"] = over
    out["overlap-reversed"] = over[::-1].copy()
    out["narrow"] = np.array([[c(3, W), c(2, H), c(3 + 7, W), c(2 + 30, H), 0], [c(20, W), c(4, H), c(90, W), c(4 + 5, H), 0]], np.int32)
    for name, n in (("many150", 150), ("max1024", 1024)):
        x1, y1 = rng.integers(0, max(W - 1, 1), n), rng.integers(0, max(H - 1, 1), n)
        x2 = np.minimum(x1 + rng.integers(0, 13, n), W)
        y2 = np.minimum(y1 + rng.integers(0, 9, n), H)
        out[name] = np.stack([x1, y1, x2, y2, rng.integers(0, 4, n)], 1).astype(np.int32)
    return out
