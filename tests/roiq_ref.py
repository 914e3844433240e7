"""A numpy restatement of the q-scale map of include/dcvc_hip_roi.h ("Q-scale map"), written from its text (not from the
kernel), and the box lists, sizes and factors the ROI-weighted quantisation tests share.  The map exists twice: `q_map`
is the literal procedure (paint a per-pixel factor image box by box with `minimum`, then reduce every 16x16 cell by
`min`), `q_map_touches` the header's closed-form "touches" rule."""
import numpy as np

from tests.pixel_ref import grid  # noqa: F401 (the tests use it as R.grid)

F32 = np.float32
CELL = 16
SIZES = [(1, 1), (16, 16), (17, 33), (64, 64), (65, 63), (135, 241)]  # (H, W)
GROWS = (0, 1, 16, 255)
BACKGROUND, CLASSES = 100, (60, 140, 10, 1000)  # hundredths: a class above, two below the background, both limits


def factors(background=BACKGROUND, classes=CLASSES):
    """[background, class 0, ...]: float32(k) / float32(100)"""
    return np.array((background,) + tuple(classes), dtype=F32) / F32(100)


def _grown(boxes, H, W, grow):
    """(x1', y1', x2', y2', cls) of every non-empty box, grown and clipped to the picture"""
    out = []
    for x1, y1, x2, y2, c in np.asarray(boxes, dtype=np.int64).reshape(-1, 5).tolist():
        if x2 > x1 and y2 > y1:
            out.append((max(x1 - grow, 0), max(y1 - grow, 0), min(x2 + grow, W), min(y2 + grow, H), c))
    return out


def q_map(boxes, H, W, grow, f):
    """The literal procedure -> (hc, wc) float32."""
    hc, wc = grid(H, W)
    image = np.full((hc * CELL, wc * CELL), np.inf, dtype=F32)  # the padded picture; inf: no box has painted here
    for x1, y1, x2, y2, c in _grown(boxes, H, W, grow):
        image[y1:y2, x1:x2] = np.minimum(image[y1:y2, x1:x2], f[1 + c])
    cells = image.reshape(hc, CELL, wc, CELL).min(axis=(1, 3))
    return np.where(np.isinf(cells), f[0], cells).astype(F32)


def q_map_touches(boxes, H, W, grow, f):
    """The closed form: min of f[1 + cls] over the grown boxes that touch the cell, f[0] where none does."""
    hc, wc = grid(H, W)
    i, j = np.mgrid[0:hc, 0:wc]
    best = np.full((hc, wc), np.inf, dtype=F32)
    for x1, y1, x2, y2, c in _grown(boxes, H, W, grow):
        touches = (x1 < CELL * j + CELL) & (x2 > CELL * j) & (y1 < CELL * i + CELL) & (y2 > CELL * i)
        best = np.where(touches, np.minimum(best, f[1 + c]), best)
    return np.where(np.isinf(best), f[0], best).astype(F32)


def box_lists(H, W, n_classes=len(CLASSES)):
    """name -> (n, 5) int32 lists for an H x W picture: random ones, edges at 15 / 16 / 17, empty boxes, 1024 boxes."""
    g = np.random.default_rng(1000 * H + W)

    def rand(n):
        xs, ys = np.sort(g.integers(0, W + 1, (n, 2)), axis=1), np.sort(g.integers(0, H + 1, (n, 2)), axis=1)
        return np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1], g.integers(0, n_classes, n)], axis=1).astype(np.int32)

    def small(n, side):
        x1, y1 = g.integers(0, W + 1, n), g.integers(0, H + 1, n)
        x2, y2 = np.minimum(x1 + g.integers(0, side + 1, n), W), np.minimum(y1 + g.integers(0, side + 1, n), H)
        return np.stack([x1, y1, x2, y2, g.integers(0, n_classes, n)], axis=1).astype(np.int32)

    clip = lambda rows: np.array([[min(x1, W), min(y1, H), min(x2, W), min(y2, H), c % n_classes] for x1, y1, x2, y2, c in rows],
                                 dtype=np.int32)
    edges = clip([(a, b, a + d, b + d, k) for k, (a, b, d) in enumerate(
        [(15, 15, 1), (16, 16, 1), (17, 17, 1), (0, 0, 15), (0, 0, 16), (0, 0, 17), (15, 0, 2), (0, 15, 2), (16, 31, 16),
         (31, 16, 17), (33, 47, 15), (W - 1, H - 1, 1), (W - 17, H - 16, 16), (max(W - 15, 0), max(H - 17, 0), 15)])
                  if a >= 0 and b >= 0])
    empties = clip([(5, 5, 5, 9, 0), (9, 3, 4, 8, 1), (0, 0, W, 0, 2), (3, 8, 9, 2, 3), (W, H, W, H, 0), (0, 0, 0, 0, 1)])
    return {"none": np.zeros((0, 5), np.int32), "one": clip([(W // 4, H // 4, W - W // 4, H - H // 4, 0)]),
            "whole": clip([(0, 0, W, H, 1)]), "random-7": rand(7), "random-40": small(40, 24), "edges": edges,
            "empty": empties, "empty-and-one": np.concatenate([empties, clip([(1, 1, W, H, 2)])]),
            "1024": small(1024, 12), "1024-large": rand(1024)}
