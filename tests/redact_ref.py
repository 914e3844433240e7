"""A numpy restatement of include/dcvc_hip_redact.h and of redact.held_boxes, written from their text (not from the kernel
or the module): the region R of the selected, grown, clipped boxes, the mosaic's integer tile means on a picture-aligned
grid, the solid fill, the counts per 16 x 16 cell -- and the sizes, pictures, box sets and settings the redact tests
share.  Integer work is int64."""
import functools

import numpy as np

from tests.pixel_ref import code, grid  # noqa: F401 (the tests use them as R.code, R.grid)

F32 = np.float32
CELL, MAX_BOXES = 16, 1024
T = np.arange(256, dtype=F32) / F32(255.0)  # T[k] = (float) k / 255.0f
TILES = (2, 4, 8, 16, 32, 64)
# (H, W): one pixel; smaller than a tile; one cell; one block; a block and one row / three columns more; no multiple of
# anything, two blocks wide; several blocks each way
SIZES = [(1, 1), (7, 5), (16, 16), (64, 64), (65, 67), (70, 100), (130, 200)]
# (tile, fill): every tile side, and two solid fills
MODES = [(t, -1) for t in TILES] + [(0, 0), (0, 200)]
NAMES = ("liplates", "faces", "motion")
MASK, GROW = 0b101, 5  # what the box sets below are written for: classes 0 and 2 selected, class 1 not


def region(boxes, H, W, mask, grow):
    """(H, W) bool: the pixels inside any non-empty box whose class bit is set in `mask`, grown and clipped."""
    R = np.zeros((H, W), dtype=bool)
    for x1, y1, x2, y2, cls in np.asarray(boxes, dtype=np.int64).reshape(-1, 5).tolist():
        if x2 <= x1 or y2 <= y1 or not (mask >> cls) & 1:
            continue
        R[max(y1 - grow, 0):min(y2 + grow, H), max(x1 - grow, 0):min(x2 + grow, W)] = True
    return R


def tile_means(src, tile):
    """(3, H, W) int64: m of the tile every pixel lies in."""
    _, H, W = src.shape
    Hp, Wp = -(-H // tile) * tile, -(-W // tile) * tile
    codes, ones = np.zeros((3, Hp, Wp), np.int64), np.zeros((Hp, Wp), np.int64)
    codes[:, :H, :W], ones[:H, :W] = code(src), 1
    S = codes.reshape(3, Hp // tile, tile, Wp // tile, tile).sum(axis=(2, 4))
    n = ones.reshape(Hp // tile, tile, Wp // tile, tile).sum(axis=(1, 3))
    m = (2 * S + n) // (2 * n)  # (every tile of the grid holds at least one pixel)
    return np.repeat(np.repeat(m, tile, axis=1), tile, axis=2)[:, :H, :W]


def redact(src, boxes, mask, grow, tile, fill):
    """(out (3, H, W) float32, count (hc, wc) int64) of one dcvc_redact."""
    src = np.asarray(src, dtype=F32)
    _, H, W = src.shape
    assert (tile in TILES and fill == -1) or (tile == 0 and 0 <= fill <= 255)
    R = region(boxes, H, W, mask, grow)
    new = T[tile_means(src, tile)] if tile else np.full((3, H, W), T[fill], F32)
    out = src.copy()  # (outside R: the bits of src)
    out[:, R] = new[:, R]
    return out, counts(R)


def counts(R):
    """(hc, wc) int64: the pixels of R in every 16 x 16 cell of the padded grid."""
    H, W = R.shape
    hc, wc = grid(H, W)
    full = np.zeros((hc * CELL, wc * CELL), dtype=np.int64)
    full[:H, :W] = R
    return full.reshape(hc, CELL, wc, CELL).sum(axis=(1, 3))


def held_boxes(frames, g, mask, hold):
    """(n, 5) int64: the selected-class boxes of pictures g - hold .. g + hold that exist, in that order."""
    rows = []
    for t in range(g - hold, g + hold + 1):
        if 0 <= t < len(frames):
            rows += [b for b in np.asarray(frames[t], dtype=np.int64).reshape(-1, 5).tolist() if (mask >> b[4]) & 1]
    if len(rows) > MAX_BOXES:
        raise ValueError(f"picture {g}: {len(rows)} boxes")
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------------------ pictures
@functools.lru_cache(maxsize=None)
def picture(H, W):
    """(3, H, W) float32: mostly 8-bit samples over 255, with samples no code represents, values below 0 and above 1,
    infinities, and NaNs of two payloads sprinkled in -- what must be copied as bits outside R and coded inside."""
    g = np.random.default_rng(7000 * H + W)
    pic = g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0)
    kind = g.integers(0, 12, (3, H, W))
    pic = np.where(kind == 0, g.uniform(-0.5, 1.5, (3, H, W)).astype(F32), pic)
    bits = pic.view(np.uint32).copy()
    bits[kind == 1] = 0x7FC00001  # a quiet NaN with a payload
    bits[kind == 2] = 0xFFC12345  # a negative one with another
    pic = bits.view(F32)
    pic = np.where(kind == 3, F32(np.inf), pic)
    pic.setflags(write=False)
    return pic


def _clip(a, H, W):
    a = np.asarray(a, dtype=np.int64).reshape(-1, 5)
    a[:, [0, 2]] = np.clip(a[:, [0, 2]], 0, W)
    a[:, [1, 3]] = np.clip(a[:, [1, 3]], 0, H)
    return a


def random_boxes(H, W, n, seed, side=24):
    """n boxes of classes 0 .. 2 with sides below `side`, every tenth one empty."""
    g = np.random.default_rng(seed)
    x1, y1 = g.integers(0, W + 1, n), g.integers(0, H + 1, n)
    a = np.stack([x1, y1, x1 + g.integers(1, side, n), y1 + g.integers(1, side, n), g.integers(0, 3, n)], axis=1)
    a[::10, 2] = a[::10, 0]  # x2 == x1: empty, not an error
    return _clip(a, H, W)


@functools.lru_cache(maxsize=None)
def box_sets(H, W):
    """name -> (n, 5) int64 boxes for an H x W picture, to be redacted with MASK and GROW (and with grow 0)."""
    cy, cx = H // 2, W // 2
    sets = {
        "none": np.zeros((0, 5), np.int64),
        "pixel": np.array([[cx, cy, cx + 1, cy + 1, 0]]),
        "whole": np.array([[0, 0, W, H, 2]]),
        # on every edge and in every corner: the grow margin is clipped at the picture
        "edges": _clip([[0, 0, 3, 2, 0], [W - 2, 0, W, 3, 2], [0, H - 3, 2, H, 0], [W - 3, H - 2, W, H, 2],
                        [cx, 0, cx + 2, 1, 0], [0, cy, 1, cy + 2, 2], [cx, H - 1, cx + 2, H, 0], [W - 1, cy, W, cy + 2, 2]], H, W),
        # selected and unselected classes overlapping, an empty selected box, and one that is empty but would not be grown
        "classes": _clip([[1, 1, cx + 2, cy + 2, 1], [cx // 2, cy // 2, cx + 1, cy + 1, 0], [cx, cy, W, H, 1],
                          [cx + 1, cy // 2, W - 1, cy + 1, 2], [2, cy, 2, H, 0], [cx, 3, W, 3, 2], [0, cy + 3, cx // 2, H, 1]], H, W),
    }
    if H > 64 and W > 66:  # these reach the blocks left of column 64 and above row 64 only through their grow margin
        sets["margin"] = _clip([[66, 64, 67, 65, 0], [66, 2, 67, 4, 2], [3, 64 + GROW - 1, 5, 64 + GROW, 0]], H, W)
    if (H, W) == (130, 200):
        sets["random300"] = random_boxes(H, W, 300, 300)
        sets["full1024"] = random_boxes(H, W, MAX_BOXES, 1024, side=12)
    for a in sets.values():
        a.setflags(write=False)
    return sets


def cases(H, W):
    """[(name of the box set, boxes, grow)]: every set with GROW, the ones a margin matters to also with 0."""
    out = []
    for name, boxes in box_sets(H, W).items():
        out.append((name, boxes, GROW))
        if name in ("edges", "classes", "pixel"):
            out.append((name, boxes, 0))
    return out


@functools.lru_cache(maxsize=None)
def expected(H, W, name, grow, tile, fill):
    """redact() of picture(H, W) with box_sets(H, W)[name]: computed once, shared, read-only."""
    out, count = redact(picture(H, W), box_sets(H, W)[name], MASK, grow, tile, fill)
    out.setflags(write=False)
    count.setflags(write=False)
    return out, count


# ---- the file loops: a clip of exactly representable pictures and boxes of all three classes with a detector's gaps
CLIP_FRAMES = 8


def clip(H, W, seed=11):
    """(8, 3, H, W) float32 of 8-bit samples over 255: 6 x 6 blocks of random colour (no tile side divides them, so a
    mosaic mixes colours) with a little noise, and a bright 20 x 20 block that moves 9 pixels a picture."""
    g = np.random.default_rng(seed)
    colour = g.integers(40, 216, (3, (H + 5) // 6, (W + 5) // 6))
    ground = np.repeat(np.repeat(colour, 6, axis=1), 6, axis=2)[:, :H, :W]
    pics = np.empty((CLIP_FRAMES, 3, H, W), F32)
    for t in range(CLIP_FRAMES):
        u8 = ground + g.integers(-3, 4, ground.shape)
        u8[:, 30:50, 9 * t + 4:9 * t + 24] = 243
        pics[t] = u8.astype(F32) / F32(255.0)
    return pics


def clip_boxes(H, W):
    """The boxes of the clip's pictures, by class: a plate (0) that a detector misses in pictures 3 and 4, a face (1) in
    every picture, the moving block (2, motion) from picture 1 on -- picture 0 has none, as run_codec boxes leaves it."""
    frames = []
    for t in range(CLIP_FRAMES):
        rows = [[W - 50, H - 40, W - 20, H - 28, 1]]
        if t not in (3, 4):
            rows.append([60 + t, 70, 84 + t, 81, 0])
        if t >= 1:
            rows.append([9 * t + 4, 30, 9 * t + 24, 50, 2])
        frames.append(_clip(rows, H, W))
    return frames
