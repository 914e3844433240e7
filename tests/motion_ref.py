"""A numpy restatement of include/dcvc_hip_motion.h and of motionroi.boxes_from_counts, written from their text (not from
the kernel or the module): the 8-bit code and luma of a float picture, one step of the background model, the per-cell
foreground counts, the boxes of a count grid (scipy.ndimage does the dilation and the labelling) -- and the pictures and
the static-camera clip the motion tests share."""
import numpy as np
from scipy import ndimage

from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as R.code, ...)
from vcm_ts_amd.synthetic import frames

F32 = np.float32
CELL = 16
SIZES = [(64, 64), (70, 100), (128, 192), (16, 16), (1, 1)]  # (H, W)
SETTINGS = [(24, 4, 8), (1, 0, 16), (254, 16, 0)]  # (T, k_bg, k_fg)


def cell_sums(mask):
    """(hc, wc) int64: the number of set pixels of an (H, W) mask in every 16 x 16 cell of the padded grid."""
    H, W = mask.shape
    hc, wc = grid(H, W)
    full = np.zeros((hc * CELL, wc * CELL), dtype=np.int64)
    full[:H, :W] = mask
    return full.reshape(hc, CELL, wc, CELL).sum(axis=(1, 3))


def init(pic):
    """(the model, the counts) after the init step."""
    Y = luma(pic)
    return Y << 8, np.zeros(grid(*Y.shape), dtype=np.int64)


def step(pic, bg, T, k_bg, k_fg):
    """(the new model, the counts) of one step with init == 0; bg is an (H, W) integer array, untouched."""
    B = np.asarray(bg, dtype=np.int64)
    delta = (luma(pic) << 8) - B
    a = np.abs(delta)
    fg = a > (T << 8)
    s = np.where(fg, a >> k_fg, a >> k_bg)
    return B + np.where(delta < 0, -s, s), cell_sums(fg)


def run(pics, T, k_bg, k_fg):
    """[(model, counts)] after the init step on pics[0] and a step on each further picture."""
    out = [init(pics[0])]
    for pic in pics[1:]:
        out.append(step(pic, out[-1][0], T, k_bg, k_fg))
    return out


def boxes(counts, H, W, min_pixels=8, grow=1, min_cells=1, max_boxes=64):
    """(n, 4) int32 x1, y1, x2, y2 of an (hc, wc) count grid: the seven steps of motionroi.boxes_from_counts."""
    counts = np.asarray(counts, dtype=np.int64)
    active = counts >= min_pixels
    dilated = ndimage.maximum_filter(active.astype(np.uint8), size=2 * grow + 1, mode="constant", cval=0) > 0
    labels, n = ndimage.label(dilated, structure=np.ones((3, 3), dtype=int))
    found = []
    for sl, k in zip(ndimage.find_objects(labels), range(1, n + 1)):
        inside = (labels == k) & active
        if inside.sum() < min_cells:
            continue
        y1, x1 = CELL * sl[0].start, CELL * sl[1].start
        y2, x2 = min(CELL * sl[0].stop, H), min(CELL * sl[1].stop, W)
        if x2 <= x1 or y2 <= y1:
            continue
        found.append((int(counts[inside].sum()), (y1, x1, y2, x2)))
    if len(found) > max_boxes:
        found = sorted(found, key=lambda f: (-f[0], f[1]))[:max_boxes]
    rows = sorted(f[1] for f in found)
    return np.array([(x1, y1, x2, y2) for y1, x1, y2, x2 in rows], dtype=np.int32).reshape(-1, 4)


def clip_boxes(pics, T, learn=(4, 8), **kw):
    """The boxes of every picture of a clip; picture 0 has none."""
    H, W = pics[0].shape[1:]
    return [np.zeros((0, 4), np.int32) if t == 0 else boxes(c, H, W, **kw) for t, (_, c) in enumerate(run(pics, T, *learn))]


# ------------------------------------------------------------------------------------------------------------ pictures
def pictures(H, W):
    """name -> (3, H, W) float32: three pictures of random 8-bit codes / 255, samples below 0 and above 1 with NaNs and an
    infinity among them, all zeros, all ones."""
    g = np.random.default_rng(1000 * H + W)
    wild = (g.standard_normal((3, H, W)) * 0.8 + 0.5).astype(F32)
    wild[0, 0, 0], wild[1, H - 1, W - 1], wild[2, H // 2, W // 2], wild[2, H - 1, 0] = np.nan, np.nan, np.inf, -np.inf
    out = {f"random{i}": g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0) for i in range(3)}
    out.update(wild=wild, zeros=np.zeros((3, H, W), F32), ones=np.ones((3, H, W), F32))
    return out


def sequences(H, W):
    """name -> four pictures (the init step and three more): random ones with the wild one among them; zeros and ones in
    turn, where every pixel of every cell is foreground at every T (|delta| = 65280 > 254 << 8)."""
    p = pictures(H, W)
    return {"random": [p["random0"], p["random1"], p["wild"], p["random2"]],
            "flip": [p["zeros"], p["ones"], p["zeros"], p["ones"]],
            "wild-first": [p["wild"], p["random2"], p["ones"], p["random0"]]}


def edge_case(H, W, T):
    """(a model, a picture) on which |delta| is exactly T << 8 at even columns (background) and (T << 8) + 1 at odd ones
    (foreground), with delta positive on even rows and negative on odd ones.  The picture is grey, where Y is the code."""
    yy, xx = np.mgrid[0:H, 0:W]
    up, odd = (yy & 1) == 0, (xx & 1) == 1
    bg = np.where(up, (1 << 8) - odd, (254 << 8) + odd).astype(np.int64)
    Y = np.where(up, 1 + T, 254 - T)
    pic = np.broadcast_to((Y.astype(F32) / F32(255.0)).astype(F32), (3, H, W)).copy()
    assert np.array_equal(luma(pic), Y)
    a = np.abs((Y << 8) - bg)
    assert ((a == (T << 8) + odd)).all()
    return bg, pic


RECT_W, RECT_H, RECT_Y, CLIP_FRAMES = 40, 24, 20, 6


def clip(H, W, rectangle=True):
    """(pictures (6, 3, H, W) float32, the rectangle of every picture as x1, y1, x2, y2 clipped to the picture): a static
    camera -- synthetic.frames(7, 1, H, W, noise=0) as the background of every picture, fresh 1/255 Gaussian noise on each,
    and a 40 x 24 rectangle of constant 0.0 or 1.0 (whichever is further from the mean of the background it covers) at
    x = 8 + 8 t, y = 20 in picture t."""
    ground = frames(7, 1, H, W, noise=0)[0]
    g = np.random.default_rng(77)
    pics, rects = np.empty((CLIP_FRAMES, 3, H, W), F32), []
    for t in range(CLIP_FRAMES):
        pic = ground + F32(1.0 / 255.0) * g.standard_normal(ground.shape).astype(F32)
        x1, y1 = min(8 + 8 * t, W), min(RECT_Y, H)
        x2, y2 = min(x1 + RECT_W, W), min(y1 + RECT_H, H)
        if rectangle and x2 > x1 and y2 > y1:
            pic[:, y1:y2, x1:x2] = F32(0.0) if ground[:, y1:y2, x1:x2].mean() >= 0.5 else F32(1.0)
        pics[t] = np.clip(pic, 0.0, 1.0)
        rects.append((x1, y1, x2, y2))
    return pics, rects


def covered(rect, bxs):
    """Every pixel of `rect` lies inside the union of the boxes."""
    x1, y1, x2, y2 = rect
    seen = np.zeros((y2 - y1, x2 - x1), dtype=bool)
    for bx1, by1, bx2, by2 in np.asarray(bxs).tolist():
        seen[max(by1 - y1, 0):max(by2 - y1, 0), max(bx1 - x1, 0):max(bx2 - x1, 0)] = True
    return bool(seen.all())
