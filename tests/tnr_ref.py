"""A numpy restatement of include/dcvc_hip_tnr.h and of tnr.TNR.table, written from their text (not from the kernel or
the module): the 8-bit code and luma of a float picture, the 5 x 5 window sum with replicated edges, the weight, the blend
in float32 operation by operation, the cells' sad / held -- and the pictures and the noisy fixed-camera clip the tnr tests
share.  Integer work is int64."""
import numpy as np

from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as R.code, ...)

F32 = np.float32
CELL, WINDOW, FULL = 16, 5, 256
STRIP_H, STRIP_W = 16, 256  # what one workgroup of csrc/tnr.hip owns: windows across these lines read the halo
# (H, W): one pixel; smaller than the window; one cell; a partial cell and a partial quad; strips crossed in both
# directions, the second strip column 3 pixels wide and the third strip row 1 pixel high; the clip's size
SIZES = [(1, 1), (3, 5), (16, 16), (17, 67), (33, 259), (70, 100)]
SETTINGS = [(12, 64, 36), (6, 32, 255), (24, 128, 12)]  # (T, floor, P)


def table(T, floor):
    """256 uint16: 256 from T on, floor + ((256 - floor) a) // T below."""
    return np.array([FULL if a >= T else floor + ((FULL - floor) * a) // T for a in range(256)], dtype=np.uint16)


def cell_sums(values):
    """(hc, wc) int64: the sum of an (H, W) integer array in every 16 x 16 cell of the padded grid."""
    H, W = values.shape
    hc, wc = grid(H, W)
    full = np.zeros((hc * CELL, wc * CELL), dtype=np.int64)
    full[:H, :W] = values
    return full.reshape(hc, CELL, wc, CELL).sum(axis=(1, 3))


def weights(cur, ref, tab, P):
    """(d, a, w) of every pixel, int64."""
    d = np.abs(luma(cur) - luma(ref))
    H, W = d.shape
    edge = np.pad(d, WINDOW // 2, mode="edge")
    S = sum(edge[dy:dy + H, dx:dx + W] for dy in range(WINDOW) for dx in range(WINDOW))
    a = S // (WINDOW * WINDOW)
    w = np.where(d > P, FULL, np.asarray(tab, dtype=np.int64)[a])
    return d, a, w


def step(cur, ref, tab, P):
    """(out (3, H, W) float32, sad (hc, wc) int64, held (hc, wc) int64) of one dcvc_tnr_step."""
    cur, ref = np.asarray(cur, dtype=F32), np.asarray(ref, dtype=F32)
    d, _, w = weights(cur, ref, tab, P)
    t = cur - ref                      # (float32 operands: every operation below rounds to float32)
    t = t * w.astype(F32)[None]
    t = t * F32(2.0 ** -8)
    blended = ref + t
    assert t.dtype == F32 and blended.dtype == F32
    out = np.where((w == FULL)[None], cur, blended)
    return out, cell_sums(d), cell_sums(w < FULL)


def run(pics, tnr, intra):
    """[(the picture the codec is handed, sad, held)] of a stream: tnr is (T, floor, P), intra the picture numbers that
    are I pictures -- passed through, sad = held = 0, and the filter restarts from them."""
    T, floor, P = tnr
    tab, out = table(T, floor), []
    zeros = np.zeros(grid(*pics[0].shape[1:]), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), zeros, zeros))
        else:
            out.append(step(pic, out[-1][0], tab, P))
    return out


def classes(cur, ref, tab, P):
    """The three pixel classes as fractions of the picture: blended (w < 256), passed through by the pixel guard (d > P),
    passed through by the window alone (d <= P and wtab[a] == 256)."""
    d, a, w = weights(cur, ref, tab, P)
    guard = d > P
    window = ~guard & (np.asarray(tab, dtype=np.int64)[a] == FULL)
    return float((w < FULL).mean()), float(guard.mean()), float(window.mean())


# ------------------------------------------------------------------------------------------------------------ pictures
CLIP_FRAMES, CLIP_SEED, BLOCK, BLOCK_FROM, BLOCK_Y, BLOCK_STEP, NOISE = 9, 5, 20, 5, 20, 10, 4


def clip(H, W, seed=CLIP_SEED):
    """(noisy (9, 3, H, W) float32, clean (9, 3, H, W) float32): a fixed camera.  The clean picture is 8 x 8-pixel blocks
    of uniform random colour in [0.2, 0.8], snapped to 8-bit codes; every picture adds fresh independent integer noise of
    -4 .. 4 codes per sample; from picture 5 on a 20 x 20 block of 0.95 (part of the clean picture, without noise) stands
    at rows 20 .. 39, columns 10 (t - 5) .. 10 (t - 5) + 19, clipped to the picture."""
    g = np.random.default_rng(seed)
    colour = g.uniform(0.2, 0.8, (3, (H + 7) // 8, (W + 7) // 8))
    ground = np.rint(255.0 * np.repeat(np.repeat(colour, 8, axis=1), 8, axis=2)[:, :H, :W]).astype(np.int64)
    noisy, clean = np.empty((CLIP_FRAMES, 3, H, W), F32), np.empty((CLIP_FRAMES, 3, H, W), F32)
    for t in range(CLIP_FRAMES):
        clean[t] = ground.astype(F32) / F32(255.0)
        noisy[t] = (ground + g.integers(-NOISE, NOISE + 1, ground.shape)).astype(F32) / F32(255.0)
        if t >= BLOCK_FROM:
            x = BLOCK_STEP * (t - BLOCK_FROM)
            clean[t, :, BLOCK_Y:BLOCK_Y + BLOCK, x:x + BLOCK] = F32(0.95)
            noisy[t, :, BLOCK_Y:BLOCK_Y + BLOCK, x:x + BLOCK] = F32(0.95)
    return noisy, clean


def bright_pixels(H, W):
    """Five pictures: grey 0.5, then the same with ONE sample column of 1.0 at a pixel on each side of the corner where
    four strips meet (the picture's middle where it has no such corner): what the neighbours across the line get is
    decided by the halo alone."""
    y, x = (STRIP_H if H > STRIP_H else H // 2), (STRIP_W if W > STRIP_W else W // 2)
    pics = [np.full((3, H, W), 0.5, F32)]
    for yy, xx in ((y - 1, x - 1), (y, x), (y - 1, x), (y, x - 1)):
        pic = pics[0].copy()
        pic[:, min(max(yy, 0), H - 1), min(max(xx, 0), W - 1)] = F32(1.0)
        pics.append(pic)
    return pics


def sequences(H, W):
    """name -> pictures, the first an I picture: the clip; all-equal pictures (w = floor everywhere, sad = 0); zeros
    against ones (every pixel guarded at P < 255, held = 0, a full cell's sad = 255 * 256); the bright pixels."""
    g = np.random.default_rng(1000 * H + W)
    same = (g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0))
    zeros, ones = np.zeros((3, H, W), F32), np.ones((3, H, W), F32)
    return {"clip": list(clip(H, W)[0]), "equal": [same, same.copy(), same.copy()], "flip": [zeros, ones, zeros],
            "bright": bright_pixels(H, W)}


def edge_case(H, W, T, P):
    """(cur, ref) grey pictures, where Y is the code and ref is code 0, so d is cur's code.  Upper half: d = T except
    T - 1 in the columns x % 9 == 4 -- a window that holds such a column sums to 25 T - 5 (a = T - 1, blended), any other
    to 25 T (a = T, passed through), side by side at x % 9 in {6, 7} and {1, 2}.  Lower half: d = P at even columns and
    P + 1 (guarded) at odd ones; P = 255 leaves 254 | 255, nothing guarded."""
    yy, xx = np.mgrid[0:H, 0:W]
    upper = np.where(xx % 9 == 4, T - 1, T)
    lower = np.minimum(P, 254) + (xx & 1)
    d = np.where(yy < (H + 1) // 2, upper, lower)
    cur = np.broadcast_to((d.astype(F32) / F32(255.0)).astype(F32), (3, H, W)).copy()
    ref = np.zeros((3, H, W), F32)
    assert np.array_equal(luma(cur), d) and not luma(ref).any()
    return cur, ref
