"""A numpy restatement of include/dcvc_hip_me.h, written from its text (not from the kernels or the module): the search by
brute force over the candidates in the order of their keys, the compensation, a stream filtered with the search in front of
tests/tnr_ref.py's step -- and the pictures the me tests share.  Integer work is int64."""
import numpy as np

from tests import tnr_ref as T
from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as R.grid, ...)

F32 = np.float32
CELL, MAX_R, MAX_LAMBDA = 16, 32, 255
SIZES = T.SIZES  # (1, 1), (3, 5), (16, 16), (17, 67), (33, 259), (70, 100)
LAMBDAS = (0, 4, 255)


def cells_of(H, W):
    """(H, W) int64: the number i * wc + j of the cell that holds each pixel."""
    _, wc = grid(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy // CELL) * wc + xx // CELL


def candidates(R):
    """Every (dy, dx) within +-R, sorted by (|dy| + |dx|, dy, dx): of equal J the first of these wins."""
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))


def sads(cur, ref, R):
    """{(dy, dx): (hc, wc) int64 SAD of every cell}, the coordinates of ref clamped to the picture."""
    yc, yr = luma(np.asarray(cur, dtype=F32)), luma(np.asarray(ref, dtype=F32))
    H, W = yc.shape
    edge = np.pad(yr, R, mode="edge")  # (edge[y + R, x + R] = Y(ref, clamp(y), clamp(x)) for every y, x within R of the picture)
    return {(dy, dx): T.cell_sums(np.abs(yc - edge[R + dy:R + dy + H, R + dx:R + dx + W])) for dy, dx in candidates(R)}


def search(cur, ref, R, lam, table=None):
    """(mv (hc, wc, 2) int64, cost (hc, wc) int64, zero (hc, wc) int64) of one dcvc_me_search; table: sads(cur, ref, R)
    where the caller has it already."""
    assert 1 <= R <= MAX_R and 0 <= lam <= MAX_LAMBDA
    table = sads(cur, ref, R) if table is None else table
    zero = table[0, 0]
    best = np.full(zero.shape, 1 << 40, dtype=np.int64)
    mv, cost = np.zeros(zero.shape + (2,), dtype=np.int64), np.zeros(zero.shape, dtype=np.int64)
    for dy, dx in candidates(R):  # (in the order of the rest of the key: only a strictly smaller J replaces)
        J = table[dy, dx] + lam * (abs(dy) + abs(dx))
        better = J < best
        best[better], cost[better] = J[better], table[dy, dx][better]
        mv[better] = (dy, dx)
    return mv, cost, zero


def compensate(ref, mv):
    """(3, H, W) float32: ref's samples (their bits) from (clamp(y + dy), clamp(x + dx)), (dy, dx) the vector of the
    pixel's cell; mv is (hc, wc, 2) of any integers."""
    ref = np.asarray(ref, dtype=F32)
    _, H, W = ref.shape
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.asarray(mv, dtype=np.int64).reshape(-1, 2)[cells_of(H, W)]
    return ref[:, np.clip(yy + v[..., 0], 0, H - 1), np.clip(xx + v[..., 1], 0, W - 1)]


def run(pics, tnr, intra, R, lam):
    """[(the picture the codec is handed, sad, held, mv, cost, zero)] of a stream filtered with the search: tnr is
    (T, floor, P), intra the picture numbers that are I pictures -- passed through, zeros in the five arrays, and the filter
    restarts from them.  A P picture is searched for in the previous handed picture, that picture is compensated, and
    tests/tnr_ref.py's step blends against the compensated one."""
    tab, out = T.table(tnr[0], tnr[1]), []
    hc, wc = grid(*pics[0].shape[1:])
    z = np.zeros((hc, wc), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), z, z, np.zeros((hc, wc, 2), dtype=np.int64), z, z))
        else:
            mv, cost, zero = search(pic, out[-1][0], R, lam)
            out.append(T.step(pic, compensate(out[-1][0], mv), tab, tnr[2]) + (mv, cost, zero))
    return out


def totals(step, H, W):
    """(held, sad, moved, zero) of a step of run(): TnrFilter.totals()'s row."""
    return int(step[2].sum()), int(step[1].sum()), int((step[3] != 0).any(axis=2).sum()), int(step[5].sum())


def cells_with_a_pixel(H, W):
    return ((H + CELL - 1) // CELL) * ((W + CELL - 1) // CELL)


# ------------------------------------------------------------------------------------------------------------ pictures
CLIP_FRAMES, CLIP_SEED, OBJECT, OBJECT_AT, OBJECT_STEP, NOISE = 8, 7, 48, (2, 10), (2, 6), 4
CLIP_SIZE = (96, 128)


def clip(H, W, seed=CLIP_SEED):
    """(noisy (8, 3, H, W) float32, clean (8, 3, H, W) float32): a fixed camera over a static texture (independent uniform
    codes 51 .. 204 per sample) and a 48 x 48 object of a texture of its own whose top left corner stands at
    (2 + 2 t, 10 + 6 t) in picture t, clipped to the picture: an integer translation of (2, 6) a picture.  Every picture
    adds fresh independent integer noise of -4 .. 4 codes per sample, on the object as on the ground."""
    g = np.random.default_rng(seed)
    ground = g.integers(51, 205, (3, H, W))
    thing = g.integers(51, 205, (3, OBJECT, OBJECT))
    noisy, clean = np.empty((CLIP_FRAMES, 3, H, W), F32), np.empty((CLIP_FRAMES, 3, H, W), F32)
    for t in range(CLIP_FRAMES):
        pic = ground.copy()
        y, x = OBJECT_AT[0] + OBJECT_STEP[0] * t, OBJECT_AT[1] + OBJECT_STEP[1] * t
        part = pic[:, y:y + OBJECT, x:x + OBJECT]
        part[...] = thing[:, :part.shape[1], :part.shape[2]]
        clean[t] = pic.astype(F32) / F32(255.0)
        noisy[t] = (pic + g.integers(-NOISE, NOISE + 1, pic.shape)).astype(F32) / F32(255.0)
    return noisy, clean


def object_cells(t):
    """The (i, j) of the cells wholly inside the object in picture t of the 96 x 128 clip."""
    y, x = OBJECT_AT[0] + OBJECT_STEP[0] * t, OBJECT_AT[1] + OBJECT_STEP[1] * t
    return [(i, j) for i in range(CLIP_SIZE[0] // CELL) for j in range(CLIP_SIZE[1] // CELL)
            if y <= CELL * i and CELL * i + CELL <= y + OBJECT and x <= CELL * j and CELL * j + CELL <= x + OBJECT]


def grey(values):
    """(3, H, W) float32 with the three planes equal to the 8-bit codes `values`: Y is then the code itself."""
    pic = np.broadcast_to((np.asarray(values).astype(F32) / F32(255.0)).astype(F32), (3,) + np.shape(values)).copy()
    assert np.array_equal(luma(pic), values)
    return pic


def period4(H, W):
    """(cur, ref): columns of codes 40, 80, 120, 160 repeating, ref the same pattern two columns on: SAD is 0 at every even
    dx = 2 mod 4 inside the picture, so (0, -2) and (0, +2) tie in J and in length, and the smaller dx wins."""
    _, xx = np.mgrid[0:H, 0:W]
    return grey(40 * (1 + xx % 4)), grey(40 * (1 + (xx + 2) % 4))


def quadrants(H, W, R, seed=3):
    """(cur, ref, vectors): ref random grey codes, cur the same picture moved by another vector within +-min(R, 7) in each
    quadrant of the picture: cur(y, x) = ref(clamp(y + dy), clamp(x + dx)).  vectors: the four (dy, dx), quadrants in
    reading order.  A cell that lies in one quadrant with its moved copy inside the picture finds the vector at SAD 0."""
    g = np.random.default_rng(seed + 1000 * H + W)
    ref = g.integers(0, 256, (H, W))
    m = min(R, 7)
    vectors = [(-m, m - 1), (m, -m), (m - 2 if m > 2 else 1, m), (-1, -m)]
    yy, xx = np.mgrid[0:H, 0:W]
    q = 2 * (yy >= (H + 1) // 2) + (xx >= (W + 1) // 2)
    v = np.array(vectors)[q]
    cur = ref[np.clip(yy + v[..., 0], 0, H - 1), np.clip(xx + v[..., 1], 0, W - 1)]
    return grey(cur), grey(ref), vectors


def corner_pixels(H, W):
    """(cur, [ref, ...]): grey 128 against grey 128 with ONE pixel of 255 on each side of the corner where four cells meet
    (the picture's middle where it has no such corner): which cell's zero the pixel lands in, and which candidates see it
    through the window's edge, is decided at the cell line."""
    y, x = (CELL if H > CELL else H // 2), (CELL if W > CELL else W // 2)
    base = np.full((H, W), 128)
    refs = []
    for yy, xx in ((y - 1, x - 1), (y, x), (y - 1, x), (y, x - 1)):
        pic = base.copy()
        pic[min(max(yy, 0), H - 1), min(max(xx, 0), W - 1)] = 255
        refs.append(grey(pic))
    return grey(base), refs


def pairs(H, W, R):
    """name -> [(cur, ref)]: what the kernels are held against the restatement on."""
    noisy = clip(H, W)[0]
    flat = grey(np.full((H, W), 77))
    qc, qr, _ = quadrants(H, W, R)
    cc, crs = corner_pixels(H, W)
    zeros, ones = np.zeros((3, H, W), F32), np.ones((3, H, W), F32)
    return {"clip": [(noisy[5], noisy[4]), (noisy[6], noisy[5])], "flat": [(flat, flat.copy())], "period4": [period4(H, W)],
            "quadrants": [(qc, qr)], "flip": [(zeros, ones), (ones, zeros)], "corner": [(cc, r) for r in crs] + [(crs[0], cc)]}


def wild_vectors(H, W, seed=11):
    """(hc, wc, 2) int64: random vectors within +-32, and a few words far outside (the int16 range's ends among them) that
    only the clamp keeps inside the picture."""
    g = np.random.default_rng(seed + 1000 * H + W)
    hc, wc = grid(H, W)
    mv = g.integers(-MAX_R, MAX_R + 1, (hc, wc, 2))
    far = [(-32768, 32767), (32767, -32768), (500, -4), (-3, 20000), (0, 32764), (-32768, 0)]
    for n, v in enumerate(far):
        mv[(n * 5) % hc, (n * 3) % wc] = v
    return mv


def odd_bits(H, W, seed=13):
    """(3, H, W) float32 whose samples include NaNs with payloads (both signs, quiet and signalling), -0.0, infinities and
    denormals: compared as bit patterns."""
    g = np.random.default_rng(seed)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF80FFFF, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32)
    bits = g.integers(0x3A000000, 0x3F800000, (3, H, W)).astype(np.uint32)
    where = g.random((3, H, W)) < 0.3
    bits[where] = special[g.integers(0, len(special), int(where.sum()))]
    return bits.view(F32)
