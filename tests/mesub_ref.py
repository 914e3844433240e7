"""A numpy restatement of include/dcvc_hip_mesub.h, written from its text (not from the kernels or the module): the
interpolated luma, the refinement of whole-pel vectors to quarter pixels by brute force over the 49 candidates in the order
of their keys, the interpolating compensation in float32 operation by operation, a stream filtered with the search and the
refinement in front of tests/tnr_ref.py's step -- and the sub-pel clip the tests share.  Integer work is int64."""
import numpy as np

from tests import me_ref as M
from tests import tnr_ref as T
from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as R.grid, ...)

F32 = np.float32
CELL, MAX_R, UNIT = 16, M.MAX_R, 4
# phase -> (offset of the first tap, the taps); each sums to 64
FILTERS = {0: (0, (64,)), 1: (-3, (-1, 4, -10, 58, 17, -5, 1)), 2: (-3, (-1, 4, -11, 40, 40, -11, 4, -1)), 3: (-2, (1, -5, 17, 58, -10, 4, -1))}
assert all(sum(taps) == 64 for _, taps in FILTERS.values())
STEPS = tuple(range(-3, 4))  # f, per direction


def split(v):
    """(whole part, phase) of a quarter-pel component: v = 4 i + p, i the floor."""
    return int(v) >> 2, int(v) & 3


def interp_luma(yr, ys, xs, vy, vx):
    """YI at the pixels ys x xs (1-D integer arrays) of the (H, W) int64 luma yr for ONE vector: (len(ys), len(xs)) int64."""
    H, W = yr.shape
    (iy, py), (ix, px) = split(vy), split(vx)
    (oy, ty), (ox, tx) = FILTERS[py], FILTERS[px]
    rows = np.clip(np.asarray(ys)[:, None] + iy + oy + np.arange(len(ty))[None, :], 0, H - 1)  # (n, taps): clamped per tap
    cols = np.clip(np.asarray(xs)[:, None] + ix + ox + np.arange(len(tx))[None, :], 0, W - 1)
    h = (yr[rows[:, :, None, None], cols[None, None, :, :]] * np.array(tx, dtype=np.int64)).sum(axis=3)  # (n, taps, m)
    assert h.min() >= -32768 and h.max() <= 32767
    s = (h * np.array(ty, dtype=np.int64)[None, :, None]).sum(axis=1)
    return np.clip((s + 2048) >> 12, 0, 255)


def interp_picture(ref, vy, vx):
    """YI of the whole picture moved by one vector, (H, W) int64."""
    yr = luma(np.asarray(ref, dtype=F32))
    return interp_luma(yr, np.arange(yr.shape[0]), np.arange(yr.shape[1]), vy, vx)


def candidates(d):
    """The 49 (vy, vx) = 4 d + f around the whole-pel d, sorted by (|vy| + |vx|, vy, vx): of equal J the first wins."""
    return sorted(((4 * d[0] + fy, 4 * d[1] + fx) for fy in STEPS for fx in STEPS), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))


def _cell_pixels(i, j, H, W):
    return np.arange(CELL * i, min(CELL * i + CELL, H)), np.arange(CELL * j, min(CELL * j + CELL, W))


def sad_table(cur, ref, mv_in):
    """{cell (i, j) that holds a pixel: {(vy, vx): SAD}} for the 49 candidates around the clamped mv_in of the cell.  The
    seven horizontal positions are made once per cell, on the rows whose coordinates are already clamped: a vertical tap at
    the unclamped row c reads the horizontal result of row clamp(c), which is what clamping per tap means."""
    yc, yr = luma(np.asarray(cur, dtype=F32)), luma(np.asarray(ref, dtype=F32))
    H, W = yc.shape
    mv_in = np.asarray(mv_in, dtype=np.int64)
    out = {}
    for i in range(-(-H // CELL)):
        for j in range(-(-W // CELL)):
            ys, xs = _cell_pixels(i, j, H, W)
            d = tuple(int(v) for v in np.clip(mv_in[i, j], -MAX_R, MAX_R))
            block = yc[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            first = ys[0] + d[0] - 4  # every tap of every candidate reads a row within first .. first + 23
            rows = yr[np.clip(first + np.arange(CELL + 8), 0, H - 1)]
            sads = {}
            for fx in STEPS:
                (ix, px) = split(4 * d[1] + fx)
                ox, tx = FILTERS[px]
                cols = np.clip(xs[:, None] + ix + ox + np.arange(len(tx))[None, :], 0, W - 1)
                h = (rows[:, cols] * np.array(tx, dtype=np.int64)).sum(axis=2)  # (24, m)
                assert h.min() >= -32768 and h.max() <= 32767
                for fy in STEPS:
                    (iy, py) = split(4 * d[0] + fy)
                    oy, ty = FILTERS[py]
                    at = ys[:, None] + iy + oy + np.arange(len(ty))[None, :] - first  # (n, taps), within 0 .. 23
                    assert at.min() >= 0 and at.max() < CELL + 8
                    s = (h[at] * np.array(ty, dtype=np.int64)[None, :, None]).sum(axis=1)
                    sads[4 * d[0] + fy, 4 * d[1] + fx] = int(np.abs(block - np.clip((s + 2048) >> 12, 0, 255)).sum())
            out[i, j] = sads
    return out


def refine(cur, ref, lam, mv_in, table=None):
    """(mvq (hc, wc, 2) int64 in quarter pixels, cost (hc, wc) int64) of one dcvc_me_refine; table: sad_table(cur, ref,
    mv_in) where the caller has it already."""
    assert 0 <= lam <= M.MAX_LAMBDA
    H, W = np.shape(cur)[1:]
    hc, wc = grid(H, W)
    table = sad_table(cur, ref, mv_in) if table is None else table
    mvq, cost = np.zeros((hc, wc, 2), dtype=np.int64), np.zeros((hc, wc), dtype=np.int64)
    for (i, j), sads in table.items():
        best = None
        for v in sorted(sads, key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1])):  # (only a strictly smaller J replaces)
            J = 4 * sads[v] + lam * (abs(v[0]) + abs(v[1]))
            if best is None or J < best:
                best, mvq[i, j], cost[i, j] = J, v, sads[v]
    return mvq, cost


def _fold(x, taps, axis):
    """The fp32 fold of a pass: a = t0 x0, a = a + tk xk in increasing offset, every product and sum rounded to float32;
    x holds the taps' samples along `axis`."""
    x = np.moveaxis(x, axis, 0)
    t = [F32(k) / F32(64.0) for k in taps]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = t[0] * x[0]
        for k in range(1, len(taps)):
            a = a + t[k] * x[k]
    assert a.dtype == F32
    return a


def compensate_sub(ref, mvq):
    """(3, H, W) float32 of one dcvc_me_compensate_sub; mvq is (hc, wc, 2) of any int16 values."""
    ref = np.asarray(ref, dtype=F32)
    _, H, W = ref.shape
    mvq = np.asarray(mvq, dtype=np.int64)
    out = np.empty_like(ref)
    for i in range(-(-H // CELL)):
        for j in range(-(-W // CELL)):
            ys, xs = _cell_pixels(i, j, H, W)
            (iy, py), (ix, px) = split(mvq[i, j, 0]), split(mvq[i, j, 1])
            (oy, ty), (ox, tx) = FILTERS[py], FILTERS[px]
            rows = np.clip(ys[:, None] + iy + oy + np.arange(len(ty))[None, :], 0, H - 1)  # (n, taps of py)
            cols = np.clip(xs[:, None] + ix + ox + np.arange(len(tx))[None, :], 0, W - 1)  # (m, taps of px)
            g = ref[:, rows[:, :, None, None], cols[None, None, :, :]]                     # (3, n, ty, m, tx): the bits
            where = (slice(None), slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
            if py == 0 and px == 0:
                out[where] = g[:, :, 0, :, 0]
                continue
            h = g[..., 0] if px == 0 else _fold(g, tx, 4)       # (3, n, ty, m)
            a = h[:, :, 0, :] if py == 0 else _fold(h, ty, 2)   # (3, n, m)
            a = np.fmin(np.fmax(a, F32(0)), F32(1))             # (fmaxf / fminf: a NaN gives the other operand)
            out[where] = np.where(a == 0, F32(0), a)            # (a zero of either sign is +0)
    return out


def run(pics, tnr, intra, R, lam, subpel=True):
    """[(the picture the codec is handed, sad, held, mvq, cost, zero)] of a stream filtered with the search and, with
    subpel, the refinement: as tests/me_ref.py's run, the vectors in QUARTER pixels (4 mv without subpel, where the
    compensation is me_ref's)."""
    tab, out = T.table(tnr[0], tnr[1]), []
    hc, wc = grid(*pics[0].shape[1:])
    z = np.zeros((hc, wc), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), z, z, np.zeros((hc, wc, 2), dtype=np.int64), z, z))
            continue
        mv, cost, zero = M.search(pic, out[-1][0], R, lam)
        if subpel:
            mvq, cost = refine(pic, out[-1][0], lam, mv)
            comp = compensate_sub(out[-1][0], mvq)
        else:
            mvq, comp = 4 * mv, M.compensate(out[-1][0], mv)
        out.append(T.step(pic, comp, tab, tnr[2]) + (mvq, cost, zero))
    return out


def run_intra(pics, tnr, intra, K, R, lam):
    """[(the picture the codec is handed, sad, held, number of references, moved, zero, frac)] of a stream with the
    look-ahead filter (tests/tnr_fuse_ref.py's run) and quarter-pel motion: every reference of an I picture is searched for
    from the I SOURCE, refined and interpolated before the fusion, a P picture's reference is the previous handed picture
    treated the same way; moved, zero and frac are those of reference 0."""
    from tests import tnr_fuse_ref as FR

    tab, out = T.table(tnr[0], tnr[1]), []
    zeros = np.zeros(grid(*pics[0].shape[1:]), dtype=np.int64)

    def moved_onto(cur, ref):
        mv, _, zero = M.search(cur, ref, R, lam)
        mvq, _ = refine(cur, ref, lam, mv)
        return compensate_sub(ref, mvq), int((mvq != 0).any(axis=2).sum()), int(zero.sum()), int(((mvq & 3) != 0).any(axis=2).sum())

    for t, pic in enumerate(pics):
        if t in intra:
            ahead = FR.ahead_of(t, len(pics), intra, K)
            if ahead:
                refs = [moved_onto(pic, pics[s]) for s in ahead]
                out.append(FR.fuse(pic, [r[0] for r in refs], tab, tnr[2]) + (len(ahead),) + refs[0][1:])
            else:
                out.append((np.asarray(pic, dtype=F32), zeros, zeros, 0, 0, 0, 0))
        else:
            ref = moved_onto(pic, out[-1][0])
            out.append(T.step(pic, ref[0], tab, tnr[2]) + (1,) + ref[1:])
    return out


def totals(step, H, W):
    """(held, sad, moved, zero, frac) of a step of run(): TnrFilter(subpel=True).totals()'s row."""
    return (int(step[2].sum()), int(step[1].sum()), int((step[3] != 0).any(axis=2).sum()), int(step[5].sum()),
            int(((step[3] & 3) != 0).any(axis=2).sum()))


# ------------------------------------------------------------------------------------------------------------ pictures
# The sub-pel clip: 96 x 128, eight pictures, a smooth 48 x 48 object on a smooth ground, fresh integer noise of -4 .. 4
# codes on every sample of every picture.  A texture is, per colour plane, 128 + the sum of six sinusoids
# A sin(2 pi (fy y + fx x) + phase) with A uniform in 10 .. 25 codes, fy and fx uniform in 0.08 .. 0.16 cycles per pixel with
# a random sign each, phase uniform in 0 .. 2 pi, drawn from numpy's default_rng(CLIP_SEED) -- the ground's first, then the
# object's, then the noise picture by picture -- evaluated at real coordinates, rounded to 8-bit codes and kept within
# 4 .. 251 (so that the noise never leaves 0 .. 255; at 96 x 128 nothing is cut).  The object's
# texture is evaluated at (y - oy, x - ox) with the corner (oy, ox) = OBJECT_AT + t * step, a REAL number of pixels: the
# object covers the pixels y in [ceil(oy), ceil(oy) + 48), x in [ceil(ox), ceil(ox) + 48).
CLIP_FRAMES, CLIP_SEED, CLIP_SIZE, OBJECT, OBJECT_AT, NOISE, WAVES = 8, 7, (96, 128), 48, (2, 10), 4, 6
SETTING, SEARCH, PENALTY = (12, 64, 36), 8, 4


def _texture(g):
    return [[(g.uniform(10, 25), g.uniform(0.08, 0.16) * g.choice((-1, 1)), g.uniform(0.08, 0.16) * g.choice((-1, 1)), g.uniform(0, 2 * np.pi))
             for _ in range(WAVES)] for _ in range(3)]


def _evaluate(texture, yy, xx):
    return np.stack([128.0 + sum(a * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph) for a, fy, fx, ph in plane) for plane in texture])


def subpel_clip(step, seed=CLIP_SEED, size=CLIP_SIZE):
    """(noisy (8, 3, H, W) float32, clean (8, 3, H, W) float32) with the object moving by `step` = (dy, dx) pixels a picture."""
    H, W = size
    g = np.random.default_rng(seed)
    ground_tex, thing_tex = _texture(g), _texture(g)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ground = _evaluate(ground_tex, yy, xx)
    noisy, clean = np.empty((CLIP_FRAMES, 3, H, W), F32), np.empty((CLIP_FRAMES, 3, H, W), F32)
    for t in range(CLIP_FRAMES):
        oy, ox = OBJECT_AT[0] + step[0] * t, OBJECT_AT[1] + step[1] * t
        y0, x0 = int(np.ceil(oy)), int(np.ceil(ox))
        inside = (yy >= y0) & (yy < y0 + OBJECT) & (xx >= x0) & (xx < x0 + OBJECT)
        pic = np.clip(np.rint(np.where(inside[None], _evaluate(thing_tex, yy - oy, xx - ox), ground)), NOISE, 255 - NOISE).astype(np.int64)
        clean[t] = pic.astype(F32) / F32(255.0)
        noisy[t] = (pic + g.integers(-NOISE, NOISE + 1, pic.shape)).astype(F32) / F32(255.0)
    return noisy, clean


def object_cells(step, t, size=CLIP_SIZE):
    """The (i, j) of the cells wholly inside the object in picture t of subpel_clip(step)."""
    y0, x0 = int(np.ceil(OBJECT_AT[0] + step[0] * t)), int(np.ceil(OBJECT_AT[1] + step[1] * t))
    return [(i, j) for i in range(size[0] // CELL) for j in range(size[1] // CELL)
            if y0 <= CELL * i and CELL * i + CELL <= y0 + OBJECT and x0 <= CELL * j and CELL * j + CELL <= x0 + OBJECT]


def ground_cells(step, size=CLIP_SIZE):
    """The (i, j) of the cells no pixel of which the object comes within SEARCH + 4 pixels of in any picture."""
    lo = [int(np.ceil(OBJECT_AT[k])) for k in range(2)]
    hi = [int(np.ceil(OBJECT_AT[k] + step[k] * (CLIP_FRAMES - 1))) + OBJECT for k in range(2)]
    m = SEARCH + 4
    return [(i, j) for i in range(size[0] // CELL) for j in range(size[1] // CELL)
            if CELL * i + CELL + m <= lo[0] or CELL * i - m >= hi[0] or CELL * j + CELL + m <= lo[1] or CELL * j - m >= hi[1]]


def relative_error(got, noisy, clean, cells):
    """The squared error of `got` to the clean picture over the cells, as a fraction of the noisy source's."""
    def sse(a):
        return sum(float(((a[:, CELL * i:CELL * i + CELL, CELL * j:CELL * j + CELL].astype(np.float64)
                           - clean[:, CELL * i:CELL * i + CELL, CELL * j:CELL * j + CELL]) ** 2).sum()) for i, j in cells)
    return sse(got) / sse(noisy)


def shifted_pair(H, W, v, seed=17):
    """(cur, ref) grey pictures: ref a smooth random texture of 8-bit codes, cur the restatement's own interpolation of
    ref moved by the quarter-pel vector v = (vy, vx): YI(ref, y, x, vy, vx) in every pixel."""
    g = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    tex = 128.0 + sum(g.uniform(10, 25) * np.sin(2 * np.pi * (g.uniform(0.05, 0.12) * g.choice((-1, 1)) * yy + g.uniform(0.05, 0.12) * xx)
                                                 + g.uniform(0, 6.28)) for _ in range(6))  # (both diagonals: no direction is ambiguous)
    ref = M.grey(np.rint(tex).astype(np.int64))
    return M.grey(interp_picture(ref, *v)), ref


def random_quarters(H, W, seed=19):
    """(hc, wc, 2) int64: random quarter-pel vectors within +-(4 * 32 + 3), every phase pair among them where the grid is
    large enough."""
    g = np.random.default_rng(seed + 1000 * H + W)
    hc, wc = grid(H, W)
    mvq = g.integers(-4 * MAX_R - 3, 4 * MAX_R + 4, (hc, wc, 2))
    for n in range(min(16, hc * wc)):  # (the cells in reading order take the 16 phase pairs from (1, 2) on, small whole parts)
        q = (n + 6) % 16
        mvq.reshape(-1, 2)[n] = (4 * int(g.integers(-2, 3)) + q // 4, 4 * int(g.integers(-2, 3)) + q % 4)
    return mvq


def far_quarters(H, W, seed=23):
    """Quarter-pel vectors with the int16 range's ends and other far words among them, fractional and whole."""
    mvq = random_quarters(H, W, seed)
    hc, wc = grid(H, W)
    far = [(-32768, 32767), (32767, -32768), (-32767, 2), (1, 32766), (2001, -4), (-3, 20000), (0, 32764), (-32768, 0)]
    rows, cols = -(-H // CELL), -(-W // CELL)  # (the cells that hold a pixel)
    for n, v in reversed(list(enumerate(far))):  # (where two land in one cell the earlier stays: the first in cell (0, 0))
        at = (n * 3) % (rows * cols)
        mvq[at // cols, at % cols] = v
    return mvq
