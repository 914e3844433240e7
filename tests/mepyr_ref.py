"""A numpy restatement of include/dcvc_hip_mepyr.h, written from its text (not from the kernels or the module): the levels,
the coarse search, the two descents, search() that chains them, a stream filtered with this search in front of
tests/tnr_ref.py's step -- and the fast clip, the pictures the hierarchical search is for.  Integer work is int64."""
import numpy as np

from tests import me_ref as M
from tests import tnr_ref as T
from tests.pixel_ref import grid, luma

F32 = np.float32
CELL, MAX_LAMBDA, FAR = 16, 255, 32
RANGES = {1: (2, 64), 2: (4, 128)}  # levels -> R's range
BIG = 1 << 12  # (more than any vector component or length: the key's digits)


def level_up(y):
    """The next level of the (H, W) int64 level y: (a + b + c + d + 2) >> 2 over rows min(2 y + {0, 1}, H - 1) and columns
    min(2 x + {0, 1}, W - 1)."""
    H, W = y.shape
    ya, yb = np.minimum(2 * np.arange((H + 1) // 2), H - 1), np.minimum(2 * np.arange((H + 1) // 2) + 1, H - 1)
    xa, xb = np.minimum(2 * np.arange((W + 1) // 2), W - 1), np.minimum(2 * np.arange((W + 1) // 2) + 1, W - 1)
    return (y[ya][:, xa] + y[ya][:, xb] + y[yb][:, xa] + y[yb][:, xb] + 2) >> 2


def pyramid(pic, levels):
    """[Y_0, Y_1(, Y_2)] of a (3, H, W) float32 picture, int64 each."""
    out = [luma(np.asarray(pic, dtype=F32)).astype(np.int64)]
    for _ in range(levels):
        out.append(level_up(out[-1]))
    return out


def level_range(R, level):
    """R_level = ceil(R / 2^level)."""
    return -(-R // (1 << level))


def supports(H, W, level, coarse):
    """(y0, y1, x0, x1), each (hc, wc) int64: the rows [y0, y1) and columns [x0, x1) of every cell's support at `level`,
    intersected with the level; y1 = y0 = 0 for a cell that holds no pixel.  coarse at level 2: the 8 x 8 block centred on
    the cell, [4 i - 2, 4 i + 6); everywhere else the cell's own rows, [side i, side i + side), side = 16 >> level."""
    hc, wc = grid(H, W)
    HL, WL = H, W
    for _ in range(level):
        HL, WL = (HL + 1) // 2, (WL + 1) // 2
    side = CELL >> level
    size, lead = (8, 2) if coarse and level == 2 else (side, 0)
    ii, jj = np.mgrid[0:hc, 0:wc]
    live = (CELL * ii < H) & (CELL * jj < W)
    y0, x0 = np.maximum(side * ii - lead, 0), np.maximum(side * jj - lead, 0)
    y1, x1 = np.minimum(side * ii - lead + size, HL), np.minimum(side * jj - lead + size, WL)
    return tuple(np.where(live, a, 0) for a in (y0, y1, x0, x1))


def support_sums(d, sup):
    """(hc, wc) int64: the sum of the (HL, WL) array d over every cell's support (an integral image)."""
    y0, y1, x0, x1 = sup
    s = np.zeros((d.shape[0] + 1, d.shape[1] + 1), np.int64)
    s[1:, 1:] = d.cumsum(0).cumsum(1)
    return s[y1, x1] - s[y0, x1] - s[y1, x0] + s[y0, x0]


def _moved(yr, dy, dx):
    """Y(ref, clamp(y + dy), clamp(x + dx)) for per-pixel (or scalar) dy, dx."""
    H, W = yr.shape
    yy, xx = np.mgrid[0:H, 0:W]
    return yr[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]


def _key(J, dy, dx):
    """The key (J, |dy| + |dx|, dy, dx) as one integer that orders as the tuple does."""
    return ((J * BIG + np.abs(dy) + np.abs(dx)) * BIG + dy + BIG // 2) * BIG + dx + BIG // 2


def coarse_sads(cur, ref, R, levels):
    """{(dy, dx): (hc, wc) int64 SAD of every cell's support} of the coarse search of two pictures: what the penalties share."""
    H, W = np.shape(cur)[1:]
    yc, yr = pyramid(cur, levels)[levels], pyramid(ref, levels)[levels]
    RL, sup = level_range(R, levels), supports(H, W, levels, True)
    edge = np.pad(yr, RL, mode="edge")  # (edge[y + RL, x + RL] = Y_L(ref, clamp(y), clamp(x)) for every y, x within RL of the level)
    HL, WL = yc.shape
    return {(dy, dx): support_sums(np.abs(yc - edge[RL + dy:RL + dy + HL, RL + dx:RL + dx + WL]), sup) for dy, dx in M.candidates(RL)}


def coarse(table, H, W, R, lam, levels):
    """(hc, wc, 2) int64: the level-`levels` vectors of the coarse search of an H x W picture; table: coarse_sads()."""
    RL, sup, mul = level_range(R, levels), supports(H, W, levels, True), 2 if levels == 1 else 1
    live = sup[1] > sup[0]
    best = np.full(live.shape, np.iinfo(np.int64).max, dtype=np.int64)
    mv = np.zeros(live.shape + (2,), dtype=np.int64)
    for dy, dx in M.candidates(RL):  # (in the order of the rest of the key: only a strictly smaller J replaces)
        J = mul * table[dy, dx] + lam * (abs(dy) + abs(dx))
        better = live & (J < best)
        best[better] = J[better]
        mv[better] = (dy, dx)
    return mv


def descend(yc, yr, H, W, R, lam, level, p):
    """(mv (hc, wc, 2), cost (hc, wc), zero (hc, wc)) of the descent to `level` (1 or 0) from the vectors p of the level
    above, on that level's lumas: the candidates clamp(2 p + e, -R_level, R_level), e in {-E .. E}^2 with E = 2 at level 0
    and 1 at level 1, and (0, 0)."""
    RL, E, mul, side = level_range(R, level), 2 if level == 0 else 1, 1 if level == 0 else 2, CELL >> level
    sup = supports(H, W, level, False)
    live = sup[1] > sup[0]
    HL, WL = yc.shape
    yy, xx = np.mgrid[0:HL, 0:WL]
    cell = (yy // side, xx // side)
    cands = [(np.clip(2 * p[..., 0] + ey, -RL, RL), np.clip(2 * p[..., 1] + ex, -RL, RL)) for ey in range(-E, E + 1) for ex in range(-E, E + 1)]
    cands.append((np.zeros_like(p[..., 0]), np.zeros_like(p[..., 1])))
    sads = [support_sums(np.abs(yc - _moved(yr, dy[cell], dx[cell])), sup) for dy, dx in cands]
    keys = np.stack([_key(mul * s + lam * (np.abs(dy) + np.abs(dx)), dy, dx) for s, (dy, dx) in zip(sads, cands)])
    pick = keys.argmin(axis=0)[None]
    mv = np.stack([np.take_along_axis(np.stack([c[k] for c in cands]), pick, 0)[0] for k in range(2)], axis=-1)
    cost = np.take_along_axis(np.stack(sads), pick, 0)[0]
    return np.where(live[..., None], mv, 0), np.where(live, cost, 0), np.where(live, sads[-1], 0)


def stages(cur, ref, R, lam, levels, table=None):
    """Every stage of the search: [the vectors of level `levels`, ..., of level 1, (mv, cost, zero) of level 0]; table:
    coarse_sads(cur, ref, R, levels) where the caller has it already."""
    lo, hi = RANGES[levels]
    assert lo <= R <= hi and 0 <= lam <= MAX_LAMBDA
    H, W = np.shape(cur)[1:]
    pc, pr = pyramid(cur, levels), pyramid(ref, levels)
    out = [coarse(coarse_sads(cur, ref, R, levels) if table is None else table, H, W, R, lam, levels)]
    for level in range(levels - 1, 0, -1):
        out.append(descend(pc[level], pr[level], H, W, R, lam, level, out[-1])[0])
    out.append(descend(pc[0], pr[0], H, W, R, lam, 0, out[-1]))
    return out


def search(cur, ref, R, lam, levels):
    """(mv (hc, wc, 2) int64, cost (hc, wc) int64, zero (hc, wc) int64): what the chain writes in place of dcvc_me_search."""
    return stages(cur, ref, R, lam, levels)[-1]


def run(pics, tnr, intra, R, lam, levels):
    """tests/me_ref.py's run() with this search in place of the full search: [(the picture the codec is handed, sad, held,
    mv, cost, zero)]."""
    tab, out = T.table(tnr[0], tnr[1]), []
    hc, wc = grid(*pics[0].shape[1:])
    z = np.zeros((hc, wc), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), z, z, np.zeros((hc, wc, 2), dtype=np.int64), z, z))
        else:
            mv, cost, zero = search(pic, out[-1][0], R, lam, levels)
            out.append(T.step(pic, M.compensate(out[-1][0], mv), tab, tnr[2]) + (mv, cost, zero))
    return out


def far(mv):
    """The cells whose vector has a component beyond 32."""
    return int((np.abs(mv) > FAR).any(axis=-1).sum())


def totals(step, H, W):
    """(held, sad, moved, zero, far) of a step of run(): TnrFilter(levels=...).totals()'s row."""
    return M.totals(step, H, W) + (far(step[3]),)


def run_refined(pics, tnr, intra, R, lam, levels):
    """tests/mesplit_ref.py's run() with subpel and split behind THIS search (R <= 32): [(the picture the codec is handed,
    sad, held, mvq, cost, zero, mv8, cost8, mv)], mv the whole-pixel vectors the chain wrote."""
    from tests import mesplit_ref as P
    from tests import mesub_ref as S

    tab, out = T.table(tnr[0], tnr[1]), []
    hc, wc = grid(*pics[0].shape[1:])
    z, z2 = np.zeros((hc, wc), dtype=np.int64), np.zeros((hc, wc, 2), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), z, z, z2, z, z, np.zeros((2 * hc, 2 * wc, 2), dtype=np.int64),
                        np.zeros((2 * hc, 2 * wc), dtype=np.int64), z2))
            continue
        ref = out[-1][0]
        mv, _, zero = search(pic, ref, R, lam, levels)
        mvq, cost = S.refine(pic, ref, lam, mv)
        mv8, cost8 = P.split(pic, ref, lam, mvq, 4)
        out.append(T.step(pic, P.compensate_split(ref, mv8), tab, tnr[2]) + (mvq, cost, zero, mv8, cost8, mv))
    return out


def run_intra(pics, tnr, intra, K, R, lam, levels):
    """tests/tnr_fuse_ref.py's run() with this search: [(the picture the codec is handed, sad, held, number of references,
    moved, zero, far)]; every reference of an I picture is searched for from the I SOURCE, a P picture's reference is the
    previous handed picture; moved, zero and far are those of reference 0."""
    from tests import tnr_fuse_ref as FR

    tab, out = T.table(tnr[0], tnr[1]), []
    zeros = np.zeros(grid(*pics[0].shape[1:]), dtype=np.int64)

    def moved_onto(cur, ref):
        mv, _, zero = search(cur, ref, R, lam, levels)
        return M.compensate(ref, mv), int((mv != 0).any(axis=2).sum()), int(zero.sum()), far(mv)

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


# ------------------------------------------------------------------------------------------------------------ pictures
# The fast clip: tests/mesub_ref.py's clip construction (six sinusoids a colour plane, amplitude 10 .. 25 codes, rounded,
# kept within 4 .. 251, fresh integer noise of -4 .. 4 codes on every sample of every picture; drawn from default_rng(7): the
# ground's texture, then the object's, then the noise picture by picture) with BAND-LIMITED texture, frequencies uniform in
# 0.02 .. 0.08 cycles a pixel, at 128 x 320, five pictures, and a 48 x 48 object that moves `step` whole pixels a picture
# from (2, 10) -- from (60, 10) where step's dy is negative.
FAST_FRAMES, FAST_SEED, FAST_SIZE, OBJECT, NOISE, WAVES, FREQ = 5, 7, (128, 320), 48, 4, 6, (0.02, 0.08)
FAST_STEPS = ((6, 50), (3, 61), (-5, 39))
SETTING, PENALTY = (12, 64, 36), 4


def _texture(g, freq):
    return [[(g.uniform(10, 25), g.uniform(*freq) * g.choice((-1, 1)), g.uniform(*freq) * g.choice((-1, 1)), g.uniform(0, 2 * np.pi))
             for _ in range(WAVES)] for _ in range(3)]


def _evaluate(texture, yy, xx):
    return np.stack([128.0 + sum(a * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph) for a, fy, fx, ph in plane) for plane in texture])


def object_at(step, t):
    return (60 if step[0] < 0 else 2) + t * step[0], 10 + t * step[1]


def fast_clip(step, freq=FREQ):
    """(noisy (5, 3, 128, 320) float32, clean (5, 3, 128, 320) float32) with the object moving by `step` = (dy, dx) whole
    pixels a picture."""
    H, W = FAST_SIZE
    g = np.random.default_rng(FAST_SEED)
    ground_tex, thing_tex = _texture(g, freq), _texture(g, freq)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ground = _evaluate(ground_tex, yy, xx)
    noisy, clean = np.empty((FAST_FRAMES, 3, H, W), F32), np.empty((FAST_FRAMES, 3, H, W), F32)
    for t in range(FAST_FRAMES):
        oy, ox = object_at(step, t)
        inside = (yy >= oy) & (yy < oy + OBJECT) & (xx >= ox) & (xx < ox + OBJECT)
        pic = np.clip(np.rint(np.where(inside[None], _evaluate(thing_tex, yy - oy, xx - ox), ground)), NOISE, 255 - NOISE).astype(np.int64)
        clean[t] = pic.astype(F32) / F32(255.0)
        noisy[t] = (pic + g.integers(-NOISE, NOISE + 1, pic.shape)).astype(F32) / F32(255.0)
    return noisy, clean


def _cells(pred):
    return [(i, j) for i in range(FAST_SIZE[0] // CELL) for j in range(FAST_SIZE[1] // CELL) if pred(CELL * i, CELL * j)]


def object_cells(step, t):
    """The (i, j) of the cells wholly inside the object in picture t of fast_clip(step)."""
    oy, ox = object_at(step, t)
    return _cells(lambda y, x: oy <= y and y + CELL <= oy + OBJECT and ox <= x and x + CELL <= ox + OBJECT)


def untouched_cells(step, t):
    """The (i, j) of the cells the object touches neither in picture t nor in picture t - 1."""
    def clear(y, x, s):
        oy, ox = object_at(step, s)
        return y + CELL <= oy or y >= oy + OBJECT or x + CELL <= ox or x >= ox + OBJECT
    return _cells(lambda y, x: clear(y, x, t) and clear(y, x, t - 1))


def random_planes(H, W, level, seed=29):
    """(cur, ref) int64 byte planes of `level` of an H x W picture: ref random codes, cur a smoothed copy moved a little, so
    that SADs differ and some vectors are found far out."""
    g = np.random.default_rng(seed + 1000 * H + W + level)
    for _ in range(level):
        H, W = (H + 1) // 2, (W + 1) // 2
    ref = g.integers(0, 256, (H, W))
    cur = np.clip(_moved(ref, 1, -2) + g.integers(-6, 7, (H, W)), 0, 255)
    return cur, ref


def wild_vectors(H, W, bound, seed=31):
    """(hc, wc, 2) int64: random vectors within +-bound and a few words far outside (the int16 range's ends among them) that
    only the clamps bound."""
    g = np.random.default_rng(seed + 1000 * H + W)
    hc, wc = grid(H, W)
    mv = g.integers(-bound, bound + 1, (hc, wc, 2))
    rows, cols = -(-H // CELL), -(-W // CELL)  # (the cells that hold a pixel)
    far_words = [(-32768, 32767), (32767, -32768), (500, -4), (-3, 20000), (0, 32764), (-32768, 0), (16384, -16384)]
    for n, v in reversed(list(enumerate(far_words))):
        at = (n * 3) % (rows * cols)
        mv[at // cols, at % cols] = v
    return mv
