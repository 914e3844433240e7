"""A numpy restatement of include/dcvc_hip_mesplit.h, written from its text (not from the kernels or the module): the
re-selection of a vector per 8 x 8 sub-cell among its cell's and the eight neighbours', by brute force over the distinct
candidates, the compensation PER PIXEL by the vector of the pixel's sub-cell, a stream filtered with both in front of
tests/tnr_ref.py's step -- and, kept only so that the figures of DESIGN.md stay reproducible, the overlapped-block blend that
was measured and rejected.  Integer work is int64."""
import numpy as np

from tests import me_ref as M
from tests import mesub_ref as S
from tests import tnr_ref as T
from tests.pixel_ref import code, grid, luma  # noqa: F401 (the tests use them as R.grid, ...)

F32 = np.float32
CELL, SUB, MAX_R = 16, 8, M.MAX_R
LIMIT = {1: MAX_R, 4: 4 * MAX_R + 3}  # unit -> what a word of mv_in is clamped to


def sub_grid(H, W):
    hc, wc = grid(H, W)
    return 2 * hc, 2 * wc


def quarters(mv_in, unit):
    """mv_in clamped and in quarter pixels, (hc, wc, 2) int64."""
    assert unit in LIMIT
    return np.clip(np.asarray(mv_in, dtype=np.int64), -LIMIT[unit], LIMIT[unit]) * (4 // unit)


def candidates(q, i, j, rows, cols):
    """The distinct candidates of the sub-cells of cell (i, j): the vectors of the cells around it that hold a pixel."""
    return sorted({tuple(int(v) for v in q[min(max(i + di, 0), rows - 1), min(max(j + dj, 0), cols - 1)]) for di in (-1, 0, 1) for dj in (-1, 0, 1)})


def sad8_table(cur, ref, mv_in, unit):
    """{sub-cell (a, b) that holds a pixel: {(vy, vx): SAD8}} over the sub-cell's distinct candidates."""
    yc, yr = luma(np.asarray(cur, dtype=F32)), luma(np.asarray(ref, dtype=F32))
    H, W = yc.shape
    q = quarters(mv_in, unit)
    rows, cols = -(-H // CELL), -(-W // CELL)
    out = {}
    for a in range(-(-H // SUB)):
        for b in range(-(-W // SUB)):
            ys, xs = np.arange(SUB * a, min(SUB * a + SUB, H)), np.arange(SUB * b, min(SUB * b + SUB, W))
            block = yc[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            out[a, b] = {v: int(np.abs(block - S.interp_luma(yr, ys, xs, *v)).sum()) for v in candidates(q, a >> 1, b >> 1, rows, cols)}
    return out


def split(cur, ref, lam, mv_in, unit, table=None):
    """(mv8 (hs, ws, 2) int64 in quarter pixels, cost8 (hs, ws) int64) of one dcvc_me_split; table: sad8_table(cur, ref,
    mv_in, unit) where the caller has it already."""
    assert 0 <= lam <= M.MAX_LAMBDA
    hs, ws = sub_grid(*np.shape(cur)[1:])
    table = sad8_table(cur, ref, mv_in, unit) if table is None else table
    mv8, cost8 = np.zeros((hs, ws, 2), dtype=np.int64), np.zeros((hs, ws), dtype=np.int64)
    for (a, b), sads in table.items():
        key = min((4 * sad + lam * (abs(v[0]) + abs(v[1])), abs(v[0]) + abs(v[1]), v[0], v[1]) for v, sad in sads.items())
        mv8[a, b], cost8[a, b] = key[2:], sads[key[2:]]
    return mv8, cost8


def _fold(x, taps):
    """a = t0 x0, a = a + tk xk in increasing offset along the LAST axis, every product and every sum rounded to float32."""
    t = [F32(k) / F32(64.0) for k in taps]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = t[0] * x[..., 0]
        for k in range(1, len(taps)):
            a = a + t[k] * x[..., k]
    assert a.dtype == F32
    return a


def move_pixels(ref, field):
    """(3, H, W) float32: every pixel moved by ITS OWN quarter-pel vector field[y, x] = (vy, vx), as the header's
    compensation defines it for one pixel.  (Pixels are gathered by the value of their vector only to let numpy work on
    arrays: each keeps its own clamped taps.)"""
    ref = np.asarray(ref, dtype=F32)
    _, H, W = ref.shape
    field = np.asarray(field, dtype=np.int64)
    out = np.empty_like(ref)
    for vy, vx in {tuple(int(c) for c in v) for v in field.reshape(-1, 2)}:
        ys, xs = np.nonzero((field[..., 0] == vy) & (field[..., 1] == vx))
        (iy, py), (ix, px) = S.split(vy), S.split(vx)
        (oy, ty), (ox, tx) = S.FILTERS[py], S.FILTERS[px]
        rows = np.clip(ys[:, None] + iy + oy + np.arange(len(ty))[None, :], 0, H - 1)  # (n, taps of py): clamped per tap
        cols = np.clip(xs[:, None] + ix + ox + np.arange(len(tx))[None, :], 0, W - 1)  # (n, taps of px)
        g = ref[:, rows[:, :, None], cols[:, None, :]]                                  # (3, n, ty, tx): the bits
        if py == 0 and px == 0:
            out[:, ys, xs] = g[:, :, 0, 0]
            continue
        h = g[..., 0] if px == 0 else _fold(g, tx)    # (3, n, ty)
        a = h[..., 0] if py == 0 else _fold(h, ty)    # (3, n)
        a = np.fmin(np.fmax(a, F32(0)), F32(1))       # (fmaxf / fminf: a NaN gives the other operand)
        out[:, ys, xs] = np.where(a == 0, F32(0), a)  # (a zero of either sign is +0)
    return out


def per_pixel(vectors, H, W, side):
    """(H, W, 2): the vector of the side x side block that holds each pixel."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.asarray(vectors, dtype=np.int64)[yy // side, xx // side]


def compensate_split(ref, mv8):
    """(3, H, W) float32 of one dcvc_me_compensate_split; mv8 is (hs, ws, 2) of any int16 values."""
    _, H, W = np.shape(ref)
    return move_pixels(ref, per_pixel(mv8, H, W, SUB))


def repeated(mvq):
    """(hs, ws, 2): every cell's vector in its four sub-cells."""
    return np.repeat(np.repeat(np.asarray(mvq, dtype=np.int64), 2, axis=0), 2, axis=1)


def left(mv8, own, H, W):
    """The sub-cells that hold a pixel and whose vector differs from their cell's `own` (hc, wc, 2), quarter pixels."""
    return int((mv8 != repeated(own)).any(axis=2)[:-(-H // SUB), :-(-W // SUB)].sum())


def _moved_onto(cur, ref, R, lam, subpel, split_):
    """(comp, mvq of the cells in quarter pixels, cost, zero, mv8, cost8) of one reference moved onto cur."""
    mv, cost, zero = M.search(cur, ref, R, lam)
    mvq = 4 * mv
    if subpel:
        mvq, cost = S.refine(cur, ref, lam, mv)
    if not split_:
        return (S.compensate_sub(ref, mvq) if subpel else M.compensate(ref, mv)), mvq, cost, zero, repeated(mvq), None
    mv8, cost8 = split(cur, ref, lam, mvq if subpel else mv, 4 if subpel else 1)
    return compensate_split(ref, mv8), mvq, cost, zero, mv8, cost8


def run(pics, tnr, intra, R, lam, subpel=True, split_=True):
    """[(the picture the codec is handed, sad, held, mvq, cost, zero, mv8, cost8)] of a stream filtered with the search,
    with subpel the refinement, and with split_ the re-selection per sub-cell: tests/mesub_ref.py's run with two more
    entries (mv8 is the cells' vectors repeated and cost8 None without split_)."""
    tab, out = T.table(tnr[0], tnr[1]), []
    hc, wc = grid(*pics[0].shape[1:])
    z = np.zeros((hc, wc), dtype=np.int64)
    for t, pic in enumerate(pics):
        if t in intra:
            out.append((np.asarray(pic, dtype=F32), z, z, np.zeros((hc, wc, 2), dtype=np.int64), z, z, np.zeros((2 * hc, 2 * wc, 2), dtype=np.int64),
                        np.zeros((2 * hc, 2 * wc), dtype=np.int64)))
            continue
        moved = _moved_onto(pic, out[-1][0], R, lam, subpel, split_)
        out.append(T.step(pic, moved[0], tab, tnr[2]) + moved[1:])
    return out


def totals(step, H, W, subpel=True):
    """(held, sad, moved, zero, [frac,] split) of a step of run(): TnrFilter(split=True).totals()'s row."""
    frac = (int(((step[3] & 3) != 0).any(axis=2).sum()),) if subpel else ()
    return (int(step[2].sum()), int(step[1].sum()), int((step[3] != 0).any(axis=2).sum()), int(step[5].sum())) + frac + (left(step[6], step[3], H, W),)


def run_intra(pics, tnr, intra, K, R, lam, subpel=True):
    """[(the picture the codec is handed, sad, held, number of references, moved, zero, [frac,] split)] of a stream with
    the look-ahead filter (tests/tnr_fuse_ref.py's run) and the re-selection: every reference of an I picture is searched
    for from the I SOURCE, refined with subpel, re-selected per sub-cell and moved before the fusion, a P picture's
    reference is the previous handed picture treated the same way; moved, zero, frac and split are those of reference 0."""
    from tests import tnr_fuse_ref as FR

    tab, out = T.table(tnr[0], tnr[1]), []
    H, W = pics[0].shape[1:]
    zeros = np.zeros(grid(H, W), dtype=np.int64)

    def moved_onto(cur, ref):
        comp, mvq, _, zero, mv8, _ = _moved_onto(cur, ref, R, lam, subpel, True)
        frac = (int(((mvq & 3) != 0).any(axis=2).sum()),) if subpel else ()
        return (comp, int((mvq != 0).any(axis=2).sum()), int(zero.sum())) + frac + (left(mv8, mvq, H, W),)

    for t, pic in enumerate(pics):
        if t in intra:
            ahead = FR.ahead_of(t, len(pics), intra, K)
            if ahead:
                refs = [moved_onto(pic, pics[s]) for s in ahead]
                out.append(FR.fuse(pic, [r[0] for r in refs], tab, tnr[2]) + (len(ahead),) + refs[0][1:])
            else:
                out.append((np.asarray(pic, dtype=F32), zeros, zeros, 0, 0, 0) + ((0,) if subpel else ()) + (0,))
        else:
            ref = moved_onto(pic, out[-1][0])
            out.append(T.step(pic, ref[0], tab, tnr[2]) + (1,) + ref[1:])
    return out


# ------------------------------------------------------------------------------------------------------------ the clip
def edge_cells(step, t, size=S.CLIP_SIZE):
    """The (i, j) of the cells of picture t of mesub_ref.subpel_clip(step) whose overlap with the object is neither 0 nor
    256 pixels."""
    y0, x0 = int(np.ceil(S.OBJECT_AT[0] + step[0] * t)), int(np.ceil(S.OBJECT_AT[1] + step[1] * t))
    out = []
    for i in range(size[0] // CELL):
        for j in range(size[1] // CELL):
            oy = max(0, min(CELL * i + CELL, y0 + S.OBJECT, size[0]) - max(CELL * i, y0))
            ox = max(0, min(CELL * j + CELL, x0 + S.OBJECT, size[1]) - max(CELL * j, x0))
            if 0 < oy * ox < CELL * CELL:
                out.append((i, j))
    return out


def overlapped(ref, mvq):
    """The overlapped-block compensation that was MEASURED AND REJECTED, kept so that its figures can be reproduced: a
    32 x 32 linear window around every cell.  Per axis a pixel at position p = 0 .. 15 of its cell gives its own cell's
    prediction the weight (17 + 2 min(p, 15 - p)) / 32 and the nearer neighbour's (the cell before for p < 8, after
    otherwise, clamped to the cells that hold a pixel) the rest; the four predictions -- the picture moved by the own, the
    vertical, the horizontal and the diagonal neighbour's vector, each as the header's compensation moves a pixel -- are
    blended with the products of the two axes' weights in float64 and rounded to float32."""
    ref = np.asarray(ref, dtype=F32)
    _, H, W = ref.shape
    mvq = np.asarray(mvq, dtype=np.int64)
    rows, cols = -(-H // CELL), -(-W // CELL)
    yy, xx = np.mgrid[0:H, 0:W]

    def axis(n, limit):
        p = n % CELL
        own = (17 + 2 * np.minimum(p, 15 - p)) / 32.0
        return n // CELL, np.clip(n // CELL + np.where(p < 8, -1, 1), 0, limit - 1), own

    ci, ni, wy = axis(yy, rows)
    cj, nj, wx = axis(xx, cols)
    out = np.zeros(ref.shape, dtype=np.float64)
    for i, a in ((ci, wy), (ni, 1 - wy)):
        for j, b in ((cj, wx), (nj, 1 - wx)):
            out += (a * b)[None] * move_pixels(ref, mvq[i, j]).astype(np.float64)
    return out.astype(F32)


def run_overlapped(pics, tnr, intra, R, lam):
    """[the picture the codec would have been handed] with the search, the refinement and `overlapped` in place of the
    compensation."""
    tab, out = T.table(tnr[0], tnr[1]), []
    for t, pic in enumerate(pics):
        if t in intra:
            out.append(np.asarray(pic, dtype=F32))
            continue
        mvq, _ = S.refine(pic, out[-1], lam, M.search(pic, out[-1], R, lam)[0])
        out.append(T.step(pic, overlapped(out[-1], mvq), tab, tnr[2])[0])
    return out


def sub_vectors(H, W, seed=29, whole=0.0):
    """(hs, ws, 2) int64: random quarter-pel vectors per SUB-cell within +-131 with the int16 range's ends and other far
    words among them; `whole`: the fraction of sub-cells whose vector is made whole."""
    g = np.random.default_rng(seed + 1000 * H + W)
    hs, ws = sub_grid(H, W)
    mv8 = g.integers(-4 * MAX_R - 3, 4 * MAX_R + 4, (hs, ws, 2))
    mv8[g.random((hs, ws)) < whole] &= ~3
    far = [(-32768, 32767), (32767, -32768), (2001, -4), (-3, 20000)]
    rows, cols = -(-H // SUB), -(-W // SUB)  # (the sub-cells that hold a pixel)
    for n, v in reversed(list(enumerate(far))):  # (where two land in one sub-cell the earlier stays)
        at = (n * 3) % (rows * cols)
        mv8[at // cols, at % cols] = v
    return mv8


def distinct_vectors(H, W):
    """(hc, wc, 2) int64 quarter-pel vectors, no two cells alike: every cell's nine candidates differ (where the grid has
    as many cells).  Whole and fractional, within +-131."""
    hc, wc = grid(H, W)
    n = np.arange(hc * wc).reshape(hc, wc)
    return np.stack([(n * 7) % 263 - 131, (n * 11 + 5) % 257 - 128], axis=2).astype(np.int64)
