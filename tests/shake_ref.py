"""include/dcvc_hip_shake.h restated in numpy, written from its text (not from the kernels or the module): the anchor plane,
the tile search by brute force over the candidates in the order of their keys, the vote, the registered picture through
tests/me_ref.py's compensation, and the two integer host functions of vcm_ts_amd/shake.py (summary, border_cells -- the
module's own are imported by the tests only to be compared with these).  And the clip the tests measure: a camera that
shakes by whole pixels over a band-limited textured ground with a moving object and sensor noise.  Integer work is int64."""
import numpy as np

from tests import me_ref as ME
from tests.pixel_ref import code, grid, luma  # noqa: F401 (re-exported)

F32 = np.float32
TILE, ROWS, MAX_R, MAX_TILES, FEW, EDGE = 64, 16, 16, 16384, 1, 2


# ------------------------------------------------------------------------------------------------------ the header
def plane(pic):
    """(H, W) int64: what dcvc_shake_plane writes below column W."""
    return luma(np.asarray(pic, dtype=F32))


def candidates(R):
    """Every (dy, dx) within +-R, sorted by (|dy| + |dx|, dy, dx): of equal SAD the first of these wins."""
    return ME.candidates(R)


def tile_sads(cur, anchor, R):
    """{(dy, dx): (th, tw) int64 SAD of every tile}: the sixteen rows 64 a + 4 i of cur's luma against the anchor plane at
    clamped coordinates."""
    yc, ya = plane(cur), np.asarray(anchor, dtype=np.int64)
    H, W = yc.shape
    th, tw = H // TILE, W // TILE
    edge = np.pad(ya, R, mode="edge")  # (edge[y + R, x + R] = anchor(clamp(y), clamp(x)) for every y, x within R of the picture)
    out = {}
    for dy, dx in candidates(R):
        d = np.abs(yc[0:TILE * th:4, :TILE * tw] - edge[R + dy:R + dy + TILE * th:4, R + dx:R + dx + TILE * tw])
        out[dy, dx] = d.reshape(th, ROWS, tw, TILE).sum(axis=(1, 3))
    return out


def tiles(cur, anchor, R):
    """(th * tw, 5) int64: dy, dx, the SAD of the choice, the largest SAD, SAD(0, 0) of every tile."""
    assert 1 <= R <= MAX_R
    table = tile_sads(cur, anchor, R)
    zero = table[0, 0]
    best, top = np.full(zero.shape, 1 << 40, dtype=np.int64), np.zeros(zero.shape, dtype=np.int64)
    mv = np.zeros(zero.shape + (2,), dtype=np.int64)
    for dy, dx in candidates(R):  # (in the order of the rest of the key: only a strictly smaller SAD replaces)
        s = table[dy, dx]
        better = s < best
        best[better] = s[better]
        mv[better] = (dy, dx)
        top = np.maximum(top, s)
    return np.concatenate([mv.reshape(-1, 2), best.reshape(-1, 1), top.reshape(-1, 1), zero.reshape(-1, 1)], axis=1)


def lower_median(values):
    """The element of rank (n - 1) // 2 in ascending order; 0 of nothing."""
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2] if v else 0


def vote(tile_words, R, min_votes):
    """[dy, dx, n, agree, n_tiles, status, my, mx] of (n_tiles, 5) tile words."""
    t = np.asarray(tile_words, dtype=np.int64).reshape(-1, 5)
    voting = t[(np.abs(t[:, 0]) <= R) & (np.abs(t[:, 1]) <= R) & (t[:, 3] > 0) & (2 * t[:, 2] <= t[:, 3])]
    n = len(voting)
    my, mx = lower_median(voting[:, 0]), lower_median(voting[:, 1])
    agree = int(((voting[:, 0] == my) & (voting[:, 1] == mx)).sum())
    status = (FEW if n < min_votes else 0) | (EDGE if abs(my) == R or abs(mx) == R else 0)
    return [0 if status else my, 0 if status else mx, n, agree, len(t), status, my, mx]


def field(record, H, W):
    """(hc, wc, 2) int64: (-dy, -dx) in every cell."""
    hc, wc = grid(H, W)
    return np.broadcast_to(np.array([-record[0], -record[1]], dtype=np.int64), (hc, wc, 2)).copy()


def register(pic, record):
    """out(y, x) = pic(clamp(y - dy), clamp(x - dx)): dcvc_me_compensate with the uniform field."""
    pic = np.asarray(pic, dtype=F32)
    return ME.compensate(pic, field(record, *pic.shape[1:]))


def run(pics, R, min_votes=8):
    """(records (n, 8) int64, the registered pictures): picture 0 is the anchor, untouched, its record zero but n_tiles."""
    H, W = pics[0].shape[1:]
    anchor = plane(pics[0])
    records, out = [[0, 0, 0, 0, (H // TILE) * (W // TILE), 0, 0, 0]], [np.asarray(pics[0], dtype=F32)]
    for pic in pics[1:]:
        records.append(vote(tiles(pic, anchor, R), R, min_votes))
        out.append(register(pic, records[-1]))
    return np.array(records, dtype=np.int64), out


# ---------------------------------------------------------------------------------------------------- host functions
def summary(log):
    """What shake.summary(log) must say.  min_agree: the smallest agree / votes over the pictures after the anchor that
    have a vote at all, as the pair [agree, votes] of the first such picture ([0, 0] where there is none)."""
    log = np.asarray(log, dtype=np.int64).reshape(-1, 8)
    worst = [0, 0]
    for dy, dx, n, agree, *_ in log[1:].tolist():
        if n > 0 and (worst[1] == 0 or agree * worst[1] < worst[0] * n):
            worst = [agree, n]
    return {"pictures": len(log), "moved": int(((log[:, 0] != 0) | (log[:, 1] != 0)).sum()), "lost": int((log[:, 5] != 0).sum()),
            "max_dy": int(np.abs(log[:, 0]).max(initial=0)), "max_dx": int(np.abs(log[:, 1]).max(initial=0)), "min_agree": worst}


def border_cells(dy, dx, H, W):
    """(hc, wc) bool: the cells that hold a pixel of the replicated band of a picture registered by (dy, dx): rows [0, dy)
    or [H + dy, H), columns [0, dx) or [W + dx, W)."""
    yy, xx = np.mgrid[0:H, 0:W]
    band = (yy < dy) | (yy >= H + dy) | (xx < dx) | (xx >= W + dx)
    hc, wc = grid(H, W)
    full = np.zeros((hc * 16, wc * 16), dtype=bool)
    full[:H, :W] = band
    return full.reshape(hc, 16, wc, 16).any(axis=(1, 3))


def masked_counts(counts, log, H, W):
    """The (n, hc, wc) counts of a motion scan with every picture's border cells zeroed."""
    out = np.array(counts, dtype=np.int64)
    for t, rec in enumerate(np.asarray(log).reshape(-1, 8).tolist()):
        out[t][border_cells(rec[0], rec[1], H, W)] = 0
    return out


def document(log, R, min_votes, max_lost, H, W):
    """What shake.json and `run_codec shake` hold."""
    log = np.asarray(log, dtype=np.int64).reshape(-1, 8)
    return {"version": 1, "height": H, "width": W, "params": {"radius": R, "min_votes": min_votes, "max_lost": max_lost},
            "records": log.tolist(), "summary": summary(log)}


# -------------------------------------------------------------------------------------------------------- the clip
MARGIN = 16
OBJECT, OBJECT_AT, OBJECT_STEP = (48, 64), (8, 10), (3, 7)


def shifts(n, limit, seed=3):
    """n whole-pixel (sy, sx) drawn uniformly from -limit .. limit per axis; picture 0 stands still."""
    g = np.random.default_rng(seed)
    return [(0, 0)] + [tuple(int(v) for v in g.integers(-limit, limit + 1, 2)) for _ in range(n - 1)]


def clip(H=128, W=192, moves=None, n=6, s=2.0, obj=OBJECT, seed=7, freq=(0.02, 0.08), flat_half=False, gain=False):
    """(n, 3, H, W) float32 of exact 8-bit samples: the world is a ground of 24 cosines of random direction and phase at
    `freq` cycles a pixel, about +-50 codes of luma around 128 and COLOURED as tests/noise_ref.py's ground is (for its
    reason), generated with a 16-pixel margin so that a shift shows real content; an object of uniformly random codes, the
    same in every picture, that starts at OBJECT_AT and moves OBJECT_STEP a picture in the world; picture t is the world
    seen from (sy, sx) = moves[t]: pic(y, x) = world(y + sy, x + sx), so the header's vector of picture t against picture 0
    is moves[t].  moves=None: a still camera.  Then, per picture, gain in 0.85 .. 1.15 around 128 and an offset within +-12
    codes (gain=True), and independent Gaussian noise of `s` codes on R, G and B.  flat_half: the right half of the world is
    one grey.  obj: (height, width) or None."""
    moves = [(0, 0)] * n if moves is None else list(moves)
    assert moves[0] == (0, 0) and all(max(abs(a), abs(b)) <= MARGIN for a, b in moves)
    g = np.random.default_rng(seed)
    Hw, Ww = H + 2 * MARGIN, W + 2 * MARGIN
    yy, xx = np.mgrid[0:Hw, 0:Ww].astype(np.float64)
    f = g.uniform(freq[0], freq[1], 24)
    th, ph = g.uniform(0.0, 2.0 * np.pi, 24), g.uniform(0.0, 2.0 * np.pi, 24)
    tex = 128.0 + 6.0 * sum(np.cos(2.0 * np.pi * fk * (np.cos(tk) * xx + np.sin(tk) * yy) + pk) for fk, tk, pk in zip(f, th, ph))
    dr, db = 30.0 * (xx / (Ww - 1) - 0.5), 40.0 * (yy / (Hw - 1) - 0.5)
    world = np.stack([tex + dr, tex - (54.0 * dr + 19.0 * db) / 183.0, tex + db])
    if flat_half:
        world[:, :, Ww // 2:] = 128.0
    thing = np.random.default_rng(seed + 1000).integers(0, 256, size=(3,) + tuple(obj)).astype(np.float64) if obj is not None else None
    noise = np.random.default_rng(seed + 2000)
    out = np.empty((len(moves), 3, H, W), dtype=F32)
    for t, (sy, sx) in enumerate(moves):
        seen = world.copy()
        if obj is not None:
            y0, x0 = MARGIN + OBJECT_AT[0] + OBJECT_STEP[0] * t, MARGIN + OBJECT_AT[1] + OBJECT_STEP[1] * t
            part = seen[:, y0:y0 + obj[0], x0:x0 + obj[1]]
            part[...] = thing[:, :part.shape[1], :part.shape[2]]
        pic = seen[:, MARGIN + sy:MARGIN + sy + H, MARGIN + sx:MARGIN + sx + W]
        if gain and t:
            pic = 128.0 + noise.uniform(0.85, 1.15) * (pic - 128.0) + noise.uniform(-12.0, 12.0)
        if s:
            pic = pic + noise.normal(0.0, s, size=pic.shape)
        out[t] = np.clip(np.rint(pic), 0, 255).astype(np.int64).astype(F32) / F32(255.0)  # (through integers: no -0.0)
    return out


# the six conditions of the README's table: name -> clip keywords
CONDITIONS = {
    "base": {},
    "fine": {"freq": (0.08, 0.16)},
    "noise8": {"s": 8.0},
    "flat-half": {"flat_half": True},
    "gain": {"gain": True},
    "large-object": {"obj": None},  # (replaced per size: a quarter of the picture)
}


def condition(name, H, W, moves):
    kw = dict(CONDITIONS[name])
    if name == "large-object":
        kw["obj"] = (H // 2, W // 2)
    return clip(H, W, moves, **kw)
