"""include/dcvc_hip_deint.h restated in numpy: the motion-adaptive deinterlacer of vcm_ts_amd/deint.py and csrc/deint.hip,
which the GPU tests hold the kernel against bit for bit, and the clips the tests run it on.

    plane(prev, cur, nxt, parity, second, depth)      one plane: (the output plane, the mask of samples with diff > 0)
    frame(prev, cur, nxt, parity, second, depth)      one (Y, U, V) frame: (the output frame, moved per band of 8 luma rows)
    parity_of(order, second), needs(g, n, mode), pictures_of(n, mode), picture(frames, g, mode, order, depth)
    interlace(pics, order)                            progressive pictures, one per field time, woven into frames
    i420(frame), planes_of(buf, H, W)                 a frame <-> the file's sample order
    clip / static_clip / moving_clip                  the test material

A frame is a tuple (Y, U, V) of 2-D unsigned integer arrays, chroma at half size.  Everything is computed in int64.
"""
import numpy as np

BAND = 8  # DCVC_DEINT_BAND
MODES, ORDERS = ("frame", "field"), ("tff", "bff")


def field_row(q, PH):
    """A row index outside 0 .. PH - 1 -> the nearest row inside that has its parity."""
    q = np.asarray(q)
    return np.where(q < 0, q & 1, np.where(q > PH - 1, PH - 2 + (q & 1), q))


def plane(prev, cur, nxt, parity, second, depth):
    PH = cur.shape[0]
    assert PH % 2 == 0 and prev.shape == cur.shape == nxt.shape
    P, C, N = (np.asarray(a).astype(np.int64) for a in (prev, cur, nxt))
    r = np.arange(1 - parity, PH, 2)
    c, e, c3, e3 = (C[field_row(r + k, PH)] for k in (-1, 1, -3, 3))
    A, B = (P[r], C[r]) if second == 0 else (C[r], N[r])
    d, td0 = (A + B) >> 1, np.abs(A - B)
    td1 = (np.abs(P[field_row(r - 1, PH)] - c) + np.abs(P[field_row(r + 1, PH)] - e)) >> 1
    td2 = (np.abs(N[field_row(r - 1, PH)] - c) + np.abs(N[field_row(r + 1, PH)] - e)) >> 1
    diff = np.maximum(td0 >> 1, np.maximum(td1, td2))
    pred = np.clip((9 * (c + e) - (c3 + e3) + 8) >> 4, 0, (1 << depth) - 1)
    out = np.array(cur, copy=True)
    out[r] = np.minimum(np.maximum(pred, d - diff), d + diff).astype(out.dtype)
    moved = np.zeros(cur.shape, dtype=bool)
    moved[r] = diff > 0
    return out, moved


def frame(prev, cur, nxt, parity, second, depth):
    done = [plane(p, c, n, parity, second, depth) for p, c, n in zip(prev, cur, nxt)]
    luma = done[0][1]
    H = luma.shape[0]
    moved = np.array([int(luma[b:b + BAND].sum()) for b in range(0, H, BAND)], dtype=np.int64)
    return tuple(o for o, _ in done), moved


def parity_of(order, second):
    assert order in ORDERS
    return second if order == "tff" else 1 - second


def pictures_of(n_frames, mode):
    return n_frames if mode == "frame" else 2 * n_frames


def needs(g, n_frames, mode):
    """(the file frames n - 1, n, n + 1 with a frame outside the file replaced by n, second) of output picture g."""
    n, second = (g, 0) if mode == "frame" else (g // 2, g % 2)
    return (n - 1 if n > 0 else n, n, n + 1 if n + 1 < n_frames else n), second


def picture(frames, g, mode, order, depth):
    (a, n, b), second = needs(g, len(frames), mode)
    return frame(frames[a], frames[n], frames[b], parity_of(order, second), second, depth)


def interlace(pics, order):
    """pics[t]: the progressive picture at field time t -> frames, frame n woven from pics[2 n] and pics[2 n + 1]."""
    assert len(pics) % 2 == 0
    out = []
    for n in range(len(pics) // 2):
        p0 = parity_of(order, 0)
        fr = []
        for early, late in zip(pics[2 * n], pics[2 * n + 1]):
            w = np.array(early, copy=True)
            w[1 - p0::2] = late[1 - p0::2]
            fr.append(w)
        out.append(tuple(fr))
    return out


def i420(fr):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in fr])


def planes_of(buf, H, W):
    n = H * W
    return buf[:n].reshape(H, W), buf[n:n + n // 4].reshape(H // 2, W // 2), buf[n + n // 4:n + n // 2].reshape(H // 2, W // 2)


# ------------------------------------------------------------------------------------------------------------ material
def random_frame(rng, H, W, depth):
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(rng.integers(0, 1 << depth, size=s, dtype=np.int64).astype(dt) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))


def _texture(y, x, seed, lo=0.03, hi=0.16, terms=6):
    """A band-limited texture in 0 .. 1 at real coordinates: a few sinusoids of lo .. hi cycles a pixel."""
    rng = np.random.default_rng(seed)
    v = np.zeros(np.broadcast(y, x).shape)
    for _ in range(terms):
        f, th, ph = rng.uniform(lo, hi), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v = v + np.cos(2 * np.pi * f * (np.cos(th) * x + np.sin(th) * y) + ph)
    return 0.5 + v / (2.6 * terms)


def _sampled(H, W, depth, ground_seed, obj, seed, t):
    """The (Y, U, V) picture at field time t: a static textured ground, and on it obj = (y0, x0, h, w, dy, dx): a textured
    box of h x w pixels whose corner is at (y0 + t dy, x0 + t dx), carrying its own texture with it."""
    dt, peak = (np.uint8 if depth == 8 else np.uint16), (1 << depth) - 1
    out = []
    for k, sub in enumerate((1, 2, 2)):
        y, x = np.mgrid[0:H // sub, 0:W // sub].astype(np.float64) * sub
        v = _texture(y, x, ground_seed + k)
        if obj is not None:
            y0, x0, h, w, dy, dx = obj
            oy, ox = y0 + t * dy, x0 + t * dx
            inside = (y >= oy) & (y < oy + h) & (x >= ox) & (x < ox + w)
            v = np.where(inside, _texture(y - oy, x - ox, seed + k), v)
        out.append(np.clip(np.rint(v * peak), 0, peak).astype(dt))
    return tuple(out)


def clip(H, W, n_fields, obj, depth=8, seed=11):
    """Progressive pictures, one per field time: a static textured ground and obj = (y0, x0, h, w, dy, dx), a textured box
    that moves (dy, dx) pixels a field (None: the ground alone)."""
    return [_sampled(H, W, depth, seed, obj, seed + 100, t) for t in range(n_fields)]


def static_clip(H, W, n_fields, depth=8, seed=3):
    pic = _sampled(H, W, depth, seed, None, 0, 0)
    return [pic for _ in range(n_fields)]


MOVING = {"size": (96, 128), "fields": 8, "box": (24, 16, 32, 40), "steps": ((1, 3), (3, 8), (0.5, 0.75))}


def moving_clip(step, depth=8, seed=11):
    """(pics, boxes): MOVING's clip with the object moving `step` = (dy, dx) pixels a field; boxes[t] = the object's box
    at field time t as whole pixels (y1, x1, y2, x2), rounded outward."""
    (H, W), (y0, x0, h, w) = MOVING["size"], MOVING["box"]
    pics = clip(H, W, MOVING["fields"], (y0, x0, h, w) + tuple(step), depth, seed)
    boxes = [(int(np.floor(y0 + t * step[0])), int(np.floor(x0 + t * step[1])), int(np.ceil(y0 + t * step[0] + h)),
              int(np.ceil(x0 + t * step[1] + w))) for t in range(MOVING["fields"])]
    return pics, boxes


def striped_frame(H, W, depth, phase=0):
    """Vertical stripes that drive pred outside 0 .. max before the clip: along a field's rows the pattern 0, max, max, 0
    (rows r +- 1 at one extreme and rows r +- 3 at the other: (18 max + 8) >> 4 > max, (-2 max + 8) >> 4 < 0), flipped from
    column to column."""
    dt, peak = (np.uint8 if depth == 8 else np.uint16), (1 << depth) - 1
    out = []
    for sub in (1, 2, 2):
        y, x = np.mgrid[0:H // sub, 0:W // sub]
        j = (y // 2 + phase) % 4
        out.append((((j == 1) | (j == 2)) ^ (x % 2 == 1)).astype(dt) * dt(peak))
    return tuple(out)
