"""numpy / pure-Python restatement of rate control for the tests: the ladder sweep of
include/dcvc_hip_bits.h -- float32 division, np.rint, counting the bin edges <= the scale, the cost rule of
tests/bitmap_ref.py -- and the controller's rule, written from the rule's text.  Shares no code with vcm_ts_amd/ratectl.py
or the kernels.  Slow on purpose (one Python step per symbol): small inputs only."""
from fractions import Fraction

import numpy as np

from tests import bitmap_ref as B

BAD_INDEX, BAD_VALUE = 1, 4


def factor(h):
    """The float32 factor of `h` hundredths."""
    return np.float32(h) / np.float32(100)


def row_of(scale, edges):
    """The number of the first 255 edges that are <= scale (the 256th is +inf and is not counted)."""
    return int(np.count_nonzero(np.asarray(edges, dtype=np.float32)[:255] <= np.float32(scale)))


def candidate(res, sc, h, edges):
    """(symbol, row) of one element for a step `h` hundredths as large, or None when the quotient is no int32."""
    f = factor(h)
    q = np.float32(res) / f
    if not abs(q) < np.float32(2147483648.0):
        return None
    return int(np.rint(q)), row_of(np.float32(sc) / f, edges)


def sweep(res, sc, edges, hundredths, table, N, stats=None):
    """(est (N, K) int64 in 2^-16 bit, status) of the planes res, sc (anything of N * per float32 values).  stats: a dict
    that receives "candidates", "escapes", "nibbles" (set), "signs" (set of the escapes' signs), "sentinel_only",
    "below_lowest_edge"."""
    cdf, sizes, offsets = table
    res = np.asarray(res, dtype=np.float32).reshape(N, -1)
    sc = np.asarray(sc, dtype=np.float32).reshape(N, -1)
    first = np.asarray(edges, dtype=np.float32)[:255]
    est = np.zeros((N, len(hundredths)), dtype=np.int64)
    status = 0
    st = dict(candidates=0, escapes=0, nibbles=set(), signs=set(), sentinel_only=0, below_lowest_edge=0)
    with np.errstate(all="ignore"):
        quot = np.stack([res / factor(h) for h in hundredths])                                  # float32 divisions
        rows = np.stack([(first[None, None, :] <= (sc / factor(h))[:, :, None]).sum(axis=2) for h in hundredths])
        good = np.isfinite(res) & np.isfinite(sc) & (np.abs(quot) < np.float32(2147483648.0)).all(axis=0)
        syms = np.rint(np.where(good[None], quot, 0)).astype(np.int64)
    if not good.all():
        status |= BAD_VALUE
    for n in range(N):
        for e in np.flatnonzero(good[n]):
            for k in range(len(hundredths)):
                sym, row = int(syms[k, n, e]), int(rows[k, n, e])
                if not 0 <= row < len(sizes) or not 2 <= sizes[row] <= cdf.shape[1]:
                    status |= BAD_INDEX
                    continue
                cost, records = B.symbol_cost(cdf, sizes, offsets, row, sym)
                est[n, k] += cost
                st["candidates"] += 1
                st["below_lowest_edge"] += row == 0
                st["sentinel_only"] += sizes[row] == 2
                if records > 1:
                    st["escapes"] += 1
                    st["nibbles"].add(records - 2)
                    st["signs"].add(-1 if sym - int(offsets[row]) < 0 else 1)
    if stats is not None:
        stats.update(st)
    return est, status


# ------------------------------------------------------------------------------------------------------- the controller
def _interp(xs, ys, x):
    """Piecewise linear through (xs, ys), constant outside."""
    if x <= xs[0]:
        return ys[0]
    if x >= xs[-1]:
        return ys[-1]
    for a in range(len(xs) - 1):
        if xs[a] <= x <= xs[a + 1]:
            t = (x - xs[a]) / (xs[a + 1] - xs[a])
            return ys[a] * (1 - t) + ys[a + 1] * t
    raise AssertionError


def _invert(xs, ys, y):
    """The x of the first segment (ascending) whose ends bracket y; else the end with the nearer y, ties to the end
    nearer x = 1, then to the lower end."""
    for a in range(len(xs) - 1):
        y0, y1 = ys[a], ys[a + 1]
        if (y0 <= y <= y1) or (y1 <= y <= y0):
            if y0 == y:
                return xs[a]
            return xs[a] + (xs[a + 1] - xs[a]) * (y - y0) / (y1 - y0)
    d0, d1 = abs(ys[0] - y), abs(ys[-1] - y)
    if d0 < d1:
        return xs[0]
    if d1 < d0:
        return xs[-1]
    return xs[-1] if abs(xs[-1] - 1) < abs(xs[0] - 1) else xs[0]


def next_q(b, G, q_range, ladder, q_start, qs, As, Es, j):
    """(q index, budget or None) of P picture j of a GOP (0 is its I picture) from the history: qs[0 .. j-1] the q
    indexes so far, As[0 .. j-2] the actual bits, Es[0 .. j-2] the sweep rows (None for the I picture)."""
    if j <= 2:
        return q_start, None
    s = j - 2
    ms = [Fraction(h, 100) for h in ladder]
    at_one = Es[s][list(ladder).index(100)]
    Ts = [As[s] + Fraction(e - at_one, 65536) for e in Es[s]]
    assumed = _interp(ms, Ts, Fraction(qs[j - 1], qs[s]))
    budget = (G * Fraction(b) - sum(As[: s + 1]) - assumed) / max(1, G - j)
    x = qs[s] * _invert(ms, Ts, budget)
    q = int((x + Fraction(1, 2)) // 1)
    return min(max(q, q_range[0]), q_range[1]), budget


def replay(b, G, q_range, ladder, q_start, log):
    """The decisions for one GOP's log [(q, A, budget, est row)]: [(q index, budget)] of its P pictures, each decided
    from the LOG's own earlier entries (the log's q of picture j - 1 included)."""
    qs, As, Es = [e[0] for e in log], [e[1] for e in log], [e[3] for e in log]
    return [next_q(b, G, q_range, ladder, q_start, qs[:j], As[: max(j - 1, 0)], Es[: max(j - 1, 0)], j) for j in range(1, len(log))]


def split_gops(log):
    """A picture-order log of several GOPs -> one log per GOP (an I picture has no sweep row)."""
    gops = []
    for entry in log:
        if entry[3] is None:
            gops.append([])
        gops[-1].append(entry)
    return gops
