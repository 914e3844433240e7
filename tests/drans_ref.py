"""Small synthetic CDF tables for the device entropy coder (include/dcvc_hip_rans.h), each named after the branch of
vcm_ts_amd/csrc/rans_device.hip it is for, and symbol lists that reach every bin of them by construction.  Every table
is valid in the sense of dcvc_drans_build_lut: rows start at 0, end at 65536 and have at least two non-empty bins.
numpy only; the expected bytes come from oracle/drans_py.py."""
import numpy as np

NAMES = ("flat", "wide", "tiny", "odd", "full", "one")


def _rows(rows, stride=None):
    """list of integer CDF rows -> (cdf (n, stride) int32 zero-padded, sizes int32)."""
    stride = stride or max(len(r) for r in rows)
    cdf = np.zeros((len(rows), stride), np.int32)
    for k, r in enumerate(rows):
        assert r[0] == 0 and r[-1] == 65536 and len(r) >= 3 and np.all(np.diff(r) >= 1), k
        cdf[k, :len(r)] = r
    return cdf, np.array([len(r) for r in rows], np.int32)


def _random_row(g, bins, last=None, conc=1.0):
    """bins widths >= 1 that add up to 65536 (Dirichlet-spread; conc << 1: a few wide bins and runs of width 1); the
    last bin (the sentinel's) has width `last` where given."""
    body = bins if last is None else bins - 1
    mass = 65536 - (last or 0) - body
    w = 1 + g.multinomial(mass, g.dirichlet(np.full(body, conc)))
    if last is not None:
        w = np.append(w, last)
    return np.concatenate([[0], np.cumsum(w)]).astype(np.int64)


def table(name):
    """-> (cdf int32 (rows, stride), sizes int32, offsets int32)."""
    g = np.random.default_rng(sorted(NAMES).index(name))
    if name == "flat":
        # 200 bins of width 1 in bucket 0 of the decoder's LUT, one of 65335, a sentinel of width 1: the LUT says bin 0
        # for every count below 256, the four probes reach bin 4 and the `while` loop walks the rest (203 entries: 202
        # bins whose widths add up to 65536)
        w = np.array([1] * 200 + [65335, 1])
        cdf, sizes = _rows([np.concatenate([[0], np.cumsum(w)])])
        return cdf, sizes, np.array([-100], np.int32)
    if name == "wide":
        # stride and size 256, the most the decoder takes: bins up to 254, so the LUT's bytes reach 254 (rows 0 and 1:
        # a sentinel at least 256 wide, so that bucket 255 starts inside it); row 1 has runs of width 1 (more than 4 bins
        # in a bucket), rows 2 and 3 a sentinel of width 1 and 2
        rows = [_random_row(g, 255, 300, 50.0), _random_row(g, 255, 256, 0.05), _random_row(g, 255, 1, 1.0),
                _random_row(g, 255, 2, 0.3)]
        cdf, sizes = _rows(rows, 256)
        return cdf, sizes, np.array([-127, -128, 0, 3], np.int32)
    if name == "tiny":
        # size 3: `size - 2 - s` is 0 or 1 and every probe index is clamped; widths 65535 and 1 either way round
        # (65536 wraps to 0 in the kernels' 16-bit image, and 65535 is the widest width they can hold)
        cdf, sizes = _rows([[0, 65535, 65536], [0, 1, 65536]])
        return cdf, sizes, np.array([0, -1], np.int32)
    if name == "odd":
        # 3 x 7 = 21 entries: five 16-byte groups and ONE scalar entry in load_tables, tab_halves rounds 21 up to 24
        cdf, sizes = _rows([_random_row(g, 6, 9), _random_row(g, 4, 700), [0, 40000, 65536]], 7)
        return cdf, sizes, np.array([-3, 2, -1], np.int32)
    if name == "full":
        # 256 x 128 = 32768 entries, the largest table accepted: 64 KB + 2 KB of LDS in the encoder, 130 KB with the
        # decoder's LUT.  Sizes 3..128 (mostly short, so that a list reaching every bin stays short), offsets -64..+5
        sizes = np.array([128 if r % 32 == 31 else 3 + r % 13 for r in range(256)])
        rows = [_random_row(g, int(s) - 1, int(g.choice([1, 2, 5, 300])), float(g.choice([0.1, 1.0, 20.0]))) for s in sizes]
        cdf, sizes = _rows(rows, 128)
        offsets = np.array([-64 if r % 32 == 31 else (r % 12) - 6 for r in range(256)], np.int32)
        assert offsets.min() == -64 and offsets.max() == 5
        return cdf, sizes, offsets
    if name == "one":
        cdf, sizes = _rows([_random_row(g, 11, 3)])   # n_cdfs == 1: the row index is always 0
        return cdf, sizes, np.array([-5], np.int32)
    raise KeyError(name)


def tables():
    return {n: table(n) for n in NAMES}


def escape_raws():
    """For nibble counts 1..8 and both signs the smallest and the largest escape value: raw in [2^(4(k-1)), 2^(4k)).
    The format folds the sign into the lowest bit (odd: below the row, raw = -2v - 1; even: above it,
    raw = 2 (v - sentinel)), so each sign takes the nearest value of its parity with the same nibble count, and the top
    case stops at 2^31 - 1 (odd) and 2^31 - 2 (even): every decoder reads the value as an int32.
    -> [(nibbles, raw)], raw = 0 (no nibble at all: v == sentinel) first."""
    out = [(0, 0)]
    for k in range(1, 9):
        lo, hi = 1 << (4 * (k - 1)), min((1 << (4 * k)) - 1, (1 << 31) - 1)
        odd = [lo | 1, hi]
        even = [lo if lo > 1 else 2, hi - 1]
        out += [(k, r) for r in sorted(set(odd + even))]
    return out


def nibbles(raw):
    return (int(raw).bit_length() + 3) // 4


def escape_symbol(raw, size, offset):
    """The symbol that a row of this size and offset codes as sentinel + `raw`."""
    sentinel = int(size) - 2
    v = -(raw + 1) // 2 if raw & 1 else sentinel + raw // 2
    return v + int(offset)


def classify(sym, idx, sizes, offsets):
    """-> (bin, raw): the bin every symbol is coded in (the sentinel for an escape) and its escape value (-1: none)."""
    v = np.asarray(sym, np.int64) - np.asarray(offsets, np.int64)[idx]
    sent = np.asarray(sizes, np.int64)[idx] - 2
    raw = np.where(v < 0, -2 * v - 1, np.where(v >= sent, 2 * (v - sent), -1))
    return np.where(raw >= 0, sent, v), raw


def covering_symbols(tab, seed=0, repeat=1):
    """(sym, idx) int32 in a shuffled order: every bin of every row at least `repeat` times, and per row escapes below
    (raw odd), above (raw even, > 0) and exactly at the sentinel (raw 0)."""
    _, sizes, offsets = tab
    sym, idx = [], []
    for r, (size, off) in enumerate(zip(sizes.tolist(), offsets.tolist())):
        sent = size - 2
        vs = list(range(sent)) * repeat + [sent, sent + 1 + r % 7, sent + 300 + r, -1, -2 - r % 5, -70000 - r]
        sym += [v + off for v in vs]
        idx += [r] * len(vs)
    p = np.random.default_rng(seed).permutation(len(sym))
    return np.array(sym, np.int32)[p], np.array(idx, np.int32)[p]


def assert_covered(sym, idx, tab):
    _, sizes, offsets = tab
    b, raw = classify(sym, idx, sizes, offsets)
    seen = set(zip(idx.tolist(), b.tolist()))
    want = {(r, s) for r, size in enumerate(sizes.tolist()) for s in range(size - 1)}
    assert seen == want, sorted(want - seen)[:5]
    for r in range(len(sizes)):
        rr = raw[idx == r]
        assert (rr == 0).any() and ((rr > 0) & (rr % 2 == 0)).any() and (rr % 2 == 1).any(), r


def lut_by_search(tab):
    """What dcvc_drans_build_lut owes: lut[row][b] = the bin that holds cumulative count b << 8."""
    cdf, sizes, _ = tab
    out = np.zeros((cdf.shape[0], 256), np.uint8)
    at = np.arange(256) << 8
    for r, size in enumerate(sizes.tolist()):
        out[r] = np.searchsorted(cdf[r, :size], at, side="right") - 1
    return out
