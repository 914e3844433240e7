"""numpy / pure-Python restatement of include/dcvc_hip_bits.h for the tests: the cost LUT through math.log2 per frequency,
the cost of one symbol with its escapes, the plane-to-map sums and the region sums.  Shares no code with
vcm_ts_amd/bitmap.py or the kernels.  Slow on purpose (one Python step per symbol): small inputs only."""
import math

import numpy as np

UNIT = 1 << 16          # map units per bit
REGION_UNIT = 1 << 20   # region-sum units per bit


def lut(freq):
    """rint((16 - log2(freq)) * 65536) in float64, round-half-to-even."""
    assert 1 <= freq <= 65536, freq
    return int(np.rint((16.0 - math.log2(freq)) * 65536.0))


def nibbles(raw):
    n = 0
    while n < 8 and (raw >> (4 * n)) != 0:
        n += 1
    return n


def symbol_cost(cdf, sizes, offsets, row, sym):
    """(cost in 2^-16 bit, coder records: the symbol plus its bypass nibbles) of `sym` coded with table row `row`."""
    sentinel = int(sizes[row]) - 2
    v = int(sym) - int(offsets[row])
    if 0 <= v < sentinel:
        return lut(int(cdf[row][v + 1]) - int(cdf[row][v])), 1
    raw = (-2 * v - 1 if v < 0 else 2 * (v - sentinel)) & 0xFFFFFFFF
    nib = nibbles(raw)
    return lut(int(cdf[row][sentinel + 1]) - int(cdf[row][sentinel])) + 4 * UNIT * (1 + nib), 2 + nib


def stream_cost(symbols, indexes, table):
    """(sum of the costs in 2^-16 bit, records) of a run of symbols as the coder takes them."""
    cdf, sizes, offsets = table
    total = records = 0
    for s, r in zip(symbols, indexes):
        c, n = symbol_cost(cdf, sizes, offsets, int(r), int(s))
        total, records = total + c, records + n
    return total, records


def bound(nbytes, units, records):
    """The check of DESIGN.md 4i: (difference in bits, lower bound, upper bound)."""
    t = records * 2.0 ** -17
    return 8 * nbytes - units / UNIT, 32 - t, 64 + 1e-4 * records + t


def map_scale(sym0, idx0, sym1, idx1, table, N, C, H, W):
    """(N, H, W) int64: planes are (N, C / 2, H, W), every entry a coded symbol at (y, x)."""
    cdf, sizes, offsets = table
    out = np.zeros((N, H, W), dtype=np.int64)
    for sym, idx in ((sym0, idx0), (sym1, idx1)):
        s, i = np.asarray(sym).reshape(N, C // 2, H, W), np.asarray(idx).reshape(N, C // 2, H, W)
        for n in range(N):
            for k in range(C // 2):
                for y in range(H):
                    for x in range(W):
                        out[n, y, x] += symbol_cost(cdf, sizes, offsets, int(i[n, k, y, x]), int(s[n, k, y, x]))[0]
    return out


def map_factorized(sym, table, N, C, H, W):
    cdf, sizes, offsets = table
    s = np.asarray(sym).reshape(N, C, H, W)
    out = np.zeros((N, H, W), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    out[n, y, x] += symbol_cost(cdf, sizes, offsets, c, int(s[n, c, y, x]))[0]
    return out


def region_sums(maps, labels, K):
    """maps: [mv_z, mv_y, z, y] (None: absent), labels (N, hc, wc) -> (N, K, 4) int64 in 2^-20 bit."""
    labels = np.asarray(labels)
    N, hc, wc = labels.shape
    out = np.zeros((N, K, 4), dtype=np.int64)
    for c, m in enumerate(maps):
        if m is None:
            continue
        m = np.asarray(m).astype(np.int64)
        for n in range(N):
            for i in range(hc):
                for j in range(wc):
                    out[n, labels[n, i, j], c] += 16 * m[n, i, j] if c in (1, 3) else m[n, i // 4, j // 4]
    return out


def random_table(rng, rows, max_len=12):
    """A valid table of `rows` rows (cdf (rows, max_len + 2), sizes, offsets) whose first rows are the corner cases: a row
    that holds only its sentinel (frequency 65536), frequencies {1, 65535} and {65535, 1}."""
    stride = max_len + 2
    cdf = np.zeros((rows, stride), dtype=np.int32)
    sizes, offsets = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32)
    fixed = [[0, 65536], [0, 1, 65536], [0, 65535, 65536]]
    for r in range(rows):
        if r < len(fixed):
            row = fixed[r]
        else:
            n = int(rng.integers(2, max_len + 1))                      # coded symbols + the sentinel
            cuts = np.sort(rng.choice(np.arange(1, 65536), size=n - 1, replace=False))
            row = [0] + cuts.tolist() + [65536]
        sizes[r] = len(row)
        cdf[r, : len(row)] = row
        offsets[r] = -((len(row) - 2) // 2) + int(rng.integers(-1, 2))
    return cdf, sizes, offsets


def random_symbols(rng, table, n, rows=None, escapes=0.05, max_nib=8):
    """n (symbol, row) pairs: in-range symbols, and a share `escapes` of escapes of both signs whose values need 1 .. max_nib
    nibbles (0 nibbles too: the first value past the table)."""
    cdf, sizes, offsets = table
    idx = rng.integers(0, len(sizes), size=n).astype(np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
    sym = np.zeros(n, dtype=np.int32)
    for k in range(n):
        r = int(idx[k])
        sentinel = int(sizes[r]) - 2
        if sentinel == 0 or rng.random() < escapes:
            nib = int(rng.integers(0, max_nib + 1))
            raw = 0 if nib == 0 else int(rng.integers(1 << (4 * (nib - 1)), 1 << (4 * nib)))
            if raw & 1:
                v = -(raw + 1) // 2                                     # raw = -2 v - 1
            else:
                v = sentinel + raw // 2                                 # raw = 2 (v - sentinel)
            v = max(min(v + int(offsets[r]), 2 ** 31 - 1), -2 ** 31) - int(offsets[r])
        else:
            v = int(rng.integers(0, sentinel))
        sym[k] = v + int(offsets[r])
    return sym, idx
