"""A restatement of include/dcvc_hip_roil.h in numpy and Python integers, written from the header's text (it shares no code
with the product): quantiser, active cells and counts, segment and record encoder, a SERIAL decoder, the record checker --
and the pictures the residual-layer tests share, whose 16 x 16 cells each have a residual spread of their own so that all
ten segment modes occur."""
import numpy as np

from tests import roi_ref as R

MAGIC, VERSION, MAX_STEP, CELL = b"RL", 1, 64, 16
STEPS = (1, 2, 7, 64)


# --------------------------------------------------------------------------------------------------------- samples
def quantise(r, S):
    """q of the 8-bit residual r: sign(e) * ((|e| + S // 2) // S), e = r - 128"""
    e = np.asarray(r, dtype=np.int64) - 128
    return np.sign(e) * ((np.abs(e) + S // 2) // S)


def reconstruct(q, S):
    return np.clip(128 + np.asarray(q, dtype=np.int64) * S, 0, 255)


def fold(q):
    return np.where(q >= 0, 2 * q, -2 * q - 1)


def unfold(u):
    u = np.asarray(u, dtype=np.int64)
    return np.where(u % 2 == 1, -((u + 1) // 2), u // 2)


# ----------------------------------------------------------------------------------------------------------- cells
def active_cells(boxes, H, W):
    """(cell indexes in raster order, the number of mask pixels of each, the binary mask)"""
    mask = R.binary_mask(boxes, H, W)
    hc, wc = -(-H // CELL), -(-W // CELL)
    cells, counts = [], []
    for i in range(hc):
        for j in range(wc):
            n = int(mask[CELL * i:CELL * i + CELL, CELL * j:CELL * j + CELL].sum())
            if n:  # (a non-empty box touches the cell iff it has a pixel of the cell: boxes lie within the picture)
                cells.append(i * wc + j)
                counts.append(n)
    return np.array(cells, np.int64), np.array(counts, np.int64), mask


def touched_cells(boxes, H, W):
    """the header's touch rule, literally (grow = 0): for tests that the two definitions of `active` agree"""
    wc = -(-W // CELL)
    out = set()
    for x1, y1, x2, y2, _ in np.asarray(boxes).reshape(-1, 5):
        if x2 <= x1 or y2 <= y1:
            continue
        for i in range(-(-H // CELL)):
            for j in range(wc):
                if x1 < CELL * j + CELL and x2 > CELL * j and y1 < CELL * i + CELL and y2 > CELL * i:
                    out.add(i * wc + j)
    return sorted(out)


def cell_samples(plane, mask, cell, W):
    """the cell's mask pixels of one (H, W) plane in raster order inside the cell"""
    wc = -(-W // CELL)
    i, j = divmod(int(cell), wc)
    ys, xs = slice(CELL * i, CELL * i + CELL), slice(CELL * j, CELL * j + CELL)
    return plane[ys, xs][mask[ys, xs]]


# --------------------------------------------------------------------------------------------------------- segment
def segment_bits(u, m):
    n = len(u)
    if m == 9:
        return 0 if not any(u) else None
    if m == 8:
        return 8 * n
    return n * (m + 1) + sum(int(v) >> m for v in u)


# Mode 7 is a mode of the FORMAT that no encoder following the rule can choose: it costs 8 n + sum(u >> 7) bits.  If some
# u >= 128 that is more than mode 8's 8 n.  If every u < 128 it is 8 n, and mode 6 costs 7 n + sum(u >> 6) <= 8 n (every
# u >> 6 is 0 or 1): at most as many bits under a smaller number, so the tie rule takes mode 6 or lower.  A decoder must
# still accept it ("any mode whose L is possible for n"), so the tests decode records in which it is FORCED.
REACHABLE_MODES = frozenset(range(10)) - {7}


def encode_segment(u, force=None):
    """(mode, bytes): the fewest bits, the smallest mode among equals -- or the mode `force`, which must be able to hold u"""
    u = [int(v) for v in u]
    best = None
    for m in range(10) if force is None else [force]:
        b = segment_bits(u, m)
        if b is not None and (best is None or b < best[0]):
            best = (b, m)
    bits, m = best
    value = 0  # the segment as one integer: bit b of the segment is bit b of it
    if m == 8:
        for i, v in enumerate(u):
            value |= v << (8 * i)
    elif m < 8:
        for i, v in enumerate(u):
            value |= (v & ((1 << m) - 1)) << (m * i)
        at = len(u) * m
        for v in u:
            at += v >> m
            value |= 1 << at
            at += 1
        assert at == bits
    return m, value.to_bytes((bits + 7) // 8, "little")


def decode_segment(mode, data, n):
    """the n values u, parsed bit by bit; None where the payload does not hold them"""
    value, end = int.from_bytes(data, "little"), 8 * len(data)
    if mode == 9:
        return [0] * n
    if mode == 8:
        return [(value >> (8 * i)) & 255 for i in range(n)]
    out, at = [], n * mode
    for i in range(n):
        zeros = 0
        while at < end and not (value >> at) & 1:
            zeros, at = zeros + 1, at + 1
        if at >= end:
            return None
        at += 1
        u = (zeros << mode) | ((value >> (mode * i)) & ((1 << mode) - 1))
        if u > 255:
            return None
        out.append(u)
    return out


def length_ok(n, mode, L):
    if mode == 9:
        return L == 0
    if mode == 8:
        return L == n
    return 0 <= mode <= 7 and -(-n * (mode + 1) // 8) <= L <= n


# ---------------------------------------------------------------------------------------------------------- record
def encode_record(res, boxes, S, force7=False):
    """res: (3, H, W) uint8 residual picture in R, G, B order (tests/roi_ref.residual).  Returns (record bytes, modes
    used as a list, the decoded picture (3, H, W) uint8).  force7: code every segment that mode 7 can hold within L <= n
    (every u < 128) in mode 7 -- a record no encoder writes and every decoder accepts."""
    H, W = res.shape[1:]
    cells, counts, mask = active_cells(boxes, H, W)
    u = fold(quantise(res, S))
    table, payload, modes = b"", b"", []
    for cell in cells:
        for c in range(3):
            seg = cell_samples(u[c], mask, cell, W)
            m, data = encode_segment(seg, 7 if force7 and seg.max() < 128 else None)
            table += ((m << 12) | len(data)).to_bytes(2, "little")
            payload += data
            modes.append(m)
    record = MAGIC + bytes([VERSION, S]) + len(cells).to_bytes(4, "little") + table + payload
    want = np.where(mask[None], reconstruct(quantise(res, S), S), 0).astype(np.uint8)
    return record, modes, want


def check_record(record, counts):
    """None, or the name of the first disagreement"""
    A = len(counts)
    if len(record) < 8:
        return "truncated"
    if record[:2] != MAGIC:
        return "magic"
    if record[2] != VERSION:
        return "version"
    if not 1 <= record[3] <= MAX_STEP:
        return "step"
    if int.from_bytes(record[4:8], "little") != A:
        return "cells"
    if len(record) < 8 + 6 * A:
        return "truncated"
    total = 8 + 6 * A
    for s in range(3 * A):
        e = int.from_bytes(record[8 + 2 * s:10 + 2 * s], "little")
        if e >> 12 > 9:
            return "mode"
        if not length_ok(int(counts[s // 3]), e >> 12, e & 0xFFF):
            return "length"
        total += e & 0xFFF
    return "truncated" if len(record) < total else ("trailing" if len(record) > total else None)


def decode_record(record, boxes, H, W):
    """(3, H, W) uint8: r' inside the mask, 0 outside; None where the record is refused or the payload does not decode"""
    cells, counts, mask = active_cells(boxes, H, W)
    if check_record(record, counts) is not None:
        return None
    S, A = record[3], len(cells)
    out = np.zeros((3, H, W), np.int64)
    at, wc = 8 + 6 * A, -(-W // CELL)
    for a, cell in enumerate(cells):
        i, j = divmod(int(cell), wc)
        ys, xs = slice(CELL * i, CELL * i + CELL), slice(CELL * j, CELL * j + CELL)
        for c in range(3):
            e = int.from_bytes(record[8 + 6 * a + 2 * c:10 + 6 * a + 2 * c], "little")
            u = decode_segment(e >> 12, record[at:at + (e & 0xFFF)], int(counts[a]))
            at += e & 0xFFF
            if u is None:
                return None
            block = out[c, ys, xs]
            block[mask[ys, xs]] = reconstruct(unfold(u), S)
            out[c, ys, xs] = block
    return out.astype(np.uint8)


# -------------------------------------------------------------------------------------------------------- pictures
SPREADS = (0, 0.4, 1, 2, 4, 8, 16, 32, 64, None)  # per cell, in turn: exact, ..., None = full-range uniform


def pictures(seed, H, W):
    """(src, rec): float32 (3, H, W), both on the 8-bit grid T[k].  Cell number k (raster order) of every channel has the
    residual spread SPREADS[(k + channel) % 10]: rec = src there (spread 0), src plus a Laplacian of that scale, or
    unrelated uniform codes (None), so that over a picture of a few cells every segment mode an encoder can choose is the
    cheapest somewhere (REACHABLE_MODES)."""
    rng = np.random.default_rng(seed + 7000)
    src = rng.integers(0, 256, (3, H, W))
    rec = src.copy()
    wc = -(-W // CELL)
    for i in range(-(-H // CELL)):
        for j in range(wc):
            ys, xs = slice(CELL * i, min(CELL * i + CELL, H)), slice(CELL * j, min(CELL * j + CELL, W))
            for c in range(3):
                spread = SPREADS[(i * wc + j + c) % len(SPREADS)]
                shape = src[c, ys, xs].shape
                if spread is None:
                    rec[c, ys, xs] = rng.integers(0, 256, shape)
                elif spread:
                    rec[c, ys, xs] = np.clip(src[c, ys, xs] - np.rint(rng.laplace(0.0, spread, shape)).astype(np.int64), 0, 255)
    return R.T[src], R.T[rec]
