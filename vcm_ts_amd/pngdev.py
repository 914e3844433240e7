"""Reconstruction PNGs written on the device (include/dcvc_hip_png.h, csrc/png.hip, csrc/png_check.cpp): the picture the
codec holds becomes a finished 8-bit RGB .png file in device memory -- row filters, a deflate coder with PRESET Huffman
tables, CRC-32 and Adler-32 -- and leaves it in one asynchronous copy; a host thread only waits for that copy and calls
write().  The format is stated in the header; tests/pngdev_ref.py restates it.

    Preset(lengths)                          one Huffman table: canonical codes and the bits of its block header
    presets(), to_words(presets)             the built-in family (data, not code: the kernels take any valid set)
    PngDevice(size, device, streams, ...)    per GOP stream: staging, a file buffer and a ring of pinned host buffers
        .put(k, picture) -> Handle           two launches and one copy on the current stream; nothing is waited for
    Handle.data() / .save(path) / .release() what a writer thread does with it

It is opt-in (run_codec --png-device).  The compression is what distance-1 matches and fixed tables give: close to zlib's
default on noisy pictures, well behind it on flat synthetic ones (README.md).  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

import ctypes as C
import heapq
import threading

import numpy as np

from . import devargs, lib

BAND_MAX, NSYM, HEADER_WORDS, PRESET_WORDS, SLOT_BYTES, MAX_W, MAX_H, MAX_PRESETS = 24576, 286, 72, 360, 24576 + 32, 8191, 32768, 32
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_SMALLEST = 47 + 33 + 12  # prefix, trailer and one band's chunk around its data: no file is shorter
_FRONT = 16  # bytes of a file buffer in front of the file: the size word, and the file stays 16-byte aligned


# ------------------------------------------------------------------------------------------------------------- presets
def huffman_lengths(freqs, limit):
    """Code lengths of plain Huffman over the symbols of nonzero frequency (0 for the others); while the longest exceeds
    `limit` the frequencies are halved (never below 1) and the tree is built again.  Ties are broken by symbol number, so
    the result is a function of the integers alone."""
    freqs = [int(f) for f in freqs]
    if sum(f > 0 for f in freqs) < 2:
        raise ValueError("a Huffman code needs two symbols of nonzero frequency")
    while True:
        heap = [(f, s, (s,)) for s, f in enumerate(freqs) if f > 0]
        heapq.heapify(heap)
        lengths = [0] * len(freqs)
        while len(heap) > 1:
            fa, sa, a = heapq.heappop(heap)
            fb, sb, b = heapq.heappop(heap)
            for s in a + b:
                lengths[s] += 1
            heapq.heappush(heap, (fa + fb, min(sa, sb), a + b))
        if max(lengths) <= limit:
            return lengths
        freqs = [max(1, f >> 1) if f > 0 else 0 for f in freqs]


def canonical_codes(lengths):
    """RFC 1951, 3.2.2: the codes of the lengths (0: unused), not reversed."""
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        if n:
            count[n] += 1
    nxt, c = [0] * (max(lengths) + 2), 0
    for b in range(1, max(lengths) + 1):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def _reversed(v, bits):
    return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0


class Preset:
    """One literal/length table of the device coder: `lengths`, 286 integers within 1..15 that are a complete prefix code;
    .codes (canonical, bit-reversed) and .header = (bits as an int, their number): HLIT = 29, HDIST = 0, HCLEN, the
    code-length code and the 287 lengths (the last one the single distance code's), runs written with symbol 16."""

    def __init__(self, lengths):
        lengths = [devargs.whole("a preset's code length", n, 1, 15) for n in lengths]
        if len(lengths) != NSYM:
            raise ValueError(f"a preset has {NSYM} code lengths, got {len(lengths)}")
        if sum(1 << (15 - n) for n in lengths) != 1 << 15:
            raise ValueError("a preset's code lengths must be a complete prefix code (the sum of 2^-length is 1)")
        self.lengths = lengths
        self.codes = [_reversed(c, n) for c, n in zip(canonical_codes(lengths), lengths)]
        self.header = self._header()

    def _header(self):
        seq, syms, i = self.lengths + [1], [], 0
        while i < len(seq):  # (symbol, extra bits, extra value)
            syms.append((seq[i], 0, 0))
            run = 1
            while i + run < len(seq) and seq[i + run] == seq[i]:
                run += 1
            i, run = i + 1, run - 1
            while run >= 3:
                n = min(run, 6)
                syms.append((16, 2, n - 3))
                i, run = i + n, run - n
        freqs = [0] * 19
        for s, _, _ in syms:
            freqs[s] += 1
        cl = huffman_lengths(freqs, 7)
        clcodes = [_reversed(c, n) for c, n in zip(canonical_codes(cl), cl)]
        ncl = max(j for j, s in enumerate(_ORDER) if cl[s]) + 1
        acc, n = 0, 0
        for value, bits in [(NSYM - 257, 5), (0, 5), (max(ncl, 4) - 4, 4)] + [(cl[s], 3) for s in _ORDER[:max(ncl, 4)]]:
            acc, n = acc | value << n, n + bits
        for s, eb, ev in syms:
            acc, n = acc | clcodes[s] << n, n + cl[s]
            acc, n = acc | ev << n, n + eb
        if n > 32 * HEADER_WORDS:
            raise ValueError(f"a preset's block header takes {n} bits, more than {32 * HEADER_WORDS}")
        return acc, n

    def words(self):
        acc, n = self.header
        w = [n_ << 16 | c for n_, c in zip(self.lengths, self.codes)] + [n]
        w += [(acc >> (32 * j)) & 0xFFFFFFFF for j in range(HEADER_WORDS)] + [0]
        return np.array(w, dtype=np.uint32)


def geometric_preset(theta_percent, run_percent):
    """A table for filtered bytes that fall off two-sidedly from 0 by `theta_percent` / 100 per code, with
    `run_percent` / 100 of the mass on the match lengths (half of that on the longest, 59..63).  All integer."""
    theta = devargs.whole("theta_percent", theta_percent, 1, 99)
    run = devargs.whole("run_percent", run_percent, 1, 99)
    one = 1 << 48
    lit = [one * theta ** min(v, 256 - v) // 100 ** min(v, 256 - v) for v in range(256)]
    total = sum(lit)
    freqs = [max(1, f * (100 - run) * 4096 // total) for f in lit]           # the literals share (100 - run) * 4096
    freqs += [max(1, (100 - run) * 4096 // 8192)]                          # the end of the block: once in thousands
    freqs += [max(1, run * 4096 // 38)] * 19 + [max(1, run * 4096 // 2)]   # 257 .. 275, and 276
    freqs += [1] * (NSYM - len(freqs))                                     # the lengths beyond a segment: never coded
    return Preset(huffman_lengths(freqs, 15))


THETAS, RUNS = (8, 20, 35, 50, 70, 80, 88, 93, 96, 98), (2, 30)


def presets():
    """The built-in family: geometric_preset over THETAS x RUNS, 20 tables from sharp (noise-free synthetic pictures) to
    nearly flat (heavy noise; beyond that a band is stored)."""
    return [geometric_preset(t, r) for t in THETAS for r in RUNS]


def to_words(tables):
    """(K, DCVC_PNG_PRESET_WORDS) uint32 of 1..32 Presets: what dcvc_png_encode takes, host and device."""
    tables = list(tables)
    if not 1 <= len(tables) <= MAX_PRESETS or not all(isinstance(t, Preset) for t in tables):
        raise ValueError(f"to_words: expected 1..{MAX_PRESETS} pngdev.Preset objects")
    return np.stack([t.words() for t in tables])


def default_rows(width):
    """The largest band that fits: DCVC_PNG_BAND_MAX // (3 W + 1) rows (4 at 1920)."""
    return BAND_MAX // (3 * devargs.whole("width", width, 1, MAX_W) + 1)


def bound(height, width, rows):
    """dcvc_png_bound: the most bytes a file takes; a ValueError for sizes the kernels refuse."""
    b = int(lib.hip().dcvc_png_bound(int(height), int(width), int(rows)))
    if b < 0:
        raise ValueError(f"a PNG of {width}x{height} in bands of {rows} rows: the width must be within 1..{MAX_W}, the height "
                         f"within 1..{MAX_H} and rows * (3 * width + 1) within 1..{BAND_MAX}")
    return b


def checked_words(words):
    """`words` as a C-contiguous (K, PRESET_WORDS) uint32 array that dcvc_png_tables_check accepts."""
    a = np.ascontiguousarray(words, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != PRESET_WORDS or not 1 <= a.shape[0] <= MAX_PRESETS:
        raise ValueError(f"preset tables: expected (1..{MAX_PRESETS}, {PRESET_WORDS}) uint32 words, got {a.shape}")
    if lib.hip().dcvc_png_tables_check(a.ctypes.data, a.shape[0]) != 0:
        raise ValueError("preset tables: refused by dcvc_png_tables_check (lengths, codes or header bits do not agree)")
    return a


# -------------------------------------------------------------------------------------------------------------- device
class Handle:
    """One picture on its way: the pinned buffer its file is copied into and the event behind the copy.  Whoever holds
    it calls save() or data() + release(); the buffer returns to its ring on release."""

    def __init__(self, host, event, capacity):
        self.host, self.event, self.capacity, self.free = host, event, capacity, threading.Event()

    def data(self):
        """The file's bytes as a memoryview into the pinned buffer (valid until release()); waits for the copy."""
        self.event.synchronize()
        a = self.host.numpy()
        size = int(a[:4].view(np.uint32)[0])
        if not _SMALLEST <= size <= self.capacity:
            raise lib.KernelError(f"png_encode wrote a size of {size} bytes into a buffer of {self.capacity}")
        return memoryview(a)[_FRONT:_FRONT + size]

    def release(self):
        self.free.set()

    def save(self, path):
        try:
            with open(path, "wb") as f:
                f.write(self.data())
        finally:
            self.release()


def save_handle(handle, path):
    """PNGWriters' `save` for a Handle."""
    handle.save(path)


class PngDevice:
    """The PNG writer of the (height, width) pictures of `streams` GOP streams on `device`.  Every stream owns its
    staging, its file buffer and `ring` pinned host buffers (the scratch rule of dcvc_hip_hash.h: calls on different
    streams share nothing).  rows: a band's rows (default: the most that fit); tables: Presets (default: presets())."""

    def __init__(self, size, device, streams=1, rows=None, tables=None, ring=4):
        import torch

        self.device = devargs.cuda_device(device, "PngDevice")
        self.height, self.width = devargs.whole("height", size[0], 1, MAX_H), devargs.whole("width", size[1], 1, MAX_W)
        self.rows = default_rows(self.width) if rows is None else devargs.whole("rows", rows, 1, BAND_MAX)
        self.capacity = bound(self.height, self.width, self.rows)
        self.words = checked_words(to_words(presets() if tables is None else tables))
        n_streams, n_ring = devargs.whole("streams", streams, 1, 64), devargs.whole("ring", ring, 1, 64)
        bands = -(-self.height // self.rows)
        total = _FRONT + -(-self.capacity // 4) * 4
        self.tables = torch.from_numpy(self.words.view(np.int32)).to(self.device)
        self.staging = [torch.empty(bands * SLOT_BYTES, dtype=torch.uint8, device=self.device) for _ in range(n_streams)]
        self.files = [torch.empty(total, dtype=torch.uint8, device=self.device) for _ in range(n_streams)]
        self.rings = [[torch.empty(total, dtype=torch.uint8).pin_memory() for _ in range(n_ring)] for _ in range(n_streams)]
        self.pending = [[None] * n_ring for _ in range(n_streams)]
        self.count, self.launches = [0] * n_streams, 0
        torch.cuda.synchronize(self.device)  # (the upload above: a stream that uses it afterwards cannot race it)

    def put(self, k, picture):
        """The file of the top-left (height, width) crop of `picture`, a (1, 3, H, W) float32 tensor on the device, read in
        place: dcvc_png_encode and one copy of the file buffer into stream k's next pinned buffer, all on the CURRENT
        stream, then an event.  Nothing is waited for, unless all of the ring's buffers are still with their writers."""
        import torch

        k = devargs.whole("stream", k, 0, len(self.files) - 1)
        x, rs, ps = devargs.picture(picture, "PngDevice.put", device=self.device, at_least=(self.height, self.width), owner="writer")
        slot = self.count[k] % len(self.rings[k])
        self.count[k] += 1
        if self.pending[k][slot] is not None:
            self.pending[k][slot].free.wait()
        buf, host = self.files[k], self.rings[k][slot]
        devargs.launch("dcvc_png_encode", self.device, x.data_ptr(), rs, ps, self.height, self.width, self.rows,
                       self.words.ctypes.data, self.tables.data_ptr(), self.words.shape[0], self.staging[k].data_ptr(),
                       buf.data_ptr() + _FRONT, C.c_int64(self.capacity), buf.data_ptr(), what="png_encode")
        self.launches += 2
        with torch.cuda.device(self.device):
            host.copy_(buf, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        self.pending[k][slot] = handle = Handle(host, event, self.capacity)
        return handle
