"""The sensor noise of a fixed-camera source, measured before anything is filtered (include/dcvc_hip_noise.h,
csrc/noise.hip), and the prefilter threshold that follows from it.

On a fixed camera most 16 x 16 cells of a picture are static, and the temporal difference of a static cell is pure noise.
Every picture of a scan is reduced on the device to one word per cell -- the sum of |Y(t) - Y(t - 1)| over the cell and the
cell's mean luma -- and the words are counted into a 16 x 512 histogram (luma in steps of 16 codes by mean absolute
difference in 1/16 code).  The host makes one number of it, in integers, so that every host gives the same answer:

    NoiseScan(device, height, width, batch=64)   .add(picture) per picture, .histogram() -> (16, 512) int64
    estimate(hist, min_cells=1024)               -> NoiseEstimate: mad32 (1/32 code) or None, sigma_milli, counts, by_luma
    auto_threshold(mad32, scale)                 -> the T of tnr.TNR that `scale` times the noise level means

THE ESTIMATOR.  Rows 0 and 15 (mean luma below 16, or from 240 up) are clipped blacks and whites whose noise is cut off:
counted as `clipped`, left out.  Column 0 (below 1/16 code) is exact repeats and noise too small to measure: counted as
`still`, left out.  Of the N cells that remain the estimate is the LOWER QUARTILE of the mean absolute difference: the
smallest column c whose cumulative count exceeds (N - 1) // 4, reported as its centre 2 c + 1 in 1/32 code.  The quartile
is chosen because motion only ever inflates a cell's difference: the estimate is untouched while fewer than three quarters
of the counted cells move.  It pays with a KNOWN DOWNWARD BIAS, which is deliberately NOT corrected: a static cell's mean of
256 absolute Gaussian differences scatters by 4.7 % (0.603 / 0.798 / 16), so the quartile sits about 3 % below the true
mean absolute difference when nothing moves at all.  Fewer than min_cells counted cells, or a quartile in the last column
(31.94 codes and beyond), give no estimate (mad32 = None).  sigma_milli = (mad32 * 886227 + 16000) // 32000 is the
standard deviation of the luma noise OF ONE PICTURE in thousandths of a code if the noise is Gaussian (a difference of two
pictures has sqrt(2) sigma and a mean absolute value of 2 sigma / sqrt(pi)); it is for information only.

`min_cells` = 1024 and tnr.AutoTNR's `scale` = 3.0 are UNTUNED PLACEHOLDERS: no machine of the project holds a real video.
LIMITS: fixed camera only -- a pan moves every cell, and what is measured is then motion, with no warning (a shake.Registrar in
front of the scan, vcm_ts_amd/shake.py, takes out a shake of a few pixels and names a pan: its pictures are lost); one estimate
per source, not per GOP; flicker and auto-gain inflate it; luma only.  The 8-bit rounding of R, G and B is counted as noise
(4 % at one code of noise a channel), and on a monochrome source (R = G = B, where the luma of the codes has no fractional
part of its own) so is the rounding of Y: 7 % high at one code, nothing from two codes on (tests/test_noise_host.py).

The kernels run on the caller's current stream and nothing is synchronised per picture.  There is no torch fallback: a CPU
tensor is a ValueError.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import MAX_SIDE, whole
from .roi import grid_of

NONE = 0xFFFFFFFF
ROWS, COLS = 16, 512
COUNTERS = ROWS * COLS
MAX_WORDS = 1 << 28  # (DCVC_NOISE_MAX_WORDS)
MIN_CELLS = 1024     # an untuned placeholder
MIN_SCALE, MAX_SCALE = 50, 1600  # hundredths


class NoiseScan:
    """The noise histogram of the pictures of `height` x `width` on `device`: two luma byte planes written alternately, a
    (batch, hc * wc) ring of cell words and the 16 x 512 counters.  One dcvc_noise_cells launch per picture, one
    dcvc_noise_hist launch per `batch` pictures; nothing is synchronised before .histogram()."""

    def __init__(self, device, height, width, batch=64):
        import torch

        device = devargs.cuda_device(device, "NoiseScan")
        if not (0 < int(height) <= MAX_SIDE and 0 < int(width) <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        self.device, self.height, self.width = device, int(height), int(width)
        self.grid = grid_of(self.height, self.width)
        self.cells = self.grid[0] * self.grid[1]
        self.batch = whole("batch", batch, 1, MAX_WORDS // self.cells)
        self.y_stride = -(-self.width // 4) * 4
        self.planes = [torch.empty((self.height, self.y_stride), dtype=torch.uint8, device=device) for _ in range(2)]
        self.ring = torch.empty((self.batch, self.cells), dtype=torch.int32, device=device)  # (uint32 words)
        self.hist = torch.zeros(COUNTERS, dtype=torch.int32, device=device)  # (uint32 counters)
        self.n, self.filled = 0, 0  # pictures added; ring rows not yet counted
        self._total = np.zeros((ROWS, COLS), dtype=np.int64)  # what was folded out of the device counters
        self._since = 0  # pictures counted into the device counters since they were last zero
        self._fold_at = (2 ** 32 - 1) // self.cells  # (a bin gains at most hc * wc a picture)
        self._stream = torch.cuda.current_stream(device)  # (the zeroing runs here: another stream's first add waits for it)
        self._mark = torch.cuda.Event()

    def add(self, picture):
        """The height x width crop of a (1, 3, Hp, Wp) float32 picture, read in place, against the picture before it, into
        the next ring row on the current stream."""
        crop = devargs.checked(picture, "NoiseScan.add", device=self.device, at_least=(self.height, self.width), owner="scan")
        x, rs, ps = devargs.planar(crop)
        self._hand_over()
        if self._since + self.filled + 1 > self._fold_at:
            self._fold()
        yprev = self.planes[(self.n - 1) % 2].data_ptr() if self.n else None
        devargs.launch("dcvc_noise_cells", self.device, x.data_ptr(), rs, ps, self.height, self.width, yprev,
                       self.planes[self.n % 2].data_ptr(), self.y_stride, self.ring[self.filled].data_ptr())
        self.n, self.filled = self.n + 1, self.filled + 1
        if self.filled == self.batch:
            self._count()

    def _hand_over(self):
        """Cross-stream use: the current stream waits on the device for everything the scan launched on the stream it used
        last (the zeroing included); the host waits for nothing."""
        import torch

        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._mark.record(self._stream)
            cur.wait_event(self._mark)
            self._stream = cur

    def _count(self):
        """The filled ring rows into the device counters: one launch (the next picture's row follows it in stream order)."""
        if self.filled:
            devargs.launch("dcvc_noise_hist", self.device, self.ring.data_ptr(), self.filled * self.cells, self.hist.data_ptr())
            self._since, self.filled = self._since + self.filled, 0

    def _fold(self):
        """The device counters into Python-side int64 numbers, and zero: before any bin could pass 2^32 - 1."""
        self._count()
        self._total += self.hist.cpu().numpy().view(np.uint32).astype(np.int64).reshape(ROWS, COLS)
        self.hist.zero_()
        self._since = 0

    @property
    def pairs(self):
        """The pairs of consecutive pictures that were compared."""
        return max(self.n - 1, 0)

    def histogram(self):
        """(16, 512) int64 on the host: flushes the partly filled ring and waits for it."""
        self._hand_over()
        self._fold()
        return self._total.copy()


@dataclass(frozen=True)
class NoiseEstimate:
    """mad32: the lower quartile of the counted cells' mean absolute luma difference of consecutive pictures, in 1/32 code
    (None: no estimate); sigma_milli: one picture's luma noise in 1/1000 code under a Gaussian (None with it); cells: the
    counted cells N; still, clipped: the cells left out; pairs: the picture pairs behind it (None when unknown); by_luma:
    the same rule per luma row, 16 entries (None for the two clipped rows); min_cells: the setting."""
    mad32: int
    sigma_milli: int
    cells: int
    still: int
    clipped: int
    pairs: int
    by_luma: tuple
    min_cells: int

    def to_json(self):
        return {"mad32": self.mad32, "sigma_milli": self.sigma_milli, "cells": self.cells, "still": self.still,
                "clipped": self.clipped, "pairs": self.pairs, "by_luma": list(self.by_luma), "min_cells": self.min_cells}

    def why_none(self):
        """What the refusals say of an estimate without a value."""
        if self.cells < self.min_cells:
            return f"too few counted cells: {self.cells} of {self.min_cells}"
        return "the noise level is out of range (the lower quartile lies at 31.94 codes or beyond)"


def _quartile(counts, min_cells):
    """mad32 of one row of 512 counts whose column 0 is already left out (Python integers throughout)."""
    n = sum(counts)
    if n < min_cells or n == 0:
        return None
    rank, run = (n - 1) // 4, 0
    for c, v in enumerate(counts):
        run += v
        if run > rank:
            return None if c == COLS - 1 else 2 * c + 1
    return None


def sigma_milli(mad32):
    return None if mad32 is None else (int(mad32) * 886227 + 16000) // 32000


def estimate(hist, min_cells=MIN_CELLS, pairs=None):
    """The NoiseEstimate of a (16, 512) histogram of cell words (NoiseScan.histogram): the module docstring's rule."""
    hist = np.asarray(hist)
    if hist.shape != (ROWS, COLS) or not np.issubdtype(hist.dtype, np.integer) or (hist < 0).any():
        raise ValueError(f"estimate: expected a ({ROWS}, {COLS}) array of counts, got {hist.shape} {hist.dtype}")
    min_cells = whole("min_cells", min_cells, 1, 2 ** 31 - 1)
    rows = [[int(v) for v in r] for r in hist.tolist()]
    clipped = sum(rows[0]) + sum(rows[ROWS - 1])
    still = sum(r[0] for r in rows[1:ROWS - 1])
    pooled = [0] + [sum(rows[i][c] for i in range(1, ROWS - 1)) for c in range(1, COLS)]
    mad32 = _quartile(pooled, min_cells)
    by_luma = tuple(_quartile([0] + r[1:], min_cells) if 0 < i < ROWS - 1 else None for i, r in enumerate(rows))
    return NoiseEstimate(mad32, sigma_milli(mad32), sum(pooled), still, clipped, None if pairs is None else int(pairs), by_luma, min_cells)


def scale100(scale):
    """`scale` snapped to hundredths within 0.50 .. 16.00, as the ROI q factors are snapped."""
    s = devargs.hundredths(scale, "scale")
    if not MIN_SCALE <= s <= MAX_SCALE:
        raise ValueError(f"scale must lie within {MIN_SCALE / 100:.2f}..{MAX_SCALE / 100:.2f}, got {scale!r}")
    return s


def auto_threshold(mad32, scale):
    """T = clamp(ceil(scale100 * mad32 / 3200), 1, tnr.MAX_T), in integers: `scale` times the measured mean absolute
    difference, in whole luma codes."""
    from .tnr import MAX_T

    mad32 = whole("mad32", mad32, 1, 2 * COLS - 1)
    return min(max(-(-scale100(scale) * mad32 // 3200), 1), MAX_T)
