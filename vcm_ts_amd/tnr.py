"""A motion-adaptive temporal noise prefilter (include/dcvc_hip_tnr.h, csrc/tnr.hip) for fixed-camera content, where a
P picture's bits are dominated by sensor noise: every P picture the codec is handed is blended with the previous filtered
picture wherever the luma of the two stays close over a 5 x 5 window, and passed through untouched wherever something
moves.  It is ENCODER SIDE ONLY: it replaces the picture the codec is handed and nothing else -- no side file, no change
of the .bin format, nothing for the decoder to know.  The arithmetic is stated in the header; tests/tnr_ref.py restates it
in numpy.

    TNR(threshold, floor=64, pixel=None)     the setting; .table() the 256 weights
    TnrFilter(tnr, size, device)             the state of ONE GOP stream on the device; .step(x_padded, intra)

There is deliberately NO default threshold, and `floor` and `pixel` are UNTUNED PLACEHOLDERS: no machine of the project
holds a real video.  This is the mechanism -- filtered, coded, decoded by an unchanged decoder -- not a claim about rate
or quality.  Moving pixels are passed through, not followed: there is no motion compensation.

The kernel runs on the caller's current stream and synchronises nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import lib
from .roi import MAX_SIDE, grid_of

MAX_T, MAX_FLOOR, MAX_P, FULL = 64, 255, 255, 256
ROWS = 64  # pictures' totals kept on the device between two copies to the host


def _whole(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer within {lo}..{hi}, got {v!r}")
    return int(v)


@dataclass(frozen=True)
class TNR:
    """threshold T: a pixel whose 5 x 5 window differs from the previous filtered picture by T luma codes or more on
    average is passed through (1..64; no default exists).  floor: the weight of the current picture, in 1/256ths, where
    nothing differs at all (1..255); between 0 and T the weight rises linearly to 256.  pixel P: a pixel whose own luma
    differs by more than P codes is passed through whatever its window says (0..255; None: min(255, 3 T)).  floor and
    pixel are untuned placeholders."""
    threshold: int
    floor: int = 64
    pixel: int = None

    def __post_init__(self):
        object.__setattr__(self, "threshold", _whole("threshold", self.threshold, 1, MAX_T))
        object.__setattr__(self, "floor", _whole("floor", self.floor, 1, MAX_FLOOR))
        object.__setattr__(self, "pixel", min(MAX_P, 3 * self.threshold) if self.pixel is None else _whole("pixel", self.pixel, 0, MAX_P))

    def table(self):
        """wtab of dcvc_tnr_step: the weight of the current picture by the window's mean difference a = 0 .. 255, as
        uint16: 256 from T on, floor + ((256 - floor) a) // T below."""
        a = np.arange(256, dtype=np.int64)
        return np.where(a >= self.threshold, FULL, self.floor + ((FULL - self.floor) * a) // self.threshold).astype(np.uint16)

    def to_json(self):
        return {"threshold": self.threshold, "floor": self.floor, "pixel": self.pixel}


class TnrFilter:
    """The filter of one GOP stream of `size` = (height, width) pictures on `device`: two zero-initialised padded
    pictures written alternately, the table, and the cells' sad / held.  The filter restarts at every I picture, so what a
    GOP is coded from depends on its own pictures and the setting only.  One TnrFilter serves one stream at a time.
    totals=False keeps no per-picture totals: a step is then the one launch and nothing else, no pinned memory and no
    event is ever made, and .totals() is refused."""

    def __init__(self, tnr, size, device, totals=True):
        import torch

        from . import stream as S

        if not isinstance(tnr, TNR):
            raise ValueError(f"tnr: expected a tnr.TNR, got {type(tnr).__name__}")
        self.tnr, self.device = tnr, torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("TnrFilter: pictures live on the GPU (no CPU fallback exists)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.height, self.width = int(size[0]), int(size[1])
        if not (0 < self.height <= MAX_SIDE and 0 < self.width <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {self.width}x{self.height}")
        l, r, t, b = S.get_padding_size(self.height, self.width)
        self.padded = (self.height + t + b, self.width + l + r)
        self.grid = grid_of(self.height, self.width)
        cells = self.grid[0] * self.grid[1]
        # (the crop is written in place by every step and the padding never: it stays the zero pad_frame would give)
        self.bufs = [torch.zeros((1, 3) + self.padded, dtype=torch.float32, device=self.device) for _ in range(2)]
        self.wtab = torch.from_numpy(tnr.table().view(np.int16)).to(self.device)  # (the bits of the uint16 table)
        self.sad = torch.empty(cells, dtype=torch.int32, device=self.device)   # (uint32 words; a cell's sum is < 2^16)
        self.held = torch.empty(cells, dtype=torch.int16, device=self.device)  # (uint16 words; a cell's count is <= 256)
        self.ref, self.n, self.launches = None, 0, 0
        # (held, sad) of the P pictures not yet flushed; the values already read, by step number
        self._rows = torch.zeros((ROWS, 2), dtype=torch.int64, device=self.device) if totals else None
        self._idx, self._done, self._read = [], [], {}
        torch.cuda.synchronize(self.device)  # (the uploads above: a stream that uses them afterwards cannot race them)

    def _check(self, x):
        import torch

        if not torch.is_tensor(x) or not x.is_cuda:
            raise ValueError("TnrFilter.step: pictures live on the GPU (no CPU fallback exists)")
        if x.device != self.device:
            raise ValueError(f"TnrFilter.step: the picture is on {x.device}, the filter on {self.device}")
        if x.dtype != torch.float32 or tuple(x.shape) != (1, 3) + self.padded:
            raise ValueError(f"TnrFilter.step: expected a (1, 3, {self.padded[0]}, {self.padded[1]}) float32 picture, got "
                             f"{tuple(x.shape)} {x.dtype}")

    def step(self, x_padded, intra):
        """The padded picture to code in place of `x_padded`.  An I picture (intra=True) launches nothing and is returned
        itself; it becomes the next step's reference.  A P picture is one dcvc_tnr_step launch on the current stream from
        the crops of x_padded and of the previous step's result into the crop of one of the two buffers, which stays valid
        until the step after the next."""
        import torch

        from .engine import _raw_stream
        from .metrics import _planar

        self._check(x_padded)
        t, self.n = self.n, self.n + 1
        if intra:
            self.flush()  # (the GOP before this one: its totals go to the host in one copy)
            self.ref = x_padded.detach()
            return x_padded
        if self.ref is None:
            raise ValueError("TnrFilter.step: the first picture of a stream is an I picture")
        out = self.bufs[0] if self.ref is not self.bufs[0] else self.bufs[1]
        (h, w), (Hp, Wp) = (self.height, self.width), self.padded
        cur, crs, cps = _planar(x_padded.detach()[..., :h, :w])  # (the crops, read in place)
        ref, rrs, rps = _planar(self.ref[..., :h, :w])
        with torch.cuda.device(self.device):
            lib.check(lib.hip().dcvc_tnr_step(cur.data_ptr(), crs, cps, ref.data_ptr(), rrs, rps, out.data_ptr(), Wp, Hp * Wp, h, w,
                                              self.wtab.data_ptr(), self.tnr.pixel, self.sad.data_ptr(), self.held.data_ptr(),
                                              C.c_void_p(_raw_stream(self.device.index))), "tnr_step")
        self.launches += 1
        if self._rows is not None:
            row = self._rows[len(self._idx)]  # (two small reductions behind the launch; the host looks at them per GOP)
            row[0].copy_(self.held.sum(dtype=torch.int64))
            row[1].copy_(self.sad.sum(dtype=torch.int64))
            self._idx.append(t)
            if len(self._idx) == ROWS:  # (a GOP longer than the rows kept: its totals travel in more than one copy)
                self.flush()
        self.ref = out
        return out

    def flush(self):
        """The totals of the P pictures since the last flush, to pinned host memory in ONE asynchronous copy on the
        current stream: no kernel, and nothing is waited for."""
        import torch

        if self._idx:
            host = torch.empty((len(self._idx), 2), dtype=torch.int64).pin_memory()
            host.copy_(self._rows[:len(self._idx)], non_blocking=True)  # (the next step's rows follow it in stream order)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._done.append((ev, host, self._idx))
            self._idx = []

    def totals(self):
        """[(held pixels, sum of d)] of every step so far, in order, as Python integers; (0, 0) for an I picture.  Flushes
        on the current stream and waits for the copies; their pinned buffers and events are let go of here, at a known
        point, and only the integers are kept."""
        if self._rows is None:
            raise ValueError("TnrFilter.totals: this filter was made with totals=False")
        self.flush()
        for ev, host, idx in self._done:
            ev.synchronize()
            self._read.update({t: (int(held), int(sad)) for t, (held, sad) in zip(idx, host.tolist())})
        self._done = []
        return [self._read.get(t, (0, 0)) for t in range(self.n)]
