"""The ROI residual layer as a bitstream of its own (include/dcvc_hip_roil.h, csrc/roil.hip): the residual picture of
vcm_ts_amd/roi.py inside the boxes, coded on the device cell by cell into one small record per picture -- lossless at
step 1, near-lossless (|r' - r| <= step // 2) above -- and decoded on the device into the 8-bit picture roi.fuse reads.

It takes the place of the raw `.gbrp` file between `encode` and `decode`; it is not HEVC, and no rate or quality result is
claimed for it.  Arithmetic and format are stated in the header and pinned bit for bit by tests/test_gpu_roil.py against
tests/roil_ref.py.  Every launch runs on the caller's current stream; encode_layer synchronises nothing (its record is
waited for in .bytes()).  There is no torch fallback: anything the kernels do not take is a ValueError.
"""
from __future__ import annotations

import numpy as np

from . import devargs, lib
from . import roi as X

MAX_STEP, HEADER, SLOT, CELL_MAX, VERSION, BAD_STREAM = 64, 8, 768, 774, 1, 1
MAGIC = b"RL"
FILE_EXT = ".rl"


class RoiLayerError(ValueError):
    """A record that is not one, that disagrees with the boxes, or whose payload does not decode."""


_REFUSALS = {-16: "truncated record", -17: "bad magic", -18: "unknown version", -19: "step out of range",
             -20: "wrong number of active cells", -21: "mode above 9", -22: "impossible segment length", -23: "trailing bytes"}


def check_step(step):
    return devargs.whole("residual step", step, 1, MAX_STEP)


def _size(height, width):
    H, W = int(height), int(width)
    if not (0 < H <= X.MAX_SIDE and 0 < W <= X.MAX_SIDE):
        raise ValueError(f"picture sides must be within 1..{X.MAX_SIDE}, got {W}x{H}")
    return H, W


def active_cells(boxes, height, width):
    """(cell indexes, counts) of the active cells of a box list in a height x width picture, both int32 arrays in raster
    order: cell row * ceil(width / 16) + column, and its number of mask pixels.  Host only (no GPU is touched); the
    answer is kept with a FrameBoxes."""
    H, W = _size(height, width)
    boxes = X.as_boxes(boxes).validate(H, W, X.MAX_CLASSES)
    kept = getattr(boxes, "_roil_cells", None)
    if kept is not None and kept[0] == (H, W):
        return kept[1], kept[2]
    L, n = lib.hip(), len(boxes)
    ptr = boxes.array.ctypes.data if n else None
    A = L.dcvc_roil_cells(H, W, ptr, n, None, None, 0)
    if A < 0:
        raise lib.KernelError(f"roil_cells failed with status {A}")
    cells, counts = np.zeros(A, np.int32), np.zeros(A, np.int32)
    if A and L.dcvc_roil_cells(H, W, ptr, n, cells.ctypes.data, counts.ctypes.data, A) != A:
        raise lib.KernelError("roil_cells: two answers for one box list")
    boxes._roil_cells = ((H, W), cells, counts)
    return cells, counts


def _parse(b, counts):
    """The order of the refusals is dcvc_roil_check's: magic, version, step, A, the table, every entry (mode, then L),
    the total size."""
    if len(b) < HEADER:
        raise RoiLayerError(f"truncated record: {len(b)} bytes, the header alone has {HEADER}")
    if b[:2] != MAGIC:
        raise RoiLayerError(f"bad magic {b[:2]!r}: not a residual-layer record")
    if b[2] != VERSION:
        raise RoiLayerError(f"unknown version {b[2]} (this is version {VERSION})")
    if not 1 <= b[3] <= MAX_STEP:
        raise RoiLayerError(f"step {b[3]} out of range 1..{MAX_STEP}")
    A = int.from_bytes(b[4:8], "little")
    if counts is not None and A != len(counts):
        raise RoiLayerError(f"wrong number of active cells: the record has {A}, the boxes give {len(counts)}")
    if len(b) < HEADER + 6 * A:
        raise RoiLayerError(f"truncated record: {len(b)} bytes cannot hold the length table of {A} cells")
    entries = np.frombuffer(b, "<u2", 3 * A, HEADER).astype(np.int64).reshape(A, 3)
    m, L = entries >> 12, entries & 0xFFF
    bad = m > 9
    if counts is not None:
        n = counts.astype(np.int64)[:, None]
        bad = bad | ~np.where(m == 9, L == 0, np.where(m == 8, L == n, (L <= n) & (8 * L >= n * (m + 1))))
    if bad.any():
        a, c = (int(v[0]) for v in np.nonzero(bad))
        what = f"mode {int(m[a, c])} above 9" if m[a, c] > 9 else \
            {9: "mode 9 with a length", 8: "mode 8 with a length other than n"}.get(int(m[a, c]), "length out of bounds") + \
            f" (mode {int(m[a, c])}, L {int(L[a, c])}, n {int(n[a, 0])})"
        raise RoiLayerError(f"cell {a} channel {c}: {what}")
    ends = HEADER + 6 * A + np.cumsum(L.reshape(-1))
    total = int(ends[-1]) if A else HEADER
    if len(b) < total:
        raise RoiLayerError(f"truncated record: {len(b)} bytes, the segments need {total}")
    if len(b) > total:
        raise RoiLayerError(f"trailing bytes: {len(b)} bytes, the record ends at {total}")
    return {"step": b[3], "cells": A, "modes": m, "lengths": L, "offsets": (ends - L.reshape(-1)).reshape(A, 3)}


def parse_record(record):
    """{"step", "cells", "modes", "lengths", "offsets"} of a record: the (A, 3) arrays of the length table and the byte
    offset of every segment.  Refused by name (RoiLayerError): what the record shows without the boxes -- magic, version,
    step, a mode above 9, a length table or segments that end beyond the record, trailing bytes."""
    return _parse(bytes(record), None)


def check_record(record, counts):
    """parse_record, and the record held against the counts n_a of the boxes' active cells (active_cells): a wrong number
    of cells, a length that is impossible for n_a and the mode.  Returns parse_record's dictionary."""
    b = bytes(record)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    info = _parse(b, counts)
    rc = lib.hip().dcvc_roil_check(b, len(b), counts.ctypes.data if len(counts) else None, len(counts))
    if rc != 0:  # (the validation the decode entry point runs before it launches; it agrees with the above)
        raise RoiLayerError(f"{_REFUSALS.get(rc, 'refused')} (status {rc})")
    return info


# ------------------------------------------------------------------------------------------------------------ device
def _pinned(n_bytes, pool=None):
    import torch

    if pool is not None:
        for i, t in enumerate(pool):
            if t.numel() >= n_bytes:
                return pool.pop(i)
    return torch.empty(max(int(n_bytes), 64), dtype=torch.uint8).pin_memory()


def _table(cells, second, device):
    """A pairs of int32 {cell, second} through pinned memory on the current stream: (pinned, device) or (None, None)"""
    import torch

    if len(cells) == 0:
        return None, None
    pin = torch.from_numpy(np.stack([cells, second], 1).astype(np.int32).reshape(-1)).pin_memory()
    return pin, pin.to(device, non_blocking=True)


class PendingRecord:
    """A record on its way to the host: .bytes() waits for the copy behind the two launches and returns the record."""

    def __init__(self, host, event, cells, keep):
        self.host, self.event, self.cells, self._keep = host, event, cells, keep

    def bytes(self):
        self.event.synchronize()
        self._keep = None
        a = self.host.numpy()
        size = int(a[:4].view("<u4")[0])
        if not HEADER + 6 * self.cells <= size <= HEADER + CELL_MAX * self.cells:
            raise lib.KernelError(f"roil_encode: a record of {size} bytes for {self.cells} cells")
        return a[4:4 + size].tobytes()


def encode_layer(source, recon, boxes, step=1, pool=None):
    """Codes clip(code(source) - code(recon) + 128, 0, 255) inside the boxes, quantised with `step`, into a record: two
    launches and one copy of 8 + 774 A bytes (A: the active cells, known on the host) to pinned memory on the current
    stream.  Returns a PendingRecord; nothing is synchronised here.  pool: a list of pinned uint8 tensors to take the
    host buffer from (the caller puts .host back when it is done with it)."""
    import torch

    step = check_step(step)
    s, s_rs, s_ps = devargs.picture(source, "source")
    r, r_rs, r_ps = devargs.picture(recon, "recon", like=source)
    H, W = s.shape[2:]
    cells, _ = active_cells(boxes, H, W)
    A = len(cells)
    capacity = HEADER + CELL_MAX * A
    keep, host_boxes, dev_boxes, n = X._box_args(boxes, H, W, X.MAX_CLASSES, s.device)
    pin, table = _table(cells, np.zeros_like(cells), s.device)
    out = torch.empty(4 + capacity, dtype=torch.uint8, device=s.device)  # the size word, then the record
    staging = torch.empty(SLOT * A, dtype=torch.uint8, device=s.device) if A else None
    devargs.launch("dcvc_roil_encode", s.device, s.data_ptr(), s_rs, s_ps, r.data_ptr(), r_rs, r_ps, H, W, host_boxes, dev_boxes, n,
                   step, table.data_ptr() if A else None, A, staging.data_ptr() if A else None,
                   out.data_ptr() + 4, capacity, out.data_ptr())
    host = _pinned(4 + capacity, pool)
    host[:4 + capacity].copy_(out, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(s.device))
    return PendingRecord(host, ev, A, (keep, pin))


def decode_layer(record, boxes, height, width, layout="planar", order="rgb", out=None, device=None):
    """The 8-bit residual picture of a record for roi.fuse: r' inside the boxes, 0 outside, as a (3, H, W) ("planar") or
    (H, W, 3) ("hwc") uint8 tensor with channel order "rgb" or "gbr".  The record is validated against the boxes by name
    before anything is launched; a payload that does not decode raises RoiLayerError here, before the picture is
    handed on (one wait for the status word)."""
    import torch

    H, W = _size(height, width)
    if layout not in X.LAYOUTS:
        raise ValueError(f"layout must be one of {X.LAYOUTS}, got {layout!r}")
    o = X._order(order)
    b = bytes(record)
    cells, counts = active_cells(boxes, H, W)
    info = check_record(b, counts)
    dev = devargs.cuda_device(out.device if out is not None else "cuda" if device is None else device, "decode_layer")
    A = len(cells)
    with torch.cuda.device(dev):
        keep, host_boxes, dev_boxes, n = X._box_args(boxes, H, W, X.MAX_CLASSES, dev)
        if out is None:
            out = torch.empty((3, H, W) if layout == "planar" else (H, W, 3), dtype=torch.uint8, device=dev)
        cs, rs, px = X._u8_strides(out, layout, H, W, "out")
        pin, table = _table(cells, info["offsets"][:, 0] if A else cells, dev)
        rec_pin = torch.frombuffer(bytearray(b), dtype=torch.uint8).pin_memory()
        rec_dev = rec_pin.to(dev, non_blocking=True)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.hip().dcvc_roil_decode(b, rec_dev.data_ptr(), len(b), H, W, host_boxes, dev_boxes, n,
                                        table.data_ptr() if A else None, out.data_ptr(), cs, rs, px, *o, status.data_ptr(),
                                        devargs.stream(dev))
        if rc in _REFUSALS:
            raise RoiLayerError(f"{_REFUSALS[rc]} (status {rc})")
        lib.check(rc, "roil_decode")
        word = int(status.item())  # (waits for the launches: the record, the table and their pinned sources may go now)
    if word & BAD_STREAM:
        err = RoiLayerError("the payload does not decode (DCVC_ROIL_BAD_STREAM): a unary section short of set bits, or a "
                            "sample above 255")
        err.status = word
        raise err
    return out
