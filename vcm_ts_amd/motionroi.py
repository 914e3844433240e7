"""Motion ROI boxes (include/dcvc_hip_motion.h, csrc/motion.hip): boxes around what moves in front of a fixed camera,
made by this repository alone -- the ROI pipeline's own source of boxes where the reference's two detectors are out of
scope.

A per-pixel background model of the luma lives on the device (`MotionScan`): one kernel per picture updates it and counts,
per 16 x 16 cell of the q-map grid, the pixels that differ from it by more than `threshold` codes.  The counts of the whole
sequence come back in ONE copy; `boxes_from_counts` turns each picture's grid into boxes with pure integer numpy, the
same decision on every host; `write_boxes` records them as a third box class ("motion") in the reference's coordinate
format, so that the folder is an ordinary --roi-root.

There is deliberately NO default threshold, and `learn`, `min_pixels` and `grow` are UNTUNED PLACEHOLDERS: no machine
of the project holds a real video.  This is the mechanism -- detected, recorded, read back and coded to identical bits --
not a claim about detection quality.  The model starts as picture 0, so picture 0 has no boxes, and an object that moves
away leaves a ghost where it stood in picture 0 until k_fg has absorbed it.

The kernel runs on the caller's current stream and synchronises nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import MAX_SIDE, whole
from .roi import CELL, MAX_BOXES, grid_of

MOTION_JSON, COORDS, VERSION = "motion.json", "motion_coords", 1
MAX_T, MAX_K, MAX_GROW_CELLS = 254, 16, 8


@dataclass(frozen=True)
class MotionParams:
    """threshold: a pixel is foreground when its luma is more than this many 8-bit codes from the model (1..254; no
    default exists).  learn = (k_bg, k_fg): the model moves by |difference| >> k toward the picture, k_bg where the pixel
    is background, k_fg where it is foreground (0..16 each; 0 follows the picture, 16 freezes).  min_pixels: a cell is
    active from this many foreground pixels (1..256).  grow: active cells are dilated by this many cells before they are
    joined (0..8).  min_cells: a region needs this many active cells (1..65535).  max_boxes: at most this many boxes per
    picture, the strongest first (1..roi.MAX_BOXES).  learn, min_pixels and grow are untuned placeholders."""
    threshold: int
    learn: tuple = (4, 8)
    min_pixels: int = 8
    grow: int = 1
    min_cells: int = 1
    max_boxes: int = 64

    def __post_init__(self):
        object.__setattr__(self, "threshold", whole("threshold", self.threshold, 1, MAX_T))
        try:
            k_bg, k_fg = self.learn
        except (TypeError, ValueError):
            raise ValueError(f"learn must be a pair (k_bg, k_fg), got {self.learn!r}") from None
        object.__setattr__(self, "learn", (whole("learn[0] (k_bg)", k_bg, 0, MAX_K), whole("learn[1] (k_fg)", k_fg, 0, MAX_K)))
        object.__setattr__(self, "min_pixels", whole("min_pixels", self.min_pixels, 1, CELL * CELL))
        object.__setattr__(self, "grow", whole("grow", self.grow, 0, MAX_GROW_CELLS))
        object.__setattr__(self, "min_cells", whole("min_cells", self.min_cells, 1, 65535))
        object.__setattr__(self, "max_boxes", whole("max_boxes", self.max_boxes, 1, MAX_BOXES))

    def to_json(self):
        return {"threshold": self.threshold, "learn": list(self.learn), "min_pixels": self.min_pixels, "grow": self.grow,
                "min_cells": self.min_cells, "max_boxes": self.max_boxes}

    @classmethod
    def from_json(cls, info):
        keys = {"threshold", "learn", "min_pixels", "grow", "min_cells", "max_boxes"}
        if not isinstance(info, dict) or set(info) != keys or not isinstance(info["learn"], list):
            raise ValueError(f"expected the keys {sorted(keys)}")
        return cls(**dict(info, learn=tuple(info["learn"])))


def _params(params):
    if not isinstance(params, MotionParams):
        raise ValueError(f"params: expected a MotionParams, got {type(params).__name__}")
    return params


class MotionScan:
    """The background model of a `height` x `width` sequence on `device` and the counts of up to `capacity` pictures, one
    row of a (capacity, hc * wc) uint16 tensor each."""

    def __init__(self, device, height, width, capacity, params):
        import torch

        device = devargs.cuda_device(device, "MotionScan")
        if not (0 < int(height) <= MAX_SIDE and 0 < int(width) <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.params = _params(params)
        self.device, self.height, self.width, self.capacity, self.n = device, int(height), int(width), int(capacity), 0
        self.grid = grid_of(self.height, self.width)
        # (every word of both is written by the kernel before anything reads it: nothing to zero, no stream to wait for)
        self.bg = torch.empty((self.height, self.width), dtype=torch.uint16, device=device)
        self.cells = torch.empty((self.capacity, self.grid[0] * self.grid[1]), dtype=torch.uint16, device=device)
        self._last = None

    def add(self, picture):
        """One step on the height x width crop of a (1, 3, Hp, Wp) float32 picture, read in place, on the current stream;
        its counts land in the next row.  The first picture initialises the model (all counts 0)."""
        import torch

        crop = devargs.checked(picture, "MotionScan.add", device=self.device, at_least=(self.height, self.width), owner="scan")
        if self.n >= self.capacity:
            raise ValueError(f"MotionScan.add: picture {self.n} of a scan of {self.capacity} pictures")
        x, rs, ps = devargs.planar(crop)
        cur = torch.cuda.current_stream(self.device)
        if self._last is not None and cur != self._last[0]:
            cur.wait_event(self._last[1])  # (the model is a recursion: a device-side dependency, the host waits for nothing)
        devargs.launch("dcvc_motion_step", self.device, x.data_ptr(), rs, ps, self.height, self.width, self.bg.data_ptr(),
                       int(self.n == 0), self.params.threshold, *self.params.learn, self.cells[self.n].data_ptr())
        done = torch.cuda.Event()
        done.record(cur)
        self._last = (cur, done)
        self.n += 1

    def counts(self):
        """(pictures added, hc, wc) int32 on the host: ONE device-to-host copy."""
        return self.cells[:self.n].cpu().numpy().astype(np.int32).reshape(self.n, *self.grid)


# --------------------------------------------------------------------------------------------------------------- host
def _dilate(active, grow):
    """The maximum of a boolean grid over the (2 grow + 1)^2 neighbourhood, clipped at the grid's edge."""
    out = active.copy()
    for axis in (0, 1):
        src = out.copy()
        for d in range(1, grow + 1):
            lo, hi = [slice(None)] * 2, [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, -d), slice(d, None)
            out[tuple(hi)] |= src[tuple(lo)]
            out[tuple(lo)] |= src[tuple(hi)]
    return out


def _components(mask):
    """Labels 1 .. n of the 8-connected components of a boolean grid (0 elsewhere), and n.  Row runs joined with a
    union-find: a run touches the runs of the row above that it overlaps by at least a corner."""
    hc, wc = mask.shape
    parent, runs, above = [], [], []  # runs: (row, start, end) with end exclusive; above: the run numbers of the last row

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in range(hc):
        edge = np.flatnonzero(np.diff(np.concatenate(([0], mask[i].astype(np.int8), [0]))))
        here = []
        for s, e in zip(edge[0::2].tolist(), edge[1::2].tolist()):
            k = len(runs)
            runs.append((i, s, e))
            parent.append(k)
            here.append(k)
            for j in above:
                if runs[j][1] <= e and s <= runs[j][2]:
                    ra, rb = find(j), find(k)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
        above = here
    labels, names = np.zeros((hc, wc), dtype=np.int32), {}
    for k, (i, s, e) in enumerate(runs):
        labels[i, s:e] = names.setdefault(find(k), len(names) + 1)
    return labels, len(names)


def boxes_from_counts(counts_2d, height, width, params):
    """The (n, 4) int32 boxes x1, y1, x2, y2 (half-open, pixels) of one picture's (hc, wc) counts:
    1. active = counts >= min_pixels;  2. dilated = the maximum of active over the (2 grow + 1)^2 cell neighbourhood,
    clipped at the grid's edge;  3. the 8-connected components of dilated;  4. a component with fewer than min_cells
    cells of active is dropped;  5. a component's box is the bounding rectangle of its cells in pixels, x2 clipped to
    width and y2 to height, dropped if empty;  6. of more than max_boxes those with the largest sum of counts over their
    active cells are kept, ties toward the smaller (y1, x1, y2, x2);  7. sorted by (y1, x1, y2, x2).
    Integer numpy on the host."""
    p = _params(params)
    H, W = int(height), int(width)
    if not (0 < H <= MAX_SIDE and 0 < W <= MAX_SIDE):
        raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {W}x{H}")
    c = np.asarray(counts_2d)
    if c.ndim != 2 or c.dtype.kind not in "iu" or tuple(c.shape) != grid_of(H, W):
        raise ValueError(f"counts: expected an integer grid of {grid_of(H, W)} cells for a {W}x{H} picture, got "
                         f"{c.shape} {c.dtype}")
    c = c.astype(np.int64)
    active = c >= p.min_pixels
    labels, n = _components(_dilate(active, p.grow))
    found = []
    for k in range(1, n + 1):
        ii, jj = np.nonzero(labels == k)
        mine = active[ii, jj]
        if int(mine.sum()) < p.min_cells:
            continue
        x1, y1 = CELL * int(jj.min()), CELL * int(ii.min())
        x2, y2 = min(CELL * (int(jj.max()) + 1), W), min(CELL * (int(ii.max()) + 1), H)
        if x2 <= x1 or y2 <= y1:
            continue
        found.append((-int(c[ii, jj][mine].sum()), y1, x1, y2, x2))
    if len(found) > p.max_boxes:
        found = sorted(found)[:p.max_boxes]
    found = sorted(f[1:] for f in found)
    return np.array([(x1, y1, x2, y2) for y1, x1, y2, x2 in found], dtype=np.int32).reshape(-1, 4)


def boxes_of_scan(counts, height, width, params):
    """boxes_from_counts of every picture of MotionScan.counts(); picture 0 (the model's own) has none."""
    return [np.zeros((0, 4), np.int32) if t == 0 else boxes_from_counts(c, height, width, params)
            for t, c in enumerate(counts)]


def scan(pictures, n_frames, size, device, params):
    """The whole pass: `pictures` yields every picture of the sequence once, in order, as the coding pass will see it (same
    reader, same conversion, padded or not); each is one launch, and the counts are read back in one copy at the end.
    size: (height, width), unpadded.  Returns the list of n_frames (n, 4) int32 box arrays."""
    import torch

    h, w = size
    if int(n_frames) < 1:
        raise ValueError(f"no frames to scan, got {n_frames}")
    run = MotionScan(device, h, w, n_frames, params)
    with torch.no_grad():
        for x in pictures:
            run.add(x)
    if run.n != n_frames:
        raise ValueError(f"the scan pass saw {run.n} pictures of {n_frames}")
    return boxes_of_scan(run.counts(), h, w, params)


# -------------------------------------------------------------------------------------------------------------- files
def read_info(root):
    """motion.json of `root` as (MotionParams, height, width, frames), or None without the file."""
    from .stream import read_sidecar

    found = read_sidecar(root, MOTION_JSON)
    if found is None:
        return None
    path, info = found
    try:
        if not isinstance(info, dict) or set(info) - {"shake"} != {"version", "height", "width", "frames", "params"}:
            raise ValueError("expected the keys version, height, width, frames and params")  # ("shake": informational, run_codec boxes --shake)
        if info["version"] != VERSION:
            raise ValueError(f"format version {info['version']!r}, this code reads {VERSION}")
        size = tuple(whole(k, info[k], 1, MAX_SIDE) for k in ("height", "width"))
        return MotionParams.from_json(info["params"]), size[0], size[1], whole("frames", info["frames"], 1, 2 ** 31 - 1)
    except ValueError as ex:
        raise ValueError(f"{path}: {ex}") from None


def write_boxes(root, per_frame_boxes, params, height, width, shake=None):
    """`root`/motion_coords/%05d, numbered from 1: one pickled np.uint16 (n, 4) array of x1, y1, x2, y2 per frame, empty
    ones included (the reference's coordinate format: roi.PickleBoxes reads the folder as class "motion"), and
    `root`/motion.json with the parameters, the size, the frame count and a format version.  Refused: a motion_coords
    that already holds the files of a run with another frame count or size (or of unknown origin) -- nothing is mixed.
    shake: what motion.json records under "shake" (the registration's setting and summary, vcm_ts_amd/shake.py); None: no
    such key."""
    from .stream import write_sidecar

    p = _params(params)
    H, W = whole("height", height, 1, MAX_SIDE), whole("width", width, 1, MAX_SIDE)
    arrays = []
    for t, b in enumerate(per_frame_boxes):
        a = np.asarray(b)
        if a.size == 0:
            a = np.zeros((0, 4), np.int32)
        if a.ndim != 2 or a.shape[1] != 4 or a.dtype.kind not in "iu":
            raise ValueError(f"frame {t + 1}: expected an (n, 4) integer array of x1, y1, x2, y2, got {a.shape} {a.dtype}")
        if len(a) > MAX_BOXES:
            raise ValueError(f"frame {t + 1}: too many boxes: {len(a)} (at most {MAX_BOXES} per picture)")
        if len(a) and (a.min() < 0 or a[:, [0, 2]].max() > W or a[:, [1, 3]].max() > H):
            raise ValueError(f"frame {t + 1}: coordinates out of range for a {W}x{H} picture")
        arrays.append(a.astype(np.uint16))
    if not arrays:
        raise ValueError("no frames to write")
    folder = os.path.join(root, COORDS)
    if os.path.isdir(folder) and os.listdir(folder):
        old = read_info(root)
        if old is None:
            raise ValueError(f"{folder} holds files and {os.path.join(root, MOTION_JSON)} does not say whose; remove them first")
        if old[1:] != (H, W, len(arrays)):
            raise ValueError(f"{folder} holds the boxes of another run ({old[3]} frames of {old[2]}x{old[1]}, this one has "
                             f"{len(arrays)} of {W}x{H}); remove them first")
    os.makedirs(folder, exist_ok=True)
    for t, a in enumerate(arrays):
        with open(os.path.join(folder, "%05d" % (t + 1)), "wb") as f:
            pickle.dump(a, f)
    write_sidecar(root, MOTION_JSON, dict({"version": VERSION, "height": H, "width": W, "frames": len(arrays), "params": p.to_json()},
                                         **({} if shake is None else {"shake": shake})))
