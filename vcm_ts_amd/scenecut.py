"""Scene-cut I pictures: where the I pictures of a sequence go (include/dcvc_hip_scene.h, csrc/scene.hip).

A picture is summarised on the device by sixteen regional luma histograms (a 4 x 4 grid of cells, 32 bins each: 512
integers).  The distance of two consecutive pictures is half the L1 distance of their histograms over the pixel count:
0 = identical regional histograms, 1 = disjoint.  `plan` turns the distances into the frame numbers of the I pictures
and `GopPlan` is the one place that knows picture types: the file loops of run_codec ask it which frames are I, where
a GOP ends and which frames a GOP stream codes.

There is deliberately NO default threshold: a good value depends on content nobody could measure here (no real video on
any machine of the project).  On the project's synthetic clips consecutive frames measure 0.01 - 0.11 depending on the
picture size.  This is I-picture PLACEMENT -- detected, recorded, coded and decoded to identical bits -- not a claim about
rate or quality.

The kernel runs on the caller's current stream and synchronises nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

import bisect

import numpy as np

from . import devargs
from .devargs import MAX_SIDE

COUNTERS = 512


class SceneScan:
    """The histograms of up to `capacity` pictures of `height` x `width` on `device`, one row of a (capacity, 512)
    uint32 tensor each, zeroed once."""

    def __init__(self, device, height, width, capacity):
        import torch

        device = devargs.cuda_device(device, "SceneScan")
        if not (0 < int(height) <= MAX_SIDE and 0 < int(width) <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.device, self.height, self.width, self.capacity, self.n = device, int(height), int(width), int(capacity), 0
        self.hist = torch.zeros((self.capacity, COUNTERS), dtype=torch.uint32, device=device)
        self._stream = torch.cuda.current_stream(device)  # (the zeroing runs here: another stream's first add waits for it)
        self._zeroed = torch.cuda.Event()
        self._zeroed.record(self._stream)

    def add(self, picture, row=None):
        """Count the height x width crop of a (1, 3, Hp, Wp) float32 picture, read in place, into the next row (or ONTO
        row `row`, which then is not advanced) on the current stream."""
        import torch

        crop = devargs.checked(picture, "SceneScan.add", device=self.device, at_least=(self.height, self.width), owner="scan")
        at = self.n if row is None else int(row)
        if not 0 <= at < self.capacity:
            raise ValueError(f"SceneScan.add: row {at} of a scan of {self.capacity} pictures")
        x, rs, ps = devargs.planar(crop)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            cur.wait_event(self._zeroed)  # (a device-side dependency: the host waits for nothing)
        devargs.launch("dcvc_scene_hist", self.device, x.data_ptr(), rs, ps, self.height, self.width, self.hist[at].data_ptr())
        if row is None:
            self.n += 1

    def histograms(self):
        """(pictures added, 512) int64 on the host: ONE device-to-host copy."""
        return self.hist[:self.n].cpu().numpy().astype(np.int64)

    def distances(self):
        """float64 d with d[0] = 0 and d[t] = sum(|hist[t] - hist[t - 1]|) / (2 H W), from the integers, on the host."""
        return distances(self.histograms(), self.height, self.width)


def distances(hists, height, width):
    hists = np.asarray(hists, dtype=np.int64)
    d = np.zeros(len(hists), dtype=np.float64)
    if len(hists) > 1:
        d[1:] = np.abs(hists[1:] - hists[:-1]).sum(axis=1) / (2.0 * height * width)
    return d


def check_options(gop, threshold, min_gop):
    """What `plan` and the file loops refuse, by name."""
    if int(gop) != gop or gop < 1:
        raise ValueError(f"gop must be a positive integer, got {gop!r}")
    if threshold is not None and not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"scenecut: the threshold must lie in (0, 1], got {threshold!r}")
    if int(min_gop) != min_gop or not 1 <= min_gop <= gop:
        raise ValueError(f"min_gop must be an integer within 1..gop ({gop}), got {min_gop!r}")


def plan(d, gop, threshold, min_gop=1):
    """The frame numbers of the I pictures of len(d) frames.  Frame 0 is I; walking t = 1 .. n - 1 with
    since = t - (the last I): since >= gop gives I (a GOP's maximum length), else d[t] > threshold (strictly) and
    since >= min_gop gives I, else P.  A cut that min_gop suppresses stays a P picture: nothing is deferred.
    threshold=None: exactly the multiples of gop."""
    check_options(gop, threshold, min_gop)
    out, last = ([0] if len(d) else []), 0
    for t in range(1, len(d)):
        since = t - last
        if since >= gop or (threshold is not None and d[t] > threshold and since >= min_gop):
            out.append(t)
            last = t
    return out


class GopPlan:
    """The I pictures of a sequence of `n_frames` frames: GOP j is the frames i_pictures[j] .. i_pictures[j + 1] - 1."""

    def __init__(self, n_frames, i_pictures):
        n_frames = int(n_frames)
        if n_frames < 0:
            raise ValueError(f"GopPlan: frames must not be negative, got {n_frames}")
        try:
            i_pictures = [int(g) for g in i_pictures]
        except (TypeError, ValueError):
            raise ValueError("GopPlan: i_pictures must be a list of frame numbers") from None
        if n_frames and (not i_pictures or i_pictures[0] != 0):
            raise ValueError("GopPlan: i_pictures does not start at 0 (the first frame is an I picture)")
        if any(b <= a for a, b in zip(i_pictures, i_pictures[1:])):
            raise ValueError("GopPlan: i_pictures is not strictly increasing")
        if i_pictures and i_pictures[-1] >= max(n_frames, 1):
            raise ValueError(f"GopPlan: i_pictures reaches frame {i_pictures[-1]} of a sequence of {n_frames} frames")
        self.n_frames, self.i_pictures, self._set = n_frames, i_pictures, frozenset(i_pictures)

    @classmethod
    def fixed(cls, n_frames, gop):
        """An I picture at every multiple of `gop`."""
        return cls(n_frames, list(range(0, int(n_frames), int(gop))))

    @property
    def n_gops(self):
        return len(self.i_pictures)

    def is_intra(self, g):
        return g in self._set

    def is_gop_end(self, g):
        """Frame g is the last picture of its GOP."""
        return g + 1 in self._set or g + 1 == self.n_frames

    def gop_of(self, g):
        if not 0 <= g < self.n_frames:
            raise IndexError(f"frame {g} of {self.n_frames}")
        return bisect.bisect_right(self.i_pictures, g) - 1

    def gop_range(self, j):
        return range(self.i_pictures[j], self.i_pictures[j + 1] if j + 1 < self.n_gops else self.n_frames)

    def order(self, k, K):
        """The frame numbers GOP stream k of K codes, in its coding order: GOPs k, k + K, ... whole and in order."""
        return [g for j in range(k, self.n_gops, K) for g in self.gop_range(j)]

    def __eq__(self, other):
        return isinstance(other, GopPlan) and (self.n_frames, self.i_pictures) == (other.n_frames, other.i_pictures)

    def __repr__(self):
        return f"GopPlan({self.n_frames}, {self.i_pictures})"

    def to_json(self):
        return {"frames": self.n_frames, "i_pictures": list(self.i_pictures)}

    @classmethod
    def from_json(cls, obj):
        if not isinstance(obj, dict) or "frames" not in obj or "i_pictures" not in obj:
            raise ValueError('GopPlan: expected {"frames": n, "i_pictures": [...]}')
        return cls(obj["frames"], obj["i_pictures"])
