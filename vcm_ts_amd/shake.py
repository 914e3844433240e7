"""The shake of a fixed camera, taken out ahead of the scans (include/dcvc_hip_shake.h, csrc/shake.hip).

`boxes`, `noise` / --tnr-auto and everything that reads their results assume that a static pixel stays at the same
coordinates.  A camera on a pole or a bridge is fixed and still shakes by a few pixels; every cell then differs from the
picture before it, `boxes` answers the whole picture and the noise estimate measures texture.  A `Registrar` stands in front
of a scan: picture 0 is the ANCHOR, and every later picture is searched for in the anchor's luma -- a 2-D whole-pixel search
within +-radius on a sparse sample of every 64 x 64 tile (dcvc_shake_tiles), a median vote over the tiles that have an
opinion (dcvc_shake_vote) -- and moved onto the anchor by the one vector found, bit for bit, with the gather the prefilter
already has (dcvc_me_compensate).  The scan is handed the registered picture.

    ShakeParams(radius, min_votes=8, max_lost=25)      the setting
    Registrar(device, height, width, capacity, params)  .add(picture) -> the picture registered onto picture 0; .log()
    summary(log)                                        what the records say, in integers
    border_cells(dy, dx, height, width)                 the cells the replicated band of a registered picture touches
    check_lost(summary, params)                         the refusal of a source whose camera really moves

There is deliberately NO default radius, and `min_votes` = 8 and `max_lost` = 25 are UNTUNED PLACEHOLDERS: no machine of the
project holds a real video.  A picture is LOST (status != 0) when fewer than min_votes tiles vote or a median lies at
+-radius (the true motion may lie beyond the range, as in a pan); a lost picture is passed on unmoved.  LIMITS: whole pixels
only (what remains is at most half a pixel); translation only, no rotation and no zoom; picture 0 is the anchor for the whole
scan, with no re-anchoring: a slow change of light is survived (the tiles' SADs rise together), a camera that was moved is
lost from then on; the coding pass is not touched (--tnr-search finds the shake cell by cell there).

The kernels run on the caller's current stream and nothing is synchronised per picture.  There is no torch fallback: a CPU
tensor is a ValueError.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import MAX_SIDE, whole
from .roi import CELL, grid_of

SHAKE_JSON, VERSION = "shake.json", 1
TILE, MAX_R, MAX_TILES, WORDS, RECORD = 64, 16, 16384, 5, 8  # (DCVC_SHAKE_*)
FEW, EDGE = 1, 2
MIN_VOTES, MAX_LOST = 8, 25  # untuned placeholders


@dataclass(frozen=True)
class ShakeParams:
    """radius: the search range in whole pixels per axis (1..16; no default exists -- it is the largest shake expected, and
    a median AT the radius is taken for a pan).  min_votes: a picture with fewer voting tiles is lost (1..16384).  max_lost:
    a source with more than this many percent of its pictures lost is refused by the noise scan (0..100).  min_votes and
    max_lost are untuned placeholders."""
    radius: int
    min_votes: int = MIN_VOTES
    max_lost: int = MAX_LOST

    def __post_init__(self):
        object.__setattr__(self, "radius", whole("radius", self.radius, 1, MAX_R, "pixels"))
        object.__setattr__(self, "min_votes", whole("min_votes", self.min_votes, 1, MAX_TILES, "tiles"))
        object.__setattr__(self, "max_lost", whole("max_lost", self.max_lost, 0, 100, "percent"))

    def to_json(self):
        return {"radius": self.radius, "min_votes": self.min_votes, "max_lost": self.max_lost}


def _params(params):
    if not isinstance(params, ShakeParams):
        raise ValueError(f"params: expected a ShakeParams, got {type(params).__name__}")
    return params


class Registrar:
    """The anchor of a `height` x `width` sequence on `device` and the records of up to `capacity` pictures: the anchor's
    luma plane, the tile words, the uniform vector field, ONE scratch picture and a (capacity, 8) int32 log live on the
    device.  The scratch picture is what .add returns, so a returned picture is good until the next .add, and WHOEVER READS IT
    MUST DO SO ON THE STREAM OF THAT NEXT .add (or make that stream wait for the reader): consecutive .add calls are chained
    by the registrar's own event, which is recorded before the reader's kernel exists, so a reader left behind on another
    stream would see the scratch picture overwritten under it.  Every caller of the project reads it with the scan's kernel
    on the one stream the whole pass runs on."""

    def __init__(self, device, height, width, capacity, params):
        import torch

        device = devargs.cuda_device(device, "Registrar")
        if not (0 < int(height) <= MAX_SIDE and 0 < int(width) <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.params = _params(params)
        self.device, self.height, self.width, self.capacity, self.n = device, int(height), int(width), int(capacity), 0
        self.grid = grid_of(self.height, self.width)
        self.n_tiles = (self.height // TILE) * (self.width // TILE)
        self.y_stride = -(-self.width // 4) * 4
        self.anchor = torch.empty((self.height, self.y_stride), dtype=torch.uint8, device=device)
        self.tiles = torch.empty((max(self.n_tiles, 1), WORDS), dtype=torch.int32, device=device)
        self.mv = torch.empty((self.grid[0] * self.grid[1], 2), dtype=torch.int16, device=device)
        self.scratch = torch.empty((1, 3, self.height, self.width), dtype=torch.float32, device=device)
        self.records = torch.zeros((self.capacity, RECORD), dtype=torch.int32, device=device)
        self.records[0, 4] = self.n_tiles  # (the anchor's record: all zero but n_tiles)
        made = torch.cuda.Event()
        made.record(torch.cuda.current_stream(device))
        self._last = (torch.cuda.current_stream(device), made)  # (the zeroing runs here: another stream's first add waits for it)

    def add(self, picture):
        """The height x width crop of a (1, 3, Hp, Wp) float32 picture, read in place on the current stream: picture 0 is
        returned untouched (the argument itself) and becomes the anchor; every later one comes back registered onto it, as
        the (1, 3, height, width) scratch picture.  Nothing is synchronised."""
        import torch

        crop = devargs.checked(picture, "Registrar.add", device=self.device, at_least=(self.height, self.width), owner="registrar")
        if self.n >= self.capacity:
            raise ValueError(f"Registrar.add: picture {self.n} of a scan of {self.capacity} pictures")
        x, rs, ps = devargs.planar(crop)
        cur = torch.cuda.current_stream(self.device)
        if cur != self._last[0]:
            cur.wait_event(self._last[1])  # (the anchor and the scratch picture: a device-side dependency, the host waits for nothing)
        H, W, R = self.height, self.width, self.params.radius
        if self.n == 0:
            devargs.launch("dcvc_shake_plane", self.device, x.data_ptr(), rs, ps, H, W, self.anchor.data_ptr(), self.y_stride)
            out = picture
        else:
            devargs.launch("dcvc_shake_tiles", self.device, x.data_ptr(), rs, ps, H, W, self.anchor.data_ptr(), self.y_stride, R,
                           self.tiles.data_ptr())
            devargs.launch("dcvc_shake_vote", self.device, self.tiles.data_ptr(), self.n_tiles, R, self.params.min_votes, H, W,
                           self.records[self.n].data_ptr(), self.mv.data_ptr())
            devargs.launch("dcvc_me_compensate", self.device, x.data_ptr(), rs, ps, self.scratch.data_ptr(), W, H * W, H, W,
                           self.mv.data_ptr(), what="shake: me_compensate")
            out = self.scratch
        done = torch.cuda.Event()
        done.record(cur)
        self._last = (cur, done)
        self.n += 1
        return out

    def log(self):
        """(pictures added, 8) int64 on the host -- dy, dx, votes, agree, n_tiles, status, and the two medians before a
        status zeroed them: ONE device-to-host copy."""
        return self.records[:self.n].cpu().numpy().astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- host
def _log(log):
    a = np.asarray(log)
    if a.ndim != 2 or a.shape[1] != RECORD or a.dtype.kind not in "iu":
        raise ValueError(f"log: expected an (n, {RECORD}) integer array, got {a.shape} {a.dtype}")
    return [[int(v) for v in row] for row in a.tolist()]


def summary(log):
    """What the records of a scan say, in Python integers: pictures; moved (a vector other than (0, 0)); lost (status !=
    0); max_dy and max_dx, the largest |dy| and |dx| applied; min_agree, the smallest agree / votes over the pictures after
    the anchor that had a vote at all, as the pair [agree, votes] (compared by cross-multiplication, the first of equals;
    [0, 0] where no picture had a vote)."""
    rows = _log(log)
    worst = [0, 0]
    for r in rows[1:]:
        if r[2] > 0 and (worst[1] == 0 or r[3] * worst[1] < worst[0] * r[2]):
            worst = [r[3], r[2]]
    return {"pictures": len(rows), "moved": sum(1 for r in rows if r[0] or r[1]), "lost": sum(1 for r in rows if r[5]),
            "max_dy": max((abs(r[0]) for r in rows), default=0), "max_dx": max((abs(r[1]) for r in rows), default=0),
            "min_agree": worst}


def border_cells(dy, dx, height, width):
    """The boolean (hc, wc) mask of the 16 x 16 cells that hold a pixel of the band a picture registered by (dy, dx) has
    replicated from its edge: rows [0, dy) or [height + dy, height), columns [0, dx) or [width + dx, width)."""
    H, W = whole("height", height, 1, MAX_SIDE), whole("width", width, 1, MAX_SIDE)
    dy, dx = whole("dy", dy, -MAX_R, MAX_R), whole("dx", dx, -MAX_R, MAX_R)
    hc, wc = grid_of(H, W)

    def touched(d, side, cells):
        first = np.arange(cells) * CELL  # (a cell's pixels: [first, min(first + 16, side)), none from `side` on)
        inside = first < side
        if d > 0:
            return inside, first < min(d, side)
        if d < 0:
            return inside, np.minimum(first + CELL, side) > max(side + d, 0)
        return inside, np.zeros(cells, dtype=bool)

    (rows, by_rows), (cols, by_cols) = touched(dy, H, hc), touched(dx, W, wc)
    return (by_rows[:, None] | by_cols[None, :]) & rows[:, None] & cols[None, :]  # (a cell of the padding holds no pixel)


def mask_border(counts, log, height, width):
    """The (n, hc, wc) counts of a motion scan of registered pictures with every picture's border cells zeroed: the
    replicated band is not the scene, and without this 20 .. 40 spurious cells a picture stand along the edges."""
    out = np.array(counts)
    for t, r in enumerate(_log(log)):
        out[t][border_cells(r[0], r[1], height, width)] = 0
    return out


def document(log, params, height, width):
    """What shake.json and `run_codec shake` hold: version, size, parameters, the per-picture records and the summary."""
    return {"version": VERSION, "height": int(height), "width": int(width), "params": _params(params).to_json(),
            "records": _log(log), "summary": summary(log)}


def check_lost(summ, params):
    """A source with more than max_lost percent of its pictures lost is a ValueError by name: the camera moves."""
    p = _params(params)
    if summ["lost"] * 100 > p.max_lost * summ["pictures"]:
        raise ValueError(f"shake: {summ['lost']} of {summ['pictures']} pictures could not be registered within +-{p.radius} pixels "
                         f"(more than {p.max_lost} %): the camera moves, and what a noise scan measured would be motion; pass --tnr T "
                         f"(tnr.TNR) instead")
