"""ROI redaction on the codec's input (include/dcvc_hip_redact.h, csrc/redact.hip): inside the boxes of the selected
classes the picture the codec is handed is a mosaic of the source (every tile of a picture-aligned grid shows the rounded
mean of its own pixels) or a solid fill, everywhere else the source bit for bit.  It is ENCODER SIDE ONLY: it replaces the
picture the codec is handed and nothing else -- the .bin format does not change and the decoder needs to know nothing.
The arithmetic is stated in the header; tests/redact_ref.py restates it in numpy.

    Redact(classes, tile=None, fill=None, grow=0, hold=0, restorable=False)    the setting
    held_boxes(frames, g, mask, hold)                                          the merged list of one picture
    Redactor(redact, roi, size, device)             the state of ONE GOP stream on the device; .step(x_padded, boxes)
    redact_picture(x, boxes, redact, names)         one (1, 3, H, W) picture, for library use

A MOSAIC IS NOT A SECURITY GUARANTEE: small tiles over text can be partly inverted.  The solid fill removes the content.
There is deliberately NO default tile or fill.  Boxes are taken as given: a detector that misses a picture leaves it
untouched, and `hold` narrows that gap, it does not close it.  This is the mechanism, not a claim about rate or quality.

The kernel runs on the caller's current stream and synchronises nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import whole
from .roi import MAX_BOXES, MAX_CLASSES, MAX_GROW, FrameBoxes, as_boxes, grid_of
from .tnr import StreamFilter

TILES, MAX_FILL, MAX_HOLD = (2, 4, 8, 16, 32, 64), 255, 32


@dataclass(frozen=True)
class Redact:
    """classes: the NAMES of the box classes to redact (of the roi's: liplates, faces, motion).  Exactly one of tile (the
    mosaic's tile side: 2, 4, 8, 16, 32 or 64 pixels) and fill (the solid fill's 8-bit code, 0..255 on all three channels);
    neither has a default.  grow: pixels added to every side of a box (0..255).  hold: a picture is also redacted inside
    the boxes of the `hold` pictures before and after it (0..32) -- for a detector that misses a picture.  restorable: allow
    residuals= / residual_bins= beside it; those files then hold what was removed."""
    classes: tuple
    tile: int = None
    fill: int = None
    grow: int = 0
    hold: int = 0
    restorable: bool = False

    def __post_init__(self):
        names = (self.classes,) if isinstance(self.classes, str) else self.classes
        try:
            names = tuple(names)
        except TypeError:
            raise ValueError(f"classes: expected class names, got {self.classes!r}") from None
        if not names or len(names) > MAX_CLASSES or not all(isinstance(n, str) and n for n in names):
            raise ValueError(f"classes: expected 1..{MAX_CLASSES} class names, got {list(names)!r}")
        for n in names:
            if names.count(n) > 1:
                raise ValueError(f"classes: {n!r} is named twice")
        object.__setattr__(self, "classes", names)
        if (self.tile is None) == (self.fill is None):
            raise ValueError("exactly one of tile (a mosaic) and fill (a solid fill) must be given; neither has a default")
        if self.tile is not None and (isinstance(self.tile, bool) or not isinstance(self.tile, (int, np.integer)) or self.tile not in TILES):
            raise ValueError(f"tile must be one of {list(TILES)}, got {self.tile!r}")
        object.__setattr__(self, "tile", None if self.tile is None else int(self.tile))
        object.__setattr__(self, "fill", None if self.fill is None else whole("fill", self.fill, 0, MAX_FILL))
        object.__setattr__(self, "grow", whole("grow", self.grow, 0, MAX_GROW))
        object.__setattr__(self, "hold", whole("hold", self.hold, 0, MAX_HOLD))
        if not isinstance(self.restorable, (bool, np.bool_)):
            raise ValueError(f"restorable must be True or False, got {self.restorable!r}")
        object.__setattr__(self, "restorable", bool(self.restorable))

    def mask(self, names):
        """class_mask of dcvc_redact against the class names of a roi, in its order: bit c for class c."""
        names = tuple(names)
        for n in self.classes:
            if n not in names:
                raise ValueError(f"redact: no class {n!r} among the roi's classes {list(names)}")
        return sum(1 << names.index(n) for n in self.classes)

    def mode(self):
        """(tile, fill) as dcvc_redact takes them."""
        return (self.tile, -1) if self.tile is not None else (0, self.fill)

    def to_json(self):
        return {"classes": list(self.classes), "tile": self.tile, "fill": self.fill, "grow": self.grow, "hold": self.hold,
                "restorable": self.restorable}


def held_boxes(frames, g, mask, hold):
    """The list picture g is redacted with: the boxes of pictures g - hold .. g + hold that exist, in that order, whose class
    bit is set in `mask`; boxes of other classes are dropped.  frames: the FrameBoxes (or (n, 5) arrays) of every picture of
    the sequence.  Host work only.  More than MAX_BOXES boxes after merging is a ValueError naming the picture."""
    parts = []
    for t in range(max(g - hold, 0), min(g + hold, len(frames) - 1) + 1):
        a = as_boxes(frames[t]).array
        parts.append(a[((mask >> a[:, 4]) & 1) == 1] if len(a) else a)
    merged = np.concatenate(parts) if parts else np.zeros((0, 5), np.int32)
    if len(merged) > MAX_BOXES:
        raise ValueError(f"redact: picture {g} would be redacted with {len(merged)} boxes (its own and those held from its "
                         f"neighbours); at most {MAX_BOXES} per picture")
    return FrameBoxes(merged)


def _launch(src, out, out_rs, out_ps, h, w, boxes, mask, redact, count, device):
    """One dcvc_redact on the current stream of `device`: src a (1, 3, h, w) view, out the base of the result's crop."""
    s, srs, sps = devargs.planar(src)
    tile, fill = redact.mode()
    n = len(boxes)
    devargs.launch("dcvc_redact", device, s.data_ptr(), srs, sps, out.data_ptr(), out_rs, out_ps, h, w,
                   boxes.array.ctypes.data if n else None, boxes.on_device(device).data_ptr() if n else None, n,
                   mask, redact.grow, tile, fill, count.data_ptr())


class Redactor(StreamFilter):
    """The redaction of one GOP stream: tnr.StreamFilter's two pictures and the cells' counts.  I pictures and P pictures
    are treated alike, and no state passes from one picture to the next.  One Redactor serves one stream at a time.
    .totals(): |R| of every step, 0 for a picture that was not touched."""
    noun, untouched = "redactor", 0

    def __init__(self, redact, roi, size, device, totals=True):
        import torch

        from .roi import as_roi

        if not isinstance(redact, Redact):
            raise ValueError(f"redact: expected a redact.Redact, got {type(redact).__name__}")
        self.redact = redact
        self.names = tuple(as_roi(roi).names)
        self.mask = redact.mask(self.names)
        super().__init__(size, device, 1, totals)
        self.count = torch.empty(self.grid[0] * self.grid[1], dtype=torch.int16, device=self.device)  # (uint16 words, <= 256)
        torch.cuda.synchronize(self.device)  # (the fills above: a stream that uses them afterwards cannot race them)

    def step(self, x_padded, boxes):
        """The padded picture to code in place of `x_padded`.  boxes: the picture's merged list (held_boxes).  A picture
        whose list is empty launches nothing and is returned itself.  Any other is one dcvc_redact launch on the current
        stream from the crop of x_padded into the crop of one of the two buffers, which stays valid until the step after
        the next."""
        self._check(x_padded)
        boxes = as_boxes(boxes).validate(self.height, self.width, len(self.names))
        t, self.n = self.n, self.n + 1
        if len(boxes) == 0:
            return x_padded
        out = self.bufs[self.launches & 1]
        (h, w), (Hp, Wp) = (self.height, self.width), self.padded
        _launch(x_padded.detach()[..., :h, :w], out, Wp, Hp * Wp, h, w, boxes, self.mask, self.redact, self.count, self.device)
        self.launches += 1
        self._keep(t, self.count)
        return out


def redact_picture(x, boxes, redact, names):
    """One (1, 3, H, W) float32 picture on the GPU, redacted inside `boxes` (its own list; nothing is held): (the new
    picture, the (hc, wc) int16 counts of R per 16 x 16 cell).  names: the class names `boxes`' cls values index.  One launch
    on the current stream, nothing synchronised; an empty list still launches (the result is a copy)."""
    import torch

    if not isinstance(redact, Redact):
        raise ValueError(f"redact: expected a redact.Redact, got {type(redact).__name__}")
    names = tuple(names)
    mask = redact.mask(names)
    src = devargs.checked(x, "redact_picture")
    h, w = src.shape[2:]
    boxes = as_boxes(boxes).validate(h, w, len(names))
    hc, wc = grid_of(h, w)
    out = torch.empty((1, 3, h, w), dtype=torch.float32, device=src.device)
    count = torch.empty((hc, wc), dtype=torch.int16, device=src.device)
    _launch(src, out, w, h * w, h, w, boxes, mask, redact, count, src.device)
    return out, count
