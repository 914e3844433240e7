"""A motion-adaptive temporal noise prefilter (include/dcvc_hip_tnr.h, csrc/tnr.hip; with a motion search in front of it
include/dcvc_hip_me.h, csrc/me.hip, to quarter pixels include/dcvc_hip_mesub.h, csrc/mesub.hip, and per 8 x 8 sub-cell
include/dcvc_hip_mesplit.h, csrc/mesplit.hip, and a hierarchical search that reaches 128 pixels include/dcvc_hip_mepyr.h,
csrc/mepyr.hip) for fixed-camera
content, where a P picture's bits are dominated by sensor noise: every
P picture the codec is handed is blended with the previous filtered picture wherever the luma of the two stays close over
a 5 x 5 window, and passed through untouched wherever something moves.  It is ENCODER SIDE ONLY: it replaces the picture the codec is handed and nothing else -- no side file, no change
of the .bin format, nothing for the decoder to know.  The arithmetic is stated in the header; tests/tnr_ref.py restates it
in numpy, tests/me_ref.py the search and the compensation, tests/mesub_ref.py the quarter-pel refinement and interpolation,
tests/mesplit_ref.py the re-selection per sub-cell, tests/mepyr_ref.py the hierarchical search.

    TNR(threshold, floor=64, pixel=None, search=None, penalty=4, intra=None, subpel=False, split=False, levels=None)
                                             the setting; .table() the 256 weights, .rcp_table() dcvc_tnr_fuse's reciprocals
    AutoTNR(scale=3.0, min_cells=1024, ...)   the setting without its threshold; .resolve(noise estimate) -> TNR
    TnrFilter(tnr, size, device)             the state of ONE GOP stream on the device; .step(x_padded, intra, ahead=())
    StreamFilter                             what TnrFilter shares with redact.Redactor: validation, pictures, totals

There is deliberately NO default threshold, and `floor` and `pixel` are UNTUNED PLACEHOLDERS: no machine of the project
holds a real video.  (AutoTNR takes the threshold from the source's own measured noise level instead, vcm_ts_amd/noise.py;
its `scale` and `min_cells` are untuned placeholders too.)  This is the mechanism -- filtered, coded, decoded by an
unchanged decoder -- not a claim about rate
or quality.  Without `search`, moving pixels are passed through, not followed.  With search=R the filter is MOTION
COMPENSATED (opt-in): every 16 x 16 cell of a P picture is searched for in the previous filtered picture within +-R whole
pixels (dcvc_me_search: luma SAD plus `penalty` codes per pixel of vector length), that picture is moved cell by cell
(dcvc_me_compensate) and the unchanged dcvc_tnr_step blends against the moved picture, so a moving object is blended with
where it was.  `penalty` is an untuned placeholder too.  Vectors are whole pixels, blocks do not overlap, and the search
is exhaustive on one level (hierarchical with levels, below).  With subpel=True (opt-in, belongs to search) every vector is refined to QUARTER pixels over the
49 candidates around it (dcvc_me_refine) and the picture is moved through a separable 7/8-tap interpolation filter
(dcvc_me_compensate_sub in place of dcvc_me_compensate): an object that moves by a fraction of a pixel is blended with an
interpolated copy of where it was, not with a misregistered one.  With split=True (opt-in, belongs to search, with or without
subpel) every 8 x 8 quarter of a cell chooses again among the vectors that exist already, its own cell's and the eight
neighbours' (dcvc_me_split: the same luma SAD and penalty, over 64 pixels), and the picture is moved sub-cell by sub-cell
(dcvc_me_compensate_split in place of the cell compensation): a cell that straddles an object's edge no longer moves all of
its pixels by a vector that is right for a part of them.  No new search range and no new filter; cells on an edge are still
worse than the unfiltered source (what remains is the blend's window test, which is unchanged).

With levels=L (opt-in, 1 or 2, belongs to search) the search is HIERARCHICAL and search may be 2 .. 64 (L = 1) or 4 .. 128
(L = 2): the luma of both pictures is reduced to L coarser levels of 2 x 2 rounded means (dcvc_me_pyramid), the coarsest level
is searched exhaustively within ceil(R / 2^L) of its pixels (dcvc_me_coarse), and every level below chooses among the few
vectors around twice the level above's and (0, 0) (dcvc_me_descend: 9 + 1 candidates at level 1, 25 + 1 at level 0).  It
writes the three arrays dcvc_me_search writes, so everything behind it is unchanged.  On tests/mepyr_ref.py's fast clip
(band-limited texture, an object moving 39 .. 61 pixels a picture) the full search at R = 32 finds the true vector in NO cell
inside the object and leaves 6.6 .. 14.8 times the noisy source's squared error there; L = 1 at R = 64 finds it in every such
cell, L = 2 in 75 .. 100 % of them, at 0.30 .. 1.51 and 0.42 .. 1.23 (one picture 3.40) of the source's error, and static
ground stays at (0, 0).  FINE TEXTURE DEFEATS IT: with the frequencies of tests/mesub_ref.py's clip (0.08 .. 0.16 cycles a
pixel) the 2 x 2 means alias the texture and the true vector is found only where the step is a multiple of the coarsest
level's pixel.  Cells on the object's edge remain what they are.  Nothing is tuned: not the descents' windows, not the
scaling of the penalty between levels.  subpel and split stop at search = 32 until their kernels (which clamp incoming
vectors to +-32 and pack 9 bits a component) are widened: beyond it both are refused.

With intra=K (opt-in, 1 .. 4, no default) the I picture is filtered too (include/dcvc_hip_tnr_fuse.h, csrc/tnr_fuse.hip;
tests/tnr_fuse_ref.py restates it): it has no filtered predecessor, so it is blended in ONE pass with up to K pictures
that FOLLOW it in its own GOP, each weighted on its own by the same window and weight rule -- with `search`, each moved onto
the I picture first.  The filtered I picture is the first reference of the recursive filter.  K is untuned as well.

The kernels run on the caller's current stream and synchronise nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import MAX_SIDE, whole
from .roi import grid_of

MAX_T, MAX_FLOOR, MAX_P, FULL = 64, 255, 255, 256
MAX_R, MAX_LAMBDA, PENALTY = 32, 255, 4  # (DCVC_ME_MAX_R, DCVC_ME_MAX_LAMBDA; the placeholder)
MAX_REFS, RCP = 4, 1021  # (DCVC_TNR_FUSE_MAX_REFS, DCVC_TNR_FUSE_RCP)
SUBPEL = 4  # (DCVC_MESUB_UNIT: with subpel, vectors are in 1 / 4 pixels)
SPLIT = 8  # (DCVC_MESPLIT_SUB: with split, a vector per 8 x 8 sub-cell)
MAX_LEVELS, PYR_R = 2, 64  # (DCVC_MEPYR_MAX_LEVELS; with levels = L, search is 2 L .. 64 L)
ROWS = 64  # pictures' totals kept on the device between two copies to the host


@dataclass(frozen=True)
class TNR:
    """threshold T: a pixel whose 5 x 5 window differs from the previous filtered picture by T luma codes or more on
    average is passed through (1..64; no default exists -- AutoTNR measures one from the source).  floor: the weight of
    the current picture, in 1/256ths, where
    nothing differs at all (1..255); between 0 and T the weight rises linearly to 256.  pixel P: a pixel whose own luma
    differs by more than P codes is passed through whatever its window says (0..255; None: min(255, 3 T)).  search R: the
    reference of the blend is the previous filtered picture moved cell by cell by the vectors of a full search within +-R
    pixels (1..32; None: no search, nothing moved).  penalty: what a pixel of vector length costs the search, in luma codes
    of the cell's SAD (0..255; belongs to search).  floor, pixel and penalty are untuned placeholders.  intra K: an I
    picture is blended with up to K pictures that follow it in its GOP (1..4; None: I pictures are passed through; no
    default of substance exists and no value is tuned).  subpel: the search's vectors are refined to quarter pixels and the
    reference is interpolated (belongs to search; False: whole pixels).  split: every 8 x 8 sub-cell chooses again among its
    cell's vector and the eight neighbours' and the reference is moved sub-cell by sub-cell (belongs to search; False: one
    vector a cell).  levels L: the search is hierarchical over L coarser levels of 2 x 2 means (1 or 2; belongs to search,
    which may then be 2..64 for L = 1 and 4..128 for L = 2; None: the full search on one level, search 1..32); subpel and
    split stop at search = 32."""
    threshold: int
    floor: int = 64
    pixel: int = None
    search: int = None
    penalty: int = PENALTY
    intra: int = None
    subpel: bool = False
    split: bool = False
    levels: int = None

    def __post_init__(self):
        object.__setattr__(self, "threshold", whole("threshold", self.threshold, 1, MAX_T))
        object.__setattr__(self, "floor", whole("floor", self.floor, 1, MAX_FLOOR))
        object.__setattr__(self, "pixel", min(MAX_P, 3 * self.threshold) if self.pixel is None else whole("pixel", self.pixel, 0, MAX_P))
        object.__setattr__(self, "penalty", whole("penalty", self.penalty, 0, MAX_LAMBDA))
        if self.search is None:
            if self.penalty != PENALTY:
                raise ValueError(f"penalty belongs to search: got penalty={self.penalty} without search")
            if self.levels is not None:
                raise ValueError(f"levels belongs to search: got levels={self.levels} without search")
        elif self.levels is None:
            object.__setattr__(self, "search", whole("search", self.search, 1, MAX_R))
        else:
            object.__setattr__(self, "levels", whole("levels", self.levels, 1, MAX_LEVELS))
            object.__setattr__(self, "search", whole("search", self.search, 2 * self.levels, PYR_R * self.levels, f"with levels={self.levels}"))
        if self.intra is not None:
            object.__setattr__(self, "intra", whole("intra", self.intra, 1, MAX_REFS))
        if not isinstance(self.subpel, bool):
            raise ValueError(f"subpel must be True or False, got {self.subpel!r}")
        if self.subpel and self.search is None:
            raise ValueError("subpel belongs to search: got subpel=True without search")
        if not isinstance(self.split, bool):
            raise ValueError(f"split must be True or False, got {self.split!r}")
        if self.split and self.search is None:
            raise ValueError("split belongs to search: got split=True without search")
        for name in ("subpel", "split"):  # (dcvc_me_refine and dcvc_me_split clamp incoming vectors to +-32)
            if getattr(self, name) and self.search > MAX_R:
                raise ValueError(f"{name} stops at search={MAX_R} until its kernel is widened: got {name}=True with search={self.search}")

    def table(self):
        """wtab of dcvc_tnr_step: the weight of the current picture by the window's mean difference a = 0 .. 255, as
        uint16: 256 from T on, floor + ((256 - floor) a) // T below."""
        a = np.arange(256, dtype=np.int64)
        return np.where(a >= self.threshold, FULL, self.floor + ((FULL - self.floor) * a) // self.threshold).astype(np.uint16)

    def to_json(self):
        rd = {"threshold": self.threshold, "floor": self.floor, "pixel": self.pixel}
        if self.search is not None:
            rd.update(search=self.search, penalty=self.penalty)
        if self.intra is not None:  # (a setting without it is written as it always was)
            rd["intra"] = self.intra
        if self.subpel:  # (the unit of the vectors: quarter pixels)
            rd["subpel"] = SUBPEL
        if self.split:  # (the side of a sub-cell)
            rd["split"] = SPLIT
        if self.levels is not None:  # (the coarser levels of the hierarchical search)
            rd["levels"] = self.levels
        return rd

    @staticmethod
    def rcp_table():
        """rtab of dcvc_tnr_fuse, 1021 float32: entry U is the float32 nearest the float64 quotient 1 / (256 + U)."""
        return (1.0 / (256.0 + np.arange(RCP, dtype=np.float64))).astype(np.float32)


@dataclass(frozen=True)
class AutoTNR:
    """A TNR whose threshold is still to be measured: the keywords of TNR but `threshold`, checked by TNR itself, and
    scale: the threshold is `scale` times the source's measured noise level, noise.auto_threshold (0.50 .. 16.00, snapped to
    hundredths); min_cells: the counted cells noise.estimate needs for an estimate.  scale = 3.0 and min_cells = 1024 are
    UNTUNED PLACEHOLDERS, as floor, pixel and penalty are.  pixel None: min(255, 3 T) of the resolved T."""
    scale: float = 3.0
    min_cells: int = 1024
    floor: int = 64
    pixel: int = None
    search: int = None
    penalty: int = PENALTY
    intra: int = None
    subpel: bool = False
    split: bool = False
    levels: int = None

    def _settings(self):
        return {name: getattr(self, name) for name in ("floor", "pixel", "search", "penalty", "intra", "subpel", "split", "levels")}

    def __post_init__(self):
        from . import noise

        object.__setattr__(self, "scale", noise.scale100(self.scale) / 100.0)
        object.__setattr__(self, "min_cells", whole("min_cells", self.min_cells, 1, 2 ** 31 - 1))
        checked = TNR(1, **self._settings())  # (TNR's own refusals; no value of theirs depends on the threshold but pixel=None's)
        for name, given in self._settings().items():
            object.__setattr__(self, name, given if name == "pixel" and given is None else getattr(checked, name))

    def resolve(self, estimate):
        """The TNR of a noise.NoiseEstimate; one without a value is a ValueError that names the cause."""
        from . import noise

        if not isinstance(estimate, noise.NoiseEstimate):
            raise ValueError(f"AutoTNR.resolve: expected a noise.NoiseEstimate, got {type(estimate).__name__}")
        if estimate.mad32 is None:
            raise ValueError(f"tnr-auto: no noise estimate for this source -- {estimate.why_none()}; pass --tnr T (tnr.TNR) instead")
        return TNR(noise.auto_threshold(estimate.mad32, self.scale), **self._settings())


class StreamFilter:
    """What TnrFilter and redact.Redactor share: a filter of the padded pictures of ONE GOP stream of `size` = (height,
    width) on `device` -- the validation of both, two zero-initialised padded pictures written alternately, and the
    per-picture totals: `row` int64 sums per filtered picture, written in place into ROWS rows on the device and sent to the
    host through a goplog.GopLog.  totals=False keeps none: a step is then the one launch and nothing else, no pinned memory
    and no event is ever made, and .totals() is refused.  noun: what the messages call the object; untouched: the totals
    of a step that launched nothing."""
    noun, untouched = "filter", (0, 0)

    def __init__(self, size, device, row, totals):
        import torch

        from . import stream as S
        from .goplog import GopLog

        self.device = devargs.cuda_device(device, type(self).__name__)
        self.height, self.width = int(size[0]), int(size[1])
        if not (0 < self.height <= MAX_SIDE and 0 < self.width <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {self.width}x{self.height}")
        l, r, t, b = S.get_padding_size(self.height, self.width)
        self.padded = (self.height + t + b, self.width + l + r)
        self.grid = grid_of(self.height, self.width)
        # (the crop is written in place by every step and the padding never: it stays the zero pad_frame would give)
        self.bufs = [torch.zeros((1, 3) + self.padded, dtype=torch.float32, device=self.device) for _ in range(2)]
        self.n, self.launches = 0, 0
        # the sums of the filtered pictures not yet flushed; the values already read, by step number
        self._rows = torch.zeros((ROWS, row), dtype=torch.int64, device=self.device) if totals else None
        self._log, self._read = GopLog(), {}

    @property
    def _done(self):
        """The flushes nobody has read yet."""
        return self._log.done

    def _check(self, x):
        devargs.checked(x, f"{type(self).__name__}.step", device=self.device, exact=self.padded, owner=self.noun)

    def _keep(self, t, *cells):
        """Step t's totals: one small reduction per tensor of `cells` behind the launch; the host looks at them per GOP."""
        import torch

        if self._rows is not None:
            row = self._rows[len(self._log.keys)]
            for i, c in enumerate(cells):
                row[i].copy_(c.sum(dtype=torch.int64))
            if self._log.add(t) == ROWS:  # (a GOP with more filtered pictures than rows: its totals travel in more than one copy)
                self.flush()

    def flush(self):
        """The totals of the pictures filtered since the last flush, to pinned host memory in ONE asynchronous copy on the
        current stream: no kernel, and nothing is waited for.  The file loops call it at every GOP's first picture."""
        if self._log.keys:
            self._log.flush(self._rows[:len(self._log.keys)])  # (the next step's rows follow the copy in stream order)

    def totals(self):
        """The totals of every step so far, in order, as Python integers; `untouched` for a step that launched nothing.
        Flushes on the current stream and waits for the copies; their pinned buffers and events are let go of here, at a
        known point, and only the integers are kept."""
        if self._rows is None:
            raise ValueError(f"{type(self).__name__}.totals: this {self.noun} was made with totals=False")
        self.flush()
        for keys, (host,) in self._log.collect():
            self._read.update(zip(keys, (v[0] if len(v) == 1 else tuple(v) for v in host.tolist())))
        return [self._read.get(t, self.untouched) for t in range(self.n)]


class TnrFilter(StreamFilter):
    """The filter of one GOP stream: StreamFilter's two pictures, the table, and the cells' sad / held.  The filter restarts at
    every I picture, so what a GOP is coded from depends on its own pictures and the setting only.  One TnrFilter serves one
    stream at a time.  .totals(): [(held pixels, sum of d)] of every step, (0, 0) for an I picture.

    With tnr.search the filter owns a third padded picture, the compensated reference, and the cells' mv / cost / zero; a
    P step is then three launches on the current stream, nothing synchronised between them: dcvc_me_search(cur, ref),
    dcvc_me_compensate(ref -> comp), dcvc_tnr_step(cur, comp -> out).  .totals(): [(held pixels, sum of d against the
    compensated reference, cells with a nonzero vector, sum of d against the reference as it stood)], (0, 0, 0, 0) for an I
    picture.  Without tnr.search none of this is allocated or launched.

    With tnr.intra the filter also owns dcvc_tnr_fuse's reciprocal table and ONE (4, 3, Hp, Wp) allocation for the
    references of an I picture (with tnr.search also four sets of mv / cost / zero, one per reference), and an I picture
    that is handed pictures `ahead` is filtered: 2 n + 1 launches with the search, 1 without.  Every row of .totals() then
    ends with one more number, the references of the step: n for a filtered I picture, 1 for a P picture, 0 for an I
    picture that was left as it was; an I picture's moved and zero are those of reference 0.  Without tnr.intra none of
    this is allocated or launched, and the rows are as above.

    With tnr.subpel the filter also owns mvq / costq, the quarter-pel vectors of every cell and their SADs (with tnr.intra
    mvqs / costqs, one set per reference), and every search is followed by dcvc_me_refine, every compensation is a
    dcvc_me_compensate_sub: four launches a P step, 3 n + 1 a filtered I picture.  `moved` then counts the nonzero
    quarter-pel vectors, and the row gains `frac`, the cells whose vector has a fractional component, after `zero` and
    before tnr.intra's number of references.  Without tnr.subpel none of this is allocated or launched.

    With tnr.split the filter also owns mv8 / cost8, the quarter-pel vector of every 8 x 8 sub-cell and its SAD (with
    tnr.intra mv8s / cost8s, one set per reference); every search (and refinement) is followed by dcvc_me_split, on mvq at
    unit 4 with tnr.subpel and on mv at unit 1 without, and every compensation is a dcvc_me_compensate_split: four launches a
    P step without tnr.subpel and five with, 3 n + 1 and 4 n + 1 a filtered I picture.  moved, zero and frac stay the
    cells'; the row gains `split`, the sub-cells whose vector differs from their cell's, after frac (after zero without
    tnr.subpel) and before tnr.intra's number of references.  Without tnr.split none of this is allocated or launched.

    With tnr.levels = L the filter also owns the byte planes of the current picture and of the reference, ycur / yref (L + 1
    levels each, rows padded to 4 bytes; with tnr.intra yrefs, one set per reference), and the coarser levels' vectors mvl
    (with tnr.intra mvls, one set per reference), and in place of every dcvc_me_search it launches dcvc_me_pyramid(cur),
    dcvc_me_pyramid(ref), dcvc_me_coarse, dcvc_me_descend to level 1 when L = 2 and dcvc_me_descend to level 0, which writes
    mv / cost / zero: 3 + L more launches a P step, 1 + (1 + L) n more a filtered I picture, whose own pyramid is built once.
    The row gains `far`, the cells whose vector has a component beyond 32, after split, frac or zero (whichever is last) and
    before tnr.intra's number of references.  Without tnr.levels none of this is allocated or launched."""

    def __init__(self, tnr, size, device, totals=True):
        import torch

        if not isinstance(tnr, TNR):
            raise ValueError(f"tnr: expected a tnr.TNR, got {type(tnr).__name__}")
        self.tnr = tnr
        if tnr.search is not None:
            self.untouched = (0, 0, 0, 0) + ((0,) if tnr.subpel else ()) + ((0,) if tnr.split else ()) + ((0,) if tnr.levels else ())
        if tnr.intra is not None:  # (one more column: the number of references of the step)
            self.untouched = self.untouched + (0,)
        super().__init__(size, device, len(self.untouched), totals)
        cells = self.grid[0] * self.grid[1]
        self.wtab = torch.from_numpy(tnr.table().view(np.int16)).to(self.device)  # (the bits of the uint16 table)
        self.sad = torch.empty(cells, dtype=torch.int32, device=self.device)   # (uint32 words; a cell's sum is < 2^16)
        self.held = torch.empty(cells, dtype=torch.int16, device=self.device)  # (uint16 words; a cell's count is <= 256)
        self.ref, self.refs = None, 0  # the last step's result; how many references it was blended with
        if tnr.intra is not None:
            self.rtab = torch.from_numpy(tnr.rcp_table()).to(self.device)
            # the references of an I picture where they cannot be used as they lie: ONE allocation (the crops are
            # written, the padding never).  With search, the first of them serves the P pictures as well.
            self.comps = torch.zeros((MAX_REFS, 3) + self.padded, dtype=torch.float32, device=self.device)
        if tnr.search is not None and tnr.intra is None:
            self.comp = torch.zeros((1, 3) + self.padded, dtype=torch.float32, device=self.device)  # (the crop is written, the padding never)
            self.mv = torch.empty(2 * cells, dtype=torch.int16, device=self.device)   # (dy, dx) of every cell
            self.cost = torch.empty(cells, dtype=torch.int32, device=self.device)     # (uint32 words; a cell's sum is < 2^16)
            self.zero = torch.empty(cells, dtype=torch.int32, device=self.device)
        elif tnr.search is not None:  # (every reference of an I picture has its own mv / cost / zero; a P picture uses the first)
            self.mvs = torch.empty((MAX_REFS, 2 * cells), dtype=torch.int16, device=self.device)
            self.costs = torch.empty((MAX_REFS, cells), dtype=torch.int32, device=self.device)
            self.zeros = torch.empty((MAX_REFS, cells), dtype=torch.int32, device=self.device)
            self.comp, self.mv, self.cost, self.zero = self.comps[:1], self.mvs[0], self.costs[0], self.zeros[0]
        if tnr.subpel and tnr.intra is None:
            self.mvq = torch.empty(2 * cells, dtype=torch.int16, device=self.device)   # (vy, vx) of every cell, quarter pixels
            self.costq = torch.empty(cells, dtype=torch.int32, device=self.device)     # (uint32 words; a cell's sum is < 2^16)
        elif tnr.subpel:
            self.mvqs = torch.empty((MAX_REFS, 2 * cells), dtype=torch.int16, device=self.device)
            self.costqs = torch.empty((MAX_REFS, cells), dtype=torch.int32, device=self.device)
            self.mvq, self.costq = self.mvqs[0], self.costqs[0]
        if tnr.split and tnr.intra is None:
            self.mv8 = torch.empty(8 * cells, dtype=torch.int16, device=self.device)    # (vy, vx) of every sub-cell, quarter pixels
            self.cost8 = torch.empty(4 * cells, dtype=torch.int32, device=self.device)  # (uint32 words; a sub-cell's sum is < 2^14)
        elif tnr.split:
            self.mv8s = torch.empty((MAX_REFS, 8 * cells), dtype=torch.int16, device=self.device)
            self.cost8s = torch.empty((MAX_REFS, 4 * cells), dtype=torch.int32, device=self.device)
            self.mv8, self.cost8 = self.mv8s[0], self.cost8s[0]
        if tnr.levels is not None:
            def planes():  # one level's luma a tensor, a byte per pixel, rows padded to a multiple of 4
                sides, out = (self.height, self.width), []
                for _ in range(tnr.levels + 1):
                    out.append(torch.empty((sides[0], -(-sides[1] // 4) * 4), dtype=torch.uint8, device=self.device))
                    sides = (-(-sides[0] // 2), -(-sides[1] // 2))
                return out

            def vectors():  # (dy, dx) of every cell at level 1 (and 2), in pixels of the level
                return [torch.empty(2 * cells, dtype=torch.int16, device=self.device) for _ in range(tnr.levels)]

            self.ycur = planes()
            if tnr.intra is None:
                self.yref, self.mvl = planes(), vectors()
            else:
                self.yrefs, self.mvls = [planes() for _ in range(MAX_REFS)], [vectors() for _ in range(MAX_REFS)]
                self.yref, self.mvl = self.yrefs[0], self.mvls[0]
        torch.cuda.synchronize(self.device)  # (the uploads above: a stream that uses them afterwards cannot race them)

    def _keep_step(self, t, n):
        """The totals' row of a step that launched: (held, sad), with search (held, sad, moved, zero) of reference 0, and
        with tnr.intra one more column, the number n of references."""
        if self._rows is None:  # (the cells that moved are counted only where somebody will read the count)
            return
        cells = (self.held, self.sad)
        if self.tnr.subpel:  # (moved and frac of the quarter-pel vectors)
            cells += ((self.mvq.view(-1, 2) != 0).any(dim=1), self.zero, (self.mvq.view(-1, 2) & 3 != 0).any(dim=1))
        elif self.tnr.search is not None:
            cells += ((self.mv.view(-1, 2) != 0).any(dim=1), self.zero)
        if self.tnr.split:  # (the sub-cells that hold a pixel and left their cell's vector, both in quarter pixels)
            hc, wc = self.grid
            own = (self.mvq if self.tnr.subpel else SUBPEL * self.mv).view(hc, 1, wc, 1, 2)
            left = (self.mv8.view(hc, 2, wc, 2, 2) != own).any(dim=4).view(2 * hc, 2 * wc)
            cells += (left[:-(-self.height // SPLIT), :-(-self.width // SPLIT)],)
        if self.tnr.levels is not None:  # (the cells that the full search could not have reached)
            cells += ((self.mv.view(-1, 2).abs() > MAX_R).any(dim=1),)
        if self.tnr.intra is not None:
            self._rows[len(self._log.keys), len(cells)] = n
        self._keep(t, *cells)

    def _pyramid(self, pic, rs, ps, planes):
        """The byte planes of a picture's crop: dcvc_me_pyramid, the only reader of fp32 in the hierarchical search."""
        y = planes + [None] * (MAX_LEVELS + 1 - len(planes))
        devargs.launch("dcvc_me_pyramid", self.device, pic.data_ptr(), rs, ps, self.height, self.width, self.tnr.levels,
                       *(v for p in y for v in ((p.data_ptr(), p.shape[1]) if p is not None else (None, 0))))

    def _search(self, cur, crs, cps, ref, rrs, rps, mv, cost, zero, j, built=False):
        """The vectors of cur in ref into mv / cost / zero of reference j: dcvc_me_search, or with tnr.levels the chain that
        stands in its place (built: cur's byte planes are there already).  -> the launches."""
        (h, w), L, R, lam = (self.height, self.width), self.tnr.levels, self.tnr.search, self.tnr.penalty
        if L is None:
            devargs.launch("dcvc_me_search", self.device, cur.data_ptr(), crs, cps, ref.data_ptr(), rrs, rps, h, w, R, lam, mv.data_ptr(),
                           cost.data_ptr(), zero.data_ptr())
            return 1
        yc, (yr, mvl) = self.ycur, (self.yref, self.mvl) if self.tnr.intra is None else (self.yrefs[j], self.mvls[j])
        if not built:
            self._pyramid(cur, crs, cps, yc)
        self._pyramid(ref, rrs, rps, yr)
        devargs.launch("dcvc_me_coarse", self.device, yc[L].data_ptr(), yc[L].shape[1], yr[L].data_ptr(), yr[L].shape[1], h, w, R, L, lam,
                       mvl[L - 1].data_ptr())
        for level in range(L - 1, -1, -1):
            out = (mvl[level - 1].data_ptr(), None, None) if level else (mv.data_ptr(), cost.data_ptr(), zero.data_ptr())
            devargs.launch("dcvc_me_descend", self.device, yc[level].data_ptr(), yc[level].shape[1], yr[level].data_ptr(), yr[level].shape[1],
                           h, w, R, L, level, lam, mvl[level].data_ptr(), *out)
        return (0 if built else 1) + 2 + L

    def _move(self, cur, crs, cps, ref, rrs, rps, comp, mv, j):
        """ref moved onto cur into comp by the searched vectors mv: dcvc_me_compensate, or with tnr.subpel dcvc_me_refine
        into the quarter-pel vectors of reference j and dcvc_me_compensate_sub; with tnr.split dcvc_me_split on the cells'
        vectors into the sub-cells' of reference j and dcvc_me_compensate_split in place of either compensation."""
        (h, w), (Hp, Wp) = (self.height, self.width), self.padded
        if not self.tnr.subpel and not self.tnr.split:
            devargs.launch("dcvc_me_compensate", self.device, ref.data_ptr(), rrs, rps, comp.data_ptr(), Wp, Hp * Wp, h, w, mv.data_ptr())
            return
        unit = 1
        if self.tnr.subpel:
            mvq, costq = (self.mvq, self.costq) if self.tnr.intra is None else (self.mvqs[j], self.costqs[j])
            devargs.launch("dcvc_me_refine", self.device, cur.data_ptr(), crs, cps, ref.data_ptr(), rrs, rps, h, w, self.tnr.penalty,
                           mv.data_ptr(), mvq.data_ptr(), costq.data_ptr())
            mv, unit = mvq, SUBPEL
        if not self.tnr.split:
            devargs.launch("dcvc_me_compensate_sub", self.device, ref.data_ptr(), rrs, rps, comp.data_ptr(), Wp, Hp * Wp, h, w, mv.data_ptr())
            return
        mv8, cost8 = (self.mv8, self.cost8) if self.tnr.intra is None else (self.mv8s[j], self.cost8s[j])
        devargs.launch("dcvc_me_split", self.device, cur.data_ptr(), crs, cps, ref.data_ptr(), rrs, rps, h, w, self.tnr.penalty, unit,
                       mv.data_ptr(), mv8.data_ptr(), cost8.data_ptr())
        devargs.launch("dcvc_me_compensate_split", self.device, ref.data_ptr(), rrs, rps, comp.data_ptr(), Wp, Hp * Wp, h, w, mv8.data_ptr())

    def _fuse(self, t, x_padded, ahead):
        """An I picture blended with the pictures `ahead` (1 .. 4 of them, checked): with tnr.search a search from the I
        source and a compensation per reference, then ONE dcvc_tnr_fuse launch into one of the two buffers."""
        out = self.bufs[0] if self.ref is not self.bufs[0] else self.bufs[1]
        (h, w), (Hp, Wp) = (self.height, self.width), self.padded
        cur, crs, cps = devargs.planar(x_padded.detach()[..., :h, :w])  # (the crops, read in place)
        refs = [devargs.planar(r.detach()[..., :h, :w]) for r in ahead]
        if self.tnr.search is not None:
            for j, (r, rrs, rps) in enumerate(refs):  # (the I source's byte planes are built once, with reference 0)
                self.launches += self._search(cur, crs, cps, r, rrs, rps, self.mvs[j], self.costs[j], self.zeros[j], j, built=j > 0)
                self._move(cur, crs, cps, r, rrs, rps, self.comps[j], self.mvs[j], j)
                refs[j] = (self.comps[j], Wp, Hp * Wp)
            self.launches += (1 + self.tnr.subpel + self.tnr.split) * len(refs)
        elif len({r[1:] for r in refs}) > 1:  # (the kernel takes ONE pair of strides: the odd ones out are copied)
            for j, (r, rrs, rps) in enumerate(refs):
                if (rrs, rps) != (Wp, Hp * Wp):
                    self.comps[j, :, :h, :w].copy_(r[0])
                    refs[j] = (self.comps[j], Wp, Hp * Wp)
        ptrs = [r[0].data_ptr() for r in refs] + [None] * (MAX_REFS - len(refs))
        devargs.launch("dcvc_tnr_fuse", self.device, cur.data_ptr(), crs, cps, *ptrs, refs[0][1], refs[0][2], len(refs), out.data_ptr(),
                       Wp, Hp * Wp, h, w, self.wtab.data_ptr(), self.rtab.data_ptr(), self.tnr.pixel, self.sad.data_ptr(),
                       self.held.data_ptr())
        self.launches += 1
        self._keep_step(t, len(refs))
        self.ref, self.refs = out, len(refs)
        return out

    def step(self, x_padded, intra, ahead=()):
        """The padded picture to code in place of `x_padded`.  An I picture (intra=True) launches nothing and is returned
        itself; it becomes the next step's reference.  A P picture is one dcvc_tnr_step launch on the current stream from
        the crops of x_padded and of the previous step's result into the crop of one of the two buffers, which stays valid
        until the step after the next.  With tnr.search the search and the compensation are launched in front of it, and
        the step blends against the compensated picture.

        ahead: with tnr.intra = K, the padded pictures that FOLLOW an I picture in its own GOP, nearest first (the caller
        answers for the GOP); the first K of them are its references, and the I picture is then filtered too -- per
        reference a search from the I source and a compensation where tnr.search asks for them, then ONE dcvc_tnr_fuse
        launch into one of the two buffers.  The result is returned and is the next step's reference.  No picture ahead
        (a GOP of one picture): nothing is launched and the source is returned.  Without tnr.intra, and for a P picture,
        `ahead` is ignored."""
        self._check(x_padded)
        t, self.n = self.n, self.n + 1
        if intra:
            self.flush()  # (the GOP before this one: its totals go to the host in one copy)
            ahead = list(ahead[:self.tnr.intra]) if self.tnr.intra is not None else []
            if ahead:
                for r in ahead:
                    self._check(r)
                return self._fuse(t, x_padded, ahead)
            self.ref, self.refs = x_padded.detach(), 0
            return x_padded
        if self.ref is None:
            raise ValueError("TnrFilter.step: the first picture of a stream is an I picture")
        out = self.bufs[0] if self.ref is not self.bufs[0] else self.bufs[1]
        (h, w), (Hp, Wp) = (self.height, self.width), self.padded
        cur, crs, cps = devargs.planar(x_padded.detach()[..., :h, :w])  # (the crops, read in place)
        ref, rrs, rps = devargs.planar(self.ref[..., :h, :w])
        if self.tnr.search is not None:
            self.launches += self._search(cur, crs, cps, ref, rrs, rps, self.mv, self.cost, self.zero, 0)
            self._move(cur, crs, cps, ref, rrs, rps, self.comp, self.mv, 0)
            ref, rrs, rps = self.comp, Wp, Hp * Wp
            self.launches += 1 + self.tnr.subpel + self.tnr.split
        devargs.launch("dcvc_tnr_step", self.device, cur.data_ptr(), crs, cps, ref.data_ptr(), rrs, rps, out.data_ptr(), Wp, Hp * Wp,
                       h, w, self.wtab.data_ptr(), self.tnr.pixel, self.sad.data_ptr(), self.held.data_ptr())
        self.launches += 1
        self._keep_step(t, 1)
        self.ref, self.refs = out, 1
        return out
