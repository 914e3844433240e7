"""Film-grain synthesis (include/dcvc_hip_grain.h, csrc/grain.hip): the other half of the temporal noise prefilter
(vcm_ts_amd/tnr.py).  The encoder MEASURES, GOP by GOP, what the filter took out of the cells it blended throughout -- how
strong by intensity, how correlated along rows and columns -- and leaves the few numbers in a grain.json beside the .bin
files; a decoder that is ASKED to (it is never followed silently) re-synthesises noise of that strength and shape on the
P pictures it displays.  Display side only: the bitstream, the DPB and every digest know nothing of it.  The arithmetic
of the two kernels is stated in the header; tests/grain_ref.py restates it, and params / table below, in numpy.

    Grain(min_samples=1024)                          the encoder's setting
    GrainMeter(size, device)                         the sums of ONE GOP stream on the device; .step(src_padded, filter, g, intra)
    params(acc, min_samples)                         32 sums -> {"points", "kh", "kv", "counts"}: Python integers only
    table(points, kh, kv, percent)                   -> the 256 uint16 of dcvc_grain_apply's stab
    write_grain / read_grain / check_record          grain.json
    GrainSynth(record, plan, size, device, percent)  the decoder's stage; .shown(t, picture)

`min_samples` is an UNTUNED PLACEHOLDER, and so is everything else here: this is the mechanism -- measured, recorded,
synthesised -- not a claim about rate, quality or what a detector makes of it.  P pictures only (an I picture is not
filtered, so it keeps what the codec kept of its own noise); achromatic; a 3-tap separable shape; one set of parameters
per GOP.  With the filter's look-ahead (tnr.TNR(intra=K)) the I picture loses its noise as well: it is then measured into
its GOP's sums like a P picture, the record's "tnr" entry says "intra", and the synthesis grains I pictures exactly when it
does -- the I picture's noise is pooled with the P pictures', still one set of parameters per GOP.

The kernels run on the caller's current stream and synchronise nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import whole

VERSION = 1
GRAIN_JSON = "grain.json"
BINS, WORDS, MAX_TAP, CENTRE, SHIFT, WHITE_VAR = 8, 32, 24, 64, 24, 43690  # (the header's constants)
MAX_POINT = 255 * 16  # a standard deviation, in 1/16 of an 8-bit code
MAX_PERCENT = 200
TAPS = sorted(range(-MAX_TAP, MAX_TAP + 1), key=lambda k: (abs(k), k))  # (ties go to the smaller |k|)


@dataclass(frozen=True)
class Grain:
    """min_samples: a bin of fewer pixels than this takes its nearest populated neighbour's strength (1 .. 2^31 - 1; an
    untuned placeholder)."""
    min_samples: int = 1024

    def __post_init__(self):
        object.__setattr__(self, "min_samples", whole("min_samples", self.min_samples, 1, 2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------ the record's arithmetic
def _tap(cross, square):
    """The tap k whose correlation 2 * 64 k / (64^2 + 2 k^2) lies nearest cross / square, by cross-multiplication."""
    if square <= 0:
        return 0
    best, err, den = 0, None, None
    for k in TAPS:
        d = CENTRE * CENTRE + 2 * k * k
        e = abs(cross * d - 2 * CENTRE * k * square)  # |cross / square - 2 * 64 k / d| * square * d
        if err is None or e * den < err * d:
            best, err, den = k, e, d
    return best


def params(acc, min_samples):
    """One GOP's record from the 32 sums of dcvc_grain_measure (word 4 b + k: count, sum e^2, sum e e_right, sum e e_below of
    bin b), in Python integers only, so that every host writes the same: points[b] = isqrt(256 * sum e^2 // count), the
    standard deviation in 1/16 code, of a bin with at least min_samples pixels -- any other bin takes the value of its
    nearest such bin, the lower one on a tie; kh (kv) the tap whose correlation lies nearest sum e e_right (e e_below) over sum
    e^2, both pooled over the bins that have min_samples; counts the eight counts.  No such bin: all zeros."""
    acc = [int(v) for v in acc]
    if len(acc) != WORDS:
        raise ValueError(f"params: expected {WORDS} sums, got {len(acc)}")
    counts = [acc[4 * b] for b in range(BINS)]
    good = [b for b in range(BINS) if counts[b] >= min_samples and counts[b] > 0]
    if not good:
        return {"points": [0] * BINS, "kh": 0, "kv": 0, "counts": counts}
    own = {b: math.isqrt(256 * acc[4 * b + 1] // counts[b]) for b in good}
    points = [own[min(good, key=lambda n: (abs(n - b), n))] for b in range(BINS)]
    square = sum(acc[4 * b + 1] for b in good)
    return {"points": points, "kh": _tap(sum(acc[4 * b + 2] for b in good), square),
            "kv": _tap(sum(acc[4 * b + 3] for b in good), square), "counts": counts}


def table(points, kh, kv, percent=100):
    """stab of dcvc_grain_apply, 256 uint16: the standard deviation at luma code Y, linear between the bin centres 16, 48,
    ... 240 and flat outside them, times percent / 100, over the standard deviation isqrt(43690 (64^2 + 2 kh^2) (64^2 + 2
    kv^2)) of the shaped field, in units of 2^-24 -- rounded to nearest in integers and held to 65535."""
    points = [whole("points", p, 0, MAX_POINT) for p in points]
    if len(points) != BINS:
        raise ValueError(f"table: expected {BINS} points, got {len(points)}")
    kh, kv = whole("kh", kh, -MAX_TAP, MAX_TAP), whole("kv", kv, -MAX_TAP, MAX_TAP)
    percent = whole("percent", percent, 1, MAX_PERCENT)
    den = 32 * 100 * math.isqrt(WHITE_VAR * (CENTRE * CENTRE + 2 * kh * kh) * (CENTRE * CENTRE + 2 * kv * kv))
    out = np.empty(256, dtype=np.uint16)
    for y in range(256):
        b, f = divmod(min(max(y, 16), 240) - 16, 32)
        sigma32 = points[b] * 32 if b == BINS - 1 else points[b] * (32 - f) + points[b + 1] * f  # (in 1/512 code)
        out[y] = min(65535, ((sigma32 * percent << SHIFT) + den // 2) // den)
    return out


# -------------------------------------------------------------------------------------------------------------- grain.json
def record_of(grain, tnr, gops):
    """grain.json's dictionary: gops = {first picture of the GOP: params(...)}."""
    return {"version": VERSION, "min_samples": grain.min_samples, "tnr": tnr.to_json(),
            "gops": {str(g): gops[g] for g in sorted(gops)}}


def write_grain(bin_dir, record):
    """grain.json beside the .bin files; record None removes a stale one."""
    from . import stream as S

    S.write_sidecar(bin_dir, GRAIN_JSON, record)


def check_record(record, plan, where=GRAIN_JSON):
    """Refuse, by name, a record of an unknown version, with a value out of range, or whose GOPs are not the plan's."""
    def bad(what):
        return ValueError(f"{where}: {what}")

    if not isinstance(record, dict) or record.get("version") != VERSION:
        raise bad(f"version {record.get('version') if isinstance(record, dict) else None!r}, this decoder knows version {VERSION}")
    try:
        whole("min_samples", record.get("min_samples"), 1, 2 ** 31 - 1)
    except ValueError as ex:
        raise bad(ex) from None
    gops = record.get("gops")
    if not isinstance(gops, dict) or sorted(gops) != sorted(str(g) for g in plan.i_pictures):
        have = sorted(gops, key=str) if isinstance(gops, dict) else gops
        raise bad(f"GOPs that start at {have}, the folder's plan starts them at {list(plan.i_pictures)}")
    setting = record.get("tnr")
    if isinstance(setting, dict) and "intra" in setting:  # (the encoder's look-ahead: I pictures were filtered and measured)
        try:
            whole("intra", setting["intra"], 1, 4)
        except ValueError as ex:
            raise bad(f"tnr: {ex}") from None
    for g, rec in gops.items():
        try:
            if not isinstance(rec, dict) or not isinstance(rec.get("points"), list) or not isinstance(rec.get("counts"), list):
                raise ValueError("expected points, kh, kv and counts")
            if len(rec["counts"]) != BINS:
                raise ValueError(f"expected {BINS} counts, got {len(rec['counts'])}")
            for c in rec["counts"]:
                whole("counts", c, 0, 2 ** 62)
            table(rec["points"], rec.get("kh"), rec.get("kv"))
        except ValueError as ex:
            raise bad(f"GOP {g}: {ex}") from None
    return record


def read_grain(bin_dir, plan):
    """The checked record of the folder's grain.json; no file is a ValueError by name."""
    from . import stream as S

    found = S.read_sidecar(bin_dir, GRAIN_JSON)
    if found is None:
        raise ValueError(f"{bin_dir}: no {GRAIN_JSON} beside the .bin files (encode --tnr T --grain writes one); nothing to synthesise")
    return check_record(found[1], plan, found[0])


# ------------------------------------------------------------------------------------------------------------- the encoder
class GrainMeter:
    """The measurement of ONE GOP stream: 32 int64 sums on the device, zeroed at every I picture and added to by one
    dcvc_grain_measure launch per P picture, right behind the filter's own launch on the same stream.  The sums of a GOP
    travel to the host in one asynchronous copy (goplog.GopLog) when the next GOP starts; the host waits for nothing until
    .sums()."""

    def __init__(self, size, device):
        import torch

        from .goplog import GopLog

        self.device = devargs.cuda_device(device, "GrainMeter")
        self.height, self.width = int(size[0]), int(size[1])
        if not (0 < self.height <= devargs.MAX_SIDE and 0 < self.width <= devargs.MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{devargs.MAX_SIDE}, got {self.width}x{self.height}")
        self.launches, self._log, self._read = 0, GopLog(), {}
        self._acc = None  # (a buffer per GOP: the one whose copy is in flight is not written again)
        self._torch = torch

    def flush(self):
        """The open GOP's sums to pinned host memory: one asynchronous copy, nothing waited for."""
        if self._log.keys:
            self._log.flush(self._acc.view(1, WORDS))

    def step(self, src_padded, filt, g, intra):
        """Picture g of the sequence, right after filt.step(src_padded, intra) (filt: the stream's tnr.TnrFilter).  An I
        picture sends the GOP before it to the host and starts its own with zeroed sums: no kernel, unless the filter blended
        it (tnr.intra: filt.refs > 0) -- then it is measured like a P picture.  A P picture is one launch that reads the
        crops of src_padded and of the picture the filter just wrote, and the filter's held cells."""
        if intra:
            self.flush()
            self._acc = self._torch.zeros(WORDS, dtype=self._torch.int64, device=self.device)
            self._log.add(int(g))
            if not getattr(filt, "refs", 0):
                return
        if self._acc is None:
            raise ValueError("GrainMeter.step: the first picture of a stream is an I picture")
        devargs.checked(src_padded, "GrainMeter.step", device=self.device, exact=filt.padded, owner="meter")
        h, w = self.height, self.width
        if (filt.height, filt.width) != (h, w):
            raise ValueError(f"GrainMeter.step: a filter of {filt.width}x{filt.height} pictures, a meter of {w}x{h}")
        src, srs, sps = devargs.planar(src_padded.detach()[..., :h, :w])
        flt, frs, fps = devargs.planar(filt.ref[..., :h, :w])
        devargs.launch("dcvc_grain_measure", self.device, src.data_ptr(), srs, sps, flt.data_ptr(), frs, fps, h, w,
                       filt.held.data_ptr(), self._acc.data_ptr())
        self.launches += 1

    def sums(self):
        """{first picture of a GOP: its 32 sums as Python integers} of every GOP so far.  Flushes and waits."""
        self.flush()
        for keys, (host,) in self._log.collect():
            self._read.update(zip(keys, host.tolist()))
        return dict(self._read)


# ------------------------------------------------------------------------------------------------------------- the decoder
class GrainSynth:
    """The decoder's display-side stage.  record: a checked grain.json; plan: the folder's GopPlan; size: the (height,
    width) of the pictures shown; percent: 1 .. 200 of the measured strength.  The tables of every GOP are built on the
    host and uploaded once, here."""

    def __init__(self, record, plan, size, device, percent=100):
        import torch

        self.device = devargs.cuda_device(device, "GrainSynth")
        self.height, self.width = int(size[0]), int(size[1])
        if not (0 < self.height <= devargs.MAX_SIDE and 0 < self.width <= devargs.MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{devargs.MAX_SIDE}, got {self.width}x{self.height}")
        self.percent = whole("percent", percent, 1, MAX_PERCENT, "--grain")
        check_record(record, plan)
        self.plan, self.launches, self._gops = plan, 0, {}
        self.intra = isinstance(record.get("tnr"), dict) and "intra" in record["tnr"]  # (I pictures were filtered: grain them too)
        for g in plan.i_pictures:
            rec = record["gops"][str(g)]
            tab = table(rec["points"], rec["kh"], rec["kv"], self.percent)
            if tab.any():  # (an all-zero table would copy the picture: such a GOP launches nothing)
                self._gops[g] = (torch.from_numpy(tab.view(np.int16)).to(self.device), int(rec["kh"]), int(rec["kv"]))
        self.bufs, self._next = [None, None], 0
        torch.cuda.synchronize(self.device)  # (the uploads above: a stream that uses them afterwards cannot race them)

    def shown(self, t, picture):
        """The picture to display for frame t: `picture` itself -- nothing launched -- for an I picture (unless the record's
        setting has `intra`) and in a GOP whose table is all zero; else a grained copy (one dcvc_grain_apply launch on the current stream) in one of two buffers of
        the stage's own, valid until the call after the next.  The crop is grained; the rest of the copy is zero."""
        import torch

        if self.plan.is_intra(t) and not self.intra:
            return picture
        gop = self._gops.get(self.plan.i_pictures[self.plan.gop_of(t)])
        if gop is None:
            return picture
        h, w = self.height, self.width
        src, srs, sps = devargs.picture(picture, "GrainSynth.shown", device=self.device, at_least=(h, w), owner="stage")
        if self.bufs[self._next] is None or self.bufs[self._next].shape != picture.shape:
            self.bufs[self._next] = torch.zeros(picture.shape, dtype=torch.float32, device=self.device)
        out, self._next = self.bufs[self._next], 1 - self._next
        Hp, Wp = out.shape[2:]
        devargs.launch("dcvc_grain_apply", self.device, src.data_ptr(), srs, sps, out.data_ptr(), Wp, Hp * Wp, h, w, int(t), gop[1],
                       gop[2], gop[0].data_ptr())
        self.launches += 1
        return out
