"""Backward-adaptive quantisation (include/dcvc_hip_aq.h, csrc/aq.hip): a q-scale map for every P picture, made on the
device from the reference picture the decoder holds too -- so the decoder rebuilds it and the bitstream carries nothing.
Flat cells get a finer step, busy ones a coarser one, in the form of x265's auto-variance mode; the arithmetic after the
8-bit code is integer only and is stated in the header, tests/aq_ref.py restates it in numpy.

    AQ(strength, lo, hi)         the setting, in hundredths; .ktab() / .ftab() the two host-built tables; aq.json
    AqMaps(aq, device)           the tables and scratch of ONE GOP stream on the device; .map(ref_frame, roi_map=None)
    write_aq / read_aq           aq.json beside the .bin files

It is the mechanism only: there are no tuned values, and nothing is claimed about rate or quality.  Every call runs on
the caller's current stream and synchronises nothing (AqMaps() itself synchronises once, after its uploads).  There is no
torch fallback: anything the kernels do not take is a ValueError.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from . import devargs
from .devargs import MAX_SIDE, whole

AQ_JSON = "aq.json"
VERSION, CELL = 1, 16
MAX_L, MAX_STRENGTH, MIN_Q, MAX_Q = 7935, 400, 10, 1000
KTAB, FTAB = 2 * MAX_L + 1, MAX_Q - MIN_Q + 1  # entries of the two tables
QP_PER_DOUBLING = 6  # of the step: d is in 1/256 of a doubling of the variance, A in 1/100 QP per doubling


@dataclass(frozen=True)
class AQ:
    """The setting of backward-adaptive quantisation, as integers in HUNDREDTHS like roi.RoiQ's factors: `strength` A,
    1..400 (A / 100 QP per doubling of a cell's variance against the picture's mean, 6 QP doubling the step), and the
    clamp `lo` <= 100 <= `hi` within 10..1000 on the factor a cell may get.  AQ.snapped() takes plain numbers instead."""
    strength: int
    lo: int = MIN_Q
    hi: int = MAX_Q

    def __post_init__(self):
        object.__setattr__(self, "strength", whole("strength", self.strength, 1, MAX_STRENGTH, "hundredths"))
        object.__setattr__(self, "lo", whole("lo", self.lo, MIN_Q, 100, "hundredths"))
        object.__setattr__(self, "hi", whole("hi", self.hi, 100, MAX_Q, "hundredths"))

    @staticmethod
    def hundredths(value, name="value"):
        """A plain number snapped to hundredths (1.0 -> 100), as roi.RoiQ.hundredths does."""
        return devargs.hundredths(value, name)

    @classmethod
    def snapped(cls, strength, lo=0.1, hi=10.0):
        """AQ from plain numbers: strength in QP per doubling (x265's --aq-strength), lo and hi as factors."""
        return cls(cls.hundredths(strength, "strength"), cls.hundredths(lo, "lo"), cls.hundredths(hi, "hi"))

    def ktab(self):
        """k(d) for d = -7935 .. 7935 as uint16: clamp(rint(100 * 2^(A d / (100 * 256 * 6))), lo, hi), in float64."""
        d = np.arange(-MAX_L, MAX_L + 1, dtype=np.float64)
        k = np.rint(100.0 * np.exp2(self.strength * d / (100.0 * 256.0 * QP_PER_DOUBLING)))
        return np.clip(k, self.lo, self.hi).astype(np.uint16)

    @staticmethod
    def ftab():
        """The float32 factor of k = 10 .. 1000 hundredths: float32(k) / float32(100), roi.RoiQ.factors()'s values."""
        return np.arange(MIN_Q, MAX_Q + 1, dtype=np.float32) / np.float32(100)

    def is_neutral(self):
        """Whether every cell gets exactly 1.0 whatever the picture (a clamp of 100..100)."""
        return self.lo == 100 and self.hi == 100

    def digests(self):
        return {"ktab": "%08x" % (zlib.crc32(self.ktab().tobytes()) & 0xFFFFFFFF),
                "ftab": "%08x" % (zlib.crc32(self.ftab().tobytes()) & 0xFFFFFFFF)}

    def to_json(self):
        return {"version": VERSION, "cell": CELL, "strength": self.strength, "clamp": [self.lo, self.hi],
                "tables": self.digests()}

    @classmethod
    def from_json(cls, info, where=AQ_JSON):
        """The AQ of an aq.json record.  The tables are rebuilt on THIS host and held against the record's digests.
        Refused by name: an unknown version or cell, missing or mistyped fields, a value out of range, and a table whose
        CRC-32 differs (a host whose exp2 moves one entry across a rounding tie must not decode silently)."""
        if not isinstance(info, dict):
            raise ValueError(f"{where}: expected a JSON object")
        if info.get("version") != VERSION:
            raise ValueError(f"{where}: unknown version {info.get('version')!r} (this build reads version {VERSION})")
        if set(info) != {"version", "cell", "strength", "clamp", "tables"}:
            raise ValueError(f"{where}: expected the keys version, cell, strength, clamp and tables, got {sorted(info)}")
        if info["cell"] != CELL:
            raise ValueError(f"{where}: cell must be {CELL}, got {info['cell']!r}")
        clamp = info["clamp"]
        if not (isinstance(clamp, list) and len(clamp) == 2):
            raise ValueError(f"{where}: clamp must be two integers [lo, hi], got {clamp!r}")
        try:
            aq = cls(info["strength"], clamp[0], clamp[1])
        except ValueError as ex:
            raise ValueError(f"{where}: {ex}") from None
        digests = info["tables"]
        if not isinstance(digests, dict) or set(digests) != {"ktab", "ftab"}:
            raise ValueError(f"{where}: tables must hold the digests of ktab and ftab")
        for name, got in aq.digests().items():
            if digests[name] != got:
                raise ValueError(f"{where}: the {name} table built on this host has the digest {got}, the file says "
                                 f"{digests[name]!r}: this host would not rebuild the encoder's maps")
        return aq


def grid_of(Hp, Wp):
    """(hc, wc) of a padded Hp x Wp picture; refused by name unless both are positive multiples of 64 up to 32768."""
    Hp, Wp = int(Hp), int(Wp)
    if not (0 < Hp <= MAX_SIDE and 0 < Wp <= MAX_SIDE and Hp % 64 == 0 and Wp % 64 == 0):
        raise ValueError(f"aq: the reference picture must be padded to positive multiples of 64 up to {MAX_SIDE}, got {Wp}x{Hp}")
    return Hp // CELL, Wp // CELL


# ------------------------------------------------------------------------------------------------------------ device
class AqMaps:
    """The device side of one GOP stream: the two tables, the activity scratch and the picture sum.  The tables are
    uploaded once and the device is synchronised before this returns, so that a stream that uses them afterwards cannot
    race the uploads.  One AqMaps serves one stream at a time (the scratch is reused from picture to picture)."""

    def __init__(self, aq, device):
        import torch

        if not isinstance(aq, AQ):
            raise ValueError(f"aq: expected an aq.AQ, got {type(aq).__name__}")
        self.aq, self.device = aq, devargs.cuda_device(device, "AqMaps")
        self.ktab = torch.from_numpy(aq.ktab().view(np.int16)).to(self.device)  # (the bits of the uint16 table)
        self.ftab = torch.from_numpy(aq.ftab()).to(self.device)
        self.sum = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.L = None
        torch.cuda.synchronize(self.device)

    def activity(self, ref_frame):
        """(L as an (hc, wc) int32 tensor, the (1,) int64 sum of it) of a padded (1, 3, Hp, Wp) float32 picture: the
        scratch of this object, valid until the next call.  A memset and one launch on the current stream."""
        import torch

        t = devargs.checked(ref_frame, "aq", device=self.device, noun="reference picture")
        hc, wc = grid_of(*t.shape[2:])
        p, rs, ps = devargs.planar(t)
        if self.L is None or self.L.numel() != hc * wc:
            self.L = torch.empty(hc * wc, dtype=torch.int32, device=self.device)
        self.sum.zero_()
        devargs.launch("dcvc_aq_activity", self.device, p.data_ptr(), rs, ps, t.shape[2], t.shape[3], self.L.data_ptr(),
                       self.sum.data_ptr())
        return self.L.view(hc, wc), self.sum

    def map(self, ref_frame, roi_map=None):
        """The (hc, wc) float32 q-scale map of the picture coded against `ref_frame` (the DPB's padded reference picture),
        multiplied into `roi_map` (roi.q_map's, hc * wc float32 on the same device) when one is given: what DMC
        .compress / .decompress take as q_map=.  A memset and two launches on the current stream, nothing synchronised."""
        import torch

        L, total = self.activity(ref_frame)
        hc, wc = L.shape
        roi_ptr = None
        if roi_map is not None:
            r = roi_map
            if not torch.is_tensor(r) or r.dtype != torch.float32 or not r.is_cuda:
                raise ValueError(f"aq: roi_map: expected a float32 tensor on the GPU, got "
                                 f"{getattr(r, 'dtype', type(r).__name__)}")
            if r.device != self.device:
                raise ValueError(f"aq: roi_map is on {r.device}, the tables on {self.device}")
            if tuple(r.shape) not in ((hc, wc), (1, 1, hc, wc)):
                raise ValueError(f"aq: roi_map: expected shape ({hc}, {wc}) or (1, 1, {hc}, {wc}), got {tuple(r.shape)}")
            roi_map = r.detach().contiguous()
            roi_ptr = roi_map.data_ptr()
        out = torch.empty((hc, wc), dtype=torch.float32, device=self.device)
        devargs.launch("dcvc_aq_map", self.device, L.data_ptr(), total.data_ptr(), hc, wc, self.ktab.data_ptr(),
                       self.ftab.data_ptr(), roi_ptr, out.data_ptr())
        return out


def as_maps(aq, device):
    """What the pipeline's aq= takes -> an AqMaps on `device` (None stays None): an AqMaps as it is, an AQ gets its own."""
    if aq is None or isinstance(aq, AqMaps):
        return aq
    return AqMaps(aq, device)


# ----------------------------------------------------------------------------------------------------------- aq.json
def write_aq(bin_dir, aq):
    """aq.json beside the .bin files -- only for an encode with backward-adaptive quantisation: without it none is needed
    (and a stale file of an earlier encode into the same folder must not describe these .bin files)."""
    from .stream import write_sidecar

    return write_sidecar(bin_dir, AQ_JSON, None if aq is None else aq.to_json())


def read_aq(bin_dir):
    """AQ.from_json of the folder's aq.json, or None without the file."""
    from .stream import read_sidecar

    found = read_sidecar(bin_dir, AQ_JSON)
    return None if found is None else AQ.from_json(found[1], found[0])
