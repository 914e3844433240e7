"""The reduced-resolution base layer's resampler (include/dcvc_hip_scale.h, csrc/scale.hip): a separable Lanczos-3 whose
integer tap tables are built here, on the host, in float64 -- the device evaluates no transcendental -- and whose fold is
stated in the header and pinned bit for bit by tests/scale_ref.py.  Encoder and decoder rebuild the same full-size picture
from the base reconstruction, which is what lets the ROI residual layer stay lossless over a half-size background.

    taps(n_in, n_out)            the table of one axis
    base_size(h, w, ratio)       the base layer's size for a ratio n/d, 1/4 <= n/d < 1
    Scale(full, ratio, device)   the four tables on the device; .down(x) and .up(x) on (..., 3, H, W) float32 pictures
    write_scale / read_scale     scale.json beside the .bin files

Every call runs on the caller's current stream and synchronises nothing (Scale() itself synchronises once, after its
uploads).  There is no torch fallback: anything the kernel does not take is a ValueError.
"""
from __future__ import annotations

import zlib
from fractions import Fraction

import numpy as np

from . import devargs
from .devargs import MAX_SIDE

SCALE_JSON = "scale.json"
VERSION, FILTER, UNIT, MAX_TAPS = 1, "lanczos3", 16384, 32
MIN_RATIO = Fraction(1, 4)
TABLES = ("down_y", "down_x", "up_y", "up_x")


# ---------------------------------------------------------------------------------------------------------- the tables
def _lanczos3(x):
    return np.where(np.abs(x) < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def taps(n_in, n_out):
    """(start int32[n_out], k int16[n_out, T]) of one axis resampled from n_in to n_out samples, by the rule of
    include/dcvc_hip_scale.h: output i is sum_t k[i, t] / 16384 * in[start[i] + t], every row sums to 16384.
    Refused by name: n_in == n_out, a ratio outside [1/4, 4], more than 32 taps, n_in < T, sides beyond 32768."""
    n_in, n_out = int(n_in), int(n_out)
    if not (0 < n_in <= MAX_SIDE and 0 < n_out <= MAX_SIDE):
        raise ValueError(f"taps: sides must be within 1..{MAX_SIDE}, got {n_in} -> {n_out}")
    if n_in == n_out:
        raise ValueError(f"taps: {n_in} -> {n_out} is no resampling (n_in == n_out)")
    if not (n_in <= 4 * n_out and n_out <= 4 * n_in):
        raise ValueError(f"taps: the ratio {n_in}/{n_out} is outside [1/4, 4]")
    r = n_in / n_out
    f = max(1.0, r)
    S = 3.0 * f
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * r
        lo, hi = max(0, int(c - S + 0.5)), min(n_in, int(c + S + 0.5))
        w = _lanczos3((np.arange(lo, hi, dtype=np.float64) + 0.5 - c) / f)
        w = w / w.sum()
        k = np.rint(UNIT * w).astype(np.int64)
        k[int(np.argmax(k))] += UNIT - int(k.sum())  # (argmax: the FIRST largest)
        rows.append((lo, k))
    T = max(len(k) for _, k in rows)
    if T > MAX_TAPS:
        raise ValueError(f"taps: {n_in} -> {n_out} needs {T} taps, more than {MAX_TAPS}")
    if n_in < T:
        raise ValueError(f"taps: {n_in} samples are fewer than the {T} taps of {n_in} -> {n_out} (n_in < T)")
    start = np.zeros(n_out, dtype=np.int32)
    table = np.zeros((n_out, T), dtype=np.int16)
    for i, (lo, k) in enumerate(rows):
        start[i] = min(lo, n_in - T)
        table[i, lo - start[i]:lo - start[i] + len(k)] = k
    return start, table


def as_ratio(ratio):
    """The ratio n/d of a base layer as a Fraction: from a Fraction, an (n, d) pair or an "n/d" string.  Refused by name:
    anything else, and a ratio outside 1/4 <= n/d < 1."""
    try:
        if isinstance(ratio, Fraction):
            q = ratio
        elif isinstance(ratio, str):
            n, d = ratio.split("/")
            q = Fraction(int(n), int(d))
        elif isinstance(ratio, (tuple, list)) and len(ratio) == 2 and all(isinstance(v, (int, np.integer)) and
                                                                          not isinstance(v, bool) for v in ratio):
            q = Fraction(int(ratio[0]), int(ratio[1]))
        else:
            raise ValueError
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"base scale: expected a ratio n/d as a Fraction, an (n, d) pair or an 'n/d' string, got {ratio!r}") from None
    if not MIN_RATIO <= q < 1:
        raise ValueError(f"base scale: the ratio must be within 1/4 <= n/d < 1, got {q}")
    return q


def base_size(height, width, ratio):
    """(hb, wb): each side as (2 side n + d) // (2 d) -- side n / d rounded half up -- for the ratio n/d."""
    q = as_ratio(ratio)
    n, d = q.numerator, q.denominator
    for side in (height, width):
        if not 0 < int(side) <= MAX_SIDE:
            raise ValueError(f"base_size: picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
    return tuple((2 * int(side) * n + d) // (2 * d) for side in (height, width))


def _tables(full, base):
    (h, w), (hb, wb) = full, base
    return {"down_y": taps(h, hb), "down_x": taps(w, wb), "up_y": taps(hb, h), "up_x": taps(wb, w)}


def table_crc(table):
    start, k = table
    return zlib.crc32(np.ascontiguousarray(k).tobytes(), zlib.crc32(np.ascontiguousarray(start).tobytes())) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ device
class _Axis:
    """One table on the host (what the entry point validates) and on the device (what the kernel reads)."""

    def __init__(self, table, device):
        import torch

        self.start, self.k = np.ascontiguousarray(table[0], np.int32), np.ascontiguousarray(table[1], np.int16)
        self.T = int(self.k.shape[1])
        self.start_dev = torch.from_numpy(self.start).to(device)
        self.k_dev = torch.from_numpy(self.k).to(device)

    def args(self):
        return self.start.ctypes.data, self.k.ctypes.data, self.start_dev.data_ptr(), self.k_dev.data_ptr(), self.T


def _planes(t, what, out=False):
    """(tensor viewed as (N, 3, H, W), row stride, plane stride, planes) of a (..., 3, H, W) float32 picture on the GPU,
    read (out: written) in place when its planes are evenly spaced dense rows, else through a contiguous copy (out: a
    ValueError)."""
    import torch

    devargs.on_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() < 3 or t.shape[-3] != 3 or t.numel() == 0:
        raise ValueError(f"{what}: expected a (..., 3, H, W) float32 picture, got {tuple(t.shape)} {t.dtype}")
    H, W = t.shape[-2:]
    t = t.detach()
    if t.dim() != 4:
        if out:
            try:
                t4 = t.view(-1, 3, H, W)
            except RuntimeError:
                raise ValueError(f"{what}: out= must hold evenly spaced planes of dense rows, got strides {t.stride()}") from None
        else:
            t4 = t.reshape(-1, 3, H, W)
    else:
        t4 = t
    p, rs, ps = devargs.planar(t4)
    if out and p is not t4:
        raise ValueError(f"{what}: out= must hold evenly spaced planes of dense rows, got strides {t.stride()}")
    return p, rs, ps, 3 * p.shape[0]


def scale_planes(x, size, y_axis, x_axis, out=None, what="scale"):
    """One launch of dcvc_scale_planes on the current stream: `x` (..., 3, H_in, W_in) -> (..., 3, *size) through the
    two tables.  out: a float32 tensor of that shape on x's device, written in place (a strided view is fine)."""
    import torch

    src, s_rs, s_ps, planes = _planes(x, what)
    H_in, W_in = src.shape[-2:]
    H_out, W_out = size
    shape = tuple(x.shape[:-2]) + (H_out, W_out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.device != src.device:
        raise ValueError(f"{what}: out= must be a {shape} float32 tensor on {src.device}")
    dst, d_rs, d_ps, _ = _planes(out, f"{what}: out=", out=True)
    if len(y_axis.start) != H_out or len(x_axis.start) != W_out:
        raise ValueError(f"{what}: tables of {len(y_axis.start)}x{len(x_axis.start)} outputs for a {H_out}x{W_out} picture")
    devargs.launch("dcvc_scale_planes", src.device, src.data_ptr(), s_rs, s_ps, dst.data_ptr(), d_rs, d_ps, planes, H_in, W_in,
                   H_out, W_out, *x_axis.args(), *y_axis.args(), what=what)
    return out


class Scale:
    """The resampler pair of one base layer: full = (height, width) of the source, ratio n/d (as_ratio), on `device`.
    The four tables are built and uploaded once, and the device is synchronised before this returns: the GOP streams that
    use them afterwards must not race the uploads.  .base is the base layer's (height, width)."""

    def __init__(self, full, ratio, device):
        import torch

        self.full, self.ratio = (int(full[0]), int(full[1])), as_ratio(ratio)
        self.base = base_size(self.full[0], self.full[1], self.ratio)
        self.device = devargs.cuda_device(device, "Scale")
        self.tables = _tables(self.full, self.base)
        self.axes = {name: _Axis(self.tables[name], self.device) for name in TABLES}
        torch.cuda.synchronize(self.device)

    def _run(self, x, src, dst, which, out):
        if not hasattr(x, "shape") or tuple(x.shape[-2:]) != src:
            raise ValueError(f"{which}: expected a (..., 3, {src[0]}, {src[1]}) picture, got {tuple(getattr(x, 'shape', ()))}")
        if hasattr(x, "device") and x.is_cuda and x.device != self.device:
            raise ValueError(f"{which}: the picture is on {x.device}, the tables on {self.device}")
        return scale_planes(x, dst, self.axes[f"{which}_y"], self.axes[f"{which}_x"], out, which)

    def down(self, x, out=None):
        """The base-size picture of a full-size one."""
        return self._run(x, self.full, self.base, "down", out)

    def up(self, x, out=None):
        """The full-size picture of a base-size one."""
        return self._run(x, self.base, self.full, "up", out)

    def to_json(self):
        q = self.ratio
        return {"version": VERSION, "filter": FILTER, "unit": UNIT, "full": list(self.full), "base": list(self.base),
                "ratio": [q.numerator, q.denominator],
                "tables": {name: "%08x" % table_crc(self.tables[name]) for name in TABLES}}


# -------------------------------------------------------------------------------------------------------- scale.json
def write_scale(bin_dir, scale):
    """scale.json beside the .bin files -- only for an encode with a base scale: without one none is needed (and a stale
    file of an earlier encode into the same folder must not describe these .bin files)."""
    from .stream import write_sidecar

    return write_sidecar(bin_dir, SCALE_JSON, None if scale is None else scale.to_json())


def parse_scale(info, where=SCALE_JSON):
    """{"full": (h, w), "base": (hb, wb), "ratio": Fraction} of a scale.json record.  The tables are rebuilt on THIS host
    and held against the record's digests.  Refused by name: an unknown version, filter or unit, missing or mistyped
    fields, a base size the ratio does not give, and a table whose CRC-32 differs (a host whose libm moves one weight
    across a rounding tie must not decode silently)."""
    if not isinstance(info, dict):
        raise ValueError(f"{where}: expected a JSON object")
    if info.get("version") != VERSION:
        raise ValueError(f"{where}: unknown version {info.get('version')!r} (this build reads version {VERSION})")
    if info.get("filter") != FILTER or info.get("unit") != UNIT:
        raise ValueError(f"{where}: unknown filter {info.get('filter')!r} with unit {info.get('unit')!r} (this build knows "
                         f"{FILTER!r} with unit {UNIT})")
    pairs = {}
    for key in ("full", "base", "ratio"):
        v = info.get(key)
        if not (isinstance(v, list) and len(v) == 2 and all(isinstance(s, int) and not isinstance(s, bool) and s > 0 for s in v)):
            raise ValueError(f"{where}: {key} must be two positive integers, got {v!r}")
        pairs[key] = (v[0], v[1])
    try:
        ratio = as_ratio(pairs["ratio"])
        base = base_size(*pairs["full"], ratio)
    except ValueError as ex:
        raise ValueError(f"{where}: {ex}") from None
    if base != pairs["base"]:
        raise ValueError(f"{where}: the ratio {ratio} of {pairs['full'][1]}x{pairs['full'][0]} pictures gives a base of "
                         f"{base[1]}x{base[0]}, the file says {pairs['base'][1]}x{pairs['base'][0]}")
    digests = info.get("tables")
    if not isinstance(digests, dict) or set(digests) != set(TABLES):
        raise ValueError(f"{where}: tables must hold the digests of {list(TABLES)}")
    try:
        tables = _tables(pairs["full"], base)
    except ValueError as ex:
        raise ValueError(f"{where}: {ex}") from None
    for name in TABLES:
        got = "%08x" % table_crc(tables[name])
        if digests[name] != got:
            raise ValueError(f"{where}: the {name} table built on this host has the digest {got}, the file says "
                             f"{digests[name]!r}: this host would not rebuild the encoder's pictures")
    return {"full": pairs["full"], "base": base, "ratio": ratio}


def read_scale(bin_dir):
    """parse_scale of the folder's scale.json, or None without the file."""
    from .stream import read_sidecar

    found = read_sidecar(bin_dir, SCALE_JSON)
    return None if found is None else parse_scale(found[1], found[0])
