"""Y4M and raw YUV 4:2:0 files, and the colour conversion between their sample planes and the codec's RGB pictures on
the device (include/dcvc_hip_color.h, csrc/color.hip).

A 4:2:0 frame is 1.5 (8-bit) or 3 (10-bit) bytes per pixel and needs no decoding: a reader fills a caller-supplied
(pinned) buffer straight from the file, one copy takes it to the device and one kernel turns it into the padded
(1, 3, Hp, Wp) float32 picture ``GopEncoder.encode_gop`` takes; a reconstruction takes the same way back.  There is no
torch fallback: anything the kernels do not take is a ValueError.

No agreement with ffmpeg's YUV -> PNG conversion is claimed: its scaler's chroma filter is its own.  For numbers to set
beside ones obtained through the reference's ffmpeg recipe, ``ColorSpec(matrix="bt601")`` with ``quantize8=True`` is
the nearest setting.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import asdict, dataclass

from . import devargs, lib
from .devargs import MAX_SIDE

MATRICES = {"bt709": 0, "bt601": 1}
SITINGS = {"left": 0, "center": 1}


@dataclass(frozen=True)
class ColorSpec:
    matrix: str = "bt709"
    full_range: bool = False
    siting: str = "left"
    bit_depth: int = 8

    def __post_init__(self):
        if self.matrix not in MATRICES:
            raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {self.matrix!r}")
        if self.siting not in SITINGS:
            raise ValueError(f"siting must be one of {sorted(SITINGS)}, got {self.siting!r}")
        if self.bit_depth not in (8, 10):
            raise ValueError(f"bit_depth must be 8 or 10, got {self.bit_depth!r}")

    def coeffs(self) -> lib.ColorCoeffs:
        """The fp32 constants of the kernels (dcvc_color_coeffs: host only, no GPU needed)."""
        cc = lib.ColorCoeffs()
        lib.check(lib.hip().dcvc_color_coeffs(MATRICES[self.matrix], int(bool(self.full_range)), self.bit_depth,
                                              SITINGS[self.siting], C.byref(cc)), "color_coeffs")
        return cc

    @property
    def sample_bytes(self):
        return 1 if self.bit_depth == 8 else 2

    def to_json(self):
        return asdict(self)

    @staticmethod
    def from_json(d):
        return ColorSpec(str(d["matrix"]), bool(d["full_range"]), str(d["siting"]), int(d["bit_depth"]))


def check_size(height, width):
    if height <= 0 or width <= 0 or height % 2 or width % 2:
        raise ValueError(f"4:2:0 pictures need even, positive sides, got {width}x{height}")
    if height > MAX_SIDE or width > MAX_SIDE:
        raise ValueError(f"picture sides beyond {MAX_SIDE} are not supported, got {width}x{height}")


def frame_samples(height, width):
    return height * width * 3 // 2


def frame_bytes(height, width, bit_depth=8):
    return frame_samples(height, width) * (1 if bit_depth == 8 else 2)


# --------------------------------------------------------------------------------------------------- device conversion
def _sample_dtype(spec):
    import torch

    return torch.uint8 if spec.bit_depth == 8 else torch.int16


def _check_plane(t, rows, cols, spec, what):
    devargs.on_gpu(t, what, noun="sample plane")
    if t.dtype != _sample_dtype(spec):
        raise ValueError(f"{what}: {spec.bit_depth}-bit samples are {_sample_dtype(spec)}, got {t.dtype}")
    if t.dim() != 2 or tuple(t.shape) != (rows, cols) or t.stride(1) != 1 or t.stride(0) < cols:
        raise ValueError(f"{what}: expected a ({rows}, {cols}) plane with dense rows, got {tuple(t.shape)} strides {t.stride()}")


def split_planes(frame, height, width):
    """The (H, W), (H/2, W/2), (H/2, W/2) views of one I420 buffer."""
    n = height * width
    flat = frame.reshape(-1)
    return (flat[:n].view(height, width), flat[n:n + n // 4].view(height // 2, width // 2),
            flat[n + n // 4:n + n // 2].view(height // 2, width // 2))


def planes_to_rgb(y, u, v, spec, out_size=None, quantize8=False):
    """Three device sample planes (rows may be strided) -> (1, 3, out_H, out_W) float32, zero beyond the picture."""
    import torch

    if not torch.is_tensor(y) or y.dim() != 2:
        raise ValueError("planes_to_rgb takes 2-D sample planes")
    H, W = y.shape
    check_size(H, W)
    _check_plane(y, H, W, spec, "y")
    _check_plane(u, H // 2, W // 2, spec, "u")
    _check_plane(v, H // 2, W // 2, spec, "v")
    if u.stride(0) != v.stride(0) or not (y.device == u.device == v.device):
        raise ValueError("the chroma planes must share one row stride and all planes one device")
    oh, ow = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if oh < H or ow < W or oh > MAX_SIDE or ow > MAX_SIDE:
        raise ValueError(f"output size {(oh, ow)} does not hold a {(H, W)} picture")
    cc = spec.coeffs()
    out = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=y.device)
    devargs.launch("dcvc_yuv420_to_rgb", y.device, y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W, y.stride(0), u.stride(0),
                   C.byref(cc), out.data_ptr(), oh, ow, ow, oh * ow, int(bool(quantize8)))
    return out


def yuv420_to_rgb(frame, height, width, spec=ColorSpec(), pad=True, quantize8=False):
    """`frame`: ONE contiguous device buffer in file order (Y plane, U plane, V plane: I420), uint8 or int16 (10-bit).
    Returns the (1, 3, Hp, Wp) float32 picture on the current stream; pad=True: Hp, Wp the next multiples of 64, zeros
    to the right and below (pipeline.pad_frame's), written by the same launch.  quantize8: every value one of the 256
    floats uint8 / 255.0 has on the host, i.e. the picture a PNG of the rounded pixels would give encode_folder."""
    from . import stream as S

    check_size(height, width)
    devargs.on_gpu(frame, "yuv420_to_rgb", noun="I420 buffer")
    if frame.dtype != _sample_dtype(spec):
        raise ValueError(f"{spec.bit_depth}-bit samples are {_sample_dtype(spec)}, got {frame.dtype}")
    if not frame.is_contiguous() or frame.numel() != frame_samples(height, width):
        raise ValueError(f"expected a contiguous I420 buffer of {frame_samples(height, width)} samples, got {tuple(frame.shape)}")
    size = None
    if pad:
        _, r, _, b = S.get_padding_size(height, width)
        size = (height + b, width + r)
    return planes_to_rgb(*split_planes(frame, height, width), spec, size, quantize8)


def rgb_to_yuv420(rgb, height, width, spec=ColorSpec(), source=None):
    """(1, 3, >=height, >=width) float32 on the GPU (clamped to [0, 1] as it is loaded; the top-left height x width
    pixels are read in place) -> the I420 device buffer.  With `source` (the I420 buffer the picture came from): also a
    (3,) int64 device tensor, the sums of squared sample differences of the Y, U and V planes (psnr_yuv)."""
    import torch

    check_size(height, width)
    crop = devargs.checked(rgb, "rgb_to_yuv420", at_least=(height, width))
    if source is not None:
        if not torch.is_tensor(source) or source.device != rgb.device or source.dtype != _sample_dtype(spec) or \
                not source.is_contiguous() or source.numel() != frame_samples(height, width):
            raise ValueError("source must be the contiguous I420 device buffer of the same size and depth")
    cc = spec.coeffs()
    crop, rs, ps = devargs.planar(crop)
    out = torch.empty(frame_samples(height, width), dtype=_sample_dtype(spec), device=rgb.device)
    y, u, v = split_planes(out, height, width)
    src = (None, None, None) if source is None else tuple(t.data_ptr() for t in split_planes(source, height, width))
    sums = None if source is None else torch.zeros(3, dtype=torch.int64, device=rgb.device)
    devargs.launch("dcvc_rgb_to_yuv420", rgb.device, crop.data_ptr(), height, width, rs, ps, C.byref(cc), y.data_ptr(), u.data_ptr(),
                   v.data_ptr(), width, width // 2, *src, width, width // 2, None if sums is None else sums.data_ptr())
    return out if source is None else (out, sums)


def psnr_yuv(sums, height, width, bit_depth=8):
    """(PSNR-Y, PSNR-U, PSNR-V, (6 Y + U + V) / 8) in dB, float64 on the host, from the three integer sums of
    rgb_to_yuv420(..., source=); an identical plane has infinite PSNR."""
    sy, su, sv = (int(s) for s in (sums.tolist() if hasattr(sums, "tolist") else sums))
    peak = float((1 << bit_depth) - 1) ** 2

    def one(s, n):
        return 10.0 * math.log10(peak / (s / n)) if s > 0 else float("inf")

    py, pu, pv = one(sy, height * width), one(su, height * width // 4), one(sv, height * width // 4)
    return py, pu, pv, (6.0 * py + pu + pv) / 8.0


# ------------------------------------------------------------------------------------------------------------- files
Y4M_CHROMA = {  # tag -> (siting, bit depth)
    "420": ("left", 8), "420jpeg": ("center", 8), "420mpeg2": ("left", 8), "420paldv": ("left", 8), "420p10": ("left", 10),
}


def y4m_chroma_tag(spec):
    return "420p10" if spec.bit_depth == 10 else ("420jpeg" if spec.siting == "center" else "420mpeg2")


def _readinto(fd, buf, offset, what):
    view = memoryview(buf).cast("B")
    got = 0
    while got < len(view):
        n = os.preadv(fd, [view[got:]], offset + got)
        if n <= 0:
            raise ValueError(f"{what}: file ends inside a frame")
        got += n


def _writefrom(fd, buf, offset):
    view = memoryview(buf).cast("B")
    done = 0
    while done < len(view):
        done += os.pwrite(fd, view[done:], offset + done)


class _Indexed:
    """Frames at a fixed stride: frame k starts at `start + k * stride` (+ `lead` bytes of per-frame header)."""

    def _close(self):
        if getattr(self, "fd", None) is not None:
            os.close(self.fd)
            self.fd = None

    close = _close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self._close()


class RawYUVReader(_Indexed):
    """Headerless I420 (`.yuv`): the caller knows size and depth -- and, for interlaced material, the field order
    (`field_order`: "tff", "bff" or None; the reader only carries it, vcm_ts_amd/deint.py uses it)."""
    field_order = None

    def __init__(self, path, width, height, bit_depth=8, field_order=None):
        if field_order not in (None, "tff", "bff"):
            raise ValueError(f"field_order must be 'tff' or 'bff', got {field_order!r}")
        self.field_order = field_order
        check_size(height, width)
        if bit_depth not in (8, 10):
            raise ValueError(f"bit_depth must be 8 or 10, got {bit_depth!r}")
        self.path, self.width, self.height, self.bit_depth = path, int(width), int(height), int(bit_depth)
        self.frame_bytes = frame_bytes(height, width, bit_depth)
        self.start = self.lead = 0
        self.fps, self.header = None, {}
        size = os.path.getsize(path)
        if size % self.frame_bytes:
            raise ValueError(f"{path}: truncated last frame ({size} bytes is not a multiple of {self.frame_bytes} for "
                             f"{width}x{height} at {bit_depth} bits)")
        self.n_frames = size // self.frame_bytes
        self.fd = os.open(path, os.O_RDONLY)

    def spec(self, matrix=None, full_range=None, siting=None):
        return ColorSpec(matrix or "bt709", bool(full_range) if full_range is not None else False, siting or "left", self.bit_depth)

    def read_into(self, index, buf):
        """Fill `buf` (any writable buffer of frame_bytes bytes, e.g. a pinned tensor's .numpy()) with frame `index`."""
        if not 0 <= index < self.n_frames:
            raise IndexError(f"frame {index} of {self.n_frames}")
        if memoryview(buf).nbytes != self.frame_bytes:
            raise ValueError(f"buffer of {memoryview(buf).nbytes} bytes for a frame of {self.frame_bytes}")
        _readinto(self.fd, buf, self.start + index * (self.lead + self.frame_bytes) + self.lead, self.path)


class Y4MReader(RawYUVReader):
    """YUV4MPEG2, progressive 4:2:0 at 8 or 10 bits.  Everything is validated when the file is opened.
    interlaced=True (opt-in: the caller deinterlaces, vcm_ts_amd/deint.py) also accepts It and Ib, and Im when a
    field_order is given; `field_order` is then "tff" / "bff" -- the explicit one, else the header's -- or None for a file
    whose header says progressive and no explicit order."""

    def __init__(self, path, interlaced=False, field_order=None):
        if field_order not in (None, "tff", "bff"):
            raise ValueError(f"field_order must be 'tff' or 'bff', got {field_order!r}")
        if field_order is not None and not interlaced:
            raise ValueError("field_order belongs to interlaced=True")
        with open(path, "rb") as f:
            head = f.read(1024)
        end = head.find(b"\n")
        if not head.startswith(b"YUV4MPEG2") or end < 0:
            raise ValueError(f"{path}: not a YUV4MPEG2 file")
        tokens = head[:end].decode("ascii", "replace").split(" ")[1:]
        h = {}
        for tok in tokens:
            if not tok:
                continue
            if tok[0] == "X":
                h.setdefault("X", []).append(tok[1:])
            else:
                h[tok[0]] = tok[1:]
        if "W" not in h or "H" not in h:
            raise ValueError(f"{path}: Y4M header without W or H")
        try:
            width, height = int(h["W"]), int(h["H"])
        except ValueError:
            raise ValueError(f"{path}: bad size in Y4M header {h.get('W')!r} x {h.get('H')!r}") from None
        mark = h.get("I", "p")
        if mark not in ("p", "?") and not interlaced:
            raise ValueError(f"{path}: interlaced material (I{h['I']}) is not supported (encode --deinterlace takes It and Ib)")
        if mark not in ("p", "?", "t", "b", "m"):
            raise ValueError(f"{path}: unknown interlacing mark I{mark}")
        if mark == "m" and field_order is None:
            raise ValueError(f"{path}: mixed interlaced material (Im) names no field order: give one (--field-order)")
        self.field_order = field_order or {"t": "tff", "b": "bff"}.get(mark)
        chroma = h.get("C", "420")
        if chroma not in Y4M_CHROMA:
            raise ValueError(f"{path}: chroma format C{chroma} is not supported (4:2:0 at 8 or 10 bits only)")
        if width <= 0 or height <= 0 or width % 2 or height % 2:
            raise ValueError(f"{path}: 4:2:0 pictures need even, positive sides, got {width}x{height}")
        self.siting, depth = Y4M_CHROMA[chroma]
        self.chroma = chroma
        self.full_range = None
        for x in h.get("X", []):
            if x.startswith("COLORRANGE="):
                val = x.split("=", 1)[1]
                if val not in ("FULL", "LIMITED"):
                    raise ValueError(f"{path}: unknown XCOLORRANGE={val}")
                self.full_range = val == "FULL"
        fps = None
        if "F" in h:
            try:
                num, den = (int(v) for v in h["F"].split(":"))
            except ValueError:
                raise ValueError(f"{path}: bad frame rate F{h['F']}") from None
            fps = (num, den) if num > 0 and den > 0 else None
        check_size(height, width)
        self.path, self.width, self.height, self.bit_depth = path, width, height, depth
        self.frame_bytes = frame_bytes(height, width, depth)
        self.start, self.lead = end + 1, 6
        self.fps, self.header = fps, h
        self.interlace, self.aspect = h.get("I"), h.get("A")
        body = os.path.getsize(path) - self.start
        stride = self.lead + self.frame_bytes
        self.fd = os.open(path, os.O_RDONLY)
        try:
            self.n_frames = body // stride
            for k in range(self.n_frames):  # (6 bytes each: a FRAME line with parameters would shift every later frame)
                line = os.pread(self.fd, 6, self.start + k * stride)
                if line != b"FRAME\n":
                    what = "FRAME line with parameters" if line.startswith(b"FRAME ") else "no FRAME marker where a frame should start"
                    raise ValueError(f"{path}: frame {k}: {what}")
            if body % stride:
                if os.pread(self.fd, 6, self.start + self.n_frames * stride).startswith(b"FRAME "):
                    raise ValueError(f"{path}: frame {self.n_frames}: FRAME line with parameters")
                raise ValueError(f"{path}: truncated last frame ({body % stride} of {stride} bytes)")
        except BaseException:
            self._close()
            raise

    def spec(self, matrix=None, full_range=None, siting=None):
        """The file's ColorSpec: what the header says, explicit arguments override it, else bt709 / limited / left."""
        fr = full_range if full_range is not None else (self.full_range if self.full_range is not None else False)
        return ColorSpec(matrix or "bt709", bool(fr), siting or self.siting, self.bit_depth)


class RawYUVWriter(_Indexed):
    """Frames are placed by index (positional writes), so pictures that finish out of order land in display order."""

    def __init__(self, path, width, height, spec=ColorSpec()):
        check_size(height, width)
        self.path, self.width, self.height, self.spec = path, int(width), int(height), spec
        self.frame_bytes = frame_bytes(height, width, spec.bit_depth)
        self.start = self.lead = 0
        self.n_frames = 0
        self.fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        self._preamble()

    def _preamble(self):
        pass

    def write(self, index, buf):
        if memoryview(buf).nbytes != self.frame_bytes:
            raise ValueError(f"buffer of {memoryview(buf).nbytes} bytes for a frame of {self.frame_bytes}")
        at = self.start + index * (self.lead + self.frame_bytes)
        if self.lead:
            _writefrom(self.fd, b"FRAME\n", at)
        _writefrom(self.fd, buf, at + self.lead)
        self.n_frames = max(self.n_frames, index + 1)


class Y4MWriter(RawYUVWriter):
    def __init__(self, path, width, height, spec=ColorSpec(), fps=(25, 1), chroma=None, interlace="p", aspect=None):
        chroma = chroma or y4m_chroma_tag(spec)
        if Y4M_CHROMA.get(chroma, (None, None))[1] != spec.bit_depth:
            raise ValueError(f"chroma tag C{chroma} does not describe {spec.bit_depth}-bit 4:2:0")
        fps = tuple(fps) if fps else (25, 1)
        head = f"YUV4MPEG2 W{int(width)} H{int(height)} F{int(fps[0])}:{int(fps[1])} I{interlace or 'p'}"
        if aspect:
            head += f" A{aspect}"
        head += f" C{chroma} XCOLORRANGE={'FULL' if spec.full_range else 'LIMITED'}\n"
        self._head = head.encode("ascii")
        super().__init__(path, width, height, spec)

    def _preamble(self):
        _writefrom(self.fd, self._head, 0)
        self.start, self.lead = len(self._head), 6


def open_video(path, size=None, bit_depth=8, fps=None, interlaced=False, field_order=None):
    """A reader for `path` by its extension: `.y4m`, or `.yuv` with size=(width, height).  interlaced, field_order: as
    Y4MReader's; a `.yuv` reader carries the field_order it is given."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        return Y4MReader(path, interlaced, field_order) if interlaced else Y4MReader(path)
    if ext == ".yuv":
        if size is None:
            raise ValueError(f"{path}: a raw .yuv file needs its size (--size WxH)")
        if field_order is not None and not interlaced:
            raise ValueError("field_order belongs to interlaced=True")
        r = RawYUVReader(path, size[0], size[1], bit_depth, field_order)
        r.fps = tuple(fps) if fps else None
        return r
    raise ValueError(f"{path}: unknown video extension {ext!r} (expected .y4m or .yuv)")


def create_video(path, width, height, spec, fps=None, chroma=None, interlace=None, aspect=None):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        return Y4MWriter(path, width, height, spec, fps or (25, 1), chroma, interlace or "p", aspect)
    if ext == ".yuv":
        return RawYUVWriter(path, width, height, spec)
    raise ValueError(f"{path}: unknown video extension {ext!r} (expected .y4m or .yuv)")


def parse_size(text):
    """'1920x1080' -> (1920, 1080)"""
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise ValueError(f"size must look like 1920x1080, got {text!r}") from None
    return w, h
