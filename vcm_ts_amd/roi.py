"""The region-of-interest enhancement layer on the device (include/dcvc_hip_roi.h, csrc/roi.hip): what the reference's
``video_coder.py`` does with pictures around its base layer -- ``compute_residuals``, ``fuse_layers`` and
``calc_visual_metrics`` -- as three streaming kernels on pictures the codec already holds on the GPU.

Boxes are taken as given (the reference's coordinate files, or any callable ``frame_index -> FrameBoxes``); the
detectors and the HEVC coding of the residual layer stay outside.  The residual layer leaves as 8-bit planes in the
order ``ffmpeg -f rawvideo -pix_fmt gbrp`` reads and writes (RawPlanarWriter / RawPlanarReader), or as RGB pictures.

All arithmetic is stated in the header and pinned bit for bit by tests/test_gpu_roi.py.  Every call runs on the caller's
current stream and synchronises nothing.  There is no torch fallback: anything the kernels do not take is a ValueError.
"""
from __future__ import annotations

import io
import math
import os
import pickle
from dataclasses import dataclass

import numpy as np

from . import devargs, lib
from .devargs import MAX_SIDE, whole
from .yuv import _Indexed, _readinto, _writefrom

MAX_BOXES, MAX_CLASSES, MAX_BORDER = 1024, 4, 64
CELL, MAX_GROW, MIN_Q, MAX_Q = 16, 255, 10, 1000  # the q-scale map: cell side in pixels, factors in hundredths
ORDERS = {"rgb": (0, 1, 2), "gbr": (1, 2, 0)}  # slot j of the 8-bit picture holds channel ORDERS[..][j]
LAYOUTS = ("planar", "hwc")


def feather_table(border):
    """The `border` values of the reference's create_gradient_mask, outermost ring first: float32(1 - linspace(0.9, 0,
    border)), evaluated in double precision on the host.  border 1 gives [0.1] (the reference's behaviour, kept);
    border 0 an empty table (the mask is then 1.0 over the whole box)."""
    border = int(border)
    if not 0 <= border <= MAX_BORDER:
        raise ValueError(f"border must be within 0..{MAX_BORDER}, got {border}")
    return (1.0 - np.linspace(0.9, 0.0, border)).astype(np.float32)


@dataclass(frozen=True)
class RoiClass:
    """One kind of box (in the reference: licence plates, faces) with its PADDING: `border` feathers the fusion mask,
    `shrink` (default: the same value, as the reference uses one PADDING for both) shrinks the box for region_sse."""
    border: int = 0
    shrink: int = None

    def __post_init__(self):
        if self.shrink is None:
            object.__setattr__(self, "shrink", self.border)
        for name in ("border", "shrink"):
            v = getattr(self, name)
            if int(v) != v or not 0 <= v <= MAX_BORDER:
                raise ValueError(f"{name} must be an integer within 0..{MAX_BORDER}, got {v!r}")
            object.__setattr__(self, name, int(v))

    def record(self):
        rec = lib.RoiClassRec()
        rec.border, rec.shrink = self.border, self.shrink
        for i, v in enumerate(feather_table(self.border)):
            rec.feather[i] = v
        return rec


def _class_records(classes):
    classes = tuple(classes)
    if len(classes) > MAX_CLASSES or not all(isinstance(c, RoiClass) for c in classes):
        raise ValueError(f"classes: at most {MAX_CLASSES} RoiClass records")
    recs = (lib.RoiClassRec * max(len(classes), 1))()
    for i, c in enumerate(classes):
        recs[i] = c.record()
    return recs, len(classes)


class FrameBoxes:
    """The boxes of one picture: an (n, 5) int32 array of {x1, y1, x2, y2, cls}, half-open as numpy slices
    [y1:y2, x1:x2]; x2 <= x1 or y2 <= y1 is an empty box.  List order matters: where boxes overlap, the last one decides
    the feather value."""

    def __init__(self, boxes=()):
        a = np.asarray(boxes)
        if a.size == 0:
            a = np.zeros((0, 5), dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != 5 or a.dtype.kind not in "iu":
            raise ValueError(f"boxes: expected an (n, 5) integer array of x1, y1, x2, y2, cls, got {a.shape} {a.dtype}")
        if len(a) > MAX_BOXES:
            raise ValueError(f"too many boxes: {len(a)} (at most {MAX_BOXES} per picture)")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("boxes: coordinates out of range")
        self.array = np.ascontiguousarray(a, dtype=np.int32)
        self._dev = self._pin = None

    def __len__(self):
        return len(self.array)

    def validate(self, height, width, n_classes=MAX_CLASSES):
        """What the entry points would refuse, by name, before any GPU work."""
        a = self.array
        if len(a) == 0:
            return self
        if (a[:, [0, 2]] < 0).any() or (a[:, [0, 2]] > width).any() or (a[:, [1, 3]] < 0).any() or (a[:, [1, 3]] > height).any():
            bad = int(np.flatnonzero((a[:, :4] < 0).any(1) | (a[:, [0, 2]] > width).any(1) | (a[:, [1, 3]] > height).any(1))[0])
            raise ValueError(f"box {bad} {a[bad, :4].tolist()}: coordinates out of range for a {width}x{height} picture")
        if (a[:, 4] < 0).any() or (a[:, 4] >= n_classes).any():
            bad = int(np.flatnonzero((a[:, 4] < 0) | (a[:, 4] >= n_classes))[0])
            raise ValueError(f"box {bad}: unknown class {int(a[bad, 4])} ({n_classes} classes)")
        return self

    def attached(self, device):
        return self._dev is not None and self._dev.device == device

    def attach(self, pin, dev):
        """Use `dev` (int32, 5 n values, part of a larger upload from the pinned tensor `pin`) as the device copy."""
        self._pin, self._dev = pin, dev

    def on_device(self, device):
        """The device copy the kernels read (made once, through pinned memory, on the current stream)."""
        import torch

        if not self.attached(device):
            self._pin = torch.from_numpy(self.array.reshape(-1).copy()).pin_memory()
            self._dev = self._pin.to(device, non_blocking=True)
        return self._dev


def as_boxes(boxes):
    return boxes if isinstance(boxes, FrameBoxes) else FrameBoxes(boxes)


@dataclass(frozen=True)
class Roi:
    """What the file loops take as `roi=`: a box source (PickleBoxes or any callable frame_index -> FrameBoxes, frame 0
    first) and the classes its `cls` values index."""
    boxes: object
    classes: tuple
    names: tuple = None

    def __post_init__(self):
        object.__setattr__(self, "classes", tuple(self.classes))
        _class_records(self.classes)
        if not callable(self.boxes):
            raise ValueError("roi: the box source must be callable (frame_index -> FrameBoxes)")
        names = self.names if self.names is not None else getattr(self.boxes, "names", None)
        object.__setattr__(self, "names", tuple(names) if names else tuple(f"class{i}" for i in range(len(self.classes))))

    def frame(self, index, height, width):
        return as_boxes(self.boxes(index)).validate(height, width, len(self.classes))

    def to_json(self):
        return {"classes": [{"name": n, "border": c.border, "shrink": c.shrink} for n, c in zip(self.names, self.classes)]}


@dataclass(frozen=True)
class RoiQ:
    """ROI-weighted quantisation (include/dcvc_hip_roi.h, "Q-scale map"): a factor on the quantisation step of the latent
    y per 16x16-pixel cell -- `background` where no box touches the cell, else the smallest of classes[cls] over the boxes
    (grown by `grow` pixels) that do.  Factors are integers in HUNDREDTHS, 10..1000; the value used is
    float32(k) / float32(100).  Below 100 quantises finer (more bits), above 100 coarser.  There are no tuned values:
    every default is 100, which codes exactly what no map codes."""
    background: int = 100
    classes: tuple = ()
    grow: int = 0

    def __post_init__(self):
        try:
            classes = tuple(self.classes)
        except TypeError:
            raise ValueError(f"classes: expected a sequence of factors in hundredths, got {self.classes!r}") from None
        if len(classes) > MAX_CLASSES:
            raise ValueError(f"classes: at most {MAX_CLASSES} factors, got {len(classes)}")

        object.__setattr__(self, "background", whole("background", self.background, MIN_Q, MAX_Q, "hundredths"))
        object.__setattr__(self, "classes", tuple(whole(f"classes[{i}]", v, MIN_Q, MAX_Q, "hundredths")
                                                  for i, v in enumerate(classes)))
        object.__setattr__(self, "grow", whole("grow", self.grow, 0, MAX_GROW, "pixels"))

    @staticmethod
    def hundredths(value, name="factor"):
        """A float factor snapped to hundredths (the command line's --plate-q 0.6 -> 60)."""
        return devargs.hundredths(value, name)

    def factors(self):
        """[background, class 0, ...] as the float32 values the kernels multiply with (the HOST's IEEE division)."""
        return np.array((self.background,) + self.classes, dtype=np.float32) / np.float32(100)

    def is_neutral(self):
        return self.background == 100 and all(k == 100 for k in self.classes)

    def to_json(self, names):
        names = tuple(names)
        if len(names) != len(self.classes) or len(set(names)) != len(names):
            raise ValueError(f"classes: {len(self.classes)} factors for the class names {list(names)}")
        return {"cell": CELL, "background": self.background, "classes": dict(zip(names, self.classes)), "grow": self.grow}

    @classmethod
    def from_json(cls, info, names=None):
        """names: the class names the factors must belong to, in order (a Roi's); None takes the file's order."""
        if not isinstance(info, dict) or set(info) != {"cell", "background", "classes", "grow"} or \
                not isinstance(info["classes"], dict):
            raise ValueError("expected the keys cell, background, classes (a name -> factor table) and grow")
        if info["cell"] != CELL:
            raise ValueError(f"cell must be {CELL}, got {info['cell']!r}")
        have = tuple(info["classes"])
        if names is not None and tuple(names) != have:
            raise ValueError(f"the class names {list(have)} are not the boxes' {list(names)}")
        return cls(info["background"], tuple(info["classes"][n] for n in have), info["grow"])


def grid_of(height, width):
    """(hc, wc): the latent grid of a height x width picture padded to multiples of 64."""
    return 4 * ((int(height) + 63) // 64), 4 * ((int(width) + 63) // 64)


def q_map(boxes, height, width, roiq, out=None, device=None):
    """The (1, 1, hc, wc) float32 q-scale map of one picture's boxes on the device, made by one kernel on the current
    stream (nothing synchronised): what IntraNoAR / DMC .compress and .decompress take as q_map=.  height, width: the
    UNPADDED picture the boxes live in.  device: where, unless `out` (a contiguous float32 tensor of hc * wc elements) or
    boxes already on a device say so; default the current one."""
    import torch

    if not isinstance(roiq, RoiQ):
        raise ValueError(f"roiq: expected a RoiQ, got {type(roiq).__name__}")
    H, W = int(height), int(width)
    if not (0 < H <= MAX_SIDE and 0 < W <= MAX_SIDE):
        raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {W}x{H}")
    hc, wc = grid_of(H, W)
    boxes = as_boxes(boxes)
    if out is not None:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.numel() == hc * wc and out.is_contiguous()):
            raise ValueError(f"out: expected a contiguous float32 tensor of {hc} x {wc} elements on the GPU")
        dev = out.device
    elif device is not None:
        dev = device
    else:
        dev = boxes._dev.device if boxes._dev is not None else "cuda"
    dev = devargs.cuda_device(dev, "q_map")
    f = np.ascontiguousarray(roiq.factors())
    keep, host, devp, n = _box_args(boxes, H, W, len(roiq.classes), dev)
    if out is None:
        out = torch.empty((1, 1, hc, wc), dtype=torch.float32, device=dev)
    devargs.launch("dcvc_roi_qmap", dev, H, W, host, devp, n, roiq.grow, f.ctypes.data, len(roiq.classes), out.data_ptr())
    return out.view(1, 1, hc, wc)


def as_roi(roi):
    return roi if isinstance(roi, Roi) or roi is None else Roi(*roi)


# ------------------------------------------------------------------------------------------------------------ device
def _u8_strides(t, layout, H, W, what):
    """(chan stride, row stride, pixel stride) of an 8-bit picture: planar (3, H, W) or interleaved (H, W, 3)."""
    import torch

    shape = (3, H, W) if layout == "planar" else (H, W, 3)
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != shape:
        raise ValueError(f"{what}: expected a {shape} uint8 tensor on the GPU for layout {layout!r}")
    s = t.stride()  # (the stride of a size-1 dimension means nothing)
    if layout == "planar":
        rs = s[1] if H > 1 else W
        if (W > 1 and s[2] != 1) or rs < W or s[0] < (H - 1) * rs + W:
            raise ValueError(f"{what}: planes must hold dense rows, got strides {s}")
        return s[0], rs, 1
    rs = s[0] if H > 1 else 3 * W
    if s[2] != 1 or (W > 1 and s[1] != 3) or rs < 3 * W:
        raise ValueError(f"{what}: pixels must be interleaved, got strides {s}")
    return 1, rs, 3


def _order(order):
    if order not in ORDERS:
        raise ValueError(f"order must be one of {sorted(ORDERS)}, got {order!r}")
    return ORDERS[order]


def _box_args(boxes, H, W, n_classes, device):
    boxes = as_boxes(boxes).validate(H, W, n_classes)
    n = len(boxes)
    return boxes, (boxes.array.ctypes.data if n else None), (boxes.on_device(device).data_ptr() if n else None), n


def residual_layer(source, recon, boxes, layout="planar", order="rgb", out=None):
    """compute_residuals: clip(code(source) - code(recon) + 128, 0, 255) inside the boxes, 0 outside, as a uint8 tensor:
    (3, H, W) planes (layout "planar"; order "gbr" gives the planes of ffmpeg's gbrp) or an (H, W, 3) picture ("hwc")."""
    import torch

    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    o = _order(order)
    s, s_rs, s_ps = devargs.picture(source, "source")
    r, r_rs, r_ps = devargs.picture(recon, "recon", like=source)
    H, W = s.shape[2:]
    keep, host, dev, n = _box_args(boxes, H, W, MAX_CLASSES, s.device)
    if out is None:
        out = torch.empty((3, H, W) if layout == "planar" else (H, W, 3), dtype=torch.uint8, device=s.device)
    cs, rs, px = _u8_strides(out, layout, H, W, "out")
    devargs.launch("dcvc_roi_residual", s.device, s.data_ptr(), s_rs, s_ps, r.data_ptr(), r_rs, r_ps, H, W, host, dev, n,
                   out.data_ptr(), cs, rs, px, *o)
    return out


def fuse(base, residual, boxes, classes, out=None, layout=None, order="rgb"):
    """fuse_layers: the base picture's 8-bit codes plus (residual - 128) through the feathered mask of the boxes, clipped
    and truncated as the reference does, returned as the (1, 3, H, W) float32 picture of those codes / 255 -- what
    save_torch_image and yuv.rgb_to_yuv420 take.  `residual`: what residual_layer returned (layout taken from its
    shape unless given; `order` as it was written)."""
    import torch

    o = _order(order)
    b, b_rs, b_ps = devargs.picture(base, "base")
    H, W = b.shape[2:]
    if layout is None:
        shape = tuple(residual.shape) if torch.is_tensor(residual) else None
        if shape == (3, H, W) and shape != (H, W, 3):
            layout = "planar"
        elif shape == (H, W, 3) and shape != (3, H, W):
            layout = "hwc"
        else:
            raise ValueError(f"residual: cannot tell the layout of {shape} for a {W}x{H} picture; pass layout=")
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    recs, n_classes = _class_records(classes)
    cs, rs, px = _u8_strides(residual, layout, H, W, "residual")
    if residual.device != b.device:
        raise ValueError("residual and base are on different devices")
    keep, host, dev, n = _box_args(boxes, H, W, n_classes, b.device)
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=b.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (1, 3, H, W) and
              out.device == b.device and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous (1, 3, {H}, {W}) float32 tensor on {b.device}")
    devargs.launch("dcvc_roi_fuse", b.device, b.data_ptr(), b_rs, b_ps, residual.data_ptr(), cs, rs, px, *o, H, W, host, dev, n,
                   recs, n_classes, out.data_ptr(), W, H * W)
    return out


def region_sse(a, b, boxes, classes, sums=None):
    """calc_visual_metrics' sums on 8-bit codes: a (3,) int64 device tensor of (squared error inside the boxes shrunk by
    their class's shrink, squared error outside, pixels inside), each error summed over the 3 channels.  `sums`: add
    onto these instead of onto zeros."""
    import torch

    x, x_rs, x_ps = devargs.picture(a, "a")
    y, y_rs, y_ps = devargs.picture(b, "b", like=a)
    H, W = x.shape[2:]
    recs, n_classes = _class_records(classes)
    keep, host, dev, n = _box_args(boxes, H, W, n_classes, x.device)
    if sums is None:
        sums = torch.zeros(3, dtype=torch.int64, device=x.device)
    elif not (torch.is_tensor(sums) and sums.dtype == torch.int64 and tuple(sums.shape) == (3,) and
              sums.device == x.device and sums.is_contiguous()):
        raise ValueError("sums: expected a contiguous (3,) int64 tensor on the pictures' device")
    devargs.launch("dcvc_roi_sse", x.device, x.data_ptr(), x_rs, x_ps, y.data_ptr(), y_rs, y_ps, H, W, host, dev, n, recs,
                   n_classes, sums.data_ptr())
    return sums


def region_psnr(sums, height, width, divisors="samples"):
    """(psnr_total, psnr_bg, psnr_roi) in dB, float64 on the host, from region_sse's three integers.
    divisors="samples": each sum over its number of samples, 3 n_in inside and 3 (H W - n_in) outside.
    divisors="reference": calc_visual_metrics' divisors -- the inside sum over n_in (PIXELS, though it sums three
    channels: its figure is 10 log10(3) = 4.77 dB below the per-sample one) and the outside sum over 3 H W - n_in.
    A region without error has infinite PSNR, a region without pixels nan."""
    if divisors not in ("samples", "reference"):
        raise ValueError(f"divisors must be 'samples' or 'reference', got {divisors!r}")
    s_in, s_out, n_in = (int(s) for s in (sums.tolist() if hasattr(sums, "tolist") else sums))
    total = 3 * height * width
    d_in, d_out = (3 * n_in, total - 3 * n_in) if divisors == "samples" else (n_in, total - n_in)

    def one(s, n):
        if n <= 0:
            return float("nan")
        return 10.0 * math.log10(255.0 ** 2 / (s / n)) if s > 0 else float("inf")

    return one(s_in + s_out, total), one(s_out, d_out), one(s_in, d_in)


# ------------------------------------------------------------------------------------------------------------- files
class _ArrayUnpickler(pickle.Unpickler):
    """Admits the names a pickled numpy array is rebuilt from and nothing else."""
    ALLOWED = {(m, n) for m in ("numpy.core.multiarray", "numpy._core.multiarray") for n in ("_reconstruct", "scalar")} | \
              {(m, "_frombuffer") for m in ("numpy.core.numeric", "numpy._core.numeric")} | \
              {("numpy", "ndarray"), ("numpy", "dtype")}

    def find_class(self, module, name):
        if (module, name) not in self.ALLOWED:
            raise pickle.UnpicklingError(f"{module}.{name} is not part of a coordinate array")
        return super().find_class(module, name)


class PickleBoxes:
    """The reference's coordinate files: `root`/liplates_coords/%05d and `root`/faces_coords/%05d (numbered from 1), each
    a pickled np.uint16 (n, 4) array of x1, y1, x2, y2.  Plates come before faces in the list (the reference's order of
    assignment) with cls 0 and 1.  Either folder may be absent; a folder that is there must hold every frame asked for.
    A third, optional folder `root`/motion_coords (motionroi.write_boxes: the same files) adds the class "motion" with
    cls 2, last in the list; `names` and `classes` have three entries only when it exists, and it may be the only one."""
    FOLDERS = (("liplates", "liplates_coords"), ("faces", "faces_coords"))
    MOTION = ("motion", "motion_coords")

    def __init__(self, root, classes=None):
        self.root = root
        known = self.FOLDERS + ((self.MOTION,) if self.has_motion(root) else ())
        self.folders = [(cls, name, os.path.join(root, sub)) for cls, (name, sub) in enumerate(known)
                        if os.path.isdir(os.path.join(root, sub))]
        if not self.folders:
            raise FileNotFoundError(f"{root}: neither liplates_coords nor faces_coords")
        self.names = tuple(name for name, _ in known)
        self.classes = tuple(classes) if classes is not None else tuple(RoiClass(0) for _ in known)
        if len(self.classes) != len(known):
            raise ValueError("PickleBoxes takes two classes: plates, faces" if len(known) == 2 else
                             "PickleBoxes takes three classes with a motion_coords folder: plates, faces, motion")

    @classmethod
    def has_motion(cls, root):
        return os.path.isdir(os.path.join(root, cls.MOTION[1]))

    @staticmethod
    def _load(path):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no coordinate file for this frame")
        with open(path, "rb") as f:
            data = f.read()
        try:
            a = _ArrayUnpickler(io.BytesIO(data)).load()
        except Exception as ex:
            raise ValueError(f"{path}: not a pickled coordinate array ({ex})") from None
        if not isinstance(a, np.ndarray) or a.dtype != np.uint16 or not (a.size == 0 or (a.ndim == 2 and a.shape[1] == 4)):
            raise ValueError(f"{path}: expected an (n, 4) uint16 array, got {getattr(a, 'shape', None)} {getattr(a, 'dtype', type(a).__name__)}")
        return a.reshape(-1, 4).astype(np.int32)

    def __call__(self, index):
        parts = []
        for cls, _, folder in self.folders:
            a = self._load(os.path.join(folder, "%05d" % (index + 1)))
            parts.append(np.concatenate([a, np.full((len(a), 1), cls, np.int32)], axis=1))
        a = np.concatenate(parts)
        if len(a) > MAX_BOXES:
            raise ValueError(f"{self.root}: frame {index + 1}: too many boxes: {len(a)} (at most {MAX_BOXES} per picture)")
        return FrameBoxes(a)


class RawPlanarReader(_Indexed):
    """Headerless 8-bit planar pictures, 3 H W bytes per frame: `ffmpeg -f rawvideo -pix_fmt gbrp` with order "gbr"."""

    def __init__(self, path, width, height):
        self.path, self.width, self.height = path, int(width), int(height)
        if not (0 < self.height <= MAX_SIDE and 0 < self.width <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        self.frame_bytes = 3 * self.height * self.width
        size = os.path.getsize(path)
        if size % self.frame_bytes:
            raise ValueError(f"{path}: truncated last frame ({size} bytes is not a multiple of {self.frame_bytes} for {width}x{height})")
        self.n_frames = size // self.frame_bytes
        self.fd = os.open(path, os.O_RDONLY)

    def read_into(self, index, buf):
        if not 0 <= index < self.n_frames:
            raise IndexError(f"frame {index} of {self.n_frames}")
        if memoryview(buf).nbytes != self.frame_bytes:
            raise ValueError(f"buffer of {memoryview(buf).nbytes} bytes for a frame of {self.frame_bytes}")
        _readinto(self.fd, buf, index * self.frame_bytes, self.path)


class RawPlanarWriter(_Indexed):
    """Frames are placed by index (positional writes): pictures that finish out of order land in display order."""

    def __init__(self, path, width, height):
        self.path, self.width, self.height = path, int(width), int(height)
        if not (0 < self.height <= MAX_SIDE and 0 < self.width <= MAX_SIDE):
            raise ValueError(f"picture sides must be within 1..{MAX_SIDE}, got {width}x{height}")
        self.frame_bytes = 3 * self.height * self.width
        self.n_frames = 0
        self.fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)

    def write(self, index, buf):
        if memoryview(buf).nbytes != self.frame_bytes:
            raise ValueError(f"buffer of {memoryview(buf).nbytes} bytes for a frame of {self.frame_bytes}")
        _writefrom(self.fd, buf, index * self.frame_bytes)
        self.n_frames = max(self.n_frames, index + 1)
