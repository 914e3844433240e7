"""The device boundary of the picture tools (metrics, yuv, roi, roilayer, bitmap, scenecut, picturehash, scale, aq, motionroi,
tnr, redact, ratectl, deint, noise, shake), written once: what a module checks about a picture before it hands its pointer and strides to a
kernel, how it names its device, and how it launches.  A new picture tool takes its checks and its launches from here.

    MAX_SIDE                          the largest picture side any kernel takes
    whole(name, v, lo, hi, unit)      an integer setting;  hundredths(value, name)  a factor snapped to hundredths
    cuda_device(device, who)          torch.device("cuda", index) or a ValueError
    on_gpu / checked / planar         the refusals of a picture, and its (tensor, row stride, plane stride)
    picture(t, what, ...)             the three in one call
    stream(device), launch(name, device, *args)

Every refusal is a ValueError raised before any GPU work; there is no torch fallback behind any of them.  torch is
imported inside the functions, as the feature modules do.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import lib

MAX_SIDE = 32768


# ------------------------------------------------------------------------------------------------------------ settings
def whole(name, v, lo, hi, unit=None):
    """`v` as an int: an integer (numpy's too, never a bool) within lo..hi."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer within {lo}..{hi}{f' ({unit})' if unit else ''}, got {v!r}")
    return int(v)


def hundredths(value, name="value"):
    """A plain number snapped to hundredths (the command line's --plate-q 0.6 -> 60)."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value):
        raise ValueError(f"{name} must be a finite number, got {value!r}")
    return int(round(float(value) * 100.0))


# -------------------------------------------------------------------------------------------------------------- device
def cuda_device(device, who):
    """`device` as torch.device("cuda", index), the current device's index where it names none."""
    import torch

    try:
        dev = torch.device(device)
    except (RuntimeError, TypeError):
        dev = None
    if dev is None or dev.type != "cuda":
        raise ValueError(f"{who}: runs on the GPU only (no CPU fallback exists), got the device {device!r}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def stream(device):
    """The current stream of `device`, as a kernel entry point takes it."""
    from .engine import _raw_stream

    return C.c_void_p(_raw_stream(device.index))


def launch(name, device, *args, what=None):
    """lib.hip().`name`(*args, stream) on the current stream of `device`; a status other than 0 is a lib.KernelError."""
    import torch

    with torch.cuda.device(device):
        lib.check(getattr(lib.hip(), name)(*args, stream(device)), what or name[len("dcvc_"):])


# ------------------------------------------------------------------------------------------------------------ pictures
def planar(t):
    """(tensor, row stride, plane stride): `t` itself when it is dense planar rows inside a contiguous NCHW buffer (a
    spatial crop), else a contiguous copy."""
    N, C_, H, W = t.shape
    sn, sc, sh, sw = t.stride()
    if C_ == 1:  # (the stride of a size-1 dimension means nothing: planes are then one sample apart)
        sc = sn if N > 1 else H * sh
    if not (sw == 1 and sh >= W and sc >= (H - 1) * sh + W and (N == 1 or sn == C_ * sc)):
        t = t.contiguous()
        sh, sc = W, H * W
    return t, sh, sc


def on_gpu(t, what, device=None, noun="picture", owner="tables"):
    """The first two refusals of every tensor argument: not a tensor on the GPU; not on `device` (its `owner`'s)."""
    import torch

    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: the {noun} lives on the GPU (no CPU fallback exists)")
    if device is not None and t.device != device:
        raise ValueError(f"{what}: the {noun} is on {t.device}, the {owner} on {device}")


def checked(t, what, *, device=None, like=None, exact=None, at_least=None, noun="picture", owner="tables"):
    """The (1, 3, H, W) float32 picture `t` a kernel may read, detached -- its top-left `at_least` = (h, w) crop when one
    is asked for -- after the refusals, in this order: on_gpu's two; a wrong dtype, rank, leading (1, 3) or size (`exact`
    = (H, W); `at_least`; `like`: another picture's shape and device); sides beyond MAX_SIDE.  No GPU work."""
    import torch

    on_gpu(t, what, device, noun, owner)
    ok = t.dtype == torch.float32 and t.dim() == 4 and tuple(t.shape[:2]) == (1, 3) and t.numel() > 0
    H, W = (int(s) for s in at_least) if at_least is not None else t.shape[2:] if ok else (0, 0)
    if ok and exact is not None:
        ok = (H, W) == tuple(exact)
    if ok and at_least is not None:
        ok = 0 < H <= t.shape[2] and 0 < W <= t.shape[3]
    if not ok:
        want = "(1, 3, H, W)" if exact is None else f"(1, 3, {exact[0]}, {exact[1]})"
        crop = "" if at_least is None else f" with a ({H}, {W}) crop"
        raise ValueError(f"{what}: expected a {want} float32 {noun}{crop}, got {tuple(t.shape)} {t.dtype}")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{what}: {tuple(t.shape)} on {t.device} does not match {tuple(like.shape)} on {like.device}")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: picture sides must be within 1..{MAX_SIDE}, got {W}x{H}")
    return t.detach() if at_least is None else t.detach()[..., :H, :W]


def picture(t, what, **kw):
    """(tensor, row stride, plane stride) of the picture `t`, or of its `at_least` crop, read in place where planar()
    allows: planar(checked(t, what, **kw))."""
    return planar(checked(t, what, **kw))
