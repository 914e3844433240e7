"""The GPU tests' scaffolding, written once: the bytes of a folder, PNG clips, device buffers laid out to catch a kernel
that reads or writes beside its picture, and the codecs the file loops share.  Plain functions that take the device where
they allocate (tests/test_gpu_util_host.py runs them on CPU tensors); the fixtures at the end are imported by name into
the modules that use them."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from tests.pixel_ref import code
from vcm_ts_amd.pipeline import intra_dpb  # noqa: F401 (the DPB an I picture leaves behind; the tests take it from here)

F32 = np.float32
GUARD = 64  # words around every guarded or strided buffer


# -------------------------------------------------------------------------------------------------------------- files
def bins(folder):
    """{name: bytes} of the folder's .bin files."""
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder)) if n.endswith(".bin")}


def others(folder):
    """The names of everything in the folder that is no .bin file."""
    return sorted(n for n in os.listdir(folder) if not n.endswith(".bin"))


def png(path, planar=False):
    """The picture as uint8 (H, W, 3), or (3, H, W) when planar."""
    from PIL import Image

    a = np.asarray(Image.open(path).convert("RGB"))
    return a.transpose(2, 0, 1) if planar else a


def write_pngs(folder, pictures):
    """im00001.png ... in a new folder, of uint8 (H, W, 3) pictures or of float (3, H, W) pictures of exact 8-bit samples."""
    from PIL import Image

    os.makedirs(folder)
    for t, a in enumerate(pictures):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            u8 = code(a).astype(np.uint8)
            assert np.array_equal(f32_bits(u8.astype(F32) / F32(255.0)), f32_bits(a)), t  # exactly 8-bit representable
            a = u8.transpose(1, 2, 0)
        Image.fromarray(a).save(os.path.join(folder, f"im{t + 1:05d}.png"))


def same_pngs(a, b, n):
    """im00001.png ... im<n>.png of the two folders are the same files, byte for byte."""
    for t in range(n):
        name = f"im{t + 1:05d}.png"
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), t


# ------------------------------------------------------------------------------------------------------------- device
def stream(device):
    """The device's current stream as the void * the entry points take."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def to_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def f32_bits(x):
    """The bit patterns of float32 values, a tensor's or an array's, as uint32."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def picture(a, crop, device):
    """(1, 3, H, W) on the device; crop: a view at a one-pixel offset inside a 64 x 192 buffer (rows unaligned, strides
    beyond the width, foreign values around it)."""
    t = to_dev(a, device)[None]
    if not crop:
        return t
    H, W = a.shape[1:]
    big = torch.full((1, 3, 64, 192), 0.77, device=device)
    big[..., 1:1 + H, 1:1 + W] = t
    return big[..., 1:1 + H, 1:1 + W]


def strided(pic, H, W, row_pad, plane_pad, offset, device, guard=GUARD):
    """A (3, H, W) float32 view with row stride W + row_pad and plane stride H * rs + plane_pad, `offset` elements into a
    buffer of NaN that goes on `guard` elements past the last plane, holding `pic` when one is given: (the buffer, the
    view, row stride, plane stride, the buffer's mask of the view's words)."""
    rs = W + row_pad
    ps = H * rs + plane_pad
    buf = torch.full((offset + 3 * ps + guard,), float("nan"), device=device)
    view = buf.as_strided((3, H, W), (ps, rs, 1), offset)
    if pic is not None:
        view.copy_(torch.from_numpy(np.array(pic)))
    mask = np.zeros(buf.numel(), dtype=bool)
    mask[offset + np.add.outer(np.add.outer(ps * np.arange(3), rs * np.arange(H)), np.arange(W))] = True
    return buf, view, rs, ps, mask


def guarded(n, shift, dtype, sentinel, device, guard=GUARD):
    """n words of `sentinel` with guard + shift words of it before and guard after; dtype is the unsigned numpy type of
    the words, the tensor is of the signed type of the same width: (the buffer, the first word's index)."""
    a = np.full(2 * guard + shift + n, sentinel, dtype=dtype)
    return torch.from_numpy(a.view(f"i{a.itemsize}")).to(device), guard + shift


def words(buf):
    """The buffer's words as unsigned integers of their width, in int64."""
    a = buf.cpu().numpy()
    return a.view(f"u{a.itemsize}").astype(np.int64)


def guards_intact(buf, first, n, sentinel):
    """Every word before `first` and from `first + n` on still holds the sentinel."""
    w = words(buf)
    return bool((w[:first] == sentinel).all() and (w[first + n:] == sentinel).all())


# ----------------------------------------------------------------------------------------------------------- codecs
DEV = torch.device("cuda:0")  # (the fixtures' device; nothing above uses it)


def seeded_pair(device, precision=None):
    """(DMC, IntraNoAR) with their name-seeded weights, tables built."""
    from vcm_ts_amd.dmc import DMC
    from vcm_ts_amd.intra import IntraNoAR

    d, i = DMC(precision=precision).to(device).eval(), IntraNoAR(precision=precision).to(device).eval()
    d.update()
    i.update()
    return d, i


@pytest.fixture(scope="module")
def seeded_nets():
    return seeded_pair(DEV)


@pytest.fixture(scope="module")
def file_nets():
    """The two codecs of a file loop with two GOP streams."""
    from vcm_ts_amd import run_codec as RC

    return [RC._nets(DEV, None) for _ in range(2)]


@pytest.fixture
def no_garbage_left_behind():
    """The file loops keep pinned buffers and events, and whatever of them ends up in a reference cycle is collected here,
    at a known point between tests with the device idle, instead of whenever the collector next runs in a later test --
    inside a graph capture, for instance.  A module that wants it for every test names it in its pytestmark."""
    yield
    torch.cuda.synchronize(DEV)
    gc.collect()
