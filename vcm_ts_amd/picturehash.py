"""Decoded-picture hashes: the CRC-32 of a reconstruction, taken on the device (include/dcvc_hip_hash.h, csrc/hash.hip).

The codec is only right while the decoder rebuilds, bit for bit, the reference pictures the encoder predicted from.
`encode --picture-hash` records two digests per coded picture in a `hashes.json` beside the `.bin` files and `decode`
holds its own pictures against them:

    pixels  the CRC-32 (zlib's) of the 8-bit R, G, B codes of the unpadded picture, interleaved per pixel, row-major --
            the bytes of the PNG run_codec writes: zlib.crc32(PIL.Image.open(png).convert("RGB").tobytes()).
            What a viewer sees.
    state   the CRC-32 of the fp32 bit patterns of the whole padded ref_frame as the decoded-picture buffer holds it.
            What the next picture is predicted from: it catches drift before it is visible.

The kernels run on the caller's current stream and synchronise nothing; the digests of a GOP leave the device in one
asynchronous copy behind its last picture.  There is no torch fallback: a CPU tensor is a ValueError.
"""
from __future__ import annotations

import os
import re
import warnings
import zlib

from . import devargs, lib
from .devargs import MAX_SIDE
from .stream import read_sidecar, write_sidecar

HASHES_JSON = "hashes.json"
VERSION, ALGORITHM = 1, "crc32"
MODES = ("strict", "pixels", "warn", "off")
_DIGEST = re.compile(r"^[0-9a-f]{8}$")


# ------------------------------------------------------------------------------------------------------- the kernels
def new_scratch(device):
    """The scratch of one stream's hash launches (DCVC_HASH_SCRATCH_BYTES; calls on one stream may share it)."""
    import torch

    return torch.empty(lib.hash_constant("dcvc_hash_scratch_bytes") // 4, dtype=torch.int32, device=device)


def _slot(out, device, what):
    import torch

    if out is None:
        return torch.empty(1, dtype=torch.uint32, device=device)
    if not torch.is_tensor(out) or out.device != device or out.dtype != torch.uint32 or out.numel() != 1:
        raise ValueError(f"{what}: out= must be one uint32 element on {device}")
    return out


def _launch(name, t, args, out, scratch, what):
    """`t`: the checked tensor, read in place where devargs.planar allows; args: what follows its strides."""
    dev = t.device
    out = _slot(out, dev, what)
    x, rs, ps = devargs.planar(t)
    if scratch is None:
        scratch = new_scratch(dev)  # (the caching allocator hands it back to this stream only)
    devargs.launch(name, dev, x.data_ptr(), rs, ps, *args, out.data_ptr(), scratch.data_ptr(), what=what)
    return out


def crc32_pixels(picture, size=None, out=None, scratch=None):
    """The `pixels` digest of the size = (height, width) crop (default: all) of a (1, 3, H, W) float32 picture on the
    GPU, read in place: a 1-element uint32 device tensor (`out`, when given: one uint32 element, written).  Enqueued on
    the current stream; nothing is synchronised."""
    crop = devargs.checked(picture, "crc32_pixels", at_least=size)
    return _launch("dcvc_hash_pixels", crop, crop.shape[2:], out, scratch, "crc32_pixels")


def crc32_f32(tensor, out=None, scratch=None):
    """The `state` digest: CRC-32 of tensor.contiguous().cpu().numpy().tobytes() for a float32 (1, C, H, W) or (C, H, W)
    tensor on the GPU, a view read in place.  Returns as crc32_pixels does."""
    import torch

    what = "crc32_f32"
    devargs.on_gpu(tensor, what, noun="tensor")
    t = tensor.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != 1 or t.numel() == 0 or max(t.shape) > MAX_SIDE or \
            4 * t.numel() >= 1 << 32:
        raise ValueError(f"{what}: expected a non-empty float32 (1, C, H, W) or (C, H, W) tensor with sides within "
                         f"1..{MAX_SIDE} and less than 4 GiB, got {tuple(tensor.shape)} {tensor.dtype}")
    return _launch("dcvc_hash_f32", t, t.shape[1:], out, scratch, what)


# ---------------------------------------------------------------------------------------------------------- the log
class HashLog:
    """The digest pair of every coded picture of one GOP stream.  Both launches of a picture are enqueued on the stream
    that coded it, into that GOP's (pictures, 2) uint32 device tensor; the pairs of a GOP go to pinned host memory in ONE
    asynchronous copy behind its last picture and are looked at later: the host never waits for a picture."""

    def __init__(self, plan):
        from .goplog import GopLog

        self.plan, self.buf, self.log, self.scratch = plan, None, GopLog(), None

    def add(self, g, ref_frame, size, display=None):
        """Picture g: `pixels` of the size = (height, width) crop of ref_frame, `state` of all of it.  display (with a
        base scale): the picture a viewer sees, whose crop `pixels` is taken from instead."""
        import torch

        if self.scratch is None:
            self.scratch = new_scratch(ref_frame.device)
        if not self.log.keys:
            n = len(self.plan.gop_range(self.plan.gop_of(g)))
            self.buf = torch.empty((n, 2), dtype=torch.uint32, device=ref_frame.device)
        i = len(self.log.keys)
        if i >= self.buf.shape[0]:
            raise ValueError(f"HashLog: picture {g} does not belong to the GOP of picture {self.log.keys[0]}")
        crc32_pixels(ref_frame if display is None else display, size, out=self.buf[i, 0:1], scratch=self.scratch)
        crc32_f32(ref_frame, out=self.buf[i, 1:2], scratch=self.scratch)
        self.log.add(g)
        if self.plan.is_gop_end(g):
            self.flush()

    def flush(self):
        if self.log.keys:
            self.log.flush(self.buf[:len(self.log.keys)])

    def poll(self, wait=False):
        """[(frame number, pixels, state)] of the GOPs whose copies have completed since the last call, in coding order;
        wait=True waits for every flushed GOP."""
        out = []
        for keys, (host,) in self.log.poll(wait):
            rows = host.numpy()
            out.extend((g, int(rows[n, 0]), int(rows[n, 1])) for n, g in enumerate(keys))
        return out

    def collect(self):
        """{frame number: (pixels, state)} of everything flushed and not polled yet (waits for the copies)."""
        return {g: (p, s) for g, p, s in self.poll(wait=True)}


# ------------------------------------------------------------------------------------------------------ hashes.json
def _hex(v):
    return "%08x" % (int(v) & 0xFFFFFFFF)


def remove_hashes(bin_dir):
    """A stale file of an earlier encode into the same folder must not describe these .bin files."""
    write_sidecar(bin_dir, HASHES_JSON, None)


def write_hashes(bin_dir, digests, height, width, padded, precision):
    """hashes.json beside the .bin files.  digests: {frame number: (pixels, state)} for the frames 0 .. N - 1."""
    n = len(digests)
    if sorted(digests) != list(range(n)):
        raise ValueError(f"write_hashes: digests of the frames {sorted(digests)}, not of 0..{n - 1}")
    info = {"version": VERSION, "algorithm": ALGORITHM, "frames": n, "height": int(height), "width": int(width),
            "padded": [int(padded[0]), int(padded[1])], "precision": str(precision),
            "pixels": [_hex(digests[g][0]) for g in range(n)], "state": [_hex(digests[g][1]) for g in range(n)]}
    return write_sidecar(bin_dir, HASHES_JSON, info)


def parse_hashes(info, where=HASHES_JSON):
    """The record as a dictionary with "pixels" and "state" as lists of integers.  Refused by name: an unknown version
    or algorithm, lists whose lengths are not `frames`, a malformed digest, missing or mistyped fields."""
    if not isinstance(info, dict):
        raise ValueError(f"{where}: expected a JSON object")
    if info.get("version") != VERSION:
        raise ValueError(f"{where}: unknown version {info.get('version')!r} (this build reads version {VERSION})")
    if info.get("algorithm") != ALGORITHM:
        raise ValueError(f"{where}: unknown algorithm {info.get('algorithm')!r} (this build knows {ALGORITHM!r})")
    out = {"version": VERSION, "algorithm": ALGORITHM}
    for key in ("frames", "height", "width"):
        v = info.get(key)
        if not isinstance(v, int) or isinstance(v, bool) or v < (0 if key == "frames" else 1):
            raise ValueError(f"{where}: {key} must be a {'non-negative' if key == 'frames' else 'positive'} integer, got {v!r}")
        out[key] = v
    pad = info.get("padded")
    if not (isinstance(pad, list) and len(pad) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in pad) and
            pad[0] >= out["height"] and pad[1] >= out["width"]):
        raise ValueError(f"{where}: padded must be [Hp, Wp] with Hp >= height and Wp >= width, got {pad!r}")
    out["padded"] = (pad[0], pad[1])
    if not isinstance(info.get("precision"), str):
        raise ValueError(f"{where}: precision must be a string, got {info.get('precision')!r}")
    out["precision"] = info["precision"]
    for key in ("pixels", "state"):
        v = info.get(key)
        if not isinstance(v, list) or len(v) != out["frames"]:
            raise ValueError(f"{where}: {key} holds {len(v) if isinstance(v, list) else 'no list of'} digests for "
                             f"{out['frames']} frames")
        for t, d in enumerate(v):
            if not isinstance(d, str) or not _DIGEST.match(d):
                raise ValueError(f"{where}: {key}[{t}] is not a digest of 8 lower-case hex digits: {d!r}")
        out[key] = [int(d, 16) for d in v]
    return out


def read_hashes(bin_dir):
    """parse_hashes of the folder's hashes.json, or None without the file."""
    found = read_sidecar(bin_dir, HASHES_JSON)
    return None if found is None else parse_hashes(found[1], found[0])


# ------------------------------------------------------------------------------------------------------ verification
class PictureHashMismatch(Exception):
    """A decoded picture is not the picture the encoder reconstructed.

    picture: 0-based; name: its .bin file; which: "pixels" or "state"; expected: hashes.json's digest; actual: this
    decoder's; kind: "I" or "P"; gop_start: the I picture its GOP began with; recorded_precision / decoding_precision."""

    def __init__(self, picture, which, expected, actual, kind, gop_start, recorded_precision=None, decoding_precision=None):
        self.picture, self.name, self.which = int(picture), "im%05d.bin" % (picture + 1), which
        self.expected, self.actual, self.kind, self.gop_start = int(expected), int(actual), kind, int(gop_start)
        self.recorded_precision, self.decoding_precision = recorded_precision, decoding_precision
        super().__init__(describe(self))


def describe(m):
    text = (f"picture {m.picture} ({m.name}, {'an I' if m.kind == 'I' else 'a P'} picture of the GOP that began at picture "
            f"{m.gop_start}): the {m.which} digest is {_hex(m.actual)}, {HASHES_JSON} says {_hex(m.expected)}")
    if m.recorded_precision != m.decoding_precision and m.recorded_precision and m.decoding_precision:
        text += f"; the pictures were coded with precision {m.recorded_precision} and are decoded with {m.decoding_precision}"
    return text


def verify_mode(verify, record, bin_dir):
    """The mode a decode loop runs in: `verify` (None: "pixels" when the folder holds a record, else "off").  Refused by
    name: an unknown mode, and a mode other than "off" without a record."""
    if verify is not None and verify not in MODES:
        raise ValueError(f"verify: expected one of {list(MODES)}, got {verify!r}")
    if record is None:
        if verify not in (None, "off"):
            raise ValueError(f"verify={verify!r}: there is no {HASHES_JSON} in {bin_dir} (encode with picture_hash=True, "
                             f"--picture-hash)")
        return "off"
    return verify or "pixels"


def check_record(record, plan, height, width, padded, where=HASHES_JSON):
    """Refused by name, before any launch: a record of another frame count, picture size or padded size."""
    if record["frames"] != plan.n_frames:
        raise ValueError(f"{where}: digests of {record['frames']} frames beside {plan.n_frames} .bin files")
    if (record["height"], record["width"]) != (int(height), int(width)):
        raise ValueError(f"{where}: digests of {record['width']}x{record['height']} pictures, decoding {width}x{height}")
    if tuple(record["padded"]) != tuple(padded):
        raise ValueError(f"{where}: digests of pictures padded to {tuple(record['padded'])}, this decoder pads to {tuple(padded)}")


class Verifier:
    """A decode loop's check: add(t, ref_frame) enqueues the two launches of picture t and compares every GOP whose
    digests have arrived meanwhile; finish() compares the rest.  Mode "pixels": PictureHashMismatch at the first picture
    whose `pixels` digest differs, one warning at the first whose `state` alone differs; "strict": raises on either;
    "warn": warns once, never raises.  (Mode "off" builds no Verifier.)  check_pixels=False (a base-only decode of a
    scaled sequence, which never builds the picture `pixels` is of): only `state` is compared."""

    def __init__(self, record, mode, plan, size, decoding_precision, check_pixels=True):
        assert mode in MODES and mode != "off"
        self.record, self.mode, self.plan, self.size, self.precision = record, mode, plan, size, decoding_precision
        self.log, self.warned, self.check_pixels = HashLog(plan), False, check_pixels

    def add(self, t, ref_frame, display=None):
        """display (with a base scale): the up-scaled picture `pixels` is of; self.size is then its size."""
        if display is None:
            self.log.add(t, ref_frame, self.size)
        else:
            self.log.add(t, ref_frame, self.size, display=display)
        self._compare(self.log.poll())

    def finish(self):
        self.log.flush()
        self._compare(self.log.poll(wait=True))

    def _compare(self, rows):
        for t, pixels, state in rows:
            for which, got in (("pixels", pixels), ("state", state)):
                want = self.record[which][t]
                if got == want or (which == "pixels" and not self.check_pixels):
                    continue
                m = PictureHashMismatch(t, which, want, got, "I" if self.plan.is_intra(t) else "P",
                                        self.plan.i_pictures[self.plan.gop_of(t)], self.record["precision"], self.precision)
                if self.mode == "strict" or (self.mode == "pixels" and which == "pixels"):
                    raise m
                if not self.warned:
                    self.warned = True
                    note = " (drift has begun, not yet visible)" if which == "state" else ""
                    warnings.warn(f"{m}{note}", stacklevel=2)
                break  # (one finding per picture)


def verify_pngs(bin_dir, recon_dir):
    """Host only: zlib.crc32 of the RGB bytes of every im%05d.png of `recon_dir` against the `pixels` digests of
    bin_dir's hashes.json.  Returns None when all agree, else (0-based picture, file name, expected, actual) of the first
    that differs.  For unfused base-layer PNG folders only.  Refused by name: no record, a missing PNG, another size."""
    from PIL import Image

    record = read_hashes(bin_dir)
    if record is None:
        raise ValueError(f"there is no {HASHES_JSON} in {bin_dir} (encode with --picture-hash)")
    for t, want in enumerate(record["pixels"]):
        name = "im%05d.png" % (t + 1)
        path = os.path.join(recon_dir, name)
        if not os.path.exists(path):
            raise ValueError(f"{path}: missing ({HASHES_JSON} lists {record['frames']} pictures)")
        with Image.open(path) as im:
            if im.size != (record["width"], record["height"]):
                raise ValueError(f"{path}: a {im.size[0]}x{im.size[1]} picture, {HASHES_JSON} is of {record['width']}x{record['height']}")
            got = zlib.crc32(im.convert("RGB").tobytes()) & 0xFFFFFFFF
        if got != want:
            return t, name, want, got
    return None
