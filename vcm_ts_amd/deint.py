"""A motion-adaptive deinterlacer for interlaced 4:2:0 sources (include/dcvc_hip_deint.h, csrc/deint.hip): the fields of
a file's frames become progressive pictures on the device, on the file's own sample planes, IN FRONT OF the unchanged
colour conversion (yuv.yuv420_to_rgb).  Where the scene is static the two fields are woven and a static progressive
picture comes back bit for bit; where something moves the missing rows are interpolated inside the field, clamped to what
the neighbouring fields allow.  It is ENCODER SIDE ONLY: no side file, no change of the .bin format, nothing for the
decoder to know.  The arithmetic is stated in the header; tests/deint_ref.py restates it in numpy.

    Deinterlace(mode, order)        the setting: mode "frame" (one picture per frame, the earlier field kept) or "field"
                                    (two pictures per frame, in field order); order "tff" or "bff"
    .pictures_of(n_frames)          the number of output pictures
    .needs(g, n_frames)             ((n - 1, n, n + 1), second): the file frames output picture g is made from -- a frame
                                    outside the FILE replaced by n -- and which field of frame n it is
    .parity(second)                 the row parity that field owns
    .step(prev, cur, nxt, height, width, bit_depth, second)
                                    ONE launch: (the progressive I420 device buffer, the `moved` tensor)

Output picture g is a pure function of the file and g.  What is NOT done: the quarter-line vertical offset of interlaced
4:2:0 chroma is not corrected (each chroma plane is treated as two co-sited fields), there is no inverse telecine and no
motion compensation, the first and the last frame of a file have one temporal neighbour replaced by themselves, and
nothing is tuned -- no real interlaced video was seen.

The kernel runs on the caller's current stream and synchronises nothing.  There is no torch fallback: a CPU tensor is a
ValueError.
"""
from __future__ import annotations

from dataclasses import dataclass

from . import devargs

MODES, ORDERS = ("frame", "field"), ("tff", "bff")
BAND = 8  # (DCVC_DEINT_BAND: luma rows per word of `moved`)


def check_height(height):
    if height % 4:
        raise ValueError(f"deinterlacing 4:2:0 needs a height that is a multiple of 4 (each chroma field a whole number of rows), got {height}")


@dataclass(frozen=True)
class Deinterlace:
    mode: str
    order: str

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"deinterlace mode must be one of {list(MODES)}, got {self.mode!r}")
        if self.order not in ORDERS:
            raise ValueError(f"field order must be one of {list(ORDERS)}, got {self.order!r}")

    @property
    def per_frame(self):
        return 1 if self.mode == "frame" else 2

    def pictures_of(self, n_frames):
        return int(n_frames) * self.per_frame

    def needs(self, g, n_frames):
        n, second = divmod(int(g), self.per_frame)
        if not 0 <= n < n_frames:
            raise IndexError(f"picture {g} of {self.pictures_of(n_frames)}")
        return (n - 1 if n > 0 else n, n, n + 1 if n + 1 < n_frames else n), second

    def parity(self, second):
        return second if self.order == "tff" else 1 - second

    def to_json(self):
        return {"mode": self.mode, "order": self.order}

    def step(self, prev, cur, nxt, height, width, bit_depth, second):
        """prev, cur, nxt: contiguous I420 device buffers of one size and depth (uint8, or int16 at 10 bits); prev or nxt
        may be cur itself.  -> (the I420 buffer of the progressive picture, moved: int32 words, one per band of 8 luma
        rows, the missing luma samples that were not simply woven)."""
        import torch

        from .yuv import check_size, frame_samples, split_planes

        check_size(height, width)
        check_height(height)
        if bit_depth not in (8, 10) or second not in (0, 1):
            raise ValueError(f"Deinterlace.step: bit_depth 8 or 10 and second 0 or 1, got {bit_depth!r} and {second!r}")
        dtype = torch.uint8 if bit_depth == 8 else torch.int16
        for t in (prev, cur, nxt):
            devargs.on_gpu(t, "Deinterlace.step", cur.device if torch.is_tensor(cur) else None, noun="I420 buffer", owner="current frame")
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != frame_samples(height, width):
                raise ValueError(f"Deinterlace.step: expected contiguous I420 buffers of {frame_samples(height, width)} {dtype} samples, "
                                 f"got {tuple(t.shape)} {t.dtype}")
        out = torch.empty(frame_samples(height, width), dtype=dtype, device=cur.device)
        moved = torch.empty(-(-height // BAND), dtype=torch.int32, device=cur.device)
        args = []
        for t in (prev, cur, nxt):
            args += [p.data_ptr() for p in split_planes(t, height, width)] + [width, width // 2]
        devargs.launch("dcvc_deinterlace420", cur.device, *args, height, width, bit_depth, self.parity(second), second,
                       *(p.data_ptr() for p in split_planes(out, height, width)), width, width // 2, moved.data_ptr(), moved.numel())
        return out, moved
