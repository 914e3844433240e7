"""Per-cell bit maps (include/dcvc_hip_bits.h): where inside a picture the bits were spent.

After ``compress()`` the six symbol planes, their CDF-index planes and the integer CDF tables are on the device: exactly
what the rANS coder turns into bytes.  The code length of a symbol is a function of those integers alone, so the maps made
here are not an estimate -- their sum agrees with the length of the host coder's byte string inside a bound that follows
from the rANS update rule.

    CostTables   the per-table integer cost arrays, built on the host from CodecBase._tables (the only place a logarithm
                 is evaluated), uploaded on first use
    BitMap       the int32 device maps of one picture (mv_z, mv_y, z, y); .cells(), .totals(), .regions(labels, K)
    labels_from_boxes   the 0 / 1 label map of a picture's ROI boxes on the 16-pixel cell grid

Units: a map entry is in 2^-16 bit (UNIT per bit); region sums are in 2^-20 bit (REGION_UNIT per bit), so that a z-type
element splits evenly over the 4 x 4 cells it covers.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import devargs

UNIT = 65536            # map units per bit
REGION_UNIT = 16 * UNIT  # region-sum units per bit
MAX_C = 512
MAX_LABELS = 8
BAD_INDEX, BAD_LABEL = 1, 2
COMPONENTS = ("mv_z", "mv_y", "z", "y")

_LUT = None


class BitMapError(RuntimeError):
    pass


def cost_lut():
    """(65537,) int32: LUT[f] = rint((16 - log2(f)) * 65536) for f in 1..65536, in float64; LUT[0] is unused (0)."""
    global _LUT
    if _LUT is None:
        lut = np.zeros(65537, dtype=np.int32)
        for f in range(1, 65537):
            lut[f] = int(round((16.0 - math.log2(f)) * 65536.0))  # (round() of a float is half-to-even, as rint)
        _LUT = lut
    return _LUT


def cost_array(cdf, sizes, offsets, name="table"):
    """The int32 cost array of one CDF table (same rows and stride): cost[r][s] = LUT[cdf[r][s+1] - cdf[r][s]] for
    0 <= s <= sizes[r] - 2, 0 elsewhere.  Refused by name: a row size outside 2..stride, a frequency of 0 or above 65536
    (neither can come from a valid table), more than 65536 rows, mismatched lengths."""
    cdf = np.asarray(cdf)
    sizes, offsets = np.asarray(sizes), np.asarray(offsets)
    if cdf.ndim != 2 or cdf.shape[1] < 2 or cdf.dtype.kind not in "iu":
        raise ValueError(f"{name}: expected a (rows, stride >= 2) integer CDF array, got {cdf.shape} {cdf.dtype}")
    rows, stride = cdf.shape
    if not 1 <= rows <= 65536:
        raise ValueError(f"{name}: {rows} rows (1..65536)")
    if sizes.shape != (rows,) or offsets.shape != (rows,) or sizes.dtype.kind not in "iu" or offsets.dtype.kind not in "iu":
        raise ValueError(f"{name}: sizes and offsets must be integer arrays of {rows} entries")
    bad = np.flatnonzero((sizes < 2) | (sizes > stride))
    if bad.size:
        raise ValueError(f"{name}: row {int(bad[0])} has size {int(sizes[bad[0]])} (2..{stride})")
    freq = np.diff(cdf.astype(np.int64), axis=1)                       # (rows, stride - 1)
    used = np.arange(stride - 1)[None, :] < (sizes.astype(np.int64) - 1)[:, None]
    wrong = used & ((freq < 1) | (freq > 65536))
    if wrong.any():
        r, s = (int(v[0]) for v in np.nonzero(wrong))
        raise ValueError(f"{name}: row {r} slot {s} has frequency {int(freq[r, s])} (1..65536)")
    cost = np.zeros((rows, stride), dtype=np.int32)
    cost[:, : stride - 1] = np.where(used, cost_lut()[np.where(used, freq, 0)], 0)
    return cost


class CostTables:
    """The cost arrays of a codec's tables ({name: (cdf, sizes, offsets)}, CodecBase._tables).  Built (and validated) on
    the host when constructed; on(device) uploads them once per device."""

    def __init__(self, tables):
        self.host = {}
        for name, (cdf, sizes, offsets) in tables.items():
            self.host[name] = (cost_array(cdf, sizes, offsets, name), np.ascontiguousarray(sizes, np.int32),
                               np.ascontiguousarray(offsets, np.int32))
        self._dev = {}

    def on(self, device):
        """{name: (cost, sizes, offsets, rows, stride)} as int32 device tensors."""
        import torch

        device = torch.device(device)
        d = self._dev.get(device)
        if d is None:
            d = {name: (torch.from_numpy(c).to(device), torch.from_numpy(s).to(device), torch.from_numpy(o).to(device),
                        c.shape[0], c.shape[1]) for name, (c, s, o) in self.host.items()}
            self._dev[device] = d
        return d


def _check_labels(labels, K, N, hc, wc):
    """Argument checks of BitMap.regions that need no GPU; returns the (n, hc, wc) shape labels have (n is 1 or N)."""
    devargs.whole("K: the number of labels", K, 1, MAX_LABELS)
    shape = tuple(getattr(labels, "shape", ()))
    dtype = str(getattr(labels, "dtype", type(labels).__name__)).replace("torch.", "")
    if dtype != "uint8":
        raise ValueError(f"labels: expected uint8 labels, got {dtype}")
    if shape not in ((hc, wc), (1, hc, wc), (N, hc, wc)):
        raise ValueError(f"labels: expected shape ({hc}, {wc}), (1, {hc}, {wc}) or ({N}, {hc}, {wc}) -- the 16-pixel cell "
                         f"grid of the padded picture -- got {shape}")
    return (1,) + shape if len(shape) == 2 else shape


class BitMap:
    """The maps of one coded picture (or of a batch of N rate points): int32 device tensors in 2^-16 bit, "mv_y" and "y"
    of shape (N, hc, wc) on the 16-pixel cell grid of the padded picture, "mv_z" and "z" of shape (N, hc / 4, wc / 4);
    an I picture has no mv maps (None).  The kernels that fill them were enqueued on the stream that coded the picture;
    nothing here waits for them except the methods that return host values."""

    def __init__(self, maps, status, N, hc, wc):
        if hc % 4 or wc % 4 or hc < 4 or wc < 4:
            raise ValueError(f"the cell grid of a padded picture is a multiple of 4 in both directions, got {hc} x {wc}")
        self.maps = {k: maps.get(k) for k in COMPONENTS}
        if all(m is None for m in self.maps.values()):
            raise ValueError("a BitMap needs at least one map")
        for k, m in self.maps.items():
            want = (N, hc, wc) if k in ("mv_y", "y") else (N, hc // 4, wc // 4)
            if m is not None and tuple(m.shape) != want:
                raise ValueError(f"map {k}: expected shape {want}, got {tuple(m.shape)}")
        self.status, self.N, self.hc, self.wc = status, int(N), int(hc), int(wc)

    # -- made from the staged planes of compress() ---------------------------------------------------------------------
    @classmethod
    def from_planes(cls, tables, planes, N):
        """tables: CostTables.on(device).  planes: the picture's planes in bitstream order as PendingStream takes them --
        (table, sym, idx or None, (N, C, H, W) for a factorised plane) -- a factorised plane followed by the two steps of
        the scale-coded latent it is the hyper latent of, once (I picture: z, y) or twice (P picture: mv_z, mv_y, z, y).
        Three launches per latent pair on the current stream, nothing synchronised."""
        import torch

        if len(planes) not in (3, 6):
            raise ValueError(f"expected 3 or 6 symbol planes, got {len(planes)}")
        dev = planes[0][1].device
        names = COMPONENTS[2:] if len(planes) == 3 else COMPONENTS
        status = torch.zeros(2, dtype=torch.int32, device=dev)  # (8 bytes: it travels in one int64 slot of a read-back)
        maps = {}
        for g in range(len(planes) // 3):
            (zt, zsym, _, (zn, zc, zh, zw)), (st, s0, i0, _), (_, s1, i1, _) = planes[3 * g : 3 * g + 3]
            H, W = 4 * zh, 4 * zw
            Cy, rem = divmod(2 * s0.numel(), N * H * W)
            if zn != N or rem or s1.numel() != s0.numel() or i0.numel() != s0.numel() or i1.numel() != s0.numel() or \
                    zsym.numel() != N * zc * zh * zw:
                raise ValueError("symbol planes do not match the latent grids")
            if Cy % 2 or Cy > MAX_C or zc > MAX_C:
                raise ValueError(f"bit maps take an even number of at most {MAX_C} channels, got {Cy} and {zc}")
            cost, sizes, offsets, rows, stride = tables[zt]
            zmap = torch.empty((N, zh, zw), dtype=torch.int32, device=dev)
            devargs.launch("dcvc_bits_map_factorized", dev, zsym.data_ptr(), cost.data_ptr(), rows, stride, sizes.data_ptr(),
                           offsets.data_ptr(), zmap.data_ptr(), N, zc, zh, zw, status.data_ptr())
            cost, sizes, offsets, rows, stride = tables[st]
            ymap = torch.empty((N, H, W), dtype=torch.int32, device=dev)
            devargs.launch("dcvc_bits_map_scale", dev, s0.data_ptr(), i0.data_ptr(), s1.data_ptr(), i1.data_ptr(), cost.data_ptr(),
                           rows, stride, sizes.data_ptr(), offsets.data_ptr(), ymap.data_ptr(), N, Cy, H, W, status.data_ptr())
            maps[names[2 * g]], maps[names[2 * g + 1]] = zmap, ymap
        m = maps["y"]
        return cls(maps, status, N, m.shape[1], m.shape[2])

    # -- region sums ---------------------------------------------------------------------------------------------------
    def _on_device(self):
        import torch

        m = next(v for v in self.maps.values() if v is not None)
        if not (torch.is_tensor(m) and m.is_cuda):
            raise ValueError("the maps live on the GPU (no CPU fallback exists)")
        return m.device

    def regions_enqueue(self, labels, K):
        """regions() without the read: a device int64 tensor of N * K * 4 sums followed by one slot that holds the status
        word, enqueued on the current stream.  decode() turns its host copy into the sums."""
        import torch

        shape = _check_labels(labels, K, self.N, self.hc, self.wc)
        dev = self._on_device()
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
        if not torch.is_tensor(labels) or labels.device != dev:
            raise ValueError(f"labels: expected a tensor on {dev}")
        lab = labels.reshape(shape)
        lab = (lab.expand(self.N, -1, -1) if shape[0] != self.N else lab).contiguous()
        n = self.N * int(K) * 4
        out = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ptrs = (C.c_void_p * 4)(*[None if self.maps[k] is None else self.maps[k].data_ptr() for k in COMPONENTS])
        devargs.launch("dcvc_bits_regions", dev, ptrs, lab.data_ptr(), int(K), out.data_ptr(), self.N, self.hc, self.wc,
                       self.status.data_ptr())
        out[n:].view(torch.int32).copy_(self.status)
        return out

    @staticmethod
    def decode(host, N, K):
        """(N, K, 4) int64 numpy sums in 2^-20 bit (components mv_z, mv_y, z, y) from the host copy of
        regions_enqueue()'s tensor; raises BitMapError if a kernel met a CDF row or a label out of range."""
        a = np.asarray(host).reshape(-1)
        status = int(a[N * K * 4:].view(np.int32)[0])
        if status:
            raise BitMapError(f"bit map status {status} ({BAD_INDEX}: a CDF row out of range, {BAD_LABEL}: a label >= K)")
        return a[: N * K * 4].reshape(N, K, 4).copy()

    def regions(self, labels, K):
        """sums[n][label][component], (N, K, 4) int64 in 2^-20 bit (REGION_UNIT per bit): the maps summed over the cells
        of each label.  labels: uint8, 0..K-1, K <= 8, shaped (hc, wc), (1, hc, wc) or (N, hc, wc), on the maps' device
        (a numpy array is uploaded).  One launch, one host read."""
        return self.decode(self.regions_enqueue(labels, K).cpu().numpy(), self.N, int(K))

    def totals(self):
        """(N, 4) int64 host array in 2^-16 bit: the picture's bits per component (mv_z, mv_y, z, y; 0 for an absent map).
        The one place that reads the maps' status back with the sums."""
        import torch

        zeros = torch.zeros((1, self.hc, self.wc), dtype=torch.uint8, device=self._on_device())
        return self.regions(zeros, 1)[:, 0, :] // 16  # (every term of a total is a multiple of 16)

    def cells_device(self):
        """(N, hc, wc) float64 device tensor: bits per 16 x 16 cell, z-type costs spread evenly over their 4 x 4 cells."""
        import torch

        self._on_device()
        acc = None
        for k in COMPONENTS:
            m = self.maps[k]
            if m is None:
                continue
            m = m.to(torch.int64)
            m = m * 16 if k in ("mv_y", "y") else m.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)
            acc = m if acc is None else acc + m
        return acc.to(torch.float64) / REGION_UNIT

    def cells(self):
        """cells_device() as a numpy array (a host read)."""
        return self.cells_device().cpu().numpy()


def labels_from_boxes(boxes, height, width, grow=0, device=None):
    """(1, hc, wc) uint8 device tensor: 1 where a box of the picture, grown by `grow` pixels, touches the 16 x 16 cell --
    the touch rule of the q-scale map (include/dcvc_hip_roi.h), and its rasteriser: the map of background 1.00 and
    every class 0.50 is made by dcvc_roi_qmap and compared with 0.75.  height, width: the UNPADDED picture."""
    from . import roi as X

    devargs.whole("grow", grow, 0, X.MAX_GROW, "pixels")
    import torch

    boxes = X.as_boxes(boxes).validate(int(height), int(width), X.MAX_CLASSES)  # (by name, before any GPU work)
    m = X.q_map(boxes, height, width, X.RoiQ(100, (50,) * X.MAX_CLASSES, int(grow)), device=device)
    return (m[0] < 0.75).to(torch.uint8)
