"""Rate control: hit a number of bits per picture by moving the quantisation step of the latent y from
picture to picture inside a GOP.

No rate model with fitted constants exists (no trained checkpoint does), so the local rate-versus-step curve is MEASURED
from the picture itself: one small kernel (dcvc_bits_sweep_scale, include/dcvc_hip_bits.h) prices the picture's own
residuals, by the coder's own integer cost tables, for a ladder of step factors; host-side feedback on the actual byte
counts does the rest.

    LADDER        the default factors, in hundredths (steps of about 2^(1/3)); check_ladder(), ladder_factors()
    RateSweep     the device result of one picture, (N, K) int64 in 2^-16 bit, on its way to pinned host memory
    RateControl   the decisions of one GOP: a pure host object (no torch, no GPU), Python integers and Fractions only, so
                  a decision is the same on every host

Each .bin header carries its picture's own q indexes, so the decoder needs nothing new.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

from . import devargs

LADDER = (50, 63, 79, 100, 126, 159, 200, 252)
MAX_LADDER = 8          # DCVC_BITS_MAX_LADDER
UNIT = 65536            # DCVC_BITS_UNIT: sweep units per bit
BAD_VALUE = 4           # DCVC_BITS_BAD_VALUE
Q_INDEX_RANGE = (1, 65500)  # the wire range of a q index (stream.get_rounded_q: q-scales 0.01 .. 655 in hundredths)


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_ladder(ladder):
    """The ladder as a tuple of ints, or ValueError by name: 2 to 8 strictly increasing integers (hundredths of a step
    factor) within 10..1000, 100 among them."""
    try:
        lad = tuple(ladder)
    except TypeError:
        raise ValueError(f"ladder: expected a sequence of integers (hundredths), got {type(ladder).__name__}") from None
    if not 2 <= len(lad) <= MAX_LADDER:
        raise ValueError(f"ladder: {len(lad)} entries (2..{MAX_LADDER})")
    if not all(_is_int(h) or (hasattr(h, "__index__") and not isinstance(h, bool)) for h in lad):
        raise ValueError(f"ladder: entries must be integers (hundredths of a factor), got {lad!r}")
    lad = tuple(int(h) for h in lad)
    if any(not 10 <= h <= 1000 for h in lad):
        raise ValueError(f"ladder: entries must lie within 10..1000 (factors 0.1 .. 10), got {lad!r}")
    if any(a >= b for a, b in zip(lad, lad[1:])):
        raise ValueError(f"ladder: entries must be strictly increasing, got {lad!r}")
    if 100 not in lad:
        raise ValueError(f"ladder: must contain 100 (the step the picture is coded with), got {lad!r}")
    return lad


def ladder_factors(ladder):
    """(K,) float32: f_k = float32(h_k) / float32(100), the factors the kernel divides by (formed here, never there)."""
    import numpy as np

    return (np.asarray(check_ladder(ladder), dtype=np.float32) / np.float32(100)).astype(np.float32)


def _check_q_range(q_range):
    try:
        lo, hi = q_range
    except (TypeError, ValueError):
        raise ValueError(f"q_range: expected (lowest, highest) q index, got {q_range!r}") from None
    if not (_is_int(lo) and _is_int(hi)) or not Q_INDEX_RANGE[0] <= lo <= hi <= Q_INDEX_RANGE[1]:
        raise ValueError(f"q_range: expected integers with {Q_INDEX_RANGE[0]} <= lowest <= highest <= {Q_INDEX_RANGE[1]} "
                         f"(q indexes, hundredths of a q-scale), got {q_range!r}")
    return lo, hi


def q_index_range(q_range):
    """A (lowest, highest) pair of q-SCALES (the --q-range of the file loops) -> the q_range of RateControl in q indexes;
    None -> the whole wire range.  Refused by name: lowest > highest, values outside [0.01, 655]."""
    if q_range is None:
        return Q_INDEX_RANGE
    try:
        lo, hi = (float(v) for v in q_range)
    except (TypeError, ValueError):
        raise ValueError(f"q_range: expected (lowest, highest) q-scale, got {q_range!r}") from None
    if not (0.01 <= lo <= 655.0 and 0.01 <= hi <= 655.0):  # (a NaN compares false)
        raise ValueError(f"q_range: q-scales lie within the wire range [0.01, 655], got {lo} {hi}")
    if lo > hi:
        raise ValueError(f"q_range: the lowest q-scale {lo} exceeds the highest {hi}")
    return int(round(lo * 100)), int(round(hi * 100))


def target_bits_of(target_bpp, height, width):
    """Bits per picture of a target in bits per pixel of the UNPADDED height x width picture, as an exact Fraction.
    Refused by name: a target that is not a finite number above 0."""
    import math

    if isinstance(target_bpp, bool) or not isinstance(target_bpp, (int, float, Fraction)) or \
            (isinstance(target_bpp, float) and not math.isfinite(target_bpp)) or target_bpp <= 0:
        raise ValueError(f"target_bpp: expected a finite number of bits per pixel above 0, got {target_bpp!r}")
    return Fraction(target_bpp) * int(height) * int(width)


class RateSweep:
    """What the latent y of one coded picture (or of a batch of N rate points) would cost for every step factor of
    `ladder`: (N, K) int64 in 2^-16 bit.  The kernel and the copy of its result to pinned host memory were enqueued on
    the stream that coded the picture, before its symbol planes were staged: the sums have arrived when the picture's
    pending.finish() returns, and sums() then waits for nothing."""

    def __init__(self, ladder, row, host, event, N):
        self.ladder, self.row, self.host, self.event, self.N = ladder, row, host, event, int(N)

    @classmethod
    def enqueue(cls, tables, edges, y_res, scales_hat, N, C_, H, W, ladder):
        """tables: CostTables.on(device); edges: the 256 bin edges of the scale index on the device; y_res, scales_hat:
        the dense NHWC planes the two dual-prior steps of this picture wrote.  A memset, one launch, one tiny fill and
        one asynchronous copy on the current stream; nothing synchronised."""
        import torch

        lad = check_ladder(ladder)
        fac = ladder_factors(lad)
        K, dev = len(lad), y_res.device
        if y_res.numel() != N * H * W * C_ or scales_hat.numel() != y_res.numel():
            raise ValueError("sweep: the residual and scale planes do not match the latent grid")
        cost, sizes, offsets, rows, stride = tables["scale"]
        row = torch.empty(N * K + 1, dtype=torch.int64, device=dev)  # (the last slot holds the status word)
        status = row[N * K:].view(torch.int32)
        status.zero_()
        devargs.launch("dcvc_bits_sweep_scale", dev, y_res.data_ptr(), scales_hat.data_ptr(), edges.data_ptr(),
                       fac.ctypes.data_as(C.c_void_p), K, cost.data_ptr(), rows, stride, sizes.data_ptr(), offsets.data_ptr(),
                       row.data_ptr(), N, C_, H, W, status.data_ptr())
        host = torch.empty(N * K + 1, dtype=torch.int64, pin_memory=True)
        host.copy_(row, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return cls(lad, row, host, ev, N)

    @staticmethod
    def decode(host, N, K):
        """(N, K) int64 numpy sums from the host copy of the device row; raises bitmap.BitMapError when the kernel met a
        value that is not finite, a symbol that is no int32, or a CDF row out of range."""
        import numpy as np

        from .bitmap import BAD_INDEX, BitMapError

        a = np.asarray(host).reshape(-1)
        status = int(a[N * K:].view(np.int32)[0])
        if status:
            raise BitMapError(f"rate sweep status {status} ({BAD_INDEX}: a CDF row out of range, {BAD_VALUE}: a residual or "
                              f"scale that is not finite, or a symbol beyond int32)")
        return a[: N * K].reshape(N, K).copy()

    def sums(self):
        """(N, K) int64 host array in 2^-16 bit; column k belongs to ladder[k]."""
        self.event.synchronize()  # (long past once the picture's planes have arrived)
        return self.decode(self.host.numpy(), self.N, len(self.ladder))


def _round_half_up(x):
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)


class RateControl:
    """The q_y decisions of ONE GOP (make a new one at every I picture).  Pictures are numbered j = 0 (the I picture),
    1, 2, ... inside the GOP.

        q = rc.decide(j, q_start)          before P picture j is enqueued: its q_y index
        rc.record(j, q, bits, est)         when picture j has been retired: its q index, its actual bits (payload plus
                                           header) and, for a P picture, row n of its RateSweep.sums()

    The rule, with b = target_bits, G = gop, m_k = ladder[k] / 100:
      the I picture keeps its q, the first two P pictures keep q_start;
      P picture j >= 3 is decided from picture s = j - 2, the newest one already retired when j is enqueued:
        T_s(m)  = A_s + (E_s(m) - E_s(1)) / 65536, E_s piecewise linear in m between the ladder points, constant outside
        assumed = T_s(q_{j-1} / q_s)               what picture j - 1, still in flight, is taken to cost
        b_j     = (G b - sum of A_0 .. A_{j-2} - assumed) / max(1, G - j)
        m*      = the point of T_s at b_j: the first ladder segment, ascending, whose ends bracket b_j, solved linearly
                  (its lower end where that end already equals b_j); without such a segment the ladder end with the
                  smaller |T - b_j|, ties to the end nearer 1, then to the lower end
        q_j     = clip(round_half_up(q_s m*), q_range)
    Every quantity is a Python integer or a Fraction."""

    def __init__(self, target_bits, gop, q_range=Q_INDEX_RANGE, ladder=LADDER):
        import math

        if isinstance(target_bits, bool) or not isinstance(target_bits, (int, float, Fraction)) or \
                (isinstance(target_bits, float) and not math.isfinite(target_bits)) or target_bits <= 0:
            raise ValueError(f"target_bits: expected a finite number of bits per picture above 0, got {target_bits!r}")
        if not _is_int(gop) or gop < 1:
            raise ValueError(f"gop: expected an integer >= 1, got {gop!r}")
        self.b, self.gop = Fraction(target_bits), gop
        self.q_range = _check_q_range(q_range)
        self.ladder = check_ladder(ladder)
        self._m = [Fraction(h, 100) for h in self.ladder]
        self._one = self.ladder.index(100)
        self._q, self._bits, self._est, self._budget = {}, {}, {}, {}

    # -- the model of one picture --------------------------------------------------------------------------------------
    def _curve(self, s):
        """[T_s(m_k)] of recorded picture s."""
        row = self._est[s]
        return [self._bits[s] + Fraction(e - row[self._one], UNIT) for e in row]

    def _at(self, T, m):
        pts = self._m
        if m <= pts[0]:
            return T[0]
        for k in range(len(pts) - 1):
            if m <= pts[k + 1]:
                return T[k] + (T[k + 1] - T[k]) * (m - pts[k]) / (pts[k + 1] - pts[k])
        return T[-1]

    def _solve(self, T, b):
        pts = self._m
        for k in range(len(pts) - 1):
            lo, hi = T[k], T[k + 1]
            if min(lo, hi) <= b <= max(lo, hi):
                return pts[k] if lo == b else pts[k] + (b - lo) * (pts[k + 1] - pts[k]) / (hi - lo)
        first, last = abs(T[0] - b), abs(T[-1] - b)
        if first != last:
            return pts[0] if first < last else pts[-1]
        return pts[-1] if abs(pts[-1] - 1) < abs(pts[0] - 1) else pts[0]

    def predict(self, s, q_index):
        """T_s(q_index / q_s): what recorded P picture s says a picture coded with `q_index` costs, as a Fraction."""
        if self._est.get(s) is None:
            raise RuntimeError(f"predict: picture {s} has no recorded sweep")
        return self._at(self._curve(s), Fraction(q_index, self._q[s]))

    # -- the two calls -------------------------------------------------------------------------------------------------
    def decide(self, j, q_start):
        if not _is_int(j) or j < 1:
            raise ValueError(f"decide: picture {j!r} is no P picture of the GOP (1, 2, ...)")
        if not _is_int(q_start) or not Q_INDEX_RANGE[0] <= q_start <= Q_INDEX_RANGE[1]:
            raise ValueError(f"decide: q_start must be a q index within {Q_INDEX_RANGE[0]}..{Q_INDEX_RANGE[1]}, got {q_start!r}")
        if j > 1 and j - 1 not in self._q:
            raise RuntimeError(f"decide: picture {j - 1} has not been decided yet")
        if j <= 2:
            self._q[j], self._budget[j] = q_start, None
            return q_start
        s = j - 2
        if any(i not in self._bits for i in range(s + 1)) or self._est.get(s) is None:
            raise RuntimeError(f"decide: picture {j} is decided from pictures 0..{s}, which have not all been recorded")
        T = self._curve(s)
        q_s = self._q[s]
        assumed = self.predict(s, self._q[j - 1])
        budget = (self.gop * self.b - sum(self._bits[i] for i in range(s + 1)) - assumed) / max(1, self.gop - j)
        q = _round_half_up(q_s * self._solve(T, budget))
        q = min(max(q, self.q_range[0]), self.q_range[1])
        self._q[j], self._budget[j] = q, budget
        return q

    def record(self, j, q_index, bits, est=None):
        if not _is_int(j) or j < 0 or j in self._bits:
            raise ValueError(f"record: picture {j!r} is out of range or already recorded")
        if j and j in self._q and self._q[j] != q_index:  # (an undecided picture: the replay of a log)
            raise ValueError(f"record: picture {j} was decided with q index {self._q[j]}, not {q_index!r}")
        if isinstance(bits, bool) or not isinstance(bits, (int, Fraction)) or bits < 0:
            raise ValueError(f"record: bits must be a non-negative integer (or Fraction), got {bits!r}")
        if est is not None:
            est = tuple(int(e) for e in est)
            if len(est) != len(self.ladder):
                raise ValueError(f"record: {len(est)} sweep sums for a ladder of {len(self.ladder)}")
        elif j:
            raise ValueError("record: a P picture is recorded with its sweep sums")
        self._q.setdefault(j, q_index)
        self._budget.setdefault(j, None)
        self._bits[j], self._est[j] = bits, est

    @property
    def log(self):
        """[(q index, actual bits, budget b_j or None where nothing was decided, sweep row or None)] of the recorded
        pictures, in order."""
        return [(self._q[j], self._bits[j], self._budget[j], self._est[j]) for j in sorted(self._bits)]


def factory(target_bits, gop, q_range=Q_INDEX_RANGE, ladder=LADDER):
    """The `rate=` argument of GopEncoder.encode_gop: a callable that makes one RateControl per GOP.  The arguments are
    checked here, once, before anything is coded."""
    RateControl(target_bits, gop, q_range, ladder)
    return lambda: RateControl(target_bits, gop, q_range, ladder)
