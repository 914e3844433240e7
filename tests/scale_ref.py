"""A numpy restatement of include/dcvc_hip_scale.h written from its text (not from the kernel): the tap table of one axis,
and the fold one tap at a time in float32, so that every product and every sum is rounded as on the device (Python 3.10
has no fma; numpy float32 arithmetic never contracts).  fold64 is the same tables folded in float64."""
import numpy as np

from tests.pixel_ref import code  # noqa: F401 (the tests use it as R.code)

UNIT = 16384


def lanczos3(x):
    x = float(x)
    return float(np.sinc(x) * np.sinc(x / 3.0)) if abs(x) < 3.0 else 0.0


def taps(n_in, n_out):
    """(start int32[n_out], k int16[n_out, T]), sample by sample as the header states the rule."""
    r = n_in / n_out
    f = max(1.0, r)
    S = 3.0 * f
    los, ks = [], []
    for i in range(n_out):
        c = (i + 0.5) * r
        lo, hi = max(0, int(c - S + 0.5)), min(n_in, int(c + S + 0.5))
        w = np.array([lanczos3((j + 0.5 - c) / f) for j in range(lo, hi)], dtype=np.float64)
        w = w / w.sum()
        k = [int(v) for v in np.rint(UNIT * w)]
        k[k.index(max(k))] += UNIT - sum(k)  # the first largest
        los.append(lo)
        ks.append(k)
    T = max(len(k) for k in ks)
    start = np.array([min(lo, n_in - T) for lo in los], dtype=np.int32)
    table = np.zeros((n_out, T), dtype=np.int16)
    for i, (lo, k) in enumerate(zip(los, ks)):
        table[i, lo - start[i]:lo - start[i] + len(k)] = k
    return start, table


def base_size(height, width, n, d):
    return (2 * height * n + d) // (2 * d), (2 * width * n + d) // (2 * d)


def _fold_last_axis(a, start, k, dtype):
    """out[..., i] = sum over t of wf[i, t] * a[..., start[i] + t], one tap at a time from +0.0 in `dtype`."""
    wf = k.astype(dtype) * dtype(1.0 / UNIT)  # exact in float32: an int16 times 2^-14
    idx = start[:, None].astype(np.int64) + np.arange(k.shape[1])[None, :]  # (n_out, T)
    acc = np.zeros(a.shape[:-1] + (len(start),), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k.shape[1]):
            acc = acc + (wf[:, t] * a[..., idx[:, t]]).astype(dtype)
    return acc


def resize(a, size, dtype=np.float32, clamp=True):
    """(..., H_in, W_in) -> (..., *size): horizontal first, then vertical, clamped to [0, 1] at the end (a NaN gives 0)."""
    a = np.asarray(a, dtype=dtype)
    H_out, W_out = size
    xs, xk = taps(a.shape[-1], W_out)
    ys, yk = taps(a.shape[-2], H_out)
    h = _fold_last_axis(a, xs, xk, dtype)
    v = np.swapaxes(_fold_last_axis(np.swapaxes(h, -1, -2), ys, yk, dtype), -1, -2)
    if clamp:
        with np.errstate(invalid="ignore"):
            v = np.fmin(np.fmax(v, dtype(0.0)), dtype(1.0))
    return np.ascontiguousarray(v)


def down(a, n, d):
    return resize(a, base_size(a.shape[-2], a.shape[-1], n, d))


def up(a, full):
    return resize(a, full)


def fold64(a, size):
    """The same tables folded in float64, unclamped."""
    return resize(np.asarray(a, dtype=np.float64), size, dtype=np.float64, clamp=False)
