"""Plain references of the non-convolution forward operators of include/dcvc_hip.h, written from the reference
operator each entry point replaces (F.interpolate, F.avg_pool2d, nn.MaxPool2d, torch.round, the Laplace / Normal /
factorised rate formulas of common_model.py:51-73), not from the kernels, on NCHW numpy arrays -- and the inputs and
error bounds that tests/test_forward_ref_host.py (CPU) and tests/test_gpu_forward_ops.py (GPU) share.

Two kinds of reference:
  * fp64 ("want64"): the operator evaluated in double on the fp32 inputs; compared within a derived bound.
  * fp32, in the order include/dcvc_hip.h documents: demanded bit for bit where every step is one IEEE operation
    whose value does not depend on FMA contraction (copies, max, rint, one multiply / one divide, sums of products
    with 0.5).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
EPS = 2.0 ** -24           # half an ulp of 1.0f: the relative error of one fp32 rounding
LN2 = math.log(2.0)
P_FLOOR = float(F32(1e-5))  # probs_to_bits adds the fp32 constant to an fp32 tensor

# k of the per-element rate bound  k * 2^-24 / ((p64 + 1e-5) ln 2) + 4 * 2^-24 * want64 : twice the largest
# |p32 - p64| / 2^-24 of the torch-CPU fp32 oracle on rate_grid() / factorized_grid(), as measured (and re-measured at
# every run) by tests/test_forward_ref_host.py::test_fp32_oracle_probability_error_sets_k -- see there for the figures.
RATE_K = {"laplace": 3.7, "gaussian": 4.5, "factorized": 5.8}  # measured 1.802, 2.215, 2.857


def bits_equal(a, b):
    """same shape and the same 32 bits in every element (so -0.0 != +0.0)"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def _quad(x):
    """the four taps of every 2x2 block: a b / c d"""
    return x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]


def fmax(a, b):
    """IEEE 754-2019 maximum of two NaN-free arrays: +0 is larger than -0, whatever the order of the operands.
    (nn.MaxPool2d keeps the FIRST of equal values in scan order, so for a tie between zeros of both signs torch's
    sign is an accident of the order; value-wise the two agree everywhere.)"""
    return np.where(a == b, np.where(np.signbit(a), b, a), np.where(a > b, a, b))


def fmin(a, b):
    return np.where(a == b, np.where(np.signbit(a), a, b), np.where(a < b, a, b))


# ---- resampling ---------------------------------------------------------------------------------------------
def up2(x, scale):
    """bilinearupsacling(x) * scale (video_net.py:58-63,139) in fp64; `scale` is the fp32 value the kernel receives"""
    y = F.interpolate(_t64(x), scale_factor=2, mode="bilinear", align_corners=False)
    return (y * float(F32(scale))).numpy()


def up2_tap_max(x):
    """max |tap| over the (at most) four source pixels each output of up2 interpolates between"""
    a = np.abs(np.asarray(x, dtype=np.float64))

    def taps(n):  # align_corners=False, factor 2: source position (o + 0.5) / 2 - 0.5, clamped at 0
        s = np.maximum((np.arange(2 * n) + 0.5) / 2.0 - 0.5, 0.0)
        i0 = np.floor(s).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1)

    y0, y1 = taps(a.shape[2])
    x0, x1 = taps(a.shape[3])
    rows = np.maximum(a[:, :, y0], a[:, :, y1])
    return np.maximum(rows[..., x0], rows[..., x1])


def down2(x, scale, mode):
    """fp64.  mode 0: bilineardownsacling(x) * scale (video_net.py:66-71); 1: F.avg_pool2d(x, 2, 2) * scale
    (video_net.py:132-133); 2: nn.MaxPool2d(2) (scale unused)"""
    t = _t64(x)
    if mode == 0:
        y = F.interpolate(t, (t.size(2) // 2, t.size(3) // 2), mode="bilinear", align_corners=False)
    elif mode == 1:
        y = F.avg_pool2d(t, 2, 2)
    else:
        return F.max_pool2d(t, 2).numpy()
    return (y * float(F32(scale))).numpy()


def down2_tap_max(x):
    a, b, c, d = _quad(np.abs(np.asarray(x, dtype=np.float64)))
    return np.maximum(np.maximum(a, b), np.maximum(c, d))


def down2_f32(x, scale, mode):
    """fp32 in the order include/dcvc_hip.h documents.  Multiplying by 0.5 is exact, so mode 0 does not depend on
    whether a compiler contracts a*b + c; bit-exact for the kernel when `scale` is a power of two."""
    a, b, c, d = _quad(np.asarray(x, dtype=F32))
    h, s = F32(0.5), F32(scale)
    if mode == 0:
        return (h * (h * a + h * b) + h * (h * c + h * d)) * s
    return ((((a + b) + c) + d) / F32(4.0)) * s


def maxpool2(x):
    a, b, c, d = _quad(np.asarray(x, dtype=F32))
    return fmax(fmax(a, b), fmax(c, d)).astype(F32)


def interp_bound(scale, tap_max):
    """|fp32 - fp64| of a convex combination of four taps times scale: at most seven roundings of values no larger
    than |scale| max|tap| (four products or sums per row pair, the two row weights, the final sum, the scale) -> 8 eps"""
    return 8.0 * EPS * abs(float(F32(scale))) * tap_max


# ---- layout, quantisation -----------------------------------------------------------------------------------
def clamp01(x):
    """clamp to [0, 1] with IEEE maximum / minimum: -0.0 and every negative become +0.0"""
    x = np.asarray(x, dtype=F32)
    return fmin(fmax(x, np.zeros_like(x)), np.ones_like(x)).astype(F32)


def round_half_even(z):
    """torch.round: to nearest, ties to even; keeps the sign of a zero result"""
    return np.rint(np.asarray(z, dtype=F32))


def symbols(z):
    """(N, C, H, W) int32 symbol planes of an NCHW latent"""
    return round_half_even(z).astype(np.int32)


def symbols_to_float(sym):
    return np.asarray(sym, dtype=np.int32).astype(F32)


def curr_q(q_basic, q_scale, dtype=F32):
    """q[n, c] = max(q_basic[c], 0.5) * q_scale[n] (video_model.py: get_curr_q), one fp32 multiply"""
    qb = np.maximum(np.asarray(q_basic, dtype=F32), F32(0.5)).astype(dtype)
    return (np.asarray(q_scale, dtype=F32).astype(dtype)[:, None] * qb[None, :])[:, :, None, None]


def scale_channels(x, q_basic, q_scale, multiply, dtype=F32):
    """y / curr_q (multiply False) or y_hat * curr_q (True): one IEEE divide or multiply per element in fp32;
    dtype=np.float64 gives the fallback reference (q itself stays the fp32 product the kernel forms)"""
    q = curr_q(q_basic, q_scale).astype(dtype)
    x = np.asarray(x, dtype=F32).astype(dtype)
    return x * q if multiply else x / q


# ---- rate ---------------------------------------------------------------------------------------------------
def probs_to_bits(p):
    """common_model.py:51-55 in fp64"""
    return np.maximum(-np.log(p + P_FLOOR) / LN2, 0.0)


def laplace_bits(y, sigma, lo=1e-5):
    """common_model.py:64-69 in fp64 -> (bits, p); the clamps are the fp32 constants the fp32 tensor is clamped to
    (`lo` is the reference's 1e-5; another value only where a test shows that its inputs would tell the difference)"""
    y = np.asarray(y, dtype=np.float64)
    s = np.clip(np.asarray(sigma, dtype=np.float64), float(F32(lo)), float(F32(1e10)))

    def cdf(t):  # torch.distributions.Laplace(0, s).cdf
        return 0.5 - 0.5 * np.sign(t) * np.expm1(-np.abs(t) / s)

    p = cdf(y + 0.5) - cdf(y - 0.5)
    return probs_to_bits(p), p


def gaussian_bits(y, sigma, lo=0.11):
    """common_model.py:57-62 in fp64 -> (bits, p); `lo` is the reference's 0.11, as in laplace_bits"""
    y = _t64(y)
    s = _t64(sigma).clamp(float(F32(lo)), float(F32(1e10)))

    def cdf(t):  # torch.distributions.Normal(0, s).cdf
        return 0.5 * (1.0 + torch.erf(t / s / math.sqrt(2.0)))

    p = (cdf(y + 0.5) - cdf(y - 0.5)).numpy()
    return probs_to_bits(p), p


def factorized_bits(z, params):
    """common_model.py:71-73 with BitEstimator.get_cdf (entropy_models.py:68-73,109-117) in fp64 -> (bits, p).
    z: (N, C, H, W); params: the (11, C) block h1,b1,a1,h2,b2,a2,h3,b3,a3,h4,b4"""
    P = np.asarray(params, dtype=np.float64)[:, None, :, None, None]

    def cdf(x):
        for i in range(3):
            x = x * np.logaddexp(0.0, P[3 * i]) + P[3 * i + 1]
            x = x + np.tanh(x) * np.tanh(P[3 * i + 2])
        x = x * np.logaddexp(0.0, P[9]) + P[10]
        return 1.0 / (1.0 + np.exp(-x))

    z = np.asarray(z, dtype=np.float64)
    p = cdf(z + 0.5) - cdf(z - 0.5)
    return probs_to_bits(p), p


def rate_bound(p64, want64, k):
    """|fp32 bits - want64| per element: k eps of absolute error in the probability through d(-log2(p + 1e-5))/dp,
    plus four roundings of the result itself (the sum, the logarithm, the sign / division by ln 2)"""
    return k * EPS / ((p64 + P_FLOOR) * LN2) + 4.0 * EPS * want64


def rate_sum_bound(p64, want64, k):
    """a sum of n such terms: the per-element bounds, plus n eps of the sum for the summation"""
    return rate_bound(p64, want64, k).sum() + want64.size * EPS * want64.sum()


def rate_grid():
    """(y, scale), 4096 fp32 pairs.  Every symbol from -60 to 60 at scales at and around the two clamps (1e-5, 0.11:
    the constant and both fp32 neighbours), negative and zero scales, and scales up to 64; the tails where p
    underflows to 0 (bits = -log2(1e-5)) are among them.

    At an integer symbol |y -+ 0.5| >= 0.5, so below a scale of about 0.03 the Laplace p is 1 at y = 0 and 0 elsewhere
    whatever the scale: those rows cannot tell a clamp of 1e-5 from one of 1e-3.  So 91 more pairs put an edge of the
    bin within a few 1e-5 of the mode -- y = +-(0.5 +- d), d = 84, 168 and 336 units of 2^-23 (1.0e-5, 2.0e-5, 4.0e-5;
    y - 0.5 and y + 0.5 are exact in fp32) -- at every scale that is clamped or close to the clamp: there p is 0.5
    exp(-d / s) or 1 - that, e.g. 0.068 at d = 2e-5 under the clamp 1e-5 against 0.41 under 1e-4.  The remaining 12
    slots repeat the start."""
    nxt = lambda v, to: np.nextafter(F32(v), F32(to))
    scales = [nxt(1e-5, 0), F32(1e-5), nxt(1e-5, 1), nxt(0.11, 0), F32(0.11), nxt(0.11, 1), -1.0, -1e-5, 0.0, -0.0,
              2e-5, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.12, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0,
              24.0, 32.0, 64.0]
    sym = np.arange(-60, 61)
    y = np.repeat(sym, len(scales)).astype(F32)
    s = np.tile(np.array(scales, dtype=F32), len(sym))
    near = np.array(scales[:13], dtype=F32)  # the clamped scales, the clamps' neighbours, 2e-5, 1e-4, 1e-3
    d = [F32(m * 2.0 ** -23) for m in (84, 168, 336)]
    off = np.array([0.5 + d[0], 0.5 + d[1], 0.5 + d[2], -(0.5 + d[1]), 0.5 - d[1], -0.5 + d[1], 0.5 - d[2]], dtype=F32)
    y = np.concatenate([y, np.repeat(off, near.size)])
    s = np.concatenate([s, np.tile(near, off.size)])
    idx = np.arange(4096) % y.size
    return y[idx], s[idx]


RATE_SUM_PER_SAMPLE = 2 * 1024 * 256 + 77  # three trips of the kernels' grid-stride loop (1024 blocks of 256), ragged tail


def rate_sum_inputs():
    """(y, scale) of shape (2, RATE_SUM_PER_SAMPLE): rounded N(0, 3) symbols, scales uniform in [-0.2, 3.8)"""
    g = torch.Generator().manual_seed(4)
    shape = (2, RATE_SUM_PER_SAMPLE)
    return torch.round(torch.randn(shape, generator=g) * 3).numpy(), (torch.rand(shape, generator=g) * 4 - 0.2).numpy()


FACTORIZED_CHANNELS = (0, 21, 42, 63)


def factorized_latents():
    """the C = 64 latents of the factorised sum test: N = 2, HW = 1 and HW = 300"""
    g = torch.Generator().manual_seed(11)
    return [torch.round(torch.randn(2, 64, h, w, generator=g) * 3).numpy() for h, w in ((1, 1), (15, 20))]


def factorized_grid():
    """the symbols -40 .. 40 of one channel, as a (81, 1, 1, 1) latent"""
    return np.arange(-40, 41).astype(F32).reshape(-1, 1, 1, 1)


# ---- squeeze-excitation -------------------------------------------------------------------------------------
def se_gate(mean, w1, w2):
    """SELayer (video_net.py:149-162) after the pooling, fp64: sigmoid(W2 relu(W1 mean)); mean (N, C)"""
    m = np.asarray(mean, dtype=np.float64)
    hid = np.maximum(m @ np.asarray(w1, dtype=np.float64).T, 0.0)
    return 1.0 / (1.0 + np.exp(-(hid @ np.asarray(w2, dtype=np.float64).T)))
