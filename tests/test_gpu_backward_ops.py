"""Per-operator gradients of the rate, quantiser and SE backward kernels (include/dcvc_hip_grad.h) on a real MI355X,
against torch autograd of the oracle's restatement of each operator (oracle/dcvc_ref.py) on the CPU in float64, with the
same autograd in float32 as the yardstick of the reference's own arithmetic.  The per-element rule (tier A / tier B /
branch masks) is grad_check.tier_check; every comparison also shows, on the same data, that it rejects the output
scaled by (1 + 1e-4) and a masked element set to its unmasked value.  The kernels are called as the product calls
them: through grad.Tape / Engine, or through lib.hip() with device buffers on the engine's stream.

The whole-picture tests (tests/test_gpu_backward.py) cannot see a wrong branch that touches a few hundred elements; the
shapes and values here are the edges where these kernels go wrong: clamp windows, LowerBound's "pass if the gradient is
negative" rule, checkerboard phases at odd widths, q_step at 0.5, max-pool ties and NaNs, denormal masks."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "diag"))

from oracle import dcvc_ref as R  # noqa: E402


def f32(v):
    return float(np.float32(v))


def ulp_step(v, toward):
    return float(np.nextafter(np.float32(v), np.float32(toward)))


@pytest.fixture(scope="module")
def eng():
    from vcm_ts_amd.engine import Engine

    return Engine(torch.device("cuda:0"), "fp32")


@pytest.fixture(scope="module")
def eng_split():
    from vcm_ts_amd.engine import Engine

    return Engine(torch.device("cuda:0"), "fp16x3")


def _ok(code, what):
    from vcm_ts_amd import lib

    lib.check(code, what)


def _p(t):
    return t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rule itself (host only)
def test_tier_rule_has_teeth():
    """grad_check.tier_check on synthetic data: accepts a result within the bounds, rejects a 1e-4 scaling on tier A, a
    masked element that is not exactly 0, a passing element that is 0 and a NaN."""
    import grad_check as G

    g = torch.Generator().manual_seed(0)
    r64 = torch.randn(1000, generator=g, dtype=torch.float64)
    r32 = r64.float().double()
    zero = torch.zeros(1000, dtype=torch.bool)
    zero[::50] = True
    r64[zero], r32[zero] = 0.0, 0.0
    tier_a = torch.ones(1000, dtype=torch.bool)
    tier_a[1::3] = False
    got = r32.clone()
    assert not G.tier_check(got, r64, r32, tier_a, zero, ~zero)[3]
    G.assert_tiers("synthetic", got, r64, r32, tier_a, zero, ~zero, unmasked=torch.randn(1000, generator=g))
    assert G.tier_check(got * (1 + 1e-4), r64, r32, tier_a)[3]
    bad = got.clone()
    bad[0] = 1e-30
    assert G.tier_check(bad, r64, r32, tier_a, zero, ~zero)[3]
    bad = got.clone()
    bad[1] = 0.0
    assert G.tier_check(bad, r64, r32, tier_a, zero, ~zero)[3]
    bad = got.clone()
    bad[2] = float("nan")
    assert G.tier_check(bad, r64, r32, tier_a)[3]


# ---------------------------------------------------------------------------------------------------------------------
# 1. dcvc_scale_bits_bwd (Laplace, Gaussian)
R04_CHAOTIC = [  # profiles/r04_rate_gradient_chaotic_elements.txt: y_bit and (negative, clamped) scale of the six elements
    (-0.5001, -9.303e-03), (-0.5001, -3.004e-02), (-0.5001, -1.257e-01), (0.5000, -2.384e-02), (-0.5001, -2.267e-01),
    (-0.5001, -6.250e-03),
]


def _bits_parts(y, s, kind, lo):
    """p and the unbounded bits of the oracle's operator (no grad), in y's dtype; s already clamped by the caller."""
    sc = s.clamp(lo, 1e10)
    if kind == 0:
        d = torch.distributions.laplace.Laplace(torch.zeros_like(sc), sc)
    else:
        d = torch.distributions.normal.Normal(torch.zeros_like(sc), sc)
    p = d.cdf(y + 0.5) - d.cdf(y - 0.5)
    return p, -torch.log(p + 1e-5) / math.log(2.0)


def _scale_bits_case(kind, N=3, per=4099):
    lo = 1e-5 if kind == 0 else 0.11
    g = torch.Generator().manual_seed(20 + kind)
    n = N * per
    half = [0.5, -0.5, ulp_step(0.5, 1), ulp_step(0.5, 0), ulp_step(-0.5, -1), ulp_step(-0.5, 0), 0.5001, -0.5001,
            1.5, -2.5]
    tails = [50.0, -50.0, 1e3, -1e3]
    y = torch.randint(-6, 7, (n,), generator=g).float()
    r = torch.rand(n, generator=g)
    noisy = r < 0.45
    y[noisy] += torch.rand(int(noisy.sum()), generator=g) - 0.5
    pick = (r >= 0.45) & (r < 0.65)
    y[pick] = torch.tensor(half)[torch.randint(0, len(half), (int(pick.sum()),), generator=g)]
    pick = (r >= 0.65) & (r < 0.70)
    y[pick] = torch.tensor(tails)[torch.randint(0, len(tails), (int(pick.sum()),), generator=g)]
    edge_y = (r >= 0.45) & (r < 0.70)
    special_s = [-1.0, -0.01, 0.0, lo * 0.98, lo, lo * 1.02, 1e3, 1e10, 2e10]
    s = torch.exp(torch.empty(n).uniform_(math.log(0.05), math.log(10.0), generator=g))
    rs = torch.rand(n, generator=g)
    pick = rs < 0.35
    s[pick] = torch.tensor(special_s)[torch.randint(0, len(special_s), (int(pick.sum()),), generator=g)]
    # fixed patterns in every sample: the r04 elements (with neighbours of their y), the p -> 1 corner (y = 0, a scale
    # that leaves bits < 0: LowerBound drops positive and passes negative upstream gradients), and the clamp bounds
    fixed = [(yy + dy, ss) for yy, ss in R04_CHAOTIC for dy in (0.0, -2e-5, 3e-5)]
    fixed += [(0.0, v) for v in ((0.02, 0.03, 0.04) if kind == 0 else (0.1, 0.1105, lo))]
    fixed += [(ulp_step(0.5, 0), lo), (-0.50001, lo), (0.50003, lo), (2.0, 1e10), (0.0, 2e10)]
    for k in range(N):
        for j, (yy, ss) in enumerate(fixed):
            for base in (k * per, (k + 1) * per - len(fixed)):  # both ends of a sample: inside 256-thread blocks
                y[base + j], s[base + j] = yy, ss
                edge_y[base + j] = True
    y, s = y.float(), s.float()
    # float64 inputs: the fp32 values, except the clamp bounds themselves, which are the double bounds there (so that the
    # clamp's "inside" predicate is the same in both precisions)
    s64 = s.double()
    for b in (lo, 1e10):
        s64[s == f32(b)] = b
    y64 = y.double()
    # every branch predicate must agree between fp32 and fp64: LowerBound(bits, 0) with a margin
    for _ in range(3):
        _, b32 = _bits_parts(y, s, kind, lo)
        p64, b64 = _bits_parts(y64, s64, kind, lo)
        bad = ((b32 >= 0) != (b64 >= 0)) | (b64.abs() < 1e-6)
        if not bad.any():
            break
        y[bad], s[bad], y64[bad], s64[bad] = 1.0, 1.0, 1.0, 1.0
    assert not bad.any()
    up = torch.tensor([1.0 / per, -0.7, 3e4])[:N]
    return y, s, y64, s64, up, p64, b64, edge_y, lo


def _cdf_cancellation(y64, s64, kind, lo):
    """(|dF1| + |dF0|) / |dF1 - dF0| of p = F(y + 0.5) - F(y - 0.5) with respect to y and to the scale, in float64: how
    strongly the two CDF terms cancel in each gradient (1: not at all)."""
    y1, y0, s1, s0 = (t.clone().requires_grad_() for t in (y64, y64, s64, s64))
    D = torch.distributions.laplace.Laplace if kind == 0 else torch.distributions.normal.Normal
    p = D(torch.zeros_like(s1), s1.clamp(lo, 1e10)).cdf(y1 + 0.5) - D(torch.zeros_like(s0), s0.clamp(lo, 1e10)).cdf(y0 - 0.5)
    p.sum().backward()
    out = []
    for a, b in ((y1.grad, y0.grad), (s1.grad, s0.grad)):
        num, den = a.abs() + b.abs(), (a + b).abs()
        out.append(torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, float("inf"), 1.0)))
    return out


def _ref_scale_bits(y, s, up, N, per, kind, dtype, bounded=True):
    yy, ss = y.to(dtype).clone().requires_grad_(), s.to(dtype).clone().requires_grad_()
    if bounded:
        bits = (R.laplace_bits if kind == 0 else R.gaussian_bits)(yy, ss)
    else:  # the unmasked values (no LowerBound): what a blocked element would carry if the branch passed
        sc = ss.clamp(1e-5 if kind == 0 else 0.11, 1e10)
        d = (torch.distributions.laplace.Laplace if kind == 0 else torch.distributions.normal.Normal)(torch.zeros_like(sc), sc)
        bits = -1.0 * torch.log(d.cdf(yy + 0.5) - d.cdf(yy - 0.5) + 1e-5) / math.log(2.0)
    (bits.view(N, per).sum(1) * up.to(dtype)).sum().backward()
    return yy.grad, ss.grad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["laplace", "gaussian"])
def test_scale_bits_bwd(eng, kind):
    """dy and dscales of dcvc_scale_bits_bwd (get_y_laplace_bits / get_y_gaussian_bits with probs_to_bits' LowerBound),
    N = 3 samples of 4099 elements (sample boundaries inside a 256-thread block), upstream 1/pixels, -0.7 and 3e4.
    Includes the six elements r04 blamed for the per-tensor gap of the whole-picture test (y_bit ~ +-0.5001 with a
    negative, clamped scale): with identical inputs the kernel reproduces torch's arithmetic there."""
    import grad_check as G

    N, per = 3, 4099
    y, s, y64, s64, up, p64, b64, edge_y, lo = _scale_bits_case(kind, N, per)
    dy64, ds64 = _ref_scale_bits(y64, s64, up, N, per, kind, torch.float64)
    dy32, ds32 = _ref_scale_bits(y, s, up, N, per, kind, torch.float32)
    dyu, dsu = _ref_scale_bits(y64, s64, up, N, per, kind, torch.float64, bounded=False)
    L = eng.L
    yd, sd, gd = y.cuda(), s.cuda(), up.cuda()
    dy, ds = torch.full_like(yd, float("nan")), torch.full_like(yd, float("nan"))
    _ok(L.dcvc_scale_bits_bwd(_p(yd), _p(sd), _p(gd), _p(dy), _p(ds), kind, N, per, eng.stream()), "scale_bits_bwd")
    dy, ds = dy.cpu(), ds.cpu()
    upe = up.repeat_interleave(per)
    blocked = (b64 < 0) & (upe > 0)
    inside = (s64 >= lo) & (s64 <= 1e10)
    assert blocked.sum() >= N and (~inside).sum() > 100 and ((b64 < 0) & (upe < 0)).sum() >= N
    # tier A by construction: p >= 0.05 (each CDF value carries ~6e-8 of absolute rounding in fp32, so p = F1 - F0 has
    # ~1e-7 / p of relative error in any fp32 evaluation), |bits| >= 1e-4, the scale 1 % inside its clamp window
    tier_a = ~edge_y & (p64 >= 0.05) & (b64.abs() >= 1e-4) & (s64 >= lo * 1.01) & (s64 <= 1e10 / 1.01)
    # tier A per gradient also needs the two CDF terms not to cancel (at most 10-fold): a nearly flat density between
    # y - 0.5 and y + 0.5 amplifies any rounding difference in them
    cy, cs = _cdf_cancellation(y64, s64, kind, lo)
    tier_y, tier_s = tier_a & (cy <= 10), tier_a & (cs <= 10)
    # compared per sample (upstreams 1/pixels .. 3e4) and per tier (the edge elements near a clamped 1e-5 scale carry
    # gradients ~1e5 times the typical ones): every group against its own max|ref64|
    for k in range(N):
        for grp, sel in (("typical", tier_a), ("edge", ~tier_a)):
            m = sel.clone()
            m[: k * per] = False
            m[(k + 1) * per:] = False
            tag = f"scale_bits kind {kind} n={k} {grp}"
            G.assert_tiers(f"{tag} dy", dy[m], dy64[m], dy32[m], tier_y[m], zero=blocked[m], passes=~blocked[m],
                           unmasked=dyu[m])
            G.assert_tiers(f"{tag} dscales", ds[m], ds64[m], ds32[m], tier_s[m], zero=(blocked | ~inside)[m],
                           passes=(~blocked & inside)[m], unmasked=dsu[m])
    if kind == 0:  # the r04 elements themselves, by value
        n_fixed = len(R04_CHAOTIC) * 3
        i = torch.cat([torch.arange(n_fixed) + k * per for k in range(N)])
        ratio = (dy[i].double() - dy64[i]).abs() / (4 * (dy32[i].double() - dy64[i]).abs() + 1e-3 * dy64[i].abs() + 1e-30)
        print(f"r04 elements: dy worst {float(ratio.max()):.3g} of the tier-B bound, largest relative difference to "
              f"fp64 {float(((dy[i].double() - dy64[i]).abs() / dy64[i].abs()).max()):.2e}", flush=True)
        assert float(ratio.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. dcvc_factorized_bits_bwd
def _fact_block(w, name):
    return torch.stack([w[f"{name}.f{i}.{k}"].reshape(-1) for i in (1, 2, 3) for k in ("h", "b", "a")]
                       + [w[f"{name}.f4.h"].reshape(-1), w[f"{name}.f4.b"].reshape(-1)]).float().contiguous()


def _random_fact_block(C_, g):
    P = torch.randn(11, C_, generator=g)
    P[[0, 3, 6, 9]] = torch.rand(4, C_, generator=g) * 2 - 0.5
    P[0, 0], P[3, 0], P[6, 0], P[9, 0] = 22.0, 0.0, 0.0, 0.0      # softplus above its threshold of 20 (first layer)
    P[9, 1] = 21.0                                                 # ... in the last layer
    P[[2, 5, 8], 2] = 0.0                                          # a = 0: no tanh term
    P[[2, 5, 8], 3] = 1e-7                                         # a ~ 0
    P[[2, 5, 8], 4] = 9.0                                          # a large: tanh(a) rounds to 1 in fp32
    return P


def _ref_fact(z, P, up, dtype):
    """autograd of oracle z_bits summed per sample (NCHW z, (11, C) block) -> dz, dP."""
    z1, z0 = z.to(dtype).clone().requires_grad_(), z.to(dtype).clone().requires_grad_()
    Pr = P.to(dtype).clone().requires_grad_()
    rows = {}
    names = [f"f{i}.{k}" for i in (1, 2, 3) for k in ("h", "b", "a")] + ["f4.h", "f4.b"]
    for r, nm in enumerate(names):
        rows[f"e.{nm}"] = Pr[r].view(1, -1, 1, 1)
    # R.z_bits with the two CDF evaluations on separate leaves: dz is the sum of their gradients, and the ratio of the
    # terms' magnitudes to their sum is the element's cancellation
    c1, c0 = R.factorized_cdf(rows, "e", z1 + 0.5), R.factorized_cdf(rows, "e", z0 - 0.5)
    bits = R.probs_to_bits(c1 - c0)
    (bits.sum((1, 2, 3)) * up.to(dtype)).sum().backward()
    dz = z1.grad + z0.grad
    with torch.no_grad():
        p = c1 - c0
        edge = torch.minimum(torch.minimum(c1, 1 - c1), torch.minimum(c0, 1 - c0))
        cancel = (z1.grad.abs() + z0.grad.abs()) / dz.abs().clamp_min(1e-300)
    return dz, Pr.grad, p.detach(), (-torch.log(p + 1e-5) / math.log(2.0)).detach(), edge.detach(), cancel


@pytest.mark.gpu
@pytest.mark.parametrize("HW,Hs", [(1, 1), (300, 15), (510, 17)], ids=["hw1", "hw300", "hw17x30"])
def test_factorized_bits_bwd(eng, HW, Hs):
    """dz (strided, +=) and dparams (11, C, +=) of dcvc_factorized_bits_bwd for the oracle's bit_estimator_z and
    bit_estimator_z_mv blocks and one random block with softplus above its threshold, a = 0, a ~ 0 and a large; z holds
    integers, noisy values and tails at |z| >= 40; HW = 1, 300 (a remainder in the 256-stride loop) and 17 x 30 (the
    1080p hyper latent); N = 2 with upstream gradients of both signs.

    Documented conditioning: dz is the difference of the gradients through cdf(z + 0.5) and cdf(z - 0.5).  Where the two
    nearly cancel (their magnitudes exceed |dz| 100-fold: a flat density) or a CDF evaluation lies within 1e-2 of 0 or 1
    (1 - cdf on fp32's grid next to 1), fp32 rounding is amplified accordingly: torch's own fp32 autograd misses fp64 there
    by up to 7x the value on this data, and the kernel, whose device expf / tanhf round differently by an ulp, by 2.3e-3
    relative where torch's fp32 happened to land within 1.5e-4 -- beyond tier B's 4x of the fp32 miss.  Those elements
    (counted in the -s output) are checked for finiteness and the LowerBound mask only; every other dz element is held to
    the tiers, and dparams, which sum all elements' contributions, to tier B."""
    import grad_check as G
    from tests.util import oracle_weights

    w = oracle_weights("dmc")
    gen = torch.Generator().manual_seed(HW)
    blocks = [("z", _fact_block(w, "bit_estimator_z")), ("z_mv", _fact_block(w, "bit_estimator_z_mv")),
              ("random", _random_fact_block(8, gen))]
    N, Ws = 2, HW // Hs
    up = torch.tensor([0.37, -2.1])
    L = eng.L
    for nm, P in blocks:
        C_ = P.shape[1]
        z = torch.randint(-3, 4, (N, C_, Hs, Ws), generator=gen).float()
        r = torch.rand(N, C_, Hs, Ws, generator=gen)
        z[r < 0.5] += (torch.rand(N, C_, Hs, Ws, generator=gen) - 0.5)[r < 0.5]
        tail = r > 0.9
        z[tail] = (torch.randint(40, 70, (N, C_, Hs, Ws), generator=gen).float()
                   * (torch.randint(0, 2, (N, C_, Hs, Ws), generator=gen) * 2 - 1))[tail]
        if HW == 1:
            z[0, :, 0, 0] = 45.0
        dz64, dP64, p64, b64, edge, cancel = _ref_fact(z.double(), P.double(), up, torch.float64)
        dz32, dP32, _, b32, _, _ = _ref_fact(z, P, up, torch.float32)
        assert torch.equal(b32 >= 0, b64 >= 0)
        # device: z as channels [4, 4 + C) of a wider buffer, dz the same, both prefilled
        cs = C_ + 8
        zb = torch.randn(N, Hs, Ws, cs, generator=gen)
        zb[..., 4:4 + C_] = z.permute(0, 2, 3, 1)
        pre_z = (torch.rand(N, Hs, Ws, C_, generator=gen) * 2 - 1) * dz64.permute(0, 2, 3, 1).abs().float()
        dzb = torch.randn(N, Hs, Ws, cs, generator=gen)
        dzb[..., 4:4 + C_] = pre_z
        pre_P = ((torch.rand(11, C_, generator=gen) * 2 - 1) * dP64.abs()).float()
        zd, dzd, Pd, dPd, gd = zb.cuda(), dzb.cuda(), P.cuda(), pre_P.clone().cuda(), up.cuda()
        _ok(L.dcvc_factorized_bits_bwd(_p(zd) + 16, cs, _p(Pd), _p(gd), _p(dzd) + 16, cs, _p(dPd), N, HW, C_, eng.stream()),
            "factorized_bits_bwd")
        dzo = dzd.cpu()
        assert torch.equal(dzo[..., :4], dzb[..., :4]) and torch.equal(dzo[..., 4 + C_:], dzb[..., 4 + C_:])
        got_dz = (dzo[..., 4:4 + C_].double() - pre_z.double()).permute(0, 3, 1, 2)
        got_dP = dPd.cpu().double() - pre_P.double()
        upe = up.view(N, 1, 1, 1).expand_as(z)
        blocked = (b64 < 0) & (upe > 0)
        tier_a = (p64 >= 0.05) & (b64.abs() >= 1e-4) & (z.abs() < 40) & (edge >= 0.05) & (cancel <= 10)
        sat = (edge < 1e-2) | (cancel > 100)  # (see the docstring: compared by the branch masks and for finiteness only)
        print(f"factorized {nm} HW={HW}: {int(sat.sum())} of {sat.numel()} dz elements conditioning-limited", flush=True)
        assert torch.isfinite(got_dz).all()
        G.assert_tiers(f"factorized {nm} HW={HW} dz", got_dz[~sat], dz64[~sat], dz32[~sat], tier_a[~sat],
                       zero=blocked[~sat], passes=~blocked[~sat])
        assert bool((got_dz[sat & blocked] == 0).all())
        # dparams sum every element's contribution, the conditioning-limited ones included: tier B
        G.assert_tiers(f"factorized {nm} HW={HW} dparams", got_dP, dP64, dP32, torch.zeros_like(dP64, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------------
# 3. dcvc_dual_prior_bwd (steps 1 and 0) with q_finish; dcvc_scale_channels_bwd
QSTEP_EDGES = [-0.3, 0.2, 0.5, ulp_step(0.5, 0), ulp_step(0.5, 1), 1.7]


def _oracle_dual_prior(y, fusion, w1, b1, qb, qsc, Gout, Gres, Gsh, dtype):
    y, fusion = y.to(dtype).clone().requires_grad_(), fusion.to(dtype).clone().requires_grad_()
    w1, qb, qsc = w1.to(dtype).clone().requires_grad_(), qb.to(dtype).clone().requires_grad_(), qsc.to(dtype).clone().requires_grad_()
    orig = R.three_convs
    R.three_convs = lambda w, name, x, slope=0.2: F.conv2d(x, w1, b1.to(dtype))
    try:
        with R.training_mode():
            qs_, sc_, mu_ = fusion.chunk(3, 1)
            o = R.dual_prior({}, "x", y, mu_, sc_, qs_)
    finally:
        R.three_convs = orig
    cq = R.lower_bound(qb, 0.5)[None, :, None, None] * qsc[:, None, None, None]
    out = o["y_hat"] * cq
    loss = (out * Gout.to(dtype)).sum() + (o["y_res"] * Gres.to(dtype)).sum() + (o["scales_hat"] * Gsh.to(dtype)).sum()
    loss.backward()
    return dict(dy=y.grad, dfusion=fusion.grad, dw=w1.grad, dqb=qb.grad, dqs=qsc.grad), o


def _tie_free(y, fusion, w1, b1, C_):
    """Moves y away from rounding ties: y / q_step - mean at least 1e-3 from x.5 in both checkerboard passes."""
    for _ in range(20):
        with torch.no_grad():
            qs = fusion[:, :C_].double().clamp_min(0.5)
            orig = R.three_convs
            R.three_convs = lambda w, name, x, slope=0.2: F.conv2d(x, w1.double(), b1.double())
            try:
                o = R.dual_prior({}, "x", y.double(), fusion[:, 2 * C_:].double(), fusion[:, C_:2 * C_].double(),
                                 fusion[:, :C_].double())
            finally:
                R.three_convs = orig
            res = o["y_res"]  # y / q_step - mean of the pass that codes the element: what quant() rounds
            frac = (res - torch.floor(res) - 0.5).abs()
            bad = frac < 1e-3
        if not bad.any():
            return y
        y = y.clone()
        y[bad] += 0.0173 * qs[bad].float()
    raise AssertionError("could not move y off the rounding ties")


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
@pytest.mark.parametrize("C_,H,W", [(64, 9, 13), (96, 9, 13)], ids=["mv", "y"])
def test_dual_prior_bwd(eng, C_, H, W, sign):
    """Engine.dual_prior("enc", 0 / 1) recorded on a Tape around one 1x1 Engine.conv (4C -> 2C) in place of the spatial
    prior, then Tape.backward (dual_prior_bwd steps 1 and 0, the conv's backward, channel_dot into dq_mul, q_finish)
    against autograd of oracle.dual_prior under training_mode with the same 1x1 conv.  Odd H and W (both checkerboard
    phases start rows), y and fusion as channel slices of wider buffers, q_step values -0.3, 0.2, 0.5, 0.5 +- 1 ulp, 1.7,
    q_basic straddling 0.5 the same way; the loss is run with both signs so every clamped channel sees a positive and a
    negative total gradient."""
    import grad_check as G
    from vcm_ts_amd.grad import Tape

    N = 2
    gen = torch.Generator().manual_seed(C_ + H)
    fusion = torch.randn(N, 3 * C_, H, W, generator=gen)
    fusion[:, :C_] = torch.rand(N, C_, H, W, generator=gen) * 1.5 + 0.55
    fusion[:, C_:2 * C_] = fusion[:, C_:2 * C_].abs() * 2
    qe = torch.tensor(QSTEP_EDGES)
    sel = torch.rand(N, C_, H, W, generator=gen) < 0.25
    fusion[:, :C_][sel] = qe[torch.randint(0, len(qe), (int(sel.sum()),), generator=gen)]
    qb = torch.rand(C_, generator=gen) + 0.6
    qb[: 2 * len(QSTEP_EDGES)] = qe.repeat(2)
    qsc = torch.tensor([1.3, 0.8])
    w1 = torch.randn(2 * C_, 4 * C_, 1, 1, generator=gen) / math.sqrt(4 * C_)
    b1 = torch.randn(2 * C_, generator=gen) * 0.1
    y = torch.randn(N, C_, H, W, generator=gen) * 3
    y = _tie_free(y, fusion, w1, b1, C_)
    Gout = torch.randn(N, C_, H, W, generator=gen) * sign
    Gres = torch.randn(N, C_, H, W, generator=gen) * sign
    Gsh = torch.randn(N, C_, H, W, generator=gen) * sign
    r64, o64 = _oracle_dual_prior(y.double(), fusion.double(), w1.double(), b1.double(), qb.double(), qsc.double(), Gout,
                                  Gres, Gsh, torch.float64)
    r32, o32 = _oracle_dual_prior(y, fusion, w1, b1, qb, qsc, Gout, Gres, Gsh, torch.float32)
    assert torch.equal(o32["y_q"], o64["y_q"].float())  # the straight-through rounds agree between the precisions
    # ---- HIP: forward recorded on a tape
    e = eng
    dev = e.device
    tape = Tape(e)
    e.tape = tape
    try:
        yb = e.buf("bo.y", N, H, W, C_ + 8)
        yv = yb.slice(4, C_)
        e.from_nchw(y.to(dev), yv)
        fb = e.buf("bo.f", N, H, W, 3 * C_ + 8)
        fv = fb.slice(4, 3 * C_)
        e.from_nchw(fusion.to(dev), fv)
        qbp = torch.nn.Parameter(qb.to(dev))
        qsd = qsc.to(dev)
        tape.qstate("t", qbp, qsd, N, C_)
        wp, bp = torch.nn.Parameter(w1.to(dev)), torch.nn.Parameter(b1.to(dev))
        pk = e.pack(("bo.sp", C_, H, sign), wp, bp, (4 * C_,), False)
        params = e.buf("bo.params", N, H, W, 4 * C_)
        n = N * H * W * C_
        y_hat, y_q, y_res, sh = (torch.empty(n, device=dev) for _ in range(4))
        out = e.buf("bo.out", N, H, W, C_)
        common = dict(y=yv, fusion=fv, params=params, y_hat=y_hat, y_q=y_q, y_res=y_res, scales_hat=sh,
                      distribution="laplace", qkey="t")
        e.dual_prior("enc", 0, **common)
        spatial = e.buf("bo.spatial", N, H, W, 2 * C_)
        e.conv(pk, [params], spatial)
        e.dual_prior("enc", 1, spatial=spatial, out=out, q_basic=qbp, q_scale=qsd, **common)
    finally:
        e.tape = None
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().view(-1)
    assert torch.equal(y_q.cpu(), nhwc(o32["y_q"]))
    e.from_nchw(Gout.to(dev), tape.grad(out))
    tape.dense[y_res.data_ptr()] = nhwc(Gres).to(dev)
    tape.dense[sh.data_ptr()] = nhwc(Gsh).to(dev)
    tape.backward()
    got_dy = e.to_nchw(tape.grad(yv)).cpu()
    got_df = e.to_nchw(tape.grad(fv)).cpu()
    got_dw = tape.pgrads[id(wp)].cpu()
    got_dqb = tape.pgrads[id(qbp)].cpu()
    got_dqs = tape.q["t"]["dq_scale"].cpu()
    qsf = fusion[:, :C_]
    far = (qsf - 0.5).abs() > 0.005
    tier_y = far.clone()
    G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} dy", got_dy, r64["dy"], r32["dy"], tier_y)
    zq = (qsf < 0.5) & (r64["dfusion"][:, :C_] == 0)
    assert torch.equal(zq, (qsf < 0.5) & (r32["dfusion"][:, :C_] == 0))  # the LowerBound predicate agrees
    assert zq.any() and ((qsf < 0.5) & ~zq).any()
    G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} dfusion q_step", got_df[:, :C_], r64["dfusion"][:, :C_],
                   r32["dfusion"][:, :C_], far, zero=zq, passes=~zq)
    for k, nm in ((1, "scales"), (2, "means")):
        sl = slice(k * C_, (k + 1) * C_)
        G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} dfusion {nm}", got_df[:, sl], r64["dfusion"][:, sl],
                       r32["dfusion"][:, sl], far)
    G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} d 1x1 weight", got_dw, r64["dw"], r32["dw"],
                   torch.ones_like(got_dw, dtype=torch.bool))
    zb = (qb < 0.5) & (r64["dqb"] == 0)
    assert torch.equal(zb, (qb < 0.5) & (r32["dqb"] == 0))
    G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} dq_basic", got_dqb, r64["dqb"], r32["dqb"], (qb - 0.5).abs() > 0.005,
                   zero=zb, passes=~zb)
    G.assert_tiers(f"dual_prior C={C_} {sign:+.0f} dq_scale", got_dqs, r64["dqs"], r32["dqs"],
                   torch.ones_like(got_dqs, dtype=torch.bool))


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["pos", "neg"])
def test_scale_channels_bwd_and_q_finish(eng, sign):
    """Engine.scale_channels dividing by curr_q and multiplying by it (one q key), then Tape.backward
    (scale_channels_bwd, channel_dot into s_div / dq_mul, q_finish) against autograd of x / (lower_bound(q_basic, 0.5) *
    q_scale) and x * (...), with q_basic at -0.3, 0.2, 0.5, 0.5 +- 1 ulp and 1.7."""
    import grad_check as G
    from vcm_ts_amd.grad import Tape

    N, C_, H, W = 3, 96, 5, 7
    gen = torch.Generator().manual_seed(5)
    x1 = torch.randn(N, C_, H, W, generator=gen) * 2
    x2 = torch.randn(N, C_, H, W, generator=gen) * 2
    qb = torch.rand(C_, generator=gen) + 0.6
    qb[: 2 * len(QSTEP_EDGES)] = torch.tensor(QSTEP_EDGES).repeat(2)
    qsc = torch.tensor([1.3, 0.8, 0.55])
    G1, G2 = torch.randn(N, C_, H, W, generator=gen) * sign, torch.randn(N, C_, H, W, generator=gen) * sign

    def ref(dtype):
        a, b = x1.to(dtype).requires_grad_(), x2.to(dtype).requires_grad_()
        q, s = qb.to(dtype).requires_grad_(), qsc.to(dtype).requires_grad_()
        cq = R.lower_bound(q, 0.5)[None, :, None, None] * s[:, None, None, None]
        ((a / cq) * G1.to(dtype)).sum().add((b * cq * G2.to(dtype)).sum()).backward()
        return a.grad, b.grad, q.grad, s.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    e, dev = eng, eng.device
    tape = Tape(e)
    e.tape = tape
    try:
        v1 = e.from_nchw(x1.to(dev), e.buf("sc.x1", N, H, W, C_))
        v2 = e.from_nchw(x2.to(dev), e.buf("sc.x2", N, H, W, C_))
        qbp, qsd = torch.nn.Parameter(qb.to(dev)), qsc.to(dev)
        tape.qstate("s", qbp, qsd, N, C_)
        o1 = e.scale_channels(v1, e.buf("sc.o1", N, H, W, C_), qbp, qsd, multiply=False, qkey="s")
        o2 = e.scale_channels(v2, e.buf("sc.o2", N, H, W, C_), qbp, qsd, multiply=True, qkey="s")
    finally:
        e.tape = None
    e.from_nchw(G1.to(dev), tape.grad(o1))
    e.from_nchw(G2.to(dev), tape.grad(o2))
    tape.backward()
    ones = lambda t: torch.ones_like(t, dtype=torch.bool)
    G.assert_tiers(f"scale_channels {sign:+.0f} d(x / q)", e.to_nchw(tape.grad(v1)).cpu(), r64[0], r32[0], ones(x1))
    G.assert_tiers(f"scale_channels {sign:+.0f} d(x * q)", e.to_nchw(tape.grad(v2)).cpu(), r64[1], r32[1], ones(x2))
    zb = (qb < 0.5) & (r64[2] == 0)
    assert torch.equal(zb, (qb < 0.5) & (r32[2] == 0)) and zb.any() and ((qb < 0.5) & ~zb).any()
    G.assert_tiers(f"q_finish {sign:+.0f} dq_basic", tape.pgrads[id(qbp)].cpu(), r64[2], r32[2], (qb - 0.5).abs() > 0.005,
                   zero=zb, passes=~zb)
    G.assert_tiers(f"q_finish {sign:+.0f} dq_scale", tape.q["s"]["dq_scale"].cpu(), r64[3], r32[3], ones(qsc))


# ---------------------------------------------------------------------------------------------------------------------
# 4. dcvc_channel_dot
@pytest.mark.gpu
@pytest.mark.parametrize("C_", [3, 96, 200, 320])
def test_channel_dot(eng, C_):
    """out (+)= sum over pixels of a * b (or of a): over_batch 0 / 1, accumulate 0 / 1, b NULL / not, C = 3, 96, 200
    (idle thread groups), 320 (a second blockIdx.z chunk), HW = 1, 5, 100 000, strided a and b; against float64 sums,
    error <= 1e-6 of sum |a b| per channel.  Half the channels hold positive data, so that a result scaled by (1 + 1e-4)
    must fail."""
    N = 2
    L = eng.L
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(C_)
    r4 = (C_ + 3) // 4 * 4
    for HW in (1, 5, 100000):
        a_cs, b_cs = r4 + 4, r4 + 8
        a = torch.randn(N, HW, a_cs, generator=gen, device=dev)
        b = torch.randn(N, HW, b_cs, generator=gen, device=dev)
        a[..., : C_ // 2] = a[..., : C_ // 2].abs() + 0.1
        b[..., : C_ // 2] = b[..., : C_ // 2].abs() + 0.1
        a64, b64 = a[..., :C_].double().cpu(), b[..., :C_].double().cpu()
        scratch = torch.empty(N * 256 * r4, device=dev)
        for with_b in (False, True):
            prod = a64 * b64 if with_b else a64
            ref_n, mag_n = prod.sum(1), prod.abs().sum(1)
            for over_batch in (0, 1):
                ref, mag = (ref_n.sum(0), mag_n.sum(0)) if over_batch else (ref_n, mag_n)
                for accumulate in (0, 1):
                    pre = torch.randn(ref.shape, dtype=torch.float64) * 0.25
                    out = pre.float().to(dev) if accumulate else torch.full(ref.shape, float("nan"), device=dev)
                    _ok(L.dcvc_channel_dot(_p(a), a_cs, _p(b) if with_b else None, b_cs if with_b else 0, _p(out), _p(scratch),
                                           N, HW, C_, over_batch, accumulate, eng.stream()), "channel_dot")
                    want = ref + (pre.float().double() if accumulate else 0)
                    bound = 1e-6 * mag + 1e-7 * (pre.abs() if accumulate else 0) + 1e-30
                    got = out.cpu().double()
                    err = float(((got - want).abs() / bound).max())
                    print(f"channel_dot C={C_} HW={HW} b={int(with_b)} over_batch={over_batch} acc={accumulate}: "
                          f"worst {err:.3g} of the bound", flush=True)
                    assert err <= 1.0, (HW, with_b, over_batch, accumulate, err)
                    # teeth: the dot product scaled by (1 + 1e-4) is seen on the positive channels
                    base = pre.float().double() if accumulate else 0.0
                    scaled = base + (got - base) * (1 + 1e-4)
                    assert float(((scaled - want).abs() / bound).max()) > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. dcvc_se_bwd + dcvc_add_channel_vec
def _se_sizes():
    from vcm_ts_amd.params import dmc_spec

    return sorted({tuple(v) for k, v in dmc_spec().items() if k.endswith("fc.0.weight")}) + [(64, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("Cr,C_", _se_sizes())
def test_se_bwd_and_add_channel_vec(eng, Cr, C_):
    """dmean, dw1, dw2 (accumulated into prefilled buffers) of dcvc_se_bwd, and dcvc_add_channel_vec's broadcast of
    dmean / HW into dt, against autograd of sigmoid(W2 relu(W1 mean)); N = 4 at the production sizes and at the kernel's
    limits (C = 256, Cr = 64).  One row of W1 is zero: that hidden unit sits exactly on the ReLU kink and gets no
    gradient, as in torch."""
    import grad_check as G

    N, H, W = 4, 3, 5
    gen = torch.Generator().manual_seed(Cr * 1000 + C_)
    mean = torch.randn(N, C_, generator=gen)
    w1 = torch.randn(Cr, C_, generator=gen) / math.sqrt(C_)
    w1[1] = 0.0
    w2 = torch.randn(C_, Cr, generator=gen) / math.sqrt(Cr)
    dgate = torch.randn(N, C_, generator=gen)

    def ref(dtype):
        m, a, b = (t.to(dtype).clone().requires_grad_() for t in (mean, w1, w2))
        gate = torch.sigmoid(F.linear(F.relu(F.linear(m, a)), b))
        gate.backward(dgate.to(dtype))
        return m.grad, a.grad, b.grad, gate.detach()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    gate = r32[3]
    pre1 = (torch.rand(Cr, C_, generator=gen) * 2 - 1) * r64[1].abs().float()
    pre2 = (torch.rand(C_, Cr, generator=gen) * 2 - 1) * r64[2].abs().float()
    L, dev = eng.L, eng.device
    md, w1d, w2d, gd, dgd = (t.contiguous().to(dev) for t in (mean, w1, w2, gate, dgate))
    dmean = torch.full((N, C_), float("nan"), device=dev)
    dw1, dw2 = pre1.clone().to(dev), pre2.clone().to(dev)
    _ok(L.dcvc_se_bwd(_p(md), _p(w1d), _p(w2d), _p(gd), _p(dgd), _p(dmean), _p(dw1), _p(dw2), N, C_, Cr, eng.stream()),
        "se_bwd")
    cs = (C_ + 3) // 4 * 4 + 4
    dt0 = torch.randn(N, H * W, cs, generator=gen)
    dt = dt0.clone().to(dev)
    _ok(L.dcvc_add_channel_vec(_p(dt), cs, _p(dmean), 1.0 / (H * W), N, H * W, C_, eng.stream()), "add_channel_vec")
    hid = F.linear(mean.double(), w1.double())
    kink = (hid == 0).expand(N, Cr)
    ones = lambda t: torch.ones_like(t, dtype=torch.bool)
    G.assert_tiers(f"se_bwd C={C_} Cr={Cr} dmean", dmean.cpu(), r64[0], r32[0], ones(mean))
    got1 = dw1.cpu().double() - pre1.double()
    z1 = torch.zeros_like(got1, dtype=torch.bool)
    z1[1] = True
    assert bool((r64[1][1] == 0).all()) and bool(kink[:, 1].all())
    G.assert_tiers(f"se_bwd C={C_} Cr={Cr} dw1", got1, r64[1], r32[1], ones(got1), zero=z1)
    G.assert_tiers(f"se_bwd C={C_} Cr={Cr} dw2", dw2.cpu().double() - pre2.double(), r64[2], r32[2], ones(pre2))
    dto = dt.cpu()
    assert torch.equal(dto[..., C_:], dt0[..., C_:])
    want64 = dt0[..., :C_].double() + (r64[0] / (H * W))[:, None, :]
    want32 = dt0[..., :C_].double() + (r32[0].double() / (H * W))[:, None, :]
    G.assert_tiers(f"add_channel_vec C={C_}", dto[..., :C_], want64, want32, ones(want64))


# ---------------------------------------------------------------------------------------------------------------------
# 6. dcvc_maxpool2_bwd
@pytest.mark.gpu
def test_maxpool2_bwd_ties_and_nan_bit_exact(eng):
    """dcvc_maxpool2_bwd on integer-valued inputs (ties), all-zero windows and windows with one or two NaNs, strided src
    and dsrc, += onto a prefilled dsrc: bit-exact against F.max_pool2d's backward on the CPU (first maximum in scan
    order, any NaN replaces the current pick)."""
    N, C_, H, W = 2, 13, 10, 14
    gen = torch.Generator().manual_seed(6)
    x = torch.randint(-2, 3, (N, C_, H, W), generator=gen).float()
    x[:, :, 0:2, 0:2] = 0.0
    x[0, 0, 2, 2] = float("nan")
    x[0, 1, 3, 3] = float("nan")
    x[0, 2, 2, 3], x[0, 2, 3, 2] = float("nan"), float("nan")
    x[1, 3, 4, 4], x[1, 3, 5, 5] = float("nan"), float("nan")
    x[1, 4, 4, 5], x[1, 4, 5, 4] = float("nan"), 7.0
    dout = torch.randn(N, C_, H // 2, W // 2, generator=gen)
    xr = x.clone().requires_grad_()
    F.max_pool2d(xr, 2).backward(dout)
    pre = torch.randn(N, C_, H, W, generator=gen)
    want = pre + xr.grad
    L, dev = eng.L, eng.device
    s_cs, d_cs, o_cs = C_ + 3, C_ + 7, C_ + 1
    src = torch.randn(N, H, W, s_cs, generator=gen)
    src[..., :C_] = x.permute(0, 2, 3, 1)
    ds0 = torch.randn(N, H, W, d_cs, generator=gen)
    ds0[..., :C_] = pre.permute(0, 2, 3, 1)
    dob = torch.randn(N, H // 2, W // 2, o_cs, generator=gen)
    dob[..., :C_] = dout.permute(0, 2, 3, 1)
    sd, dsd, dod = src.to(dev), ds0.clone().to(dev), dob.to(dev)
    _ok(L.dcvc_maxpool2_bwd(_p(sd), s_cs, _p(dod), o_cs, _p(dsd), d_cs, N, H, W, C_, eng.stream()), "maxpool2_bwd")
    got = dsd.cpu()
    assert torch.equal(got[..., C_:], ds0[..., C_:])
    assert torch.equal(got[..., :C_].permute(0, 3, 1, 2), want)
    # teeth: the tie order matters on this data (the "last maximum" rule gives other bits)
    xl = x.flip(-1).flip(-2).clone().requires_grad_()
    F.max_pool2d(xl, 2).backward(dout)
    assert not torch.equal(pre + xl.grad.flip(-1).flip(-2), want)


# ---------------------------------------------------------------------------------------------------------------------
# 7. dcvc_mask_accumulate, dcvc_sq_err_bwd
@pytest.mark.gpu
@pytest.mark.parametrize("slope", [0.01, 0.0])
def test_mask_accumulate_signed_zero_and_denormal(eng, slope):
    """dst += src * (x > 0 ? 1 : slope) for x = +0.0, -0.0, the smallest positive subnormal, +-1e-30 and random values:
    within 1 ulp of the correctly rounded fp32 fma(src, m, dst), with torch's x > 0 (a subnormal is positive)."""
    n, C_ = 257, 12
    gen = torch.Generator().manual_seed(7)
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    special = torch.tensor([0.0, -0.0, tiny, -tiny, 1e-30, -1e-30], dtype=torch.float32)
    x = torch.randn(n, C_, generator=gen)
    sel = torch.rand(n, C_, generator=gen) < 0.5
    x[sel] = special[torch.randint(0, len(special), (int(sel.sum()),), generator=gen)]
    x[0, : len(special)] = special
    src = torch.randn(n, C_, generator=gen)
    dst0 = torch.randn(n, C_, generator=gen)
    m = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
    assert bool((x[0, 2] > 0)) and not bool(x[0, 0] > 0)
    want = (src.double() * m.double() + dst0.double()).float()
    L, dev = eng.L, eng.device
    xs, ss = C_ + 4, C_ + 8
    xb = torch.zeros(n, xs)
    xb[:, :C_] = x
    sb = torch.zeros(n, ss)
    sb[:, :C_] = src
    sd, xd, db = sb.to(dev), xb.to(dev), dst0.clone().to(dev)
    _ok(L.dcvc_mask_accumulate(_p(sd), ss, _p(xd), xs, slope, _p(db), C_, n, C_, eng.stream()), "mask_accumulate")
    got = db.cpu()
    sp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    err = (got.double() - want.double()).abs()
    assert bool((err <= sp.double()).all()), (got[err > sp.double()][:4], want[err > sp.double()][:4],
                                               x[err > sp.double()][:4])
    assert torch.equal(got[0, 2], want[0, 2])  # the subnormal: mask 1, not slope


@pytest.mark.gpu
def test_sq_err_bwd_strided_accumulate(eng):
    """da += 2 (a - b) g[n]: strided a, b and da, N = 3 with a different g per sample, onto a prefilled da."""
    import grad_check as G

    N, H, W, C_ = 3, 7, 9, 5
    gen = torch.Generator().manual_seed(8)
    a = torch.randn(N, H * W, C_ + 3, generator=gen)
    b = torch.randn(N, H * W, C_ + 7, generator=gen)
    g = torch.tensor([0.25, -3.0, 1e-4])
    pre = torch.randn(N, H * W, C_ + 1, generator=gen)

    def ref(dtype):
        aa = a[..., :C_].to(dtype).clone().requires_grad_()
        ((aa - b[..., :C_].to(dtype)) ** 2).sum((1, 2)).mul(g.to(dtype)).sum().backward()
        return aa.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    L, dev = eng.L, eng.device
    ad, bd, dd, gd = a.to(dev), b.to(dev), pre.clone().to(dev), g.to(dev)
    _ok(L.dcvc_sq_err_bwd(_p(ad), C_ + 3, _p(bd), C_ + 7, _p(gd), _p(dd), C_ + 1, N, H * W, C_, eng.stream()), "sq_err_bwd")
    got = dd.cpu()
    assert torch.equal(got[..., C_:], pre[..., C_:])
    G.assert_tiers("sq_err_bwd", got[..., :C_].double() - pre[..., :C_].double(), r64, r32,
                   torch.ones_like(r64, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------------
# 8. dcvc_conv2d's mask epilogue (out_act 3) and its argument check
@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", [(1, 20, 36), (8, 96, 128)], ids=["rows4", "rows8"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_conv_mask_epilogue_matches_fp64(eng, eng_split, N, H, W, with_res):
    """out = (conv(x) + b) * (res2 > 0 ? 1 : slope) [+ res] with res2 holding exact zeros, -0.0 and negatives, in both
    arithmetic modes, on a launch small enough for the 4-row tiles and on one that takes the 8-row tiles."""
    Cin, Cout, ks, slope = 32, 64, 3, 0.1
    gen = torch.Generator().manual_seed(N * 10 + int(with_res))
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, ks, ks, generator=gen) / math.sqrt(Cin * ks * ks)
    b = torch.randn(Cout, generator=gen) * 0.1
    r2 = torch.randn(N, Cout, H, W, generator=gen)
    sel = torch.rand(N, Cout, H, W, generator=gen)
    r2[sel < 0.2] = 0.0
    r2[(sel >= 0.2) & (sel < 0.4)] = -0.0
    res = torch.randn(N, Cout, H, W, generator=gen) if with_res else None
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    scale = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    want = conv * torch.where(r2 > 0, 1.0, slope).double() + (res.double() if with_res else 0.0)
    for e, tol in ((eng, 2e-6), (eng_split, 2e-5)):
        pk = e.pack(("maskepi", N, with_res), torch.nn.Parameter(w.to(e.device)), torch.nn.Parameter(b.to(e.device)), (Cin,),
                    False)
        xv = e.from_nchw(x.to(e.device), e.buf("me.x", N, H, W, Cin))
        r2v = e.from_nchw(r2.to(e.device), e.buf("me.r2", N, H, W, Cout))
        rv = e.from_nchw(res.to(e.device), e.buf("me.res", N, H, W, Cout)) if with_res else None
        out = e.buf("me.out", N, H, W, Cout)
        out.base.fill_(float("nan"))
        e.conv(pk, [xv], out, out_slope=("mask", slope), res=rv, res2=r2v)
        got = e.to_nchw(out).cpu().double()
        err = float(((got - want).abs() / (tol * scale + 1e-30)).max())
        print(f"conv mask epilogue {e.precision} N={N} {H}x{W} res={with_res}: worst {err:.3g} of the bound", flush=True)
        assert err <= 1.0, (e.precision, err)
        # teeth: an exact zero (or -0.0) of the mask source taken as positive would be seen
        alt = conv * torch.where(r2 >= 0, 1.0, slope).double() + (res.double() if with_res else 0.0)
        assert float(((got - alt).abs() / (tol * scale + 1e-30)).max()) > 1.0


@pytest.mark.gpu
def test_conv2d_refuses_bad_mask_epilogue_arguments(eng):
    """dcvc_conv2d returns DCVC_E_ARG for out_act outside 0..3, for out_act 3 without res2, and for out_act 3 together
    with res_gate, chan_partial or pixel_shuffle.  Every buffer is a real device allocation large enough for any reading
    of the arguments, so a regression of the check shows as a wrong status, never as a launch on bad pointers."""
    from vcm_ts_amd import lib

    N, H, W, Cin, Cout = 1, 8, 32, 16, 32
    dev = eng.device
    pk = eng.pack(("refuse", Cin, Cout), torch.nn.Parameter(torch.randn(Cout, Cin, 3, 3, device=dev) * 0.1),
                  torch.nn.Parameter(torch.zeros(Cout, device=dev)), (Cin,), False)
    big = N * (2 * H) * (2 * W) * Cout
    x = torch.randn(N * H * W * Cin, device=dev)
    out, res, res2 = (torch.zeros(big, device=dev) for _ in range(3))
    gate = torch.ones(N * Cout, device=dev)
    parts = int(eng.L.dcvc_conv_chan_partial_parts(3, 1, H, W))
    cp = torch.zeros(N * max(parts, 1) * pk.Cout_pad, device=dev)

    def args(**kw):
        a = lib.ConvArgs()
        a.seg[0].ptr, a.seg[0].C, a.seg[0].cs = x.data_ptr(), Cin, Cin
        a.nseg, a.N, a.Hin, a.Win = 1, N, H, W
        a.wpack, a.bpack = pk.w.data_ptr(), pk.b.data_ptr()
        a.ks, a.stride, a.Cout, a.Cout_pad = 3, 1, Cout, pk.Cout_pad
        a.out, a.out_cs = out.data_ptr(), Cout
        a.res2, a.res2_cs = res2.data_ptr(), Cout
        a.out_act, a.out_slope, a.precision = 3, 0.1, pk.precision
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    run = lambda a: int(eng.L.dcvc_conv2d(C.byref(a), eng.stream()))
    assert run(args()) == 0  # the valid mask epilogue
    assert run(args(res=res.data_ptr(), res_cs=Cout)) == 0
    refused = {"out_act -1": args(out_act=-1), "out_act 4": args(out_act=4), "out_act 99": args(out_act=99),
               "out_act 3 without res2": args(res2=None, res2_cs=0),
               "out_act 3 with res_gate": args(res=res.data_ptr(), res_cs=Cout, res_gate=gate.data_ptr()),
               "out_act 3 with chan_partial": args(chan_partial=cp.data_ptr()),
               "out_act 3 with pixel_shuffle": args(pixel_shuffle=1)}
    for what, a in refused.items():
        assert run(a) == -1, what
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
