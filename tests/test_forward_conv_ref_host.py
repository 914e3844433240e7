"""The properties tests/test_gpu_conv_exact.py relies on, shown on the references alone (no GPU).

Exact families: float64 == fp32 == fp32 on the flipped problem == the split-fp16 arithmetic in float64, bit for bit.

The split-fp16 bound (kernel_common.h "split-fp16 mode", dcvc_hip.h "Arithmetic of dcvc_conv2d").  With X = 8 x and
W = 64 w, hi = fp16(X) and lo = fp16(X - hi):
    |X - hi| <= 2^-11 |X|                       (11-bit significand, round to nearest)   or <= 2^-25 where hi is subnormal
    |X - hi - lo| <= 2^-11 |X - hi| <= 2^-22 |X|                                        or <= 2^-25 where lo is subnormal
so the represented operand x~ = (hi + lo) / 8 has |x - x~| <= max(2^-22 |x|, 2^-28), and likewise |w - w~| <=
max(2^-22 |w|, 2^-31).  The kernels form xh.wh + xh.wl + xl.wh = X~ W~ - xl.wl, hence per product
    |x w - (xh.wh + xh.wl + xl.wh) / 512| <= |x - x~||w| + |x~||w - w~| + |xl||wl| / 512
                                          <= (2^-22 |x| + 2^-28)|w| + |x|(2^-22 |w| + 2^-31) + 2^-22 |x w|   (+ 2nd order)
                                           = 3 2^-22 |x w| + 2^-28 |w| + 2^-31 |x|                           (+ 2nd order).
The second-order terms (|x~| instead of |x|, the subnormal-hi case of |xl|) are below 2^-10 of the first-order ones;
forward_conv_ref.split_bound multiplies by 1 + 2^-10 for them.  Measured: |split64 - ref64| reaches 0.43 (1x1 40->33) and
0.35 (1x1 64->32) of that bound, 0.13 .. 0.21 on the 3x3 and 7x7 cases: the documents' figures hold.  The fp32 constant c of
test_float_bounds_have_teeth came out as 58.5, 13.9, 20.1, 11.4, 14.2, 61.2 for forward_conv_ref.FLOAT_CASES in order."""
import numpy as np
import pytest
import torch

from tests import backward_ref as BR
from tests import forward_conv_ref as FR

HOST_CASES = [
    dict(seg_C=(24,), Cout=24, ks=3, stride=1, H=13, W=37),
    dict(seg_C=(16, 24), Cout=40, ks=3, stride=2, H=26, W=75, out_act=1, out_slope=0.25, res=True, gate=True),
    dict(seg_C=(24,), Cout=33, ks=7, stride=1, H=13, W=37, in_slope=0.25, res=True, res2=True),
    dict(seg_C=(40,), Cout=96, ks=1, stride=2, H=26, W=75, ps=True, out_act=1, out_slope=0.5),
    dict(seg_C=(64, 32, 32), Cout=64, ks=3, stride=1, H=13, W=37, out_act=3, out_slope=0.25, res=True, res2=True),
    dict(seg_C=(16,), Cout=2, ks=7, stride=1, H=13, W=37, out_act=2),
]


def split_forward(c):
    """the layer with split64 in place of the convolution, float64"""
    x = torch.cat(c["xs"], 1)
    y = FR.split64(x, c["w"], c["b"], c["ks"], c["stride"], c["in_slope"])
    return FR.epilogue(y, c, torch.float64)


@pytest.mark.parametrize("family", FR.FAMILIES)
@pytest.mark.parametrize("i", range(len(HOST_CASES)))
def test_exact_families_do_not_depend_on_order_or_precision(i, family):
    kw = dict(HOST_CASES[i])
    if family == "sub":
        kw = {k: v for k, v in kw.items() if k in ("seg_C", "Cout", "ks", "stride", "H", "W", "ps")}
    if family != "int" and kw["ks"] == 7:
        kw.pop("in_slope", None)  # a slope of 1/4 on the 2^-10 grid leaves a 24-channel 7x7 sum no headroom
    c = FR.exact_case(family, seed=i, **kw)
    assert c["headroom"] > 1
    want = FR.forward(c).float()
    assert want.abs().max() > 0
    BR.assert_bits(FR.forward(c, torch.float32), want, f"fp32 {family} {i}", "n,c,y,x")
    f, back = FR.flipped(c)
    BR.assert_bits(back(FR.forward(f, torch.float32)), want, f"fp32 flipped {family} {i}", "n,c,y,x")
    BR.assert_bits(back(FR.forward(f)).float(), want, f"fp64 flipped {family} {i}", "n,c,y,x")
    # the split-fp16 arithmetic loses nothing on these data: hi + lo is the operand, the dropped xl.wl is zero
    got = split_forward(c)
    assert torch.equal(got, FR.forward(c)), f"split64 {family} {i}"


def test_grid_families_carry_lo_parts_and_the_subnormal_family_is_subnormal():
    g = torch.Generator().manual_seed(1)
    uniform = torch.randint(-4096, 4097, (100000,), generator=g).float() * FR.GRID
    assert 0.2 < FR.lo_share(uniform, FR.ACT_SCALE) < 0.3  # what the generators' assertion of >= 1/2 guards against
    cx = FR.exact_case("gridx", (24,), 24, 3, 1, 13, 37)
    cw = FR.exact_case("gridw", (24,), 24, 3, 1, 13, 37)
    assert FR.lo_share(torch.cat(cx["xs"], 1), FR.ACT_SCALE) >= 0.5 and FR.lo_share(cx["w"], FR.WGT_SCALE) == 0
    assert FR.lo_share(cw["w"], FR.WGT_SCALE) >= 0.5 and FR.lo_share(torch.cat(cw["xs"], 1), FR.ACT_SCALE) == 0
    # dropping the lo planes changes the result: these families see them
    hi_only = FR.split64(torch.cat(cx["xs"], 1), cx["w"], cx["b"], 3, 1, x_lo=False)
    assert float((hi_only != FR.forward(cx)).double().mean()) > 0.9
    # the 7x7 cases lower the integer operand instead of losing exactness
    assert FR.exact_case("gridx", (24,), 32, 7, 1, 13, 37)["imax"] < BR.VMAX
    cs = FR.exact_case("sub", (24,), 24, 3, 1, 13, 37)
    xs = torch.cat(cs["xs"], 1)
    assert float(xs.abs().max()) * 8 <= 2.0 ** -14 and float(FR.forward(cs).abs().max()) > 0


@pytest.mark.parametrize("ks,Cin,Cout", FR.FLOAT_CASES, ids=lambda v: str(v))
def test_split64_is_within_the_documented_bound_of_float64(ks, Cin, Cout):
    d = FR.float_case(ks, Cin, Cout)
    bound = FR.split_bound(d["x"], d["w"], ks, 1)
    err = (d["split"] - d["ref64"]).abs()
    print(f"k{ks} {Cin}->{Cout}: worst |split64 - ref64| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert float((err / bound).max()) > 0.01  # the bound is not vacuous


@pytest.mark.parametrize("ks,Cin,Cout", FR.FLOAT_CASES, ids=lambda v: str(v))
def test_float_bounds_have_teeth(ks, Cin, Cout):
    """c comes from torch's fp32 CPU convolution against float64 -- never from a kernel.  The bound c 2^-24 M_e around
    split64 (what the GPU test demands of every split-fp16 kernel) and around ref64 (fp32 mode) must reject a kernel that
    reduces x to its hi part, one that flushes subnormal lo parts to zero, and one that drops a single product."""
    d = FR.float_case(ks, Cin, Cout)
    x, w, b, M = d["x"], d["w"], d["b"], d["M"]
    c = BR.fp32_constant(d["ref32"], d["ref64"], M)
    bound = c * 2.0 ** -24 * M
    print(f"k{ks} {Cin}->{Cout}: c = {c:.2f}; image magnitudes {d['xm'].tolist()}")
    assert 1.0 < c < 64.0
    for name, bad in (("x without lo", FR.split64(x, w, b, ks, 1, x_lo=False)),
                      ("subnormal lo flushed", FR.split64(x, w, b, ks, 1, flush_subnormal_lo=True))):
        over = (bad - d["split"]).abs() > bound
        assert bool(over.any()), name
        print(f"   {name}: {int(over.sum())} of {over.numel()} elements beyond the bound")
    # one dropped product: the largest term of output (n, co, y, x) = (1, 0, 8, 20), for both references
    n, co, y, xx = 1, 0, 8, 20
    pad = ks // 2
    xp = torch.nn.functional.pad(x.double(), (pad, pad, pad, pad))
    prod = xp[n, :, y:y + ks, xx:xx + ks] * w.double()[co]
    drop = float(prod.flatten()[prod.abs().argmax()])
    for ref in (d["split"], d["ref64"]):
        assert abs(drop) > float(bound[n, co, y, xx]), (drop, float(bound[n, co, y, xx]))
    # and the honest candidates pass: fp32 CPU against float64, split64 against itself
    assert bool(((d["ref32"].double() - d["ref64"]).abs() <= bound).all())


def test_split_f16_is_the_host_packers_split():
    """forward_conv_ref.split_f16 (numpy's conversion) against split_f16 of kernel_common.h as the plain host packer applies
    it: the hi and lo planes of a one-tap 16-channel layer, bit for bit, incl. values whose lo is an fp16 subnormal"""
    import ctypes as C

    from vcm_ts_amd import lib

    L = lib.hip()
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(32, 16, 1, 1, generator=g) * torch.tensor([1e-6, 1e-3, 1.0, 500.0]).repeat(4).view(1, 16, 1, 1)).clamp(-1000, 1000)
    wn = w.numpy()
    segs = (C.c_int32 * 1)(16)
    cp = C.c_int32(0)
    total = L.dcvc_conv_pack_size(32, 1, 1, segs, C.byref(cp))
    wp, bp = np.zeros(total, np.float32), np.zeros(cp.value, np.float32)
    assert L.dcvc_conv_pack_weights(wn.ctypes.data, None, 32, 1, 1, segs, 0, 1, wp.ctypes.data, bp.ctypes.data) == 0
    rows = wp.view(np.float16).reshape(4, 32, 8)  # [hi h0, hi h1, lo h0, lo h1][n][jj]
    hi, lo = FR.split_f16(w[:, :, 0, 0], FR.WGT_SCALE)
    got_hi = np.concatenate([rows[0], rows[1]], 1).astype(np.float64)
    got_lo = np.concatenate([rows[2], rows[3]], 1).astype(np.float64)
    assert np.array_equal(got_hi, hi) and np.array_equal(got_lo, lo)
    assert (np.abs(lo[lo != 0]) < 2.0 ** -14).any()


def test_engine_refuses_a_non_finite_weight_in_split_fp16_mode():
    """The plain packer keeps a NaN weight (tests/test_pack_host.py), conv_mfma's range guard drops a NaN output and the
    next split-fp16 layer's clamp on load would turn it into a finite number: a broken checkpoint must fail at packing.
    fp32 mode keeps propagating the NaN as the reference does.  (_pack_host is host code: no GPU needed.)"""
    from vcm_ts_amd import lib
    from vcm_ts_amd.engine import Engine

    e = Engine.__new__(Engine)
    e.L, e.device = lib.hip(), torch.device("cpu")
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = torch.ones(32, 16, 3, 3)
        w[3, 5, 1, 1] = bad
        e.precision = "fp16x3"
        for variant, ww, segs in (("mfma", w, (16,)), ("small", w[:16], (16,)), ("k32", torch.cat([w, w], 1), (32,))):
            with pytest.raises(lib.KernelError):
                e._pack_host(variant, "bad", ww, None, segs, False, None, 0)
        e.precision = "fp32"
        pk = e._pack_host("mfma", "bad", w, None, (16,), False, None, 0)
        assert int((~torch.isfinite(pk.w)).sum()) == 1
    e.precision = "fp16x3"
    e._pack_host("mfma", "good", torch.ones(32, 16, 3, 3), None, (16,), False, None, 0)


# =====================================================================================================================
# fp32 mode as an fmaf chain
def _round_fraction_to_f32(v):
    """round-to-nearest-even of an exact Fraction to fp32 (normal range), by integer arithmetic"""
    from fractions import Fraction

    if v == 0:
        return np.float32(0.0)
    sign, v = (-1 if v < 0 else 1), abs(v)
    e = 0
    while v >= 2 ** 24:
        v, e = v / 2, e + 1
    while v < 2 ** 23:
        v, e = v * 2, e - 1
    n = v.numerator // v.denominator
    rem = v - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** e))


def test_fma32_is_the_correctly_rounded_fma():
    """forward_conv_ref.fma32 against exact rational arithmetic: random triples, triples with heavy cancellation, and
    constructed ones whose float64 sum lands exactly on an fp32 tie with a non-zero remainder on either side -- the case a
    plain float64 multiply-add-round gets wrong"""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    n = 1500
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    c[::3] = -(a[::3] * b[::3]) * (1 + rng.integers(-3, 4, len(c[::3])) * 2.0 ** -23)  # cancellation
    t = 2.0 ** -23
    ties = []
    for s in (1.0, -1.0):
        for k in (0.0, 1.0, 2.0, 3.0):
            for db in (-t, t):
                # a b = +-(64 - 2^-40) or +-(64 + 2^-16 ...): around the tie 2^30 + k 2^7 + 2^6 of fp32 numbers 2^7 apart
                ties.append((s * 8 * (1 + t), 8 * (1 + db), s * (2.0 ** 30 + k * 2.0 ** 7)))
                ties.append((s * 8 * (1 - t), 8 * (1 + db), s * (2.0 ** 30 + k * 2.0 ** 7)))
    ta, tb, tc = (np.array(v, np.float32) for v in zip(*ties))
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = FR.fma32(a, b, c)
    want = np.array([_round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive != want).any()  # the constructed ties do fool the double rounding


@pytest.mark.parametrize("i", range(len(FR.CHAIN_CASES)), ids=lambda i: "k%ds%d" % FR.CHAIN_CASES[i][:2])
def test_fmaf_chain_is_a_convolution(i):
    """the chain is the layer: bit for bit the float64 result on exact data (so no tap, channel or segment is missed or
    doubled), and within 2^-24 (n + 1) M_e of float64 on the float data, n = Cin ks^2 roundings"""
    ks, stride, seg_C, Cout = FR.CHAIN_CASES[i]
    H, W = (13, 37) if stride == 1 else (26, 75)
    c = FR.exact_case("int", seg_C, Cout, ks, stride, H, W, N=1, seed=i)
    BR.assert_bits(FR.fmaf_chain(c["xs"], c["w"], c["b"], ks, stride), FR.forward(c).float(), f"chain on integers {i}", "n,c,y,x")
    layer, chain, ref64, M = FR.chain_case(i)
    err = (chain.double() - ref64).abs()
    assert bool((err <= 2.0 ** -24 * (sum(seg_C) * ks * ks + 1) * M).all()) and float(err.max()) > 0
