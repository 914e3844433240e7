"""The non-convolution forward kernels (csrc/resample.hip, the elementwise and reduction part of
csrc/entropy_kernels.hip) element by element against tests/forward_ref.py, on a real MI355X.

Every operand is a View into a WIDER buffer -- a channel slice at offset 4 (16-byte aligned) or 1 / 3 (not), with a
channel stride that differs from operand to operand -- as the product uses these kernels (nets.py writes up2 into
v.slice(6, 2)).  The whole base buffer of every output is filled with NaN before the launch; afterwards every element
of the view must be a number that matches the reference and every element outside the view's channels must still be
NaN.  Inputs are written with torch indexing, results are read from the base buffer: no kernel under test carries
another's data.  Bit-for-bit where forward_ref says the value is one IEEE operation deep; otherwise within the bounds
derived there (no tolerance here comes from what the kernels return)."""
import numpy as np
import pytest
import torch

from oracle import dcvc_ref as R
from tests import forward_ref as FR

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from vcm_ts_amd.engine import Engine

    return Engine("cuda:0")


def wide(eng, name, shape, off, pad=8, cs=None):
    """an (N, C, H, W) view at channel offset `off` of a NaN-filled (N, H, W, C + pad) buffer"""
    N, C, H, W = shape
    full = eng.buf(name, N, H, W, C + pad, cs=cs)
    full.base.fill_(NAN)
    return full.slice(off, C) if (off or pad) else full


def put(eng, name, x, off, pad=8, cs=None):
    """`wide` holding x (numpy or torch NCHW), written by torch"""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    v = wide(eng, name, tuple(x.shape), off, pad, cs)
    v.nchw().copy_(x.to(v.base.device))
    return v


def read(v, may_be_inf=False):
    """the view's content as NCHW numpy, after checking that the launch left every other channel of the base NaN and
    wrote a number to every element of the view"""
    torch.cuda.synchronize()
    b = v.base.cpu().numpy()
    inside = np.ascontiguousarray(b[..., v.coff:v.coff + v.C].transpose(0, 3, 1, 2))
    outside = np.delete(b, np.s_[v.coff:v.coff + v.C], axis=3)
    assert np.isnan(outside).all(), f"{v}: wrote outside its channels"
    assert not np.isnan(inside).any() if may_be_inf else np.isfinite(inside).all(), f"{v}: left elements unwritten"
    return inside


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {np.unravel_index(bad[0], got.shape)}: " \
                          f"{got.ravel()[bad[0]]!r} != {want.ravel()[bad[0]]!r}"


def assert_within(got, want64, bound, what=""):
    err = np.abs(got.astype(np.float64) - want64)
    assert err.shape == np.shape(want64), (what, got.shape, np.shape(want64))
    bound = np.broadcast_to(bound, err.shape)
    bad = err > bound
    worst = np.unravel_index((err - bound).argmax(), err.shape)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} beyond the bound, worst at {worst}: got {got[worst]!r}, " \
                          f"want {want64[worst]!r}, error {err[worst]:.3e} > {bound[worst]:.3e}"


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).numpy()


# ---- up2 / down2 / maxpool2 / copy --------------------------------------------------------------------------
@pytest.mark.parametrize("with_out2", [False, True], ids=["out", "out+out2"])
@pytest.mark.parametrize("shape", [(2, 2, 5, 7), (1, 3, 1, 1), (1, 2, 1, 9), (2, 67, 6, 5)], ids=str)
def test_up2_matches_fp64_and_out2_holds_the_same_bits(eng, shape, with_out2):
    """dcvc_up2 = F.interpolate(x2, bilinear, align_corners=False) * scale, per element within 8 * 2^-24 * |scale| *
    max|four taps| of fp64 (forward_ref.interp_bound), for scale 1, 2 (SpyNet's flow) and 0.3; one-pixel pictures
    and rows, more than one block (2 x 67 x 12 x 10 outputs); out2 has its own channel stride and offset."""
    N, C, H, W = shape
    x = rnd(shape, 10 + C, 3.0)
    src = put(eng, "up/src", x, 3, pad=5)
    for scale in (1.0, 2.0, 0.3):
        out = wide(eng, "up/out", (N, C, 2 * H, 2 * W), 4, pad=8)
        out2 = wide(eng, "up/out2", (N, C, 2 * H, 2 * W), 1, pad=16) if with_out2 else None
        assert out2 is None or out2.cs > out.cs
        eng.up2(src, out, scale=scale, out2=out2)
        got = read(out)
        assert_within(got, FR.up2(x, scale), FR.interp_bound(scale, FR.up2_tap_max(x)), f"up2 x{scale}")
        if with_out2:
            assert_bits(read(out2), got, f"up2 out2 x{scale}")


DOWN_SHAPES = [(2, 3, 6, 10), (1, 2, 2, 2), (2, 64, 4, 6)]


@pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "avgpool"])
@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=str)
def test_down2_matches_the_documented_fp32_order_bit_for_bit(eng, shape, mode):
    """dcvc_down2 in both orders of include/dcvc_hip.h: with scale 1 and 0.5 (the product's) the fp32 value is
    independent of FMA contraction (products with 0.5 are exact), so every bit is demanded; scale 0.3 within the
    interpolation bound of fp64."""
    N, C, H, W = shape
    x = rnd(shape, 20 + C + mode, 3.0)
    src = put(eng, "dn/src", x, 1, pad=7)
    for scale in (1.0, 0.5, 0.3):
        out = wide(eng, "dn/out", (N, C, H // 2, W // 2), 4, pad=4)
        eng.down2(src, out, scale=scale, avgpool_order=bool(mode))
        got = read(out)
        if scale != 0.3:
            assert_bits(got, FR.down2_f32(x, scale, mode), f"down2 mode {mode} x{scale}")
        assert_within(got, FR.down2(x, scale, mode), FR.interp_bound(scale, FR.down2_tap_max(x)), f"down2 mode {mode} x{scale}")


@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=str)
def test_maxpool2_bit_for_bit_with_ties_signed_zeros_and_infinities(eng, shape):
    """nn.MaxPool2d(2): values drawn from a small set, so most 2x2 blocks hold ties, blocks of only zeros of both
    signs (+0 is the maximum, forward_ref.fmax) and infinities.  NaN inputs are not part of this test."""
    N, C, H, W = shape
    vals = np.array([-np.inf, -1.5, -0.0, 0.0, 0.0, -0.0, 1.0, 2.0, np.inf], dtype=F32)
    idx = torch.randint(0, len(vals), shape, generator=torch.Generator().manual_seed(30 + C)).numpy()
    x = vals[idx]
    x[0, 0, :2, :2] = [[-0.0, 0.0], [-0.0, -0.0]]   # mixed zeros, either order
    x[0, 1, :2, :2] = [[0.0, -0.0], [-0.0, -0.0]]
    x[-1, -1, -2:, -2:] = -0.0                         # only negative zeros: stays -0
    out = wide(eng, "mp/out", (N, C, H // 2, W // 2), 3, pad=5)
    eng.maxpool2(put(eng, "mp/src", x, 4, pad=8), out)
    assert_bits(read(out, may_be_inf=True), FR.maxpool2(x), "maxpool2")


@pytest.mark.parametrize("npix", [1, 255, 257])
@pytest.mark.parametrize("C", [1, 3, 64])
def test_copy_channels_bit_for_bit(eng, C, npix):
    """Engine.copy (dcvc_copy_channels) between two slices with different strides and offsets; 255 / 257 pixels of
    one channel sit on either side of the 256-thread block."""
    x = rnd((1, C, 1, npix), 40 + C)
    out = wide(eng, "cp/out", (1, C, 1, npix), 4, pad=12)
    eng.copy(put(eng, "cp/src", x, 1, pad=3), out)
    assert_bits(read(out), x, "copy")


# ---- layout -------------------------------------------------------------------------------------------------
LAYOUT_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (10, 20)]  # 1, 63, 64, 65, 200 pixels: the 64-pixel LDS tile and its edges


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_layout_conversions_bit_for_bit(eng, C):
    """dcvc_nchw_to_nhwc into an offset slice and dcvc_nhwc_to_nchw out of one, each on its own: channel counts
    around the 64-channel pass of the LDS tile, pixel counts around its 64 pixels, two images."""
    for H, W in LAYOUT_HW:
        x = rnd((2, C, H, W), C + H)
        v = wide(eng, "ly/in", x.shape, 1, pad=7)
        eng.from_nchw(torch.from_numpy(x).cuda(), v)
        assert_bits(read(v), x, f"from_nchw {H}x{W}")
        back = eng.to_nchw(put(eng, "ly/out", x, 3, pad=6))
        assert_bits(back.cpu().numpy(), x, f"to_nchw {H}x{W}")


def test_to_nchw_clamp01(eng):
    """to_nchw(clamp01=True), the last step of every decoded picture: [0, 1] with -0.0 and tiny negatives to +0,
    1 + ulp and inf to 1, everything inside untouched -- bit for bit."""
    one_up, one_dn = np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))
    special = np.array([-0.0, 0.0, 1.0, one_up, one_dn, -1e-30, 1e-30, np.inf, -np.inf, 0.5, -3.0, 7.0], dtype=F32)
    x = (torch.rand((2, 3, 9, 15), generator=torch.Generator().manual_seed(50)) * 2 - 0.5).numpy()
    x.reshape(-1)[:: 7][: 2 * len(special)] = np.tile(special, 2)
    x.reshape(-1)[-len(special):] = special
    v = put(eng, "cl/in", x, 4, pad=4)
    assert_bits(eng.to_nchw(v, clamp01=True).cpu().numpy(), FR.clamp01(x), "clamp01")
    assert_bits(eng.to_nchw(v).cpu().numpy(), x, "no clamp")


# ---- warp ---------------------------------------------------------------------------------------------------
def _warp_case(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    im = torch.randn(2, C, H, W, generator=g)
    fl = torch.randn(2, 2, H, W, generator=g) * 30  # mostly out of the picture -> border clamp
    fl[:, :, : H // 2] *= 0.05                       # and sub-pixel motion in the upper half
    return im, fl, R.warp(im, fl).numpy()


def _warp_err(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-20))


@pytest.mark.parametrize("H,W", [(7, 5), (9, 31)])
@pytest.mark.parametrize("C,off,cs", [(3, 1, None), (6, 4, None), (8, 0, 9), (8, 1, None)],
                         ids=["C3", "C6", "C8-stride9", "C8-offset1"])
def test_warp_scalar_path(eng, C, off, cs, H, W):
    """warp_scalar: taken when C is no multiple of 4, when a channel stride is no multiple of 4 floats, or when a
    slice offset breaks the 16-byte alignment -- each within the 3e-6 of R.warp the vector path is held to."""
    im, fl, want = _warp_case(C, H, W, 60 + C + H)
    pad = 0 if cs else 8
    src = put(eng, "ws/src", im, off, pad=pad, cs=cs)
    out = wide(eng, "ws/out", im.shape, off, pad=pad, cs=cs)
    assert C % 4 or src.cs % 4 or src.ptr % 16 or out.ptr % 16  # the scalar path's condition (resample.hip: dcvc_warp)
    eng.warp(src, put(eng, "ws/fl", fl, 1, pad=4), out)
    assert _warp_err(read(out), want) < 3e-6


@pytest.mark.parametrize("H,W", [(7, 5), (9, 31)])
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 24])
def test_warp_vector_paths_in_strided_views(eng, C, H, W):
    """The wave-shuffle kernels (C / 4 = 2, 4, 8, 16, 32 lanes per pixel) and warp_vec4 (C = 24) on views at channel
    offset 4 of buffers with stride C + 8: within 3e-6 of R.warp, and -- no tolerance -- bit-identical to the same
    picture and flow through dense aligned views (the same kernel; the view must not enter the result)."""
    im, fl, want = _warp_case(C, H, W, 70 + C + H)
    src = put(eng, "wv/src", im, 4, pad=8)
    out = wide(eng, "wv/out", im.shape, 4, pad=8)
    assert src.cs == C + 8 and src.ptr % 16 == 0 and out.ptr % 16 == 0
    eng.warp(src, put(eng, "wv/fl", fl, 1, pad=4), out)
    got = read(out)
    assert _warp_err(got, want) < 3e-6
    dense = wide(eng, "wv/dense", im.shape, 0, pad=0)
    eng.warp(put(eng, "wv/dsrc", im, 0, pad=0), put(eng, "wv/dfl", fl, 0, pad=0), dense)
    assert_bits(read(dense), got, "dense against strided view")


# ---- squeeze-excitation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 7, 2047, 2049, 5000])
@pytest.mark.parametrize("C", [4, 16, 64, 256])
def test_channel_mean_is_exact_and_se_gate_matches_fp64(eng, C, HW):
    """dcvc_channel_mean on small integers (uniform in [-8, 8]): every partial sum in every order is exact, so the
    mean must be float32(exact sum) / float32(HW) to the bit -- a dropped or doubled pixel cannot hide.  C sets the
    pixels per pass (256 / (C / 4)), HW < 2048 leaves blocks empty, 2049 and 5000 give 2 and 3 pixels to a block.
    Then dcvc_se_gate with Cr = 1, 4, 16 against the fp64 gate of that mean within rtol 1e-5, atol 1e-6 (the bound of
    test_se_gate): W1 ~ N(0, 1) / (8 sqrt C) and W2 ~ N(0, 1) / sqrt Cr keep both sums O(1), where C fp32 products
    and sums, expf and the division err by a few 1e-7 of a gate in (0, 1)."""
    N = 2
    g = torch.Generator().manual_seed(C + HW)
    xi = torch.randint(-8, 9, (N, C, 1, HW), generator=g)
    exact = xi.sum(dim=(2, 3)).numpy()
    want_mean = exact.astype(F32) / F32(HW)
    assert np.abs(exact).max() < 2 ** 24
    t = put(eng, "cm/t", xi.float(), 4, pad=8)
    for Cr in (1, 4, 16):
        w1 = torch.randn(Cr, C, generator=g) / (8.0 * C ** 0.5)
        w2 = torch.randn(C, Cr, generator=g) / Cr ** 0.5
        name = f"cm/{Cr}"
        eng.fbuf(name + ".mean", N * C).fill_(NAN)
        eng.fbuf(name + ".gate", N * C).fill_(NAN)
        gate = eng.se_gate(name, t, w1.cuda(), w2.cuda())
        mean = eng.fbuf(name + ".mean", N * C).cpu().numpy().reshape(N, C)
        assert_bits(mean, want_mean, f"channel mean C={C} HW={HW}")
        want = FR.se_gate(mean, w1.numpy(), w2.numpy())
        got = gate.cpu().numpy().reshape(N, C)
        assert np.isfinite(got).all()
        assert_within(got, want, 1e-6 + 1e-5 * np.abs(want), f"gate Cr={Cr}")
    assert_bits(read(t), xi.float().numpy(), "the input")  # untouched, and the NaN around it too


# ---- quantisation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multiply", [False, True], ids=["divide", "multiply"])
@pytest.mark.parametrize("C,HW", [(2, 1), (2, 35), (96, 1), (96, 35)])
def test_scale_channels_bit_for_bit(eng, C, HW, multiply):
    """y / curr_q and y_hat * curr_q with q = max(q_basic[c], 0.5) * q_scale[n]: one fp32 multiply for q, then one
    IEEE divide or multiply per element; three samples with three q_scale, q_basic on both sides of 0.5, exactly
    0.5, its two neighbours and a negative value."""
    N = 3
    x = rnd((N, C, 1, HW), 80 + C + HW, 5.0)
    if C == 2:
        qb = np.array([[-1.0, 0.8], [0.5, 0.3]][HW > 1], dtype=F32)
    else:
        qb = np.linspace(0.2, 1.3, C).astype(F32)
        qb[:4] = [0.5, -1.0, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))]
    qs = np.array([0.7, 1.0, 1.9], dtype=F32)
    out = wide(eng, "sc/out", x.shape, 1, pad=3)
    qb_d, qs_d = torch.from_numpy(qb).cuda(), torch.from_numpy(qs).cuda()
    eng.scale_channels(put(eng, "sc/src", x, 4, pad=8), out, qb_d, qs_d, multiply=multiply)
    assert_bits(read(out), FR.scale_channels(x, qb, qs, multiply), "scale_channels")


def _rounding_values():
    half = np.arange(-6, 6).astype(F32) + F32(0.5)  # every k + 0.5, k in [-6, 6)
    v = np.concatenate([half, np.nextafter(half, F32(np.inf)), np.nextafter(half, F32(-np.inf)),
                        np.array([0.0, -0.0, 2.0 ** 23, -(2.0 ** 23)], dtype=F32)])
    assert v.size == 40
    return v


@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (1, 64, 4, 6)], ids=str)
def test_round_symbols_and_symbols_to_nhwc(eng, shape):
    """torch.round + .int() into (n, c, y, x) symbol planes and back: N > 1, H != W, strided views on both sides.
    Values: every tie k + 0.5 in [-6, 6) (half to even) with both neighbours, zeros of both signs, +-2^23, and
    N(0, 3) in between.  All three forms (z_hat + sym, z_hat only, sym only); the planes lie between guard words that
    must survive."""
    N, C, H, W = shape
    n = N * C * H * W
    z = rnd(shape, 90 + C, 3.0)
    special = _rounding_values()
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(C))[: 3 * special.size].numpy()
    z.reshape(-1)[pos] = np.tile(special, 3)
    want_zh, want_sym = FR.round_half_even(z), FR.symbols(z)
    zv = put(eng, "rs/z", z, 3, pad=5)
    guard, mark = 1024, 0x5A5A5A5A
    assert guard >= H * W

    def planes():
        big = torch.full((guard + n + guard,), mark, dtype=torch.int32, device="cuda")
        return big, big[guard: guard + n]

    def check_planes(big, what):
        got = big.cpu().numpy()
        assert (got[:guard] == mark).all() and (got[guard + n:] == mark).all(), what
        np.testing.assert_array_equal(got[guard: guard + n].reshape(N, C, H, W), want_sym, err_msg=what)

    big, sym = planes()
    zh = wide(eng, "rs/zh", shape, 1, pad=7)
    eng.round_symbols(zv, zh, sym)
    assert_bits(read(zh), want_zh, "z_hat (with sym)")
    check_planes(big, "sym (with z_hat)")
    zh = wide(eng, "rs/zh", shape, 1, pad=7)
    eng.round_symbols(zv, zh, None)
    assert_bits(read(zh), want_zh, "z_hat alone")
    big2, sym2 = planes()
    eng.round_symbols(zv, None, sym2)
    check_planes(big2, "sym alone")
    back = wide(eng, "rs/back", shape, 4, pad=4)
    eng.symbols_to_nhwc(sym, back)
    assert_bits(read(back), FR.symbols_to_float(want_sym), "symbols_to_nhwc")
    check_planes(big, "sym after the way back")
    assert_bits(read(zv), z, "the input")


# ---- rate and distortion ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_scale_bits_per_element(eng, kind):
    """dcvc_scale_bits with per_sample = 1 and N = 4096: every output is ONE element's bits, so a wrong clamp or tail
    cannot hide in a sum.  Inputs: forward_ref.rate_grid (symbols -60 .. 60; scales at and around the clamps 1e-5 and
    0.11, negative, zero, up to 64; the tails where p underflows and bits = -log2(1e-5); and y = +-(0.5 +- a few 1e-5)
    at the clamped scales, where the Laplace clamp decides p -- at integer symbols it does not, see rate_grid and
    test_forward_ref_host.py::test_rate_grid_tells_a_wrong_scale_clamp).  Against fp64 within
    k 2^-24 / ((p64 + 1e-5) ln 2) + 4 2^-24 want64, where k is TWICE the fp32 oracle's own largest |p32 - p64| / 2^-24
    on these inputs and those of the sum tests below (torch CPU, tests/test_forward_ref_host.py; twice because the
    device's expm1f / erff / tanhf are not the host's to the last ulp):
        measured  Laplace 1.802   Gaussian 2.215   factorised 2.857
        k         Laplace 3.7     Gaussian 4.5     factorised 5.8"""
    y, s = FR.rate_grid()
    want, p64 = (FR.gaussian_bits if kind == "gaussian" else FR.laplace_bits)(y, s)
    got = eng.scale_bits(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), y.size, 1, gaussian=kind == "gaussian")
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    assert_within(got, want, FR.rate_bound(p64, want, FR.RATE_K[kind]), f"{kind} bits per element")


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_scale_bits_sum_over_three_trips_of_the_stride_loop(eng, kind):
    """per_sample = 2 * 1024 * 256 + 77, N = 2: each of the 1024 blocks of a sample goes round its grid-stride loop
    two or three times and the last trip is ragged.  Against the fp64 sum within the sum of the per-element bounds
    plus n 2^-24 of the sum for the summation (k as in test_scale_bits_per_element): a dense sum first, then a sparse
    one in which a dropped first or last element of a trip cannot hide."""
    y, s = FR.rate_sum_inputs()
    want, p64 = (FR.gaussian_bits if kind == "gaussian" else FR.laplace_bits)(y, s)
    got = eng.scale_bits(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), 2, y.shape[1], gaussian=kind == "gaussian")
    got = got.cpu().numpy().astype(np.float64)
    for n in range(2):
        bound = FR.rate_sum_bound(p64[n], want[n], FR.RATE_K[kind])
        print(f"[{kind} sum {n}] got {got[n]:.3f} want {want[n].sum():.3f} bound {bound:.3f}")
        assert abs(got[n] - want[n].sum()) <= bound
    # That bound is 3 % of a dense sum, where a trip's first or last element can hide.  So once more with every element
    # worth exactly 0 bits (y = 0 at the smallest scale: p + 1e-5 > 1) except the first and the last element of each
    # trip of the loop and of the first block: the same bound formula is now a fraction of ONE element's bits.
    per = y.shape[1]
    y, s = np.zeros_like(y), np.full_like(s, 1e-5)
    edges = [0, 255, 256, 1024 * 256 - 1, 1024 * 256, 2 * 1024 * 256 - 1, 2 * 1024 * 256, per - 1]
    y[:, edges], s[:, edges] = 3.0, 1.0
    want, p64 = (FR.gaussian_bits if kind == "gaussian" else FR.laplace_bits)(y, s)
    assert np.count_nonzero(want[0]) == len(edges)
    got = eng.scale_bits(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), 2, per, gaussian=kind == "gaussian")
    got = got.cpu().numpy().astype(np.float64)
    for n in range(2):
        bound = FR.rate_sum_bound(p64[n], want[n], FR.RATE_K[kind])
        print(f"[{kind} sparse sum {n}] got {got[n]:.5f} want {want[n].sum():.5f} bound {bound:.5f}")
        assert bound < 0.5 * want[n, edges].min()
        assert abs(got[n] - want[n].sum()) <= bound


@pytest.fixture(scope="module")
def z_block():
    from tests.util import oracle_weights
    from vcm_ts_amd import entropy as E

    return E.factorized_param_block(E.factorized_params(oracle_weights("dmc"), "bit_estimator_z")).numpy()


@pytest.mark.parametrize("c", FR.FACTORIZED_CHANNELS)
def test_factorized_bits_per_element(eng, z_block, c):
    """dcvc_factorized_bits with the (11, 1) parameter block of ONE channel, C = 1, HW = 1 and N = 81: each output is
    the bits of one symbol in -40 .. 40 under that channel's factorised prior; bound as test_scale_bits_per_element
    (k = 5.8)."""
    z = FR.factorized_grid()
    blk = np.ascontiguousarray(z_block[:, c: c + 1])
    want, p64 = FR.factorized_bits(z, blk)
    got = eng.factorized_bits(put(eng, "fb/z1", z, 3, pad=5), torch.from_numpy(blk).cuda()).cpu().numpy()
    assert np.isfinite(got).all()
    assert_within(got, want.reshape(-1), FR.rate_bound(p64, want, FR.RATE_K["factorized"]).reshape(-1), f"channel {c}")


def test_factorized_bits_sums_in_a_strided_view(eng, z_block):
    """C = 64 with HW = 1 and 300, N = 2, the latent a slice of a wider buffer: per-sample sums against fp64 within the
    summed per-element bounds plus n 2^-24 of the sum."""
    for z in FR.factorized_latents():
        want, p64 = FR.factorized_bits(z, z_block)
        got = eng.factorized_bits(put(eng, "fb/z", z, 4, pad=8), torch.from_numpy(z_block).cuda()).cpu().numpy()
        for n in range(z.shape[0]):
            bound = FR.rate_sum_bound(p64[n], want[n], FR.RATE_K["factorized"])
            print(f"[factorized sum HW={z.shape[2] * z.shape[3]} {n}] got {got[n]:.4f} want {want[n].sum():.4f} bound {bound:.4f}")
            assert abs(float(got[n]) - want[n].sum()) <= bound


@pytest.mark.parametrize("C,HW", [(3, 1), (3, 600), (64, 1), (64, 600)])
def test_sq_err_is_exact_on_integers(eng, C, HW):
    """dcvc_sq_err on integer-valued operands in [-4, 4]: every square and every partial sum is an integer below
    2^24, so the result must be the exact integer sum in any order; different strides and offsets per operand.
    Then the LAST element of one operand moves by 1: the sum must move with it (a dropped tail element shows)."""
    N = 2
    g = torch.Generator().manual_seed(C + HW)
    a = torch.randint(-4, 5, (N, C, 1, HW), generator=g)
    b = torch.randint(-4, 5, (N, C, 1, HW), generator=g)
    b[:, -1, 0, -1] = a[:, -1, 0, -1]  # (so that the move below changes the sum by exactly 1)
    for step in (0, 1):
        a2 = a.clone()
        a2[1, -1, 0, -1] += step
        want = ((a2 - b) ** 2).sum(dim=(1, 2, 3)).numpy()
        assert want.max() < 2 ** 24
        got = eng.sq_err(put(eng, "sq/a", a2.float(), 1, pad=3), put(eng, "sq/b", b.float(), 4, pad=8)).cpu().numpy()
        assert_bits(got, want.astype(F32), f"sq_err step {step}")
