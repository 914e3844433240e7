"""tests/backward_ref.py checked on the CPU alone: every exact generator's float64 gradient, cast to fp32, is
bit-identical to torch's fp32 autograd of the same problem AND of the problem with batch / pixel order reversed
(order-independence shown on the references, before any kernel is involved); the magnitude reference M of the
float-valued bounds against a brute-force loop; the teeth of those bounds; and torch's grid_sample backward against the
documented floor / mask convention at the planted integer, border and out-of-picture positions."""
import numpy as np
import pytest
import torch

from tests import backward_ref as BR

# the epilogues of tests/test_gpu_backward.py::CONV_CASES on small shapes, the odd stride-2 sizes, slopes {0, .25, .5}
HOST_CONV = [
    dict(seg_C=(8,), Cout=8, ks=3, stride=1, H=6, W=9, out_slope=0.25, res=True),
    dict(seg_C=(5,), Cout=7, ks=3, stride=2, H=7, W=9, out_slope=0.5),
    dict(seg_C=(5,), Cout=7, ks=3, stride=2, H=6, W=9, out_slope=0.0),
    dict(seg_C=(6,), Cout=4, ks=1, stride=2, H=7, W=6),
    dict(seg_C=(4, 4), Cout=8, ks=1, stride=1, H=5, W=6, res=True, gate=True),
    dict(seg_C=(3,), Cout=5, ks=7, stride=1, H=9, W=10, out_slope=0.0, res=True),
    dict(seg_C=(6,), Cout=16, ks=3, stride=1, H=4, W=5, out_slope=0.25, ps=True),
    dict(seg_C=(6,), Cout=8, ks=3, stride=1, H=5, W=5, in_slope=0.25, out_slope=0.5, res=True, res2=True),
    dict(seg_C=(3, 2, 4), Cout=6, ks=3, stride=1, H=4, W=6, out_slope=0.5),
    dict(seg_C=(6,), Cout=5, ks=3, stride=1, H=4, W=6, out_slope=0.25, cin_slice=(2, 8, 11)),
]


@pytest.mark.parametrize("i", range(len(HOST_CONV)))
def test_exact_conv_reference_is_order_independent(i):
    c = BR.conv_exact(seed=i, **HOST_CONV[i])
    assert c["headroom"] > 1
    r64, r32 = BR.conv_backward(c, torch.float64), BR.conv_backward(c, torch.float32)
    f, back = BR.conv_flipped(c)
    rf = back(BR.conv_backward(f, torch.float32))
    assert set(r64) == set(r32) == set(rf)
    for k in r64:
        BR.assert_bits(r32[k], r64[k], f"case {i} {k} fp32 vs fp64", BR.conv_axes(k))
        BR.assert_bits(rf[k], r64[k], f"case {i} {k} flipped fp32 vs fp64", BR.conv_axes(k))
    # the plants are there: pre-activations of exactly 0 (even channels, top-left corner), and gradients that are not 0
    if c["out_slope"] is not None and not c["ps"] and c["res"] is None:
        assert bool((r64["out"][0, ::2, 0, 0] == 0).all())
    assert float(r64["dw"].abs().max()) > 0 and float(r64["dx0"].abs().max()) > 0


def test_generator_rejects_data_that_would_not_be_exact():
    with pytest.raises(AssertionError):
        BR._headroom({"dw": (BR.TWO24 * 0.25, 0.25)})
    assert BR._headroom({"dw": (BR.TWO24 * 0.25 - 1, 0.25)}) > 1


@pytest.mark.parametrize("ks,stride,H,W,in_slope", [(1, 1, 5, 7, None), (3, 1, 5, 7, 0.25), (7, 1, 4, 9, None),
                                                     (3, 2, 7, 9, 0.0), (3, 2, 6, 9, None), (1, 2, 7, 6, None),
                                                     (3, 1, 1, 1, None)])
def test_exact_wgrad_reference_is_order_independent(ks, stride, H, W, in_slope):
    x, d = BR.wgrad_exact(5, 6, ks, stride, H, W, N=2, in_slope=in_slope, seed=ks + H)
    (w64, b64), (w32, b32) = BR.wgrad(x, d, ks, stride, in_slope), BR.wgrad(x, d, ks, stride, in_slope, torch.float32)
    wf, bf = BR.wgrad(x.flip([0]).flip([1]), d.flip([0]), ks, stride, in_slope, torch.float32)
    BR.assert_bits(w32, w64.float(), "dw fp32 vs fp64", "co,ci,ky,kx")
    BR.assert_bits(wf.flip([1]), w64.float(), "dw batch/channel-flipped fp32 vs fp64", "co,ci,ky,kx")
    BR.assert_bits(b32, b64.float(), "db", "co")
    BR.assert_bits(bf, b64.float(), "db flipped", "co")
    assert torch.equal(w64, w64.float().double())  # the fp64 value itself is an fp32 number


def test_magnitude_reference_against_a_brute_force_loop():
    for ks, stride, H, W in ((3, 1, 4, 5), (3, 2, 5, 4), (1, 2, 3, 4), (7, 1, 3, 4)):
        x, dy = BR.wgrad_float(3, 2, ks, H, W, 2, 1.0, seed=ks)
        if stride == 2:
            Ho, Wo = BR.conv_geometry(ks, 2, H, W)
            dy = dy[:, :, :Ho, :Wo]
        M = BR.wgrad_magnitude(x, dy, ks, stride).numpy()
        np.testing.assert_allclose(M, BR.wgrad_magnitude_brute(x, dy, ks, stride), rtol=1e-12, atol=0)


@pytest.mark.parametrize("mag", BR.DY_MAGS)
@pytest.mark.parametrize("ks,C,Cout", BR.FLOAT_CASES)
def test_float_bounds_have_teeth(ks, C, Cout, mag):
    """The per-element bounds of the float-valued weight-gradient test, built from the references alone, reject a kernel
    that lost its hi.lo term (X rounded to bf16), one that lost lo.hi (dY rounded to bf16) and one that dropped a single
    product -- under the LOOSER of the two bounds (fp16x3: 2^-16 M_e + c 2^-24 M_e)."""
    x, dy, ref64, ref32, M = BR.float_case(ks, C, Cout, mag)
    c = BR.fp32_constant(ref32, ref64, M)
    print(f"ks {ks} {C}->{Cout} |dY|~{mag:g}: c = {c:.3f}")
    assert 0 < c < 64  # (2^-16 / 2^-24 = 256: the fp32 term must stay a small part of the fast bound)
    bound = (2.0 ** -16 + c * 2.0 ** -24) * M
    assert bool(((ref32.double() - ref64).abs() <= c * 2.0 ** -24 * M).all())
    lost_x = BR.wgrad(BR.bf16_round(x), dy, ks, 1)[0]
    lost_d = BR.wgrad(x, BR.bf16_round(dy), ks, 1)[0]
    assert bool(((lost_x - ref64).abs() > bound).any()), "X rounded to bf16 passes the bound"
    assert bool(((lost_d - ref64).abs() > bound).any()), "dY rounded to bf16 passes the bound"
    idx = (Cout - 1, C // 2, ks // 2, ks // 2)
    assert abs(BR.largest_product(x, dy, ks, 1, idx)) > float(bound[idx]), "a dropped product passes the bound"


# ---------------------------------------------------------------------------------------------------------------------
WARP_HOST = [(1, 1, 3, 3), (3, 2, 3, 5), (8, 2, 5, 9), (24, 1, 9, 3), (5, 2, 17, 5), (2, 1, 33, 17), (130, 1, 5, 5)]


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -30, 2.0 ** 14], ids=["x1", "x2^-30", "x2^14"])
@pytest.mark.parametrize("C,N,H,W", WARP_HOST)
def test_exact_warp_reference_is_order_independent_and_follows_the_documented_convention(C, N, H, W, scale):
    d = BR.warp_exact(C, N, H, W, seed=C + H, dout_scale=scale)
    assert d["headroom"] > 1
    s64, f64 = BR.warp_backward(d["src"], d["flow"], d["dout"])
    s32, f32 = BR.warp_backward(d["src"], d["flow"], d["dout"], torch.float32)
    (fs, ff, fd), back = BR.warp_flipped(d)
    sf, ffl = back(*BR.warp_backward(fs, ff, fd, torch.float32))
    # (mirrored in x, a position exactly on an integer line takes its one-sided x derivative from the other side: the
    # floor convention is not mirror-symmetric there, so those x components are not part of the flipped comparison)
    ix0 = BR.warp_positions(d["flow"])[0]
    ffl = ffl.clone()
    ffl[:, 0] = torch.where(ix0 == ix0.round(), f64[:, 0].float(), ffl[:, 0])
    for got, want, what, ax in ((s32, s64, "dsrc fp32", "n,c,y,x"), (f32, f64, "dflow fp32", "n,xy,y,x"),
                                (sf, s64, "dsrc flipped", "n,c,y,x"), (ffl, f64, "dflow flipped", "n,xy,y,x")):
        BR.assert_bits(got, want.float(), what, ax)
    assert torch.equal(s64, s64.float().double()) and torch.equal(f64, f64.float().double())
    # torch's float64 grid_sample backward IS the documented convention, at every planted position
    ps, pf = BR.warp_backward_plain(d["src"], d["flow"], d["dout"])
    assert np.array_equal(s64.numpy(), ps), "dsrc: torch's scatter differs from floor taps with dropped outside taps"
    assert np.array_equal(f64.numpy(), pf), "dflow: torch differs from the documented masks"
    mask = BR.warp_masks(d["flow"])
    assert bool((f64[~mask] == 0).all())
    ix, iy = BR.warp_positions(d["flow"])
    cat = d["cat"]
    assert bool(((ix == ix.round()) & (iy == iy.round()) & mask[:, 0] & mask[:, 1])[cat == 1].all())
    on_border = (ix == 0) | (ix == W - 1) | (iy == 0) | (iy == H - 1)
    assert bool(on_border[cat == 2].all()) and bool((~(mask[:, 0] & mask[:, 1]))[cat == 2].all())
    beyond = (ix < 0) | (ix > W - 1) | (iy < 0) | (iy > H - 1)
    assert bool(beyond[cat == 3].all())
    if H * W >= 24:
        for n in range(N):
            sides = [(ix[n] < 0), (ix[n] > W - 1), (iy[n] < 0), (iy[n] > H - 1), (ix[n] == 0), (ix[n] == W - 1),
                     (iy[n] == 0), (iy[n] == H - 1)]
            assert all(bool(s.any()) for s in sides)
    assert int((cat == 4).sum()) >= N and int((cat == 5).sum()) >= N
    assert float(f64.abs().max()) > 0 and float(s64.abs().max()) > 0


@pytest.mark.parametrize("N,C,H,W", [(1, 2, 1, 1), (2, 2, 1, 9), (1, 3, 2, 2), (2, 2, 5, 7), (1, 67, 6, 5)])
def test_exact_up2_reference_is_order_independent(N, C, H, W):
    dout, pre = BR.resample_exact(N, C, H, W, 2, seed=H * W)
    for scale in (2.0, 1.0, 0.5):
        r64 = BR.up2_backward(dout, scale, pre)
        BR.assert_bits(BR.up2_backward(dout, scale, pre, torch.float32), r64.float(), f"up2 x{scale} fp32", "n,c,y,x")
        rf = BR.up2_backward(dout.flip([0, 2, 3]), scale, pre.flip([0, 2, 3]), torch.float32).flip([0, 2, 3])
        BR.assert_bits(rf, r64.float(), f"up2 x{scale} flipped", "n,c,y,x")
        assert torch.equal(r64, r64.float().double())
    if H == 1 and W == 1:  # both taps of every output land on the only source element
        want = dout.double().sum((2, 3), keepdim=True) * 2.0 + pre.double()
        assert torch.equal(BR.up2_backward(dout, 2.0, pre), want)


@pytest.mark.parametrize("N,C,H,W", [(1, 3, 2, 2), (2, 3, 6, 10), (2, 64, 4, 6)])
def test_exact_down2_reference_is_one_multiply_deep(N, C, H, W):
    dout, pre = BR.resample_exact(N, C, H, W, 0.5, seed=H + W)
    r64 = BR.down2_backward(dout, 0.5, pre)
    BR.assert_bits(BR.down2_backward(dout, 0.5, pre, torch.float32), r64.float(), "down2 fp32", "n,c,y,x")
    rf = BR.down2_backward(dout.flip([0, 2, 3]), 0.5, pre.flip([0, 2, 3]), torch.float32).flip([0, 2, 3])
    BR.assert_bits(rf, r64.float(), "down2 flipped", "n,c,y,x")
    fl = torch.randn(N, C, H // 2, W // 2, generator=torch.Generator().manual_seed(5)) * 1e-3
    want = fl.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.125  # arbitrary floats: dout * (scale / 4), exactly
    BR.assert_bits(BR.down2_backward(fl, 0.5).float(), want, "down2 float dout", "n,c,y,x")


def test_assert_bits_reports_index_and_bit_patterns():
    a = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    b = a.clone()
    b[1, 2, 3] = float(np.nextafter(np.float32(23), np.float32(24)))
    with pytest.raises(AssertionError) as ei:
        BR.assert_bits(b, a, "dw", "co,ci,k")
    msg = str(ei.value)
    assert "(co,ci,k)=(1, 2, 3)" in msg and "0x41b80001" in msg and "0x41b80000" in msg and "dw" in msg
    nan = torch.full((2,), float("nan"))
    with pytest.raises(AssertionError):
        BR.assert_bits(nan, torch.zeros(2), "canary")
