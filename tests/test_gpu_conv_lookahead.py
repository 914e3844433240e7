"""dcvc_conv_set_lookahead: the two load schedules of conv_mfma (vcm_ts_amd/csrc/conv_mfma.hip) give the same bits.

Mode 1 requests every input patch one step before it is staged; mode 2 (the default) requests the next chunk of a 3x3
stride-2 or 7x7 layer a whole chunk ahead.  (The 1x1 stride-1 layers were measured with their chunks requested in groups
of four, lost, and run the same schedule in both modes: their cases stay, so that a later schedule for them is held to
the same bits.)  Only the time at which a global load is issued differs, so every comparison here is torch.equal -- on random data, with a residual, LeakyReLU on
the input and on the output, outputs prefilled with NaN, in the exact-fp32 and in the split-fp16 mode.  Pictures are
21 x 37 (stride 2: 43 x 75 in, 22 x 38 out) unless a case says otherwise: ragged both ways, more than one tile each way.
What the kernels compute is held against references by the other conv tests, which all run the default mode."""
import math

import pytest
import torch

from vcm_ts_amd.synthetic import frames

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    from vcm_ts_amd.engine import Engine

    return {"fp32": Engine("cuda:0"), "fp16x3": Engine("cuda:0", precision="fp16x3")}


def _in_both_modes(e, fn):
    """fn() under lookahead 1 and 2 -> the two results; the default mode is restored whatever happens."""
    got = {}
    try:
        for mode in (1, 2):
            assert e.L.dcvc_conv_set_lookahead(mode) == 0
            got[mode] = fn()
    finally:
        assert e.L.dcvc_conv_set_lookahead(2) == 0
    return got[1], got[2]


def _layer(e, tag, segs, cout, ks, stride=1, H=21, W=37, N=1, ps=False, in_cs=None, chan=False, band=None, of=None):
    """A closure that runs one layer (fresh NaN-filled output each time) and returns its output rows, plus the fused channel
    sums when asked for.  of: draw the data of that many pictures and use the first N of them."""
    g = torch.Generator().manual_seed(1000 * ks + 10 * sum(segs) + cout + stride)
    cin = sum(segs)
    w = torch.randn(cout, cin, ks, ks, generator=g) / math.sqrt(cin * ks * ks)
    b = torch.randn(cout, generator=g)
    pk = e.pack(("lookahead", tag, e.precision), torch.nn.Parameter(w.cuda()), torch.nn.Parameter(b.cuda()), segs, ps)
    srcs = []
    for i, c in enumerate(segs):
        x = torch.randn(of or N, c, H, W, generator=g)[:N]
        srcs.append(e.from_nchw(x.cuda(), e.buf(f"la/{tag}/in{i}", N, H, W, c, cs=None if in_cs is None else in_cs[i])))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    m = 2 if ps else 1
    cfin = cout // 4 if ps else cout
    res = e.from_nchw(torch.randn(of or N, cfin, Ho * m, Wo * m, generator=g)[:N].cuda(), e.buf(f"la/{tag}/res", N, Ho * m, Wo * m, cfin))
    out = e.buf(f"la/{tag}/out", N, Ho * m, Wo * m, cfin)
    sums = e.chan_partial_buf(f"la/{tag}", pk, out, stride) if chan else None
    rows = slice(None)
    if band is not None:
        th = int(e.L.dcvc_conv_tile_rows(ks, stride))
        rows = slice(band[0] * th, min((band[0] + band[1]) * th, Ho))

    def run():
        out.base.fill_(float("nan"))
        if chan:
            sums[0].fill_(float("nan"))
        e.conv(pk, srcs, out, stride=stride, in_slope=0.01, out_slope=0.1, res=res, chan_partial=sums[0] if chan else None, band=band)
        got = [e.to_nchw(out)[:, :, rows].clone()]
        if chan:
            got.append(sums[0][: N * sums[1] * pk.Cout_pad].clone())
        if band is not None:  # nothing outside the band is written
            rest = e.to_nchw(out).clone()
            rest[:, :, rows] = float("nan")
            assert torch.isnan(rest).all()
        return got

    return pk, run


def _same_bits(e, run):
    a, b = _in_both_modes(e, run)
    for u, v in zip(a, b):
        assert torch.isfinite(v).all() and u.numel() > 0
        assert torch.equal(u, v)


CASES = {
    # 1x1 stride 1 (four 16-channel chunks would be one group)
    "k1_one_full_group": dict(segs=(64,), cout=64, ks=1),
    "k1_group_across_segments": dict(segs=(32, 32), cout=64, ks=1),
    "k1_ragged_last_group_shuffle": dict(segs=(144,), cout=576, ks=1, H=17, W=30, ps=True),
    "k1_narrow_chunk_tail": dict(segs=(40,), cout=32, ks=1),
    "k1_channel_sums": dict(segs=(64,), cout=64, ks=1, chan=True),
    "k1_band": dict(segs=(96,), cout=64, ks=1, band=(1, 1)),
    # 3x3 stride 2: the next chunk's patch a chunk ahead
    "k3s2_64": dict(segs=(64,), cout=64, ks=3, stride=2, H=43, W=75),
    "k3s2_tail_in_first_segment": dict(segs=(3, 64), cout=64, ks=3, stride=2, H=43, W=75, in_cs=(8, 64)),
    "k3s2_144_192": dict(segs=(144,), cout=192, ks=3, stride=2, H=43, W=75),
    # 7x7
    "k7_32_64": dict(segs=(32,), cout=64, ks=7),
    "k7_64_32": dict(segs=(64,), cout=32, ks=7),
    "k7_8_32_tap_pairs": dict(segs=(8,), cout=32, ks=7),
}


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_lookahead_modes_give_the_same_bits(engines, name, prec):
    e = engines[prec]
    pk, run = _layer(e, name, **CASES[name])
    if name == "k7_8_32_tap_pairs" and prec == "fp16x3":
        assert e.pair_capable(pk, 1)  # the engine's tap-paired route (split fp16 only; exact fp32 runs it unpaired)
    _same_bits(e, run)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("ks,stride", [(1, 1), (3, 2), (7, 1)], ids=["k1", "k3s2", "k7"])
def test_lookahead_modes_and_tile_heights_give_the_same_bits(engines, ks, stride, prec):
    """Stride-1 layers run on 4-row tiles when 8-row tiles would give fewer than 384 workgroups: 6 tiles x 4 blocks of 64
    output channels x 16 pictures is 384 (8-row tiles), the first picture alone is 24 (4-row tiles).  Both tile heights
    in both modes: four results, all equal."""
    e = engines[prec]
    H, W = (43, 75) if stride == 2 else (21, 37)
    _, batch = _layer(e, f"rows/{ks}/16", (32,), 256, ks, stride, H, W, N=16)
    _, alone = _layer(e, f"rows/{ks}/1", (32,), 256, ks, stride, H, W, N=1, of=16)  # the batch's first picture
    b1, b2 = _in_both_modes(e, batch)
    a1, a2 = _in_both_modes(e, alone)
    assert torch.isfinite(b2[0]).all()
    for other in (b1[0][:1], a1[0], a2[0]):
        assert torch.equal(other, b2[0][:1])


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_a_short_gop_codes_to_the_same_bytes_in_both_modes(prec):
    """I + 2 P at 128 x 192 (nearly every layer of the two networks runs on conv_mfma at this size): payload bytes and the
    final decoded-picture buffer are identical."""
    from vcm_ts_amd.dmc import DMC
    from vcm_ts_amd.intra import IntraNoAR
    from vcm_ts_amd.pipeline import GopEncoder

    dev = torch.device("cuda:0")
    d, i = DMC(precision=prec).to(dev).eval(), IntraNoAR(precision=prec).to(dev).eval()
    d.update()
    i.update()
    seq = [torch.from_numpy(f[None]).to(dev) for f in frames(5, 3, 128, 192)]
    enc = GopEncoder(i, d, gop_size=3)

    def run():
        coded, bits, dpb = enc.encode_gop(seq, 1.0, 1.0, 1.0)
        return [c[2] for c in coded], bits, {k: v.clone() for k, v in dpb.items() if torch.is_tensor(v)}

    (pay1, bits1, dpb1), (pay2, bits2, dpb2) = _in_both_modes(d.engine(), run)
    assert len(pay2) == 3 and all(len(p) > 0 for p in pay2)
    assert pay1 == pay2 and bits1 == bits2
    assert set(dpb1) == set(dpb2) and "ref_frame" in dpb2
    for k in dpb2:
        assert torch.isfinite(dpb2[k]).all() and torch.equal(dpb1[k], dpb2[k]), k


def test_lookahead_hook_accepts_modes_1_and_2_only():
    """Host-only: every other value answers DCVC_E_ARG and changes nothing."""
    from vcm_ts_amd import lib

    L = lib.hip()
    try:
        for bad in (0, 3, 8):
            assert L.dcvc_conv_set_lookahead(bad) == -1
        assert L.dcvc_conv_set_lookahead(1) == 0
        assert L.dcvc_conv_set_lookahead(2) == 0
    finally:
        L.dcvc_conv_set_lookahead(2)
