"""ROI-weighted quantisation on a real MI355X: the q-scale map kernel and the map's multiply in the two quantisation
kernels bit for bit against numpy restatements (tests/roiq_ref.py), a map of ones against no map, the codecs with a
real map against the CPU oracle (which broadcasts a q-scale TENSOR, so it needs no change), the bitstream round trip,
and the file loops with their roiq.json side file."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import dcvc_ref as OR
from tests import gpu_util as U
from tests import roiq_ref as R
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from tests.util import oracle_weights
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X
from vcm_ts_amd.synthetic import frames

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32


# -------------------------------------------------------------------------------------------------- the map kernel
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_q_map_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    roiq = {g: X.RoiQ(R.BACKGROUND, R.CLASSES, g) for g in R.GROWS}
    f = R.factors()
    hc, wc = R.grid(H, W)
    guard = 64
    for name, boxes in R.box_lists(H, W).items():
        fb = X.FrameBoxes(boxes)
        for grow in R.GROWS:
            buf = torch.full((hc * wc + 2 * guard,), float("nan"), device=DEV)
            before = U.f32_bits(buf).copy()
            got = X.q_map(fb, H, W, roiq[grow], out=buf[guard:guard + hc * wc])
            assert got.shape == (1, 1, hc, wc) and got.data_ptr() == buf[guard:].data_ptr()
            after = U.f32_bits(buf)
            want = R.q_map(boxes, H, W, grow, f)
            assert np.array_equal(after[guard:guard + hc * wc].reshape(hc, wc), want.view(np.uint32)), (name, grow)
            assert np.array_equal(after[:guard], before[:guard]) and np.array_equal(after[-guard:], before[-guard:]), (name, grow)
    # without `out`: a fresh tensor on the current device; two classes only -> a box of class 2 is refused by name
    got = X.q_map(boxes, H, W, roiq[0])
    assert got.device == DEV and np.array_equal(U.f32_bits(got).reshape(hc, wc), R.q_map(boxes, H, W, 0, f).view(np.uint32))
    with pytest.raises(ValueError, match="unknown class"):
        X.q_map(np.array([[0, 0, W, H, 2]]), H, W, X.RoiQ(100, (60, 140)))


# ------------------------------------------------------------------------------------------- dcvc_scale_channels_map
@pytest.mark.parametrize("multiply", [False, True], ids=["divide", "multiply"])
def test_scale_channels_map_bit_for_bit(multiply):
    N, H, W, Cc, cs = 2, 3, 5, 96, 100
    g = np.random.default_rng(7 + multiply)
    x = (g.standard_normal((N, H, W, cs)) * 5).astype(F32)
    qb = np.linspace(0.2, 1.3, Cc).astype(F32)
    qs = np.array([0.7, 1.9], dtype=F32)
    m = g.uniform(0.1, 10.0, (N, H, W)).astype(F32)
    m.reshape(-1)[:3] = [0.1, 10.0, 1.0]
    q = (np.maximum(qb, F32(0.5))[None, None, None, :] * qs[:, None, None, None]) * m[..., None]
    assert q.dtype == F32
    want = x[..., :Cc] * q if multiply else x[..., :Cc] / q
    xd, qbd, qsd, md = (torch.from_numpy(a).to(DEV) for a in (x, qb, qs, m))
    ones = torch.ones_like(md)
    L, st = lib.hip(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def run(q_map, plain=False):
        out = torch.full((N, H, W, cs), float("nan"), device=DEV)
        if plain:
            lib.check(L.dcvc_scale_channels(xd.data_ptr(), cs, out.data_ptr(), cs, qbd.data_ptr(), qsd.data_ptr(), int(multiply),
                                            N, H * W, Cc, st), "scale_channels")
        else:
            lib.check(L.dcvc_scale_channels_map(xd.data_ptr(), cs, out.data_ptr(), cs, qbd.data_ptr(), qsd.data_ptr(), int(multiply),
                                                N, H * W, Cc, None if q_map is None else q_map.data_ptr(), H, W, st),
                      "scale_channels_map")
        assert bool(torch.isnan(out[..., Cc:]).all())  # the stride's padding is not written
        return U.f32_bits(out[..., :Cc].contiguous())

    assert np.array_equal(run(md), want.view(np.uint32))
    plain = run(None, plain=True)
    assert np.array_equal(run(ones), plain) and np.array_equal(run(None), plain)
    assert not np.array_equal(run(md), plain)


# ------------------------------------------------------------------------------------------------------- the codecs
@pytest.fixture(scope="module", params=["fp32", "fp16x3"])
def nets(request):
    """Both arithmetic modes of the convolution kernels, as in tests/test_gpu_codec.py."""
    return U.seeded_pair(DEV, request.param)


def _i_planes(v):
    return [v["sym_z"], v["r"]["sym"][0], v["r"]["sym"][1], v["r"]["idx"][0], v["r"]["idx"][1]]


def _p_planes(v):
    return [v["sym_mv_z"], v["sym_z"]] + [v[r][k][j] for r in ("r_mv", "r_y") for k in ("sym", "idx") for j in (0, 1)]


def test_a_map_of_ones_is_no_map(nets):
    d, i = nets
    h, w = 64, 128
    fr = frames(5, 3, h, w)
    xs = [torch.from_numpy(fr[t:t + 1]).to(DEV) for t in range(3)]
    ones = torch.ones((1, 1, h // 16, w // 16), device=DEV)
    a = i.compress(xs[0], 1.0)
    keep = (a["x_hat"].clone(), [p.clone() for p in _i_planes(a["_views"])], a["bit_stream"])
    b = i.compress(xs[0], 1.0, q_map=ones)
    assert torch.equal(b["x_hat"], keep[0]) and b["bit_stream"] == keep[2]
    assert all(torch.equal(p, q) for p, q in zip(_i_planes(b["_views"]), keep[1]))
    dpb = U.intra_dpb(keep[0])
    for t, shape in ((1, ones), (2, ones[0, 0])):  # (both accepted shapes of a one-picture map)
        a = d.compress(xs[t], dpb, 1.0, 1.0)
        keep = ({k: v.clone() for k, v in a["dpb"].items()}, [p.clone() for p in _p_planes(a["_views"])], a["bit_stream"])
        b = d.compress(xs[t], dpb, 1.0, 1.0, q_map=shape)
        assert b["bit_stream"] == keep[2]
        assert all(torch.equal(b["dpb"][k], keep[0][k]) for k in keep[0])
        assert all(torch.equal(p, q) for p, q in zip(_p_planes(b["_views"]), keep[1]))
        dpb = keep[0]


def _box_map(hc, wc, inside, outside):
    m = np.full((1, 1, hc, wc), outside, dtype=F32)
    m[:, :, 2:5, 3:8] = inside
    return m


_ORACLE = {}


def _oracle_with_a_map(xs, m):
    """The CPU oracle on the clip with q * map as its q-scale tensor, computed once for both precisions: the I picture's
    result and the two P pictures' (each against the oracle's own clamped DPB)."""
    if not _ORACLE:
        wd, wi = oracle_weights("dmc"), oracle_weights("intra")
        with torch.no_grad():
            ro = OR.intra_forward(wi, xs[0], 0.8 * m)
            dpb_o, ps = U.intra_dpb(ro["x_hat"].clamp(0, 1)), []
            for t in (1, 2):
                po = OR.dmc_forward_one_frame(wd, xs[t], dpb_o, 1.1, 0.9 * m)
                ps.append(po)
                dpb_o = dict(po["dpb"], ref_frame=po["_inter"]["recon"].clamp(0, 1))
        _ORACLE.update(i=ro, p=ps)
    return _ORACLE["i"], _ORACLE["p"]


def test_intermediates_and_symbols_match_oracle_with_a_map(nets):
    """test_gpu_codec.test_intermediates_and_symbols_match_oracle -- its clip, q-scales and bounds -- with a q-scale map of
    0.6 on cells [2:5, 3:8] and 1.4 elsewhere; the oracle takes q * map as its q-scale tensor."""
    d, i = nets
    fr = frames(11, 3, 128, 192)
    xs = [torch.from_numpy(fr[t:t + 1]) for t in range(3)]
    m = torch.from_numpy(_box_map(8, 12, F32(60) / F32(100), F32(140) / F32(100)))
    md = m.to(DEV)
    ro, ps = _oracle_with_a_map(xs, m)
    with torch.no_grad():
        rg = i.compress(xs[0].cuda(), 0.8, q_map=md)
        og = rg["_views"]
        for tag, sym, sc in OR.intra_symbol_planes(ro["_inter"]):
            key = {"z": og["sym_z"], "y0": og["r"]["sym"][0], "y1": og["r"]["sym"][1]}[tag]
            got = key.cpu().numpy().reshape(sym.shape)
            share = (got != sym.numpy()).mean()
            print("I", tag, "symbol mismatch share", share)
            assert share < 1e-4, tag
        dpb_o = U.intra_dpb(ro["x_hat"].clamp(0, 1))
        dpb_g = U.intra_dpb(rg["x_hat"])
        print("I x_hat max abs diff", float((rg["x_hat"].cpu() - dpb_o["ref_frame"]).abs().max()))
        np.testing.assert_allclose(rg["x_hat"].cpu().numpy(), dpb_o["ref_frame"].numpy(), atol=2e-5)
        for t in (1, 2):
            po = ps[t - 1]
            pg = d.compress(xs[t].cuda(), dpb_g, 1.1, 0.9, q_map=md)
            v, o = pg["_views"], po["_inter"]
            for name in ("est_mv", "mv_hat", "c1", "c2", "c3", "y_hat", "mv_y_hat", "feature"):
                got, want = v[name].nchw().cpu(), o[name]
                rel = ((got - want).abs().max() / want.abs().max()).item()
                print("P", t, name, "relative", rel)
                assert rel < 5e-5, name
            planes = {"mv_z": v["sym_mv_z"], "mv_y0": v["r_mv"]["sym"][0], "mv_y1": v["r_mv"]["sym"][1],
                      "z": v["sym_z"], "y0": v["r_y"]["sym"][0], "y1": v["r_y"]["sym"][1]}
            for tag, sym, sc in OR.dmc_symbol_planes(o):
                got = planes[tag].cpu().numpy().reshape(sym.shape)
                share = (got != sym.numpy()).mean()
                print("P", t, tag, "symbol mismatch share", share)
                assert share < 1e-4, tag
            print("P", t, "recon max abs diff", float((pg["dpb"]["ref_frame"].cpu() - o["recon"].clamp(0, 1)).abs().max()))
            np.testing.assert_allclose(pg["dpb"]["ref_frame"].cpu().numpy(), o["recon"].clamp(0, 1).numpy(), atol=3e-5)
            dpb_g = pg["dpb"]


def test_round_trip_needs_the_encoders_map(nets):
    d, i = nets
    h, w = 64, 128
    fr = frames(5, 3, h, w)
    xs = [torch.from_numpy(fr[t:t + 1]).to(DEV) for t in range(3)]
    m = torch.full((1, 1, 4, 8), 1.4, device=DEV)
    m[:, :, 1:3, 2:6] = 0.6
    ones = torch.ones_like(m)
    ci = i.compress(xs[0], 1.0, q_map=m)
    x_hat = ci["x_hat"].clone()
    assert torch.equal(i.decompress(ci["bit_stream"], h, w, 1.0, q_map=m)["x_hat"], x_hat)
    assert not torch.equal(i.decompress(ci["bit_stream"], h, w, 1.0, q_map=ones)["x_hat"], x_hat)
    assert not torch.equal(i.decompress(ci["bit_stream"], h, w, 1.0)["x_hat"], x_hat)
    dpb = U.intra_dpb(x_hat)
    for t in (1, 2):
        c = d.compress(xs[t], dpb, 1.0, 1.0, q_map=m)
        enc = {k: v.clone() for k, v in c["dpb"].items()}
        dd = d.decompress(dpb, c["bit_stream"], h, w, 1.0, 1.0, q_map=m)["dpb"]
        for k in enc:
            assert torch.equal(dd[k], enc[k]), k
        other = d.decompress(dpb, c["bit_stream"], h, w, 1.0, 1.0, q_map=ones)["dpb"]
        assert not torch.equal(other["ref_frame"], enc["ref_frame"]) and not torch.equal(other["ref_y"], enc["ref_y"])
        assert torch.equal(other["ref_mv_y"], enc["ref_mv_y"])  # mv_y keeps its scalar
        dpb = enc


def test_codecs_refuse_by_name(nets):
    d, i = nets
    x = torch.zeros((1, 3, 64, 128), device=DEV)
    dpb = U.intra_dpb(x)
    good = torch.ones((4, 8), device=DEV)
    for bad, match in ((torch.ones((8, 4), device=DEV), "shape"), (torch.ones((2, 1, 4, 8), device=DEV), "shape"),
                       (torch.ones((4, 8), device=DEV, dtype=torch.float64), "float32"), (torch.ones((4, 8)), "cpu"),
                       (np.ones((4, 8), F32), "float32")):
        for call in (lambda: i.compress(x, 1.0, q_map=bad), lambda: d.compress(x, dpb, 1.0, 1.0, q_map=bad),
                     lambda: i.decompress(b"", 64, 128, 1.0, q_map=bad), lambda: d.decompress(dpb, b"", 64, 128, 1.0, 1.0, q_map=bad)):
            with pytest.raises(ValueError, match=match):
                call()
    with pytest.raises(NotImplementedError, match="graph"):
        d.compress(x, dpb, 1.0, 1.0, graph=True, q_map=good)
    for net, call in ((i, lambda: i.compress(x, 1.0, q_map=good)), (d, lambda: d.compress(x, dpb, 1.0, 1.0, q_map=good))):
        net.train()
        try:
            with pytest.raises(ValueError, match="train"):
                call()
        finally:
            net.eval()


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, SIDE = 8, 16, 64
BOX = [[16, 16, 48, 48, 0]]  # 4 of the 16 cells
Q_IN = X.RoiQ(140, (60,), 0)      # 0.6 inside the box, 1.4 outside
Q_OUT = X.RoiQ(60, (140,), 0)     # 1.4 inside, 0.6 outside


def _roi():
    return X.Roi(lambda t: X.FrameBoxes(BOX), (X.RoiClass(0),), ("plate",))


def _size(folder):
    return sum(len(v) for v in U.bins(folder).values())


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the clip as PNGs; a plain encode (the parent's bins) and the encode with 0.6 inside / 1.4 outside the box"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("roiq_e2e")
    clip = np.rint(frames(21, N_FRAMES, SIDE, SIDE) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    U.write_pngs(tmp / "png", clip)
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "in"), str(tmp / "in_rec"), gop=GOP, nets=file_nets, roi=_roi(),
                                  roi_q=Q_IN)
    assert size == (SIDE, SIDE) and len(bits) == N_FRAMES
    return dict(tmp=tmp, clip=clip)


def test_folder_side_file_and_decoder_output(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert json.loads((tmp / "in" / "roiq.json").read_text()) == {"cell": 16, "background": 140, "classes": {"plate": 60}, "grow": 0}
    assert sorted(n for n in os.listdir(tmp / "in") if not n.endswith(".bin")) == ["roiq.json"]
    assert U.bins(tmp / "in") != U.bins(tmp / "plain") and list(U.bins(tmp / "in")) == list(U.bins(tmp / "plain"))
    assert RC.decode_folder(str(tmp / "in"), str(tmp / "in_dec"), SIDE, SIDE, gop=GOP, roi=_roi()) == N_FRAMES
    for t in range(N_FRAMES):
        name = f"im{t + 1:05d}.png"
        assert (tmp / "in_dec" / name).read_bytes() == (tmp / "in_rec" / name).read_bytes(), t
    with pytest.raises(ValueError, match=r"roiq\.json.*boxes"):
        RC.decode_folder(str(tmp / "in"), str(tmp / "x"), SIDE, SIDE, gop=GOP)


def test_two_gop_streams_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "in2"), gop=GOP, nets=file_nets, gop_streams=2, roi=_roi(), roi_q=Q_IN)
    assert U.bins(tmp / "in2") == U.bins(tmp / "in")
    assert (tmp / "in2" / "roiq.json").read_text() == (tmp / "in" / "roiq.json").read_text()


def test_neutral_factors_and_feature_off_give_the_plain_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    plain = U.bins(tmp / "plain")
    assert sorted(os.listdir(tmp / "plain")) == sorted(plain)  # no roiq.json, nothing but the .bin files
    RC.encode_folder(str(tmp / "png"), str(tmp / "neutral"), gop=GOP, nets=file_nets, roi=_roi(), roi_q=X.RoiQ(100, (100,), 7))
    assert U.bins(tmp / "neutral") == plain and (tmp / "neutral" / "roiq.json").exists()
    # the feature off, with the boxes and into a folder that holds a stale side file: the parent's bins, the file gone
    RC.encode_folder(str(tmp / "png"), str(tmp / "neutral"), gop=GOP, nets=file_nets, roi=_roi())
    assert U.bins(tmp / "neutral") == plain and sorted(os.listdir(tmp / "neutral")) == sorted(plain)


def test_y4m_round_trip_with_a_map(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(a.transpose(2, 0, 1).astype(F32) / F32(255.0), dtype=np.float64))
              for a in e2e["clip"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, SIDE, SIDE, fps="30:1")
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), gop=GOP, nets=file_nets, gop_streams=2,
                    roi=_roi(), roi_q=Q_IN)
    assert json.loads((tmp / "vbins" / "roiq.json").read_text())["classes"] == {"plate": 60}
    assert "roiq" not in json.dumps(RC.read_sequence_info(str(tmp / "vbins")), default=str)
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m"), roi=_roi()) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()
    assert (tmp / "dec.y4m").stat().st_size > N_FRAMES * SIDE * SIDE * 3 // 2
    with pytest.raises(ValueError, match=r"roiq\.json.*boxes"):
        RC.decode_video(str(tmp / "vbins"), str(tmp / "x.y4m"))


def test_rate_follows_the_map(e2e, file_nets):
    """Summed .bin sizes of the clip: coarser everywhere < mixed < finer everywhere, strictly, both ways round.  (On the
    CPU oracle at 128x192 the gaps were at least 4 %.)"""
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    size = {"in": _size(tmp / "in")}
    for name, q in (("140", X.RoiQ(140, (140,))), ("60", X.RoiQ(60, (60,))), ("out", Q_OUT)):
        RC.encode_folder(str(tmp / "png"), str(tmp / name), gop=GOP, nets=file_nets, roi=_roi(), roi_q=q)
        size[name] = _size(tmp / name)
    print("bytes:", size, "plain", _size(tmp / "plain"))
    assert size["140"] < size["in"] < size["60"]
    assert size["140"] < size["out"] < size["60"]
