"""Backward-adaptive quantisation on a real MI355X: the activity and map kernels bit for bit against the numpy
restatement (tests/aq_ref.py), a flat reference against no map, the GOP loop with the decoder rebuilding every map from its
own reference pictures, the refusals, and the file loops with their aq.json side file."""
import json
import os

import numpy as np
import pytest
import torch

from tests import aq_ref as R
from tests import gpu_util as U
from tests import roiq_ref as QR
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from vcm_ts_amd import aq as A
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X
from vcm_ts_amd.pipeline import GopEncoder, intra_dpb
from vcm_ts_amd.synthetic import frames

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
GUARD = U.GUARD


# ------------------------------------------------------------------------------------------------ the activity kernel
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_activity_kernel_equals_the_restatement_bit_for_bit(size):
    Hp, Wp = size
    hc, wc = Hp // 16, Wp // 16
    # (row pad, plane pad, offset): 16-byte loads; an odd offset, an odd row stride, an odd plane stride -> 4-byte loads
    layouts = [(8, 24, 12), (8, 24, 13), (5, 24, 12), (8, 23, 12)]
    for n, (name, pic) in enumerate(R.pictures(Hp, Wp).items()):
        want_L, want_sum = R.activity(pic)
        for row_pad, plane_pad, offset in (layouts if n < 2 else [layouts[0], layouts[1 + n % 3]]):
            buf, view, rs, ps = U.strided(pic, Hp, Wp, row_pad, plane_pad, offset, DEV)[:4]
            L = torch.full((hc * wc + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
            total = torch.tensor([12345, -1], dtype=torch.int64, device=DEV)  # pre-loaded: the kernel ADDS
            lib.check(lib.hip().dcvc_aq_activity(view.data_ptr(), rs, ps, Hp, Wp, L[GUARD:].data_ptr(), total.data_ptr(), U.stream(DEV)),
                      "aq_activity")
            got = L.cpu().numpy()
            where = (name, row_pad, plane_pad, offset)
            assert np.array_equal(got[GUARD:GUARD + hc * wc].reshape(hc, wc), want_L), where
            assert (got[:GUARD] == -7).all() and (got[GUARD + hc * wc:] == -7).all(), where
            assert total.tolist() == [12345 + want_sum, -1], where
    # what the pictures were chosen for
    pics = R.pictures(Hp, Wp)
    assert R.activity(pics["zeros"])[1] == R.activity(pics["ones"])[1] == R.activity(pics["flat-cells"])[1] == 0
    assert (R.variance256(R.luma(pics["checker"])) == 1065369600).all()


def test_activity_through_python_zeroes_its_sum():
    maps = A.AqMaps(A.AQ(100), DEV)
    for Hp, Wp in ((64, 128), (128, 192), (64, 128)):  # (the scratch is resized, and the sum starts from zero every time)
        pic = R.pictures(Hp, Wp)["random"]
        want_L, want_sum = R.activity(pic)
        L, total = maps.activity(torch.from_numpy(pic[None]).to(DEV))
        assert L.shape == want_L.shape and np.array_equal(L.cpu().numpy(), want_L) and total.tolist() == [want_sum]
    # a crop of a wider buffer is read in place through its strides
    wide = torch.rand((1, 3, 128, 256), device=DEV)
    L, total = maps.activity(wide[..., :64, 64:192])
    want_L, want_sum = R.activity(wide[0, :, :64, 64:192].cpu().numpy())
    assert np.array_equal(L.cpu().numpy(), want_L) and total.tolist() == [want_sum]


# ----------------------------------------------------------------------------------------------------- the map kernel
SETTINGS = [(1, 10, 1000), (100, 10, 1000), (400, 10, 1000), (100, 50, 200), (400, 50, 200)]


@pytest.mark.parametrize("size", [(64, 64), (128, 192)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_kernel_equals_the_restatement_bit_for_bit(size):
    Hp, Wp = size
    hc, wc = Hp // 16, Wp // 16
    roiq = X.RoiQ(QR.BACKGROUND, QR.CLASSES, 0)
    lists = QR.box_lists(Hp, Wp)
    rois = {name: X.q_map(lists[name], Hp, Wp, roiq) for name in ("random-7", "random-40", "edges", "whole")}
    roi_host = {name: QR.q_map(lists[name], Hp, Wp, 0, QR.factors()) for name in rois}
    for name in rois:  # (the maps the products below are formed with are the restatement's)
        assert np.array_equal(U.f32_bits(rois[name]).reshape(hc, wc), roi_host[name].view(np.uint32))
    pics = R.pictures(Hp, Wp)
    seen = set()
    for strength, lo, hi in SETTINGS:
        maps = A.AqMaps(A.AQ(strength, lo, hi), DEV)
        for pname in ("random", "lone-busy", "half-smooth", "wild", "flat-cells"):
            x = torch.from_numpy(pics[pname][None]).to(DEV)
            got = maps.map(x)
            want = R.picture_map(pics[pname], strength, lo, hi)
            assert got.shape == (hc, wc) and got.dtype == torch.float32 and got.device == DEV
            assert np.array_equal(U.f32_bits(got), want.view(np.uint32)), (strength, lo, hi, pname)
            seen.update(np.unique(want).tolist())
            for rname, roi in rois.items():
                got = maps.map(x, roi if pname != "random" else roi[0, 0])  # (both accepted shapes)
                want = R.picture_map(pics[pname], strength, lo, hi, roi_host[rname])
                assert np.array_equal(U.f32_bits(got), want.view(np.uint32)), (strength, lo, hi, pname, rname)
    assert min(seen) < 0.9 and max(seen) > 2.0 and 1.0 in seen
    # one busy cell among flat ones at full strength: both clamps' neighbourhood
    lone = R.picture_map(pics["lone-busy"], 400)
    assert lone.max() == F32(10.0) and lone.min() < F32(1.0) and (lone == lone.max()).sum() == 1
    assert (R.picture_map(pics["flat-cells"], 400) == 1).all() and (R.picture_map(pics["zeros"], 400) == 1).all()


def test_map_kernel_at_both_ends_of_the_table():
    """d = +7935 and -7935 cannot come from a picture (V < 2^30 keeps L below 7680): L and the sum are given directly."""
    hc, wc = 4, 8
    g = np.random.default_rng(9)
    cases = []
    L = np.zeros((hc, wc), np.int64)
    L[1, 2] = R.MAX_L
    cases.append((L, 0))                           # M = 0: d = 7935 in one cell, 0 elsewhere
    cases.append((L, R.MAX_L * hc * wc))           # M = 7935: d = 0 in one cell, -7935 elsewhere
    cases.append((L, R.MAX_L * hc * wc - 1))       # M = 7934 (the mean floors)
    cases.append((g.integers(0, R.MAX_L + 1, (hc, wc)), None))
    roi = np.array(g.choice([10, 60, 100, 140, 1000], (hc, wc)), dtype=F32) / F32(100)
    for strength, lo, hi in SETTINGS:
        aq = A.AQ(strength, lo, hi)
        maps = A.AqMaps(aq, DEV)
        for L, total in cases:
            total = int(L.sum()) if total is None else total
            Ld = torch.from_numpy(L.astype(np.int32)).to(DEV)
            sd = torch.tensor([total], dtype=torch.int64, device=DEV)
            for r in (None, roi):
                out = torch.full((hc * wc + 2 * GUARD,), float("nan"), device=DEV)
                rd = None if r is None else torch.from_numpy(r).to(DEV)
                lib.check(lib.hip().dcvc_aq_map(Ld.data_ptr(), sd.data_ptr(), hc, wc, maps.ktab.data_ptr(), maps.ftab.data_ptr(),
                                                None if rd is None else rd.data_ptr(), out[GUARD:].data_ptr(), U.stream(DEV)), "aq_map")
                got = U.f32_bits(out)
                want = R.q_map(L, total, strength, lo, hi, r)
                assert np.array_equal(got[GUARD:GUARD + hc * wc].reshape(hc, wc), want.view(np.uint32)), (strength, lo, hi, total)
                assert np.isnan(out[:GUARD].cpu().numpy()).all() and np.isnan(out[GUARD + hc * wc:].cpu().numpy()).all()
    k = A.AQ(400).ktab()
    assert R.q_map(cases[0][0], 0, 400)[1, 2] == F32(k[-1]) / F32(100) == F32(10.0)
    assert R.q_map(cases[1][0], cases[1][1], 400)[0, 0] == F32(k[0]) / F32(100) == F32(10) / F32(100)


# ------------------------------------------------------------------------------------------------------- the codecs
@pytest.fixture(scope="module", params=["fp32", "fp16x3"])
def nets(request):
    """Both arithmetic modes of the convolution kernels, as in tests/test_gpu_codec.py; the name-seeded weights of
    tests.util.oracle_weights."""
    return U.seeded_pair(DEV, request.param)


def test_a_flat_reference_gives_no_map(nets):
    d, i = nets
    h, w = 64, 128
    x = torch.from_numpy(frames(5, 1, h, w)).to(DEV)
    maps = A.AqMaps(A.AQ(400), DEV)
    for level in (0.0, 0.3, 1.0):
        ref = torch.full((1, 3, h, w), level, device=DEV)
        m = maps.map(ref)
        assert np.array_equal(U.f32_bits(m), np.full((4, 8), F32(1.0)).view(np.uint32))
        a = d.compress(x, intra_dpb(ref), 1.0, 1.0)
        keep = (a["bit_stream"], {k: v.clone() for k, v in a["dpb"].items()})
        b = d.compress(x, intra_dpb(ref), 1.0, 1.0, q_map=m)
        assert b["bit_stream"] == keep[0] and all(torch.equal(b["dpb"][k], keep[1][k]) for k in keep[1])


class _Spy(A.AqMaps):
    """AqMaps that keeps a copy of every map it hands out."""

    def __init__(self, aq, device):
        super().__init__(aq, device)
        self.seen = []

    def map(self, ref_frame, roi_map=None):
        out = super().map(ref_frame, roi_map)
        self.seen.append(out.clone())
        return out


STRENGTH = 400  # (on the CPU oracle's I-picture reconstruction of these clips: maps of 0.80 .. 1.11 and 0.72 .. 1.07)


@pytest.mark.parametrize("size,seed", [((64, 64), 5), ((128, 192), 11)], ids=["64x64", "128x192"])
def test_gop_round_trip_rebuilds_every_map(nets, size, seed):
    """I + 3 P.  With the name-seeded weights the reconstructions are busy everywhere, so full strength is used: on the CPU
    oracle (oracle.dcvc_ref.intra_forward of picture 0, clamped) tests.aq_ref gives maps within 0.80 .. 1.11 at 64x64 (all 16
    cells off 1.0) and 0.72 .. 1.07 at 128x192 (89 of 96)."""
    d, i = nets
    h, w = size
    fr = frames(seed, 4, h, w)
    xs = [torch.from_numpy(fr[t:t + 1]).to(DEV) for t in range(4)]
    enc = GopEncoder(i, d, gop_size=4)
    recon = {}
    spy = _Spy(A.AQ(STRENGTH), DEV)
    with torch.no_grad():
        coded, bits, dpb = enc.encode_gop(xs, 1.0, 1.0, 1.0, on_recon=lambda t, r: recon.__setitem__(t, r.clone()), aq=spy)
        assert [k for k, _, _ in coded] == ["I", "P", "P", "P"] and len(spy.seen) == 3
        host = {t: recon[t].cpu().numpy()[0] for t in range(4)}
        for t in (1, 2, 3):  # the map of picture t is the restatement's on the reconstruction of t - 1
            want = R.picture_map(host[t - 1], STRENGTH)
            assert np.array_equal(U.f32_bits(spy.seen[t - 1]), want.view(np.uint32)), t
        assert any(not bool((m == 1).all()) for m in spy.seen)
        print("maps:", [(float(m.min()), float(m.max())) for m in spy.seen])
        # the decoder, given the setting alone, rebuilds every reference picture bit for bit
        dec = enc.decode_gop(coded, h, w, aq=A.AQ(STRENGTH))
        assert len(dec) == 4 and all(torch.equal(dec[t], recon[t]) for t in range(4))
        dspy = _Spy(A.AQ(STRENGTH), DEV)
        dec = enc.decode_gop(coded, h, w, aq=dspy)
        assert all(torch.equal(dec[t], recon[t]) for t in range(4))
        assert all(torch.equal(a, b) for a, b in zip(dspy.seen, spy.seen)) and len(dspy.seen) == 3
        # ... and without it decodes something else: another picture, or -- the scale indexes of y then come from other
        # steps than the encoder's, so the rANS decoder may run off its stream -- no picture at all.  The I picture, which
        # is not adapted, stays.
        from vcm_ts_amd.entropy import RansError

        assert torch.equal(enc.decode_gop(coded[:1], h, w)[0], recon[0])
        try:
            plain = enc.decode_gop(coded, h, w)
        except RansError as ex:
            print("decoding without aq:", ex)
        else:
            assert not torch.equal(plain[1], recon[1]) and not torch.equal(plain[3], recon[3])
        dec = enc.decode_gop(coded, h, w, aq=A.AQ(STRENGTH))  # (and the decoder is none the worse for it)
        assert all(torch.equal(dec[t], recon[t]) for t in range(4))
        # the payloads differ from a plain encode's from the first P picture on
        ref, _, _ = enc.encode_gop(xs, 1.0, 1.0, 1.0)
        assert ref[0] == coded[0] and ref[1][2] != coded[1][2]


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_name(nets):
    d, i = nets
    aq = A.AQ(100)
    xs = [torch.zeros((1, 3, 64, 64), device=DEV)] * 2
    with pytest.raises(NotImplementedError, match="aq: graph replay"):
        GopEncoder(i, d, gop_size=2, graphs=True).encode_gop(xs, 1.0, 1.0, 1.0, aq=aq)
    with pytest.raises(ValueError, match="aq.AQ"):
        GopEncoder(i, d, gop_size=2).encode_gop(xs, 1.0, 1.0, 1.0, aq=100)
    maps = A.AqMaps(aq, DEV)
    good = torch.zeros((1, 3, 64, 128), device=DEV)
    for bad, match in ((torch.zeros((1, 3, 64, 128)), "GPU"), (good.double(), "float32"), (good[0], "float32 reference picture"),
                       (torch.zeros((2, 3, 64, 128), device=DEV), "float32 reference picture"), (np.zeros((1, 3, 64, 128), F32), "GPU"),
                       (torch.zeros((1, 3, 72, 128), device=DEV), "multiples of 64"),
                       (torch.zeros((1, 3, 64, 96), device=DEV), "multiples of 64")):
        with pytest.raises(ValueError, match=match):
            maps.map(bad)
    for bad, match in ((torch.ones((4, 8)), "GPU"), (torch.ones((4, 8), device=DEV, dtype=torch.float64), "float32"),
                       (torch.ones((8, 4), device=DEV), "shape"), (np.ones((4, 8), F32), "float32")):
        with pytest.raises(ValueError, match=match):
            maps.map(good, bad)
    assert bool((maps.map(good, torch.ones((4, 8), device=DEV)) == 1).all())


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW = 4, 8, 128, 192
AQ_FILE = A.AQ(STRENGTH)
BOX = [[32, 32, 96, 112, 0]]


def _roi():
    return X.Roi(lambda t: X.FrameBoxes(BOX), (X.RoiClass(0),), ("plate",))


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the clip as PNGs; a plain encode and the encode with backward-adaptive quantisation"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("aq_e2e")
    clip = np.rint(frames(11, N_FRAMES, FH, FW) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    U.write_pngs(tmp / "png", clip)
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "aq"), str(tmp / "aq_rec"), gop=GOP, nets=file_nets, aq=AQ_FILE)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, clip=clip)


def test_folder_side_file_and_decoder_output(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert json.loads((tmp / "aq" / "aq.json").read_text()) == AQ_FILE.to_json()
    assert sorted(n for n in os.listdir(tmp / "aq") if not n.endswith(".bin")) == ["aq.json"]
    aq, plain = U.bins(tmp / "aq"), U.bins(tmp / "plain")
    assert list(aq) == list(plain) and aq != plain
    for t in range(N_FRAMES):  # I pictures are not adapted; the first P picture of each GOP already is
        name = f"im{t + 1:05d}.bin"
        assert (aq[name] == plain[name]) == (t % GOP == 0), t
    assert RC.decode_folder(str(tmp / "aq"), str(tmp / "aq_dec"), FH, FW, gop=GOP) == N_FRAMES
    U.same_pngs(tmp / "aq_dec", tmp / "aq_rec", N_FRAMES)
    # a record this host would build differently is refused by name, before anything is decoded
    info = AQ_FILE.to_json()
    info["tables"]["ktab"] = "%08x" % (int(info["tables"]["ktab"], 16) ^ 1)
    os.makedirs(tmp / "bad")
    for name, data in aq.items():
        (tmp / "bad" / name).write_bytes(data)
    (tmp / "bad" / "aq.json").write_text(json.dumps(info))
    with pytest.raises(ValueError, match=r"aq\.json.*ktab table built on this host"):
        RC.decode_folder(str(tmp / "bad"), str(tmp / "never"), FH, FW, gop=GOP)
    assert not (tmp / "never").exists()


def test_command_line(e2e, capsys):
    """encode --aq-strength and decode (which takes no option) through main(): the bins of the function call."""
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_rec"), "--gop", str(GOP),
             "--aq-strength", str(STRENGTH)])
    assert U.bins(tmp / "cli") == U.bins(tmp / "aq") and (tmp / "cli" / "aq.json").read_text() == (tmp / "aq" / "aq.json").read_text()
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP)])
    U.same_pngs(tmp / "cli_dec", tmp / "cli_rec", N_FRAMES)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--aq-strength", "100",
             "--aq-clamp", "50", "200"])
    assert json.loads((tmp / "cli" / "aq.json").read_text())["clamp"] == [50, 200]
    assert U.bins(tmp / "cli") != U.bins(tmp / "aq")


def test_two_gop_streams_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "aq2"), gop=GOP, nets=file_nets, gop_streams=2, aq=AQ_FILE)
    assert U.bins(tmp / "aq2") == U.bins(tmp / "aq")
    assert (tmp / "aq2" / "aq.json").read_text() == (tmp / "aq" / "aq.json").read_text()


def test_feature_off_gives_the_plain_bins_and_no_file(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S
    from vcm_ts_amd.pipeline import pad_frame

    tmp = e2e["tmp"]
    plain = U.bins(tmp / "plain")
    assert sorted(os.listdir(tmp / "plain")) == sorted(plain)  # no aq.json, nothing but the .bin files
    # the bytes of the GOP loop called directly, without the argument
    xs = [pad_frame(RC.u8_to_unit_float(torch.from_numpy(a).to(DEV))) for a in e2e["clip"]]
    with torch.no_grad():
        coded, _, _ = GopEncoder(*file_nets[0], gop_size=GOP).encode_gop(xs, 1.0, 1.0, 1.0)
    for g, (kind, q, payload) in enumerate(coded):
        got = (S.decode_i if kind == "I" else S.decode_p)(str(tmp / "plain" / f"im{g + 1:05d}.bin"))
        assert got[-1] == payload and tuple(got[-1 - len(q):-1]) == q
    # into a folder that holds a stale side file: the plain bins, the file gone
    RC.encode_folder(str(tmp / "png"), str(tmp / "stale"), gop=GOP, nets=file_nets, aq=A.AQ(100, 50, 200))
    assert (tmp / "stale" / "aq.json").exists()
    RC.encode_folder(str(tmp / "png"), str(tmp / "stale"), gop=GOP, nets=file_nets)
    assert U.bins(tmp / "stale") == plain and sorted(os.listdir(tmp / "stale")) == sorted(plain)
    # a clamp of 100 .. 100 adapts nothing: the plain bins, with the file
    RC.encode_folder(str(tmp / "png"), str(tmp / "stale"), gop=GOP, nets=file_nets, aq=A.AQ(STRENGTH, 100, 100))
    assert U.bins(tmp / "stale") == plain and (tmp / "stale" / "aq.json").exists()


def test_y4m_round_trip(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(a.transpose(2, 0, 1).astype(F32) / F32(255.0), dtype=np.float64))
              for a in e2e["clip"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, FH, fps="30:1")
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), gop=GOP, nets=file_nets, gop_streams=2,
                    aq=AQ_FILE)
    assert json.loads((tmp / "vbins" / "aq.json").read_text()) == AQ_FILE.to_json()
    assert "aq" not in RC.read_sequence_info(str(tmp / "vbins"))
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()
    assert (tmp / "dec.y4m").stat().st_size > N_FRAMES * FH * FW * 3 // 2
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vplain"), gop=GOP, nets=file_nets)
    assert U.bins(tmp / "vplain") != U.bins(tmp / "vbins") and not (tmp / "vplain" / "aq.json").exists()


def test_with_roi_weighted_quantisation(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    roi_q = X.RoiQ(140, (60,), 0)
    RC.encode_folder(str(tmp / "png"), str(tmp / "both"), str(tmp / "both_rec"), gop=GOP, nets=file_nets, roi=_roi(), roi_q=roi_q,
                     aq=AQ_FILE)
    assert sorted(n for n in os.listdir(tmp / "both") if not n.endswith(".bin")) == ["aq.json", "roiq.json"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "roiq"), gop=GOP, nets=file_nets, roi=_roi(), roi_q=roi_q)
    both, roiq, aq = U.bins(tmp / "both"), U.bins(tmp / "roiq"), U.bins(tmp / "aq")
    for t in range(N_FRAMES):  # an I picture keeps its ROI map; a P picture is coded under the product
        name = f"im{t + 1:05d}.bin"
        assert (both[name] == roiq[name]) == (t % GOP == 0) and both[name] != aq[name], t
    assert RC.decode_folder(str(tmp / "both"), str(tmp / "both_dec"), FH, FW, gop=GOP, roi=_roi()) == N_FRAMES
    U.same_pngs(tmp / "both_dec", tmp / "both_rec", N_FRAMES)


def test_with_rate_control(e2e, file_nets):
    """At 128x192 no report exists (MS-SSIM needs sides above 160, and frame_q_y is a key of the report): there the run, the
    decode and the q indexes in the P headers are checked; frame_q_y itself on a 176x192 clip, the smallest that reports."""
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S

    tmp = e2e["tmp"]
    bpp = 0.5 * 8 * sum(len(v) for v in U.bins(tmp / "aq").values()) / (N_FRAMES * FH * FW)
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "rate"), str(tmp / "rate_rec"), gop=GOP, nets=file_nets,
                                  target_bpp=bpp, q_range=(0.5, 3.0), aq=AQ_FILE)
    assert len(bits) == N_FRAMES and (tmp / "rate" / "aq.json").exists()
    q_y = [S.decode_p(str(tmp / "rate" / f"im{t + 1:05d}.bin"))[1] for t in range(N_FRAMES) if t % GOP]
    print("q_y indexes in the P headers", q_y)
    assert all(50 <= q <= 300 for q in q_y) and any(q != 100 for q in q_y)
    assert RC.decode_folder(str(tmp / "rate"), str(tmp / "rate_dec"), FH, FW, gop=GOP) == N_FRAMES
    U.same_pngs(tmp / "rate_dec", tmp / "rate_rec", N_FRAMES)
    # with a report
    h, w = 176, 192
    clip = np.rint(frames(12, N_FRAMES, h, w) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    U.write_pngs(tmp / "png176", clip)
    plain, _ = RC.encode_folder(str(tmp / "png176"), str(tmp / "plain176"), gop=GOP, nets=file_nets, aq=AQ_FILE)
    bits, size, rd = RC.encode_folder(str(tmp / "png176"), str(tmp / "rate176"), str(tmp / "rate176_rec"), gop=GOP, nets=file_nets,
                                      report=True, target_bpp=0.5 * sum(plain) / (N_FRAMES * h * w), q_range=(0.5, 3.0), aq=AQ_FILE)
    print("frame_q_y", rd["frame_q_y"])
    assert len(rd["frame_q_y"]) == N_FRAMES and all(0.5 <= q <= 3.0 for q in rd["frame_q_y"]) and any(q != 1.0 for q in rd["frame_q_y"])
    assert RC.decode_folder(str(tmp / "rate176"), str(tmp / "rate176_dec"), h, w, gop=GOP) == N_FRAMES
    U.same_pngs(tmp / "rate176_dec", tmp / "rate176_rec", N_FRAMES)


def test_with_a_base_scale(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "half"), str(tmp / "half_rec"), gop=GOP, nets=file_nets, base_scale="1/2", aq=AQ_FILE)
    assert sorted(n for n in os.listdir(tmp / "half") if not n.endswith(".bin")) == ["aq.json", "scale.json"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "half_plain"), gop=GOP, nets=file_nets, base_scale="1/2")
    assert U.bins(tmp / "half") != U.bins(tmp / "half_plain")  # (the map is taken from the base-size reference)
    assert RC.decode_folder(str(tmp / "half"), str(tmp / "half_dec"), FH, FW, gop=GOP) == N_FRAMES
    U.same_pngs(tmp / "half_dec", tmp / "half_rec", N_FRAMES)
    assert RC.decode_folder(str(tmp / "half"), str(tmp / "half_base"), FH, FW, gop=GOP, base_scale=None) == N_FRAMES  # --base-only
    with pytest.raises(NotImplementedError, match="base_scale= with roi_q="):
        RC.encode_folder(str(tmp / "png"), str(tmp / "never2"), gop=GOP, nets=file_nets, base_scale="1/2", roi=_roi(),
                         roi_q=X.RoiQ(140, (60,), 0), aq=AQ_FILE)
