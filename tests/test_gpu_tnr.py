"""The temporal noise prefilter on a real MI355X: the kernel bit for bit against the numpy restatement (tests/tnr_ref.py)
in strided, offset, NaN-surrounded layouts with guarded outputs, its refusals, TnrFilter, and the file loops end to end:
the pictures the codec is handed, an unchanged decoder, the report, two GOP streams, a Y4M file, the command line."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import tnr_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
SENT16, SENT32 = 0xABCD, 0xABCD1234


def _check_cells(buf, at, n, want, sentinel, where):
    got = U.words(buf)
    assert np.array_equal(got[at:at + n], np.asarray(want, dtype=np.int64).reshape(-1)), where
    assert U.guards_intact(buf, at, n, sentinel), where


# (row pad, plane pad, offset of cur / ref / out, shift of sad / held): 16-byte accesses; an odd offset, an odd row
# stride, an odd plane stride -> 4-byte accesses; sad and held at every alignment their types allow
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]


def _step(cur, ref, tab_dev, P, H, W, layout, want, where):
    """One dcvc_tnr_step in `layout`, held against want = (out, sad, held)."""
    row_pad, plane_pad, offset, shift = layout
    hc, wc = R.grid(H, W)
    kc, vc, crs, cps, _ = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)
    kr, vr, rrs, rps, _ = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    ko, vo, ors, ops, mask = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    sad, s0 = U.guarded(hc * wc, shift, np.uint32, SENT32, DEV)  # (fresh sentinels every step: every cell is WRITTEN)
    held, h0 = U.guarded(hc * wc, shift, np.uint16, SENT16, DEV)
    lib.check(lib.hip().dcvc_tnr_step(vc.data_ptr(), crs, cps, vr.data_ptr(), rrs, rps, vo.data_ptr(), ors, ops, H, W,
                                      tab_dev.data_ptr(), P, sad.data_ptr() + 4 * s0, held.data_ptr() + 2 * h0, U.stream(DEV)), "tnr_step")
    got = ko.cpu().numpy()
    assert np.array_equal(got[mask].view(np.uint32), want[0].reshape(-1).view(np.uint32)), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    _check_cells(sad, s0, hc * wc, want[1], SENT32, where)
    _check_cells(held, h0, hc * wc, want[2], SENT16, where)
    for k, pic in ((kc, cur), (kr, ref)):  # the inputs are only read
        assert np.array_equal(k.cpu().numpy()[mask].view(np.uint32), pic.reshape(-1).view(np.uint32)), where


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    hc, wc = R.grid(H, W)
    assert X.grid_of(H, W) == (hc, wc)
    seqs = R.sequences(H, W)
    for T, floor, P in R.SETTINGS:
        tab = N.TNR(T, floor, P).table()
        assert np.array_equal(tab, R.table(T, floor))
        tab_dev = torch.from_numpy(tab.view(np.int16)).to(DEV)
        for name, pics in seqs.items():
            want = R.run(pics, (T, floor, P), {0})
            for n, layout in enumerate(LAYOUTS):
                if name != "clip" and n not in (0, 1 + (T + len(name)) % 3):  # (every layout on the clip, two on the others)
                    continue
                for t in range(1, len(pics)):  # (the reference of step t is the restatement's picture t - 1: steps stand alone)
                    _step(pics[t], want[t - 1][0], tab_dev, P, H, W, layout, want[t], (name, T, floor, P, layout, t))
            for t in range(1, len(pics)):
                out, sad, held = want[t]
                assert not sad[(H + 15) // 16:].any() and not sad[:, (W + 15) // 16:].any() and not held[(H + 15) // 16:].any()
                if name == "equal":  # nothing differs: the floor's weight everywhere
                    assert not sad.any() and int(held.sum()) == H * W and tab[0] == floor
                if name == "flip":  # everything differs by 255 codes: passed through, by the guard or by the table's end
                    assert not held.any() and int(sad.sum()) == 255 * H * W and np.array_equal(out, pics[t])
                    assert H < 16 or W < 16 or sad[0, 0] == 255 * 256
            if name == "bright":  # the neighbours across the strip lines are blended with a weight the halo decided
                d, a, w = R.weights(pics[1], want[0][0], tab, P)
                (y, x), = np.argwhere(d > 0)
                if 0 < y < H - 1 and 0 < x < W - 1:  # (a pixel on the picture's edge is replicated into its neighbours' windows)
                    near = a[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3]
                    assert (near == d[y, x] // 25).all() and d[y, x] // 25 > 0
        # a at T - 1 and T side by side, d at P and P + 1 side by side, written by the host
        cur, ref = R.edge_case(H, W, T, P)
        edge_want = R.step(cur, ref, tab, P)
        for layout in LAYOUTS[:2]:
            _step(cur, ref, tab_dev, P, H, W, layout, edge_want, ("edge", T, floor, P, layout))
        d, a, w = R.weights(cur, ref, tab, P)
        if H >= 6 and W >= 9:
            assert {T - 1, T} <= set(a[:(H + 1) // 2].ravel().tolist())
        if H >= 2 and W >= 2 and P < 255:
            low = d[(H + 1) // 2:]
            assert set(low.ravel().tolist()) == {P, P + 1} and (w[(H + 1) // 2:][low > P] == 256).all()
    if size == (70, 100):  # the three pixel classes all occur on the clip (the host test holds their shares)
        pics, tnr = seqs["clip"], R.SETTINGS[0]
        want = R.run(pics, tnr, {0})
        for t in range(5, 9):
            assert min(R.classes(pics[t], want[t - 1][0], R.table(*tnr[:2]), tnr[2])) > 0, t


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    pics = R.sequences(H, W)["clip"]
    kc, vc, crs, cps, _ = U.strided(pics[1], H, W, 8, 24, 12, DEV)
    kr, vr, rrs, rps, _ = U.strided(pics[0], H, W, 8, 24, 12, DEV)
    ko, vo, ors, ops, mask = U.strided(None, H, W, 8, 24, 12, DEV)
    sad, s0 = U.guarded(hc * wc, 0, np.uint32, SENT32, DEV)
    held, h0 = U.guarded(hc * wc, 0, np.uint16, SENT16, DEV)
    tab = torch.from_numpy(R.table(12, 64).view(np.int16)).to(DEV)
    good = dict(cur=vc.data_ptr(), crs=crs, cps=cps, ref=vr.data_ptr(), rrs=rrs, rps=rps, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W,
                wtab=tab.data_ptr(), P=36, sad=sad.data_ptr() + 4 * s0, held=held.data_ptr() + 2 * h0)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "wtab", "P", "sad", "held")
    span = 4 * (2 * cps + (H - 1) * crs + W)
    bad = [{k: None} for k in ("cur", "ref", "out", "wtab", "sad", "held")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"P": -1}, {"P": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs", "ors")] + [{k: (H - 1) * crs + W - 1} for k in ("cps", "rps", "ops")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "out", "sad")] + [{k: good[k] + 1} for k in ("wtab", "held")] + \
          [{"out": good["cur"]}, {"out": good["ref"]}, {"out": good["cur"] + span - 4}, {"out": good["ref"] - span + 4},
           {"cur": good["out"] + 4 * ops}, {"ref": good["out"] + 4 * (H - 1) * ors}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_tnr_step(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(sad) == SENT32).all() and (U.words(held) == SENT16).all()
    assert np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_tnr_step(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.step(pics[1], pics[0], R.table(12, 64), 36)
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), want[0].reshape(-1).view(np.uint32))
    _check_cells(sad, s0, hc * wc, want[1], SENT32, "good")
    _check_cells(held, h0, hc * wc, want[2], SENT16, "good")
    # cur and ref may be the same picture: only out must stand apart
    assert lib.hip().dcvc_tnr_step(*[dict(good, ref=good["cur"])[k] for k in order], U.stream(DEV)) == 0
    _check_cells(sad, s0, hc * wc, np.zeros(hc * wc), SENT32, "cur is ref")


def _padded(pic, Hp, Wp):
    out = np.zeros((1, 3, Hp, Wp), F32)
    out[0, :, :pic.shape[1], :pic.shape[2]] = pic
    return out


def test_filter_restarts_at_i_pictures_and_keeps_the_padding_zero():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = R.sequences(H, W)["clip"], R.SETTINGS[0], {0, 4}
    want = R.run(pics, setting, intra)
    f = N.TnrFilter(N.TNR(*setting), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.grid == R.grid(H, W) and f.launches == 0
    got, launches = [], []
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        y = f.step(x, t in intra)
        assert (y is x) == (t in intra), t  # an I picture is returned itself ...
        launches.append(f.launches)
        got.append(y.cpu().numpy())  # (a buffer of the filter is valid until the step after the next: copy now)
        assert y.shape == x.shape and torch.equal(x, torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV))  # the source is only read
    assert launches == [0, 1, 2, 3, 3, 4, 5, 6, 7]  # ... and launches nothing
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t  # (the padding: zeros)
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum())) for w in want]
    assert f.totals()[4] == (0, 0) and f.totals()[5][0] > 0 and not f._done  # (read once: the pinned buffers are let go of)
    bare = N.TnrFilter(N.TNR(*setting), (H, W), DEV, totals=False)  # the same pictures without the bookkeeping
    for t, pic in enumerate(pics[:3]):
        y = bare.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == 2 and not bare._done and bare._rows is None
    with pytest.raises(ValueError, match="totals=False"):
        bare.totals()
    wide = torch.zeros((1, 3, Hp, Wp), device=DEV)
    with pytest.raises(ValueError, match="first picture of a stream is an I picture"):
        N.TnrFilter(N.TNR(12), (H, W), DEV).step(wide, False)
    for bad in (wide[0], wide[:, :2], wide.double(), wide[..., :H, :W]):
        with pytest.raises(ValueError, match="expected a"):
            f.step(bad, False)
    with pytest.raises(ValueError, match="no CPU fallback"):
        f.step(wide.cpu(), False)
    assert f.n == len(pics)


# -------------------------------------------------------------------------------------------------------- file loops
# At 128 x 192 no report exists (MS-SSIM needs sides above 160): there the handed pictures, the decoder, the hashes, the GOP
# streams and the command line are checked; everything about --report on a 176 x 192 clip, the smallest that reports (and
# one that is padded, to 192 x 192).
GOP, N_FRAMES, FH, FW, RH = 4, 8, 128, 192, 176
SETTING = N.TNR(12, 64, 36)
INTRA = {0, 4}


def _write_pngs(folder, H, W):
    """The first pictures of the noisy clip as PNGs -> what u8_to_unit_float uploads of them, (3, H, W) float32 each."""
    u8 = np.rint(R.clip(H, W)[0][:N_FRAMES] * 255).astype(np.uint8)
    U.write_pngs(folder, u8.transpose(0, 2, 3, 1))
    return [a.astype(F32) / F32(255.0) for a in u8]


def _handed(seen, want, H, W):
    """The pictures the codec was handed are the restatement's, bit for bit, in a padding of zeros."""
    assert sorted(seen) == list(range(N_FRAMES))
    for t in range(N_FRAMES):
        Hp, Wp = seen[t].shape[2:]
        assert (Hp, Wp) == ((H + 63) // 64 * 64, (W + 63) // 64 * 64)
        assert np.array_equal(seen[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t


@contextlib.contextmanager
def _spies():
    """(the padded picture the codec was handed, the source the report measured against) by frame number, of the encodes
    run inside."""
    from vcm_ts_amd import run_codec as RC

    seen, measured = {}, {}
    encode, add, add_yuv = RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv

    def spy_encode(self, frames, *a, **kw):
        def wrapped(k):
            for t, x in enumerate(frames(k)):
                seen[self.global_index(k, t)] = x.cpu().numpy()
                yield x
        return encode(self, wrapped, *a, **kw)

    def spy_add(self, g, recon, source, size):
        measured[g] = source.cpu().numpy()
        return add(self, g, recon, source, size)

    def spy_add_yuv(self, g, recon, source, size, sums):
        measured[g] = source.cpu().numpy()
        return add_yuv(self, g, recon, source, size, sums)

    RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv = spy_encode, spy_add, spy_add_yuv
    try:
        yield seen, measured
    finally:
        RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv = encode, add, add_yuv


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the noisy clip as PNGs; a plain encode, and the encode with the prefilter -- the pictures its codec was handed
    captured on the way"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("tnr_e2e")
    pics = _write_pngs(tmp / "png", FH, FW)
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    with _spies() as (seen, _):
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), str(tmp / "tnr_rec"), gop=GOP, nets=file_nets,
                                      picture_hash=True, tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, seen=seen, want=R.run(pics, (12, 64, 36), INTRA))


def test_the_codec_is_handed_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    for t in range(N_FRAMES):  # an I picture is the source itself, a P picture is not
        assert np.array_equal(e2e["seen"][t][0], e2e["pics"][t]) == (t in INTRA), t


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert sorted(n for n in os.listdir(tmp / "tnr") if not n.endswith(".bin")) == ["hashes.json"]  # no side file of the filter
    tnr, plain = U.bins(tmp / "tnr"), U.bins(tmp / "plain")
    assert list(tnr) == list(plain)
    for t in range(N_FRAMES):  # I pictures are handed over as they are; every P picture is another picture
        name = f"im{t + 1:05d}.bin"
        assert (tnr[name] == plain[name]) == (t in INTRA), t
    assert RC.decode_folder(str(tmp / "tnr"), str(tmp / "tnr_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "tnr_dec", tmp / "tnr_rec", N_FRAMES)


def test_two_gop_streams_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "tnr2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "tnr2") == U.bins(tmp / "tnr")
    _handed(seen, e2e["want"], FH, FW)


def test_feature_off_gives_the_plain_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    plain = U.bins(tmp / "plain")
    assert sorted(os.listdir(tmp / "plain")) == sorted(plain)
    RC.encode_folder(str(tmp / "png"), str(tmp / "none"), gop=GOP, nets=file_nets, tnr=None)
    assert U.bins(tmp / "none") == plain and sorted(os.listdir(tmp / "none")) == sorted(plain)
    with pytest.raises(ValueError, match="tnr.TNR"):
        RC.encode_folder(str(tmp / "png"), str(tmp / "never"), gop=GOP, nets=file_nets, tnr=12)
    assert not (tmp / "never").exists()


def test_command_line(e2e, file_nets, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "12", "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "tnr")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "tnr_rec", N_FRAMES)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli2"), "--gop", str(GOP), "--tnr", "6", "--tnr-floor", "32",
             "--tnr-pixel", "255"])
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "api2"), gop=GOP, nets=file_nets, tnr=N.TNR(6, 32, 255))
    assert U.bins(tmp / "cli2") == U.bins(tmp / "api2") and U.bins(tmp / "cli2") != U.bins(tmp / "tnr")
    _handed(seen, R.run(e2e["pics"], (6, 32, 255), INTRA), FH, FW)


@pytest.fixture(scope="module")
def reported(tmp_path_factory, file_nets):
    """the 176 x 192 clip coded with a report, plain and with the prefilter"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("tnr_report")
    pics = _write_pngs(tmp / "png", RH, FW)
    _, _, plain_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets, report=True)
    with _spies() as (seen, measured):
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), gop=GOP, nets=file_nets, report=str(tmp / "tnr.json"),
                                       tnr=SETTING)
    assert size == (RH, FW)
    return dict(tmp=tmp, pics=pics, seen=seen, measured=measured, rd=rd, plain_rd=plain_rd, want=R.run(pics, (12, 64, 36), INTRA))


def test_report_speaks_of_the_filter_and_measures_against_the_source(reported, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, rd, want, pics = reported["tmp"], reported["rd"], reported["want"], reported["pics"]
    _handed(reported["seen"], want, RH, FW)
    assert rd["tnr"] == {"threshold": 12, "floor": 64, "pixel": 36}
    assert rd["frame_tnr_held"] == [int(w[2].sum()) / (RH * FW) for w in want]
    assert rd["frame_tnr_mad"] == [int(w[1].sum()) / (RH * FW) for w in want]
    assert all((rd["frame_tnr_held"][t] == 0.0) == (t in INTRA) for t in range(N_FRAMES))
    assert all((rd["frame_tnr_mad"][t] == 0.0) == (t in INTRA) for t in range(N_FRAMES))
    assert json.loads((tmp / "tnr.json").read_text()) == rd
    assert set(rd) - set(reported["plain_rd"]) == {"tnr", "frame_tnr_held", "frame_tnr_mad"}
    assert set(reported["plain_rd"]) <= set(rd) and sorted(os.listdir(tmp / "tnr")) == sorted(U.bins(tmp / "tnr"))
    # PSNR and MS-SSIM are measured against the UNFILTERED source, which is not what the codec was handed
    for t in range(N_FRAMES):
        assert np.array_equal(reported["measured"][t][0, :, :RH, :FW].view(np.uint32), pics[t].view(np.uint32)), t
        assert np.array_equal(reported["measured"][t], reported["seen"][t]) == (t in INTRA), t
    assert len(rd["frame_psnr"]) == N_FRAMES and all(np.isfinite(rd["frame_psnr"]))
    # two GOP streams: the same bytes and the same figures of the filter
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, tnr=SETTING)
    assert U.bins(tmp / "tnr2") == U.bins(tmp / "tnr")
    for key in ("tnr", "frame_tnr_held", "frame_tnr_mad", "frame_bpp"):
        assert rd2[key] == rd[key], key
    # tnr=None: the bytes and the report keys of a run without the argument
    _, _, rd0 = RC.encode_folder(str(tmp / "png"), str(tmp / "none"), gop=GOP, nets=file_nets, report=True, tnr=None)
    assert U.bins(tmp / "none") == U.bins(tmp / "plain") and list(rd0) == list(reported["plain_rd"])
    assert rd0["frame_bpp"] == reported["plain_rd"]["frame_bpp"]


def test_y4m_file(reported, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp = reported["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(pic, dtype=np.float64)) for pic in reported["pics"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, RH, fps="30:1")
    # the pictures the conversion gives, taken through the coding pass's own path
    with Y.open_video(str(tmp / "src.y4m")) as reader:
        src = [x.cpu().numpy()[0, :, :RH, :FW] for x, _ in RC._video_pictures(reader, range(N_FRAMES), reader.spec(), False, DEV)]
    want = R.run(src, (12, 64, 36), INTRA)
    with _spies() as (seen, measured):
        _, _, rd = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), gop=GOP, nets=file_nets,
                                   gop_streams=2, report=True, tnr=SETTING)
    _handed(seen, want, RH, FW)
    for t in range(N_FRAMES):  # the report's source: unfiltered
        assert np.array_equal(measured[t][0, :, :RH, :FW].view(np.uint32), np.ascontiguousarray(src[t]).view(np.uint32)), t
    assert rd["frame_tnr_held"] == [int(w[2].sum()) / (RH * FW) for w in want] and rd["tnr"] == SETTING.to_json()
    assert rd["frame_tnr_mad"] == [int(w[1].sum()) / (RH * FW) for w in want] and "frame_psnr_yuv" in rd
    assert "tnr" not in RC.read_sequence_info(str(tmp / "vbins"))
    assert sorted(n for n in os.listdir(tmp / "vbins") if not n.endswith(".bin")) == ["sequence.json"]
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vplain"), gop=GOP, nets=file_nets)
    assert U.bins(tmp / "vplain") != U.bins(tmp / "vbins")
    assert (tmp / "vplain" / "sequence.json").read_text() == (tmp / "vbins" / "sequence.json").read_text()
