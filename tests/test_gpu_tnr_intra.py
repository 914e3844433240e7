"""The look-ahead filter of I pictures on a real MI355X, above the kernel: tnr.TnrFilter with tnr.intra bit for bit against
the stream rule of tests/tnr_fuse_ref.py (with and without the search), and the file loops end to end -- the pictures the
codec is handed, the bytes of a plain encode of the restatement's pictures, two GOP streams, a Y4M file whose report reads
the samples of pictures that waited, an unchanged decoder, the report's keys, the command line, and the film grain of
filtered I pictures."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import grain_ref as G
from tests import tnr_fuse_ref as FR
from tests import tnr_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from tests.test_gpu_tnr import FH, FW, GOP, N_FRAMES, RH, _handed, _padded, _spies, _write_pngs
from vcm_ts_amd import grain as GR
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ TnrFilter
def _gop_ahead(xs, t, intra):
    """Every later picture of picture t's GOP (more than any K: the filter takes the first K)."""
    out = []
    for s in range(t + 1, len(xs)):
        if s in intra:
            break
        out.append(xs[s])
    return out


@pytest.mark.parametrize("search", [None, 4], ids=["still", "search"])
@pytest.mark.parametrize("intra", [{0, 4}, {0, 8}], ids=["i04", "i08"])
def test_filter_blends_i_pictures_with_the_pictures_ahead(intra, search):
    H, W, Hp, Wp, K = 70, 100, 128, 128, 2
    pics, setting = R.sequences(H, W)["clip"], R.SETTINGS[0]
    want = FR.run(pics, setting, intra, K, search=None if search is None else (search, N.PENALTY))
    f = N.TnrFilter(N.TNR(*setting, search=search, intra=K), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.launches == 0 and f.comps.shape == (4, 3, Hp, Wp)
    xs = [torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV) for pic in pics]
    got, launches = [], []
    for t, x in enumerate(xs):
        before = f.launches
        y = f.step(x, t in intra, _gop_ahead(xs, t, intra))
        assert (y is x) == (want[t][3] == 0), t  # only an I picture with nothing ahead is returned itself
        assert f.refs == want[t][3], t
        launches.append(f.launches - before)
        got.append(y.cpu().numpy())  # (a buffer of the filter is valid until the step after the next: copy now)
    per_ref = 0 if search is None else 2  # (a search and a compensation per reference, then ONE blend)
    assert launches == [per_ref * w[3] + 1 if w[3] else 0 for w in want]
    assert [w[3] for w in want] == ([2, 1, 1, 1, 2, 1, 1, 1, 1] if intra == {0, 4} else [2, 1, 1, 1, 1, 1, 1, 1, 0])
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t  # (the padding: zeros)
        assert torch.equal(xs[t], torch.from_numpy(_padded(pics[t], Hp, Wp)).to(DEV)), t  # the sources are only read
    assert not np.array_equal(got[0][0, :, :H, :W], pics[0])  # the I picture is filtered
    if search is None:
        assert f.totals() == [(int(w[2].sum()), int(w[1].sum()), w[3]) for w in want]
    else:
        assert f.totals() == [(int(w[2].sum()), int(w[1].sum()), w[4], w[5], w[3]) for w in want]
    assert f.totals()[0][0] > 0 and f.totals()[0][1] > 0 and not f._done
    if intra == {0, 8}:
        assert f.totals()[8] == f.untouched and set(f.untouched) == {0}
    # the same pictures without the bookkeeping
    bare = N.TnrFilter(N.TNR(*setting, search=search, intra=K), (H, W), DEV, totals=False)
    for t in range(3):
        y = bare.step(xs[t], t in intra, _gop_ahead(xs, t, intra))
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == sum(launches[:3]) and bare._rows is None


def test_every_k_and_a_reference_with_strides_of_its_own():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting = R.sequences(H, W)["clip"], R.SETTINGS[0]
    tab = R.table(*setting[:2])
    xs = [torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV) for pic in pics[:5]]
    wide = torch.full((1, 3, Hp, Wp + 64), float("nan"), device=DEV)
    wide[..., :Wp] = xs[2]
    odd = wide[..., :Wp]  # (the same picture in rows 192 apart)
    assert odd.stride() != xs[2].stride() and torch.equal(odd, xs[2])
    for K in (1, 2, 3, 4):
        f = N.TnrFilter(N.TNR(*setting, intra=K), (H, W), DEV)
        y = f.step(xs[0], True, xs[1:])
        want = FR.fuse(pics[0], pics[1:1 + K], tab, setting[2])
        assert f.launches == 1 and f.refs == K
        assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(want[0], Hp, Wp).view(np.uint32)), K
        assert f.totals() == [(int(want[2].sum()), int(want[1].sum()), K)]
        if K >= 2:  # one reference lies elsewhere with other strides: it is copied, the result is the same
            g = N.TnrFilter(N.TNR(*setting, intra=K), (H, W), DEV)
            z = g.step(xs[0], True, [xs[1], odd] + xs[3:])
            assert g.launches == 1 and torch.equal(z, y), K
    with pytest.raises(ValueError, match="expected a"):
        N.TnrFilter(N.TNR(*setting, intra=2), (H, W), DEV).step(xs[0], True, [xs[1][..., :H, :W]])
    with pytest.raises(ValueError, match="no CPU fallback"):
        N.TnrFilter(N.TNR(*setting, intra=2), (H, W), DEV).step(xs[0], True, [xs[1].cpu()])


def test_without_intra_the_pictures_ahead_are_ignored():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = R.sequences(H, W)["clip"], R.SETTINGS[0], {0, 4}
    want = R.run(pics, setting, intra)
    f = N.TnrFilter(N.TNR(*setting), (H, W), DEV)
    assert not hasattr(f, "comps") and not hasattr(f, "rtab")  # nothing is allocated for what is not asked for
    xs = [torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV) for pic in pics]
    launches = []
    for t, x in enumerate(xs):
        y = f.step(x, t in intra, _gop_ahead(xs, t, intra))
        assert (y is x) == (t in intra), t
        launches.append(f.launches)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert launches == [0, 1, 2, 3, 3, 4, 5, 6, 7]
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum())) for w in want]


# -------------------------------------------------------------------------------------------------------- file loops
SETTING = N.TNR(8, intra=2)
TUPLE = (8, 64, 24)  # (T, floor, P) of SETTING
INTRA = {0, 4}
REFS = [2, 1, 1, 1, 2, 1, 1, 1]


@contextlib.contextmanager
def _png_source_of(pictures):
    """Inside, a PNG folder's pictures are `pictures` ((3, H, W) float32 by frame number) instead of its files': a plain
    encode of pictures that no 8-bit file can hold."""
    from vcm_ts_amd import run_codec as RC

    real = RC._png_pictures

    def fake(reader, order, size, dev, pool, io_workers, sharers):
        for g in order:
            yield RC.pad_frame(torch.from_numpy(np.ascontiguousarray(pictures[g]))[None].to(dev))

    RC._png_pictures = fake
    try:
        yield
    finally:
        RC._png_pictures = real


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the noisy clip as PNGs, coded with the look-ahead filter -- the pictures its codec was handed captured on the way --
    and, plainly, without any filter and from the restatement's filtered pictures"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("tnr_intra_e2e")
    pics = _write_pngs(tmp / "png", FH, FW)
    want = FR.run(pics, TUPLE, INTRA, 2)
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    with _spies() as (seen, _):
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), str(tmp / "tnr_rec"), gop=GOP, nets=file_nets,
                                      picture_hash=True, tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    with _png_source_of([w[0] for w in want]):
        RC.encode_folder(str(tmp / "png"), str(tmp / "restated"), gop=GOP, nets=file_nets)
    return dict(tmp=tmp, pics=pics, seen=seen, want=want)


def test_the_bins_are_those_of_a_plain_encode_of_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    assert [w[3] for w in e2e["want"]] == REFS
    for t in range(N_FRAMES):  # no picture is the source itself any more
        assert not np.array_equal(e2e["seen"][t][0], e2e["pics"][t]), t
    tmp = e2e["tmp"]
    tnr, restated, plain = U.bins(tmp / "tnr"), U.bins(tmp / "restated"), U.bins(tmp / "plain")
    assert list(tnr) == list(plain) and tnr == restated
    assert all(tnr[name] != plain[name] for name in tnr)  # the I pictures are other pictures now as well


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert sorted(n for n in os.listdir(tmp / "tnr") if not n.endswith(".bin")) == ["hashes.json"]  # no side file of the filter
    assert RC.decode_folder(str(tmp / "tnr"), str(tmp / "tnr_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "tnr_dec", tmp / "tnr_rec", N_FRAMES)


def test_two_gop_streams_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "tnr2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "tnr2") == U.bins(tmp / "tnr")
    _handed(seen, e2e["want"], FH, FW)


def test_command_line(e2e, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "8", "--tnr-intra", "2",
             "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "tnr")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "tnr_rec", N_FRAMES)
    with pytest.raises(SystemExit):
        RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "never"), "--gop", str(GOP), "--tnr-intra", "2"])
    assert "--tnr-intra belongs to --tnr" in capsys.readouterr().err and not (tmp / "never").exists()
    # K = 1 and a scene-cut-like plan of short GOPs: GOP 2 at K = 4 leaves one picture ahead of every I picture
    with _spies() as (seen, _):
        RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli2"), "--gop", "2", "--tnr", "8", "--tnr-intra", "4"])
    _handed(seen, FR.run(e2e["pics"], TUPLE, {0, 2, 4, 6}, 4), FH, FW)


@pytest.fixture(scope="module")
def reported(tmp_path_factory, file_nets):
    """the 176 x 192 clip coded with a report: plain, and with the searching look-ahead filter"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("tnr_intra_report")
    pics = _write_pngs(tmp / "png", RH, FW)
    _, _, plain_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets, report=True)
    with _spies() as (seen, measured):
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), gop=GOP, nets=file_nets, report=str(tmp / "tnr.json"),
                                       tnr=N.TNR(8, search=4, intra=2))
    assert size == (RH, FW)
    want = FR.run(pics, TUPLE, INTRA, 2, search=(4, N.PENALTY))
    return dict(tmp=tmp, pics=pics, seen=seen, measured=measured, rd=rd, plain_rd=plain_rd, want=want)


def test_report_has_figures_for_i_pictures_and_measures_against_the_source(reported, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, rd, want, pics = reported["tmp"], reported["rd"], reported["want"], reported["pics"]
    _handed(reported["seen"], want, RH, FW)
    cells = -(-RH // 16) * -(-FW // 16)
    assert rd["tnr"] == {"threshold": 8, "floor": 64, "pixel": 24, "search": 4, "penalty": 4, "intra": 2}
    assert rd["frame_tnr_held"] == [int(w[2].sum()) / (RH * FW) for w in want]
    assert rd["frame_tnr_mad"] == [int(w[1].sum()) / (RH * FW) for w in want]
    assert rd["frame_tnr_moved"] == [w[4] / cells for w in want]
    assert rd["frame_tnr_mad_zero"] == [w[5] / (RH * FW) for w in want]
    assert rd["frame_tnr_refs"] == REFS
    for key in ("frame_tnr_held", "frame_tnr_mad", "frame_tnr_mad_zero"):  # nonzero for the filtered I pictures too
        assert all(v > 0 for v in rd[key]), key
    assert json.loads((tmp / "tnr.json").read_text()) == rd
    assert set(rd) - set(reported["plain_rd"]) == {"tnr", "frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero",
                                                   "frame_tnr_refs"}
    assert set(reported["plain_rd"]) <= set(rd) and sorted(os.listdir(tmp / "tnr")) == sorted(U.bins(tmp / "tnr"))
    # PSNR and MS-SSIM are measured against the UNFILTERED source of the picture being coded, never of one pulled ahead
    for t in range(N_FRAMES):
        assert np.array_equal(reported["measured"][t][0, :, :RH, :FW].view(np.uint32), pics[t].view(np.uint32)), t
        assert not np.array_equal(reported["measured"][t], reported["seen"][t]), t
    assert len(rd["frame_psnr"]) == N_FRAMES and all(np.isfinite(rd["frame_psnr"]))
    # two GOP streams: the same bytes and the same figures
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr2"), gop=GOP, nets=file_nets, gop_streams=2, report=True,
                                 tnr=N.TNR(8, search=4, intra=2))
    assert U.bins(tmp / "tnr2") == U.bins(tmp / "tnr")
    for key in rd:
        if key.startswith("frame_") or key == "tnr":
            assert rd2[key] == rd[key], key
    # without intra the report has no new key
    _, _, rd1 = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr1"), gop=GOP, nets=file_nets, report=True, tnr=N.TNR(8, search=4))
    assert set(rd) - set(rd1) == {"frame_tnr_refs"} and "intra" not in rd1["tnr"]
    assert all((rd1["frame_tnr_held"][t] == 0.0) == (t in INTRA) for t in range(N_FRAMES))


@contextlib.contextmanager
def _samples_spy():
    """{frame number: the file's samples the report's YUV figures were measured against} of the encodes run inside."""
    from vcm_ts_amd import run_codec as RC

    seen, last = {}, [None]
    measure, add_yuv = RC._VideoStage.measure, RC._VideoQualityLog.add_yuv

    def spy_measure(self, k, frame, samples):
        last[0] = samples.cpu().numpy().copy()
        return measure(self, k, frame, samples)

    def spy_add_yuv(self, g, recon, source, size, sums):
        seen[g] = last[0]
        return add_yuv(self, g, recon, source, size, sums)

    RC._VideoStage.measure, RC._VideoQualityLog.add_yuv = spy_measure, spy_add_yuv
    try:
        yield seen
    finally:
        RC._VideoStage.measure, RC._VideoQualityLog.add_yuv = measure, add_yuv


def test_y4m_file_with_a_report(reported, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp = reported["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(pic, dtype=np.float64)) for pic in reported["pics"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, RH, fps="30:1")
    with Y.open_video(str(tmp / "src.y4m")) as reader:  # the pictures and the samples, through the coding pass's own path
        pairs = [(x.cpu().numpy()[0, :, :RH, :FW], s.cpu().numpy().copy())
                 for x, s in RC._video_pictures(reader, range(N_FRAMES), reader.spec(), False, DEV)]
    src, samples = [p[0] for p in pairs], [p[1] for p in pairs]
    assert all(not np.array_equal(samples[t], samples[t + 1]) for t in range(N_FRAMES - 1))
    want = FR.run(src, TUPLE, INTRA, 2)
    runs = {}
    for streams in (1, 2):
        with _spies() as (seen, measured), _samples_spy() as aux:
            _, _, rd = RC.encode_video(str(tmp / "src.y4m"), str(tmp / f"vbins{streams}"), str(tmp / f"enc{streams}.y4m"), gop=GOP,
                                       nets=file_nets, gop_streams=streams, report=True, tnr=SETTING)
        _handed(seen, want, RH, FW)
        for t in range(N_FRAMES):  # the report's source and samples: the unfiltered picture being coded, even where it had waited
            assert np.array_equal(measured[t][0, :, :RH, :FW].view(np.uint32), np.ascontiguousarray(src[t]).view(np.uint32)), t
            assert np.array_equal(aux[t], samples[t]), t
        assert rd["frame_tnr_held"] == [int(w[2].sum()) / (RH * FW) for w in want] and rd["tnr"] == SETTING.to_json()
        assert rd["frame_tnr_mad"] == [int(w[1].sum()) / (RH * FW) for w in want] and rd["frame_tnr_refs"] == REFS
        assert "frame_tnr_moved" not in rd and len(rd["frame_psnr_yuv"]) == N_FRAMES and all(np.isfinite(rd["frame_psnr_yuv"]))
        runs[streams] = rd
    assert U.bins(tmp / "vbins2") == U.bins(tmp / "vbins1")
    assert (tmp / "enc2.y4m").read_bytes() == (tmp / "enc1.y4m").read_bytes()
    for key in runs[1]:
        if key.startswith("frame_"):
            assert runs[2][key] == runs[1][key], key
    assert "tnr" not in RC.read_sequence_info(str(tmp / "vbins1"))
    assert sorted(n for n in os.listdir(tmp / "vbins1") if not n.endswith(".bin")) == ["sequence.json"]
    assert RC.decode_video(str(tmp / "vbins1"), str(tmp / "dec.y4m")) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc1.y4m").read_bytes()


# ------------------------------------------------------------------------------------------------------------- the grain
def _record(pics, want):
    """{first picture of a GOP: params} where every picture the filter blended is measured, the I pictures included."""
    gops, acc, first = {}, None, None
    for t in range(len(pics)):
        if t in INTRA:
            if first is not None:
                gops[first] = G.params(acc, 1024)
            first, acc = t, np.zeros(G.WORDS, dtype=np.int64)
        if want[t][3]:
            acc = G.measure(np.asarray(pics[t], dtype=F32), want[t][0], want[t][2], acc)
    gops[first] = G.params(acc, 1024)
    return gops


def test_grain_measures_and_grains_the_filtered_i_pictures(e2e, file_nets):
    from tests.test_gpu_grain import _files, _shown
    from vcm_ts_amd import run_codec as RC

    tmp, pics, want = e2e["tmp"], e2e["pics"], e2e["want"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "grain"), gop=GOP, nets=file_nets, picture_hash=True, tnr=SETTING, grain=GR.Grain())
    gops = _record(pics, want)
    record = json.loads((tmp / "grain" / "grain.json").read_text())
    assert record == {"version": 1, "min_samples": 1024, "tnr": {"threshold": 8, "floor": 64, "pixel": 24, "intra": 2},
                      "gops": {str(g): gops[g] for g in sorted(gops)}}
    # the GOP's counts include the I picture's pixels: more than the P pictures' alone
    p_only = G.record(pics, TUPLE, INTRA, 1024)[0]
    for g in gops:
        i_counts = G.measure(np.asarray(pics[g], dtype=F32), want[g][0], want[g][2])[0::4]
        assert int(i_counts.sum()) > 0 and sum(gops[g]["counts"]) > int(i_counts.sum())
        assert all(max(rec["points"]) > 0 for rec in gops.values()) and sum(gops[g]["counts"]) != sum(p_only[g]["counts"])
    with_, without = _files(tmp / "grain"), _files(tmp / "tnr")
    assert sorted(set(with_) - set(without)) == ["grain.json"] and all(with_[n] == without[n] for n in without)
    RC.encode_folder(str(tmp / "png"), str(tmp / "grain2"), gop=GOP, nets=file_nets, gop_streams=2, picture_hash=True, tnr=SETTING,
                     grain=GR.Grain())
    assert _files(tmp / "grain2") == with_  # two GOP streams: the same record, the same bytes
    # decode --grain changes the I pictures too, by the restatement's rule
    with _shown() as plain:
        assert RC.decode_folder(str(tmp / "grain"), str(tmp / "dec"), FH, FW, gop=GOP) == N_FRAMES
    with _shown() as grained:
        assert RC.decode_folder(str(tmp / "grain"), str(tmp / "dec_g"), FH, FW, gop=GOP, grain=100, verify="strict") == N_FRAMES
    first = None
    for t in range(N_FRAMES):
        first = t if t in INTRA else first
        rec = gops[first]
        pic = plain[t][0, :, :FH, :FW]
        shown = G.apply(pic, t, rec["kh"], rec["kv"], G.table(rec["points"], rec["kh"], rec["kv"], 100))
        assert np.array_equal(_bits(grained[t][0, :, :FH, :FW]), _bits(shown)), t
        assert not np.array_equal(grained[t][0, :, :FH, :FW], pic), t
    # a record without `intra` leaves the I pictures untouched: the same folder under a record that does not say it
    stripped = dict(record, tnr={k: v for k, v in record["tnr"].items() if k != "intra"})
    (tmp / "grain" / "grain.json").write_text(json.dumps(stripped))
    with _shown() as old:
        RC.decode_folder(str(tmp / "grain"), str(tmp / "dec_o"), FH, FW, gop=GOP, grain=100)
    for t in range(N_FRAMES):
        assert np.array_equal(old[t], plain[t]) == (t in INTRA), t
        if t not in INTRA:
            assert np.array_equal(old[t], grained[t]), t
