"""Quarter-pel motion on a real MI355X: dcvc_me_refine and dcvc_me_compensate_sub bit for bit against the numpy restatement
(tests/mesub_ref.py) in tests/test_gpu_me.py's strided, offset, NaN-surrounded layouts with guarded outputs, whole vectors
against dcvc_me_compensate on the device, TnrFilter(subpel=True) with and without the look-ahead, and the file loops end to
end: the pictures the codec is handed, an unchanged decoder, the report, two GOP streams, the command line."""
import json

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import me_ref as M
from tests import mesub_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from tests.test_gpu_me import LAYOUTS, SENT16, SENT32, _cells, _handed, _padded, _spy, _tensors
from vcm_ts_amd import lib
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
RADIUS = 8


def _refine(cur, ref, lam, mv_in, H, W, layout, want, where):
    """One dcvc_me_refine in `layout`, held against want = (mvq, cost)."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kc, vc, crs, cps, mask = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)
    kr, vr, rrs, rps, _ = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
    mv[m0:m0 + 2 * n] = torch.from_numpy(np.asarray(mv_in).astype(np.int16).reshape(-1)).to(DEV)
    mvq, q0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)  # (fresh sentinels every time: every cell is WRITTEN)
    cost, c0 = U.guarded(n, shift, np.uint32, SENT32, DEV)
    lib.check(lib.hip().dcvc_me_refine(vc.data_ptr(), crs, cps, vr.data_ptr(), rrs, rps, H, W, lam, mv.data_ptr() + 2 * m0,
                                       mvq.data_ptr() + 2 * q0, cost.data_ptr() + 4 * c0, U.stream(DEV)), "me_refine")
    _cells(mvq, q0, 2 * n, want[0], SENT16, where)
    _cells(cost, c0, n, want[1], SENT32, where)
    _cells(mv, m0, 2 * n, mv_in, SENT16, where)  # the inputs are only read, and nothing beside them is written
    for k, pic in ((kc, cur), (kr, ref)):
        got = k.cpu().numpy()
        assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(pic).reshape(-1).view(np.uint32)), where
        assert np.isnan(got[~mask]).all(), where


def _compensate(ref, vectors, H, W, layout, where, whole=False):
    """One dcvc_me_compensate_sub in `layout`, held against the restatement on the bits the device holds; whole: the
    vectors are all multiples of 4, and dcvc_me_compensate with a quarter of them gives the same bits on the device."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kr, vr, rrs, rps, mask = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
    mv[m0:m0 + 2 * n] = torch.from_numpy(np.asarray(vectors).astype(np.int16).reshape(-1)).to(DEV)
    before = kr.cpu().numpy()
    held = before[mask].reshape(3, H, W)  # (the bits as the device holds them)
    lib.check(lib.hip().dcvc_me_compensate_sub(vr.data_ptr(), rrs, rps, vo.data_ptr(), ors, ops, H, W, mv.data_ptr() + 2 * m0,
                                               U.stream(DEV)), "me_compensate_sub")
    got = ko.cpu().numpy()
    want = R.compensate_sub(held, vectors)
    assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32)), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    assert np.array_equal(kr.cpu().numpy().view(np.uint32), before.view(np.uint32)), where
    _cells(mv, m0, 2 * n, vectors, SENT16, where)
    if whole:
        assert not (np.asarray(vectors) & 3).any()
        k2, v2, _, _, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
        mv[m0:m0 + 2 * n] = torch.from_numpy((np.asarray(vectors) >> 2).astype(np.int16).reshape(-1)).to(DEV)
        lib.check(lib.hip().dcvc_me_compensate(vr.data_ptr(), rrs, rps, v2.data_ptr(), ors, ops, H, W, mv.data_ptr() + 2 * m0, U.stream(DEV)),
                  "me_compensate")
        assert np.array_equal(k2.cpu().numpy()[mask].view(np.uint32), got[mask].view(np.uint32)), where
    return want


def _refine_pairs(H, W):
    """name -> [(cur, ref)]: tests/me_ref.py's pairs, and pairs whose cur is ref moved by a fraction of a pixel."""
    pairs = dict(M.pairs(H, W, RADIUS))
    pairs["shifted"] = [R.shifted_pair(H, W, (0, 2)), R.shifted_pair(H, W, (-7, 13))]
    return pairs


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_refine_equals_the_restatement(size):
    H, W = size
    fractional = 0
    for name, todo in _refine_pairs(H, W).items():
        for n, (cur, ref) in enumerate(todo):
            fields = {"search": M.search(cur, ref, RADIUS, 4)[0]}
            if name in ("clip", "shifted"):  # (the clamp of d: words far outside +-32)
                fields["wild"] = M.wild_vectors(H, W)
            for kind, mv_in in fields.items():
                table = R.sad_table(cur, ref, mv_in)
                for lam in M.LAMBDAS:
                    want = R.refine(cur, ref, lam, mv_in, table)
                    for k, layout in enumerate(LAYOUTS):
                        if name != "clip" and k not in (0, 1 + (lam + n + len(name)) % 3):  # (every layout on the clip, two on the others)
                            continue
                        _refine(cur, ref, lam, mv_in, H, W, layout, want, (name, n, kind, lam, layout))
                    mvq, cost = want
                    fractional += int((mvq & 3).any())
                    assert not mvq[(H + 15) // 16:].any() and not mvq[:, (W + 15) // 16:].any() and not cost[(H + 15) // 16:].any()
                    if name == "flat" and kind == "search":  # every candidate matches: the shortest, around d = 0
                        assert not mvq.any() and not cost.any()
                    if name == "shifted" and kind == "search" and lam == 0 and n == 0 and H >= 48 and W >= 48:
                        assert (mvq[1:H // 16 - 1, 1:W // 16 - 1] == (0, 2)).all()
    assert fractional or H * W < 16


def test_refine_finds_the_fraction_a_picture_was_moved_by():
    """64 x 96, searched within +-2: every full cell returns the quarter-pel vector at cost 0."""
    H, W = 64, 96
    for v, layout in (((0, 2), LAYOUTS[0]), ((-7, 13), LAYOUTS[1]), ((5, -3), LAYOUTS[2])):
        cur, ref = R.shifted_pair(H, W, v)
        mv = M.search(cur, ref, 4, 0)[0]
        want = R.refine(cur, ref, 0, mv)
        assert (want[0][:4, :6] == v).all() and not want[1].any(), v
        _refine(cur, ref, 0, mv, H, W, layout, want, v)


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compensation_equals_the_restatement(size):
    H, W = size
    g = np.random.default_rng(H + 1000 * W)
    pics = {"arbitrary": g.uniform(-0.1, 1.1, (3, H, W)).astype(F32), "8 bit": g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0),
            "odd bits": M.odd_bits(H, W)}
    fields = {"random": R.random_quarters(H, W), "far": R.far_quarters(H, W), "whole": 4 * M.wild_vectors(H, W).clip(-8000, 8000),
              "fours": 16 * M.wild_vectors(H, W, seed=5).clip(-8, 8), "still": np.zeros(R.grid(H, W) + (2,), dtype=np.int64)}
    assert {-32768, 32767} <= set(fields["far"].reshape(-1).tolist()) and (fields["random"] & 3).any()
    for name, vectors in fields.items():
        whole = name in ("whole", "fours", "still")
        for k, layout in enumerate(LAYOUTS):
            for kind, pic in pics.items():
                if whole and kind == "8 bit":  # (bits are copied: the arbitrary and the odd samples say it all)
                    continue
                want = _compensate(pic, vectors, H, W, layout, (name, kind, layout), whole=whole)
                if not whole:
                    frac = np.repeat(np.repeat((vectors & 3).any(axis=2), 16, axis=0), 16, axis=1)[:H, :W]
                    assert (want[:, frac] >= 0).all() and (want[:, frac] <= 1).all()
                if name == "still" and kind == "arbitrary":
                    assert np.array_equal(want.view(np.uint32), pic.view(np.uint32))
    # the refined vectors of the clip, as TnrFilter hands them over
    noisy = M.clip(H, W)[0]
    mvq = R.refine(noisy[5], noisy[4], 4, M.search(noisy[5], noisy[4], RADIUS, 4)[0])[0]
    _compensate(noisy[4], mvq, H, W, LAYOUTS[0], "clip")


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    n = int(np.prod(R.grid(H, W)))
    noisy = M.clip(H, W)[0]
    kc, vc, crs, cps, mask = U.strided(noisy[5], H, W, 8, 24, 12, DEV)
    kr, vr, rrs, rps, _ = U.strided(noisy[4], H, W, 8, 24, 12, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, 8, 24, 12, DEV)
    found = M.search(noisy[5], noisy[4], RADIUS, 4)[0]
    mv, m0 = U.guarded(2 * n, 0, np.uint16, SENT16, DEV)
    mv[m0:m0 + 2 * n] = torch.from_numpy(found.astype(np.int16).reshape(-1)).to(DEV)
    mvq, q0 = U.guarded(2 * n, 0, np.uint16, SENT16, DEV)
    cost, c0 = U.guarded(n, 0, np.uint32, SENT32, DEV)
    good = dict(cur=vc.data_ptr(), crs=crs, cps=cps, ref=vr.data_ptr(), rrs=rrs, rps=rps, H=H, W=W, lam=4, mv=mv.data_ptr() + 2 * m0,
                mvq=mvq.data_ptr() + 2 * q0, cost=cost.data_ptr() + 4 * c0)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "lam", "mv", "mvq", "cost")
    bad = [{k: None} for k in ("cur", "ref", "mv", "mvq", "cost")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"lam": -1}, {"lam": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * crs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost")] + [{"mv": good["mv"] + 1}, {"mvq": good["mvq"] + 1}] + \
          [{"mvq": good["mv"]}, {"mvq": good["mv"] + 4 * n - 2}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_refine(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(mvq) == SENT16).all() and (U.words(cost) == SENT32).all()
    _cells(mv, m0, 2 * n, found, SENT16, "refused")
    assert lib.hip().dcvc_me_refine(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.refine(noisy[5], noisy[4], 4, found)
    _cells(mvq, q0, 2 * n, want[0], SENT16, "good")
    _cells(cost, c0, n, want[1], SENT32, "good")

    span = 4 * (2 * rps + (H - 1) * rrs + W)
    good = dict(ref=vr.data_ptr(), rrs=rrs, rps=rps, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W, mv=mvq.data_ptr() + 2 * q0)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rrs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"ref": good["out"] + 4 * ops},
           {"ref": good["out"] + 4 * (H - 1) * ors}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate_sub(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_me_compensate_sub(*[good[k] for k in order], U.stream(DEV)) == 0
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), R.compensate_sub(noisy[4], want[0]).reshape(-1).view(np.uint32))
    assert np.array_equal(kr.cpu().numpy()[mask].view(np.uint32), noisy[4].reshape(-1).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ TnrFilter
STEP = (0.5, 0.75)  # what the object of the sub-pel clip moves by, pixels a picture


def test_filter_with_subpel_equals_the_restatement():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = list(R.subpel_clip(STEP, size=(H, W))[0]), R.SETTING, {0, 4}
    want = R.run(pics, setting, intra, RADIUS, 4)
    f = N.TnrFilter(N.TNR(*setting, search=RADIUS, subpel=True), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.grid == R.grid(H, W) and f.launches == 0 and f.untouched == (0, 0, 0, 0, 0)
    assert _tensors(f) == sorted(["bufs", "wtab", "sad", "held", "_rows", "comp", "mv", "cost", "zero", "mvq", "costq"])
    got, launches = [], []
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        y = f.step(x, t in intra)
        assert (y is x) == (t in intra), t
        launches.append(f.launches)
        got.append(y.cpu().numpy())
        assert torch.equal(x, torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV))  # the source is only read
        if t not in intra:  # the cells of the step, and an interpolated picture whose padding stays zero
            assert np.array_equal(f.mvq.cpu().numpy().astype(np.int64), want[t][3].reshape(-1)), t
            assert np.array_equal(U.words(f.costq), want[t][4].reshape(-1)) and np.array_equal(U.words(f.zero), want[t][5].reshape(-1)), t
            comp = _padded(R.compensate_sub(want[t - 1][0], want[t][3]), Hp, Wp)
            assert np.array_equal(f.comp.cpu().numpy().view(np.uint32), comp.view(np.uint32)), t
    assert launches == [0, 4, 8, 12, 12, 16, 20, 24]  # a P picture: search, refine, compensate_sub, step
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [R.totals(w, H, W) for w in want]
    assert f.totals()[4] == (0, 0, 0, 0, 0) and 0 < f.totals()[5][4] <= f.totals()[5][2] and not f._done  # (frac among moved)
    bare = N.TnrFilter(N.TNR(*setting, search=RADIUS, subpel=True), (H, W), DEV, totals=False)
    for t, pic in enumerate(pics[:3]):
        y = bare.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == 8 and bare._rows is None
    # without subpel the filter owns and launches what it did
    plain = N.TnrFilter(N.TNR(*setting, search=RADIUS), (H, W), DEV)
    assert _tensors(plain) == sorted(["bufs", "wtab", "sad", "held", "_rows", "comp", "mv", "cost", "zero"]) and plain.untouched == (0, 0, 0, 0)


def test_filter_with_subpel_and_look_ahead_equals_the_restatement():
    H, W, Hp, Wp, K = 70, 100, 128, 128, 2
    pics, setting, intra = list(R.subpel_clip(STEP, size=(H, W))[0]), R.SETTING, {0, 4}
    want = R.run_intra(pics, setting, intra, K, RADIUS, 4)
    f = N.TnrFilter(N.TNR(*setting, search=RADIUS, intra=K, subpel=True), (H, W), DEV)
    assert f.mvqs.shape == (4, 2 * 64) and f.costqs.shape == (4, 64) and f.untouched == (0, 0, 0, 0, 0, 0)
    xs = [torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV) for pic in pics]
    launches, got = [], []
    for t, x in enumerate(xs):
        ahead = []
        for s in range(t + 1, len(xs)):
            if s in intra:
                break
            ahead.append(xs[s])
        before = f.launches
        y = f.step(x, t in intra, ahead)
        launches.append(f.launches - before)
        got.append(y.cpu().numpy())
    assert [w[3] for w in want] == [2, 1, 1, 1, 2, 1, 1, 1]
    assert launches == [3 * w[3] + 1 for w in want]  # per reference a search, a refinement and a compensation, then ONE blend
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum()), w[4], w[5], w[6], w[3]) for w in want]
    assert any(w[6] for w in want)


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW, RH, RW = 4, 8, 96, 128, 176, 192
SETTING = N.TNR(*R.SETTING, search=RADIUS, subpel=True)
INTRA = {0, 4}


def _write_pngs(folder, size):
    """The noisy sub-pel clip as PNGs -> what u8_to_unit_float uploads of them, (3, H, W) float32 each."""
    u8 = np.rint(R.subpel_clip(STEP, size=size)[0] * 255).astype(np.uint8)
    U.write_pngs(folder, u8.transpose(0, 2, 3, 1))
    return [a.astype(F32) / F32(255.0) for a in u8]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the 96 x 128 sub-pel clip as PNGs, coded with the whole-pel search and with the refinement behind it"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("mesub_e2e")
    pics = _write_pngs(tmp / "png", (FH, FW))
    RC.encode_folder(str(tmp / "png"), str(tmp / "me"), gop=GOP, nets=file_nets, tnr=N.TNR(*R.SETTING, search=RADIUS))
    with _spy() as seen:
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "sub"), str(tmp / "sub_rec"), gop=GOP, nets=file_nets, picture_hash=True,
                                      tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, seen=seen, want=R.run(pics, R.SETTING, INTRA, RADIUS, 4))


def test_the_codec_is_handed_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    assert any((w[3] & 3).any() for w in e2e["want"])  # (and fractional vectors were chosen: the test is about interpolated pictures)
    whole = R.run(e2e["pics"], R.SETTING, INTRA, RADIUS, 4, subpel=False)
    assert any(not np.array_equal(whole[t][0], e2e["want"][t][0]) for t in range(N_FRAMES))


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert U.others(tmp / "sub") == ["hashes.json"]  # no side file of the filter, the search or the refinement
    sub, me = U.bins(tmp / "sub"), U.bins(tmp / "me")
    assert list(sub) == list(me) and sub != me
    for t in INTRA:  # I pictures are handed over as they are
        assert sub[f"im{t + 1:05d}.bin"] == me[f"im{t + 1:05d}.bin"], t
    assert RC.decode_folder(str(tmp / "sub"), str(tmp / "sub_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "sub_dec", tmp / "sub_rec", N_FRAMES)


def test_two_gop_streams_and_the_command_line_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spy() as seen:
        RC.encode_folder(str(tmp / "png"), str(tmp / "sub2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "sub2") == U.bins(tmp / "sub")
    _handed(seen, e2e["want"], FH, FW)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "12", "--tnr-search", "8",
             "--tnr-subpel", "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "sub")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "sub_rec", N_FRAMES)


def test_report_speaks_of_the_refinement(tmp_path, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path
    pics = _write_pngs(tmp / "png", (RH, RW))
    want = R.run(pics, R.SETTING, INTRA, RADIUS, 4)
    _, _, whole_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "me"), gop=GOP, nets=file_nets, report=True, tnr=N.TNR(*R.SETTING, search=RADIUS))
    with _spy() as seen:
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "sub"), gop=GOP, nets=file_nets, report=str(tmp / "sub.json"), tnr=SETTING)
    assert size == (RH, RW)
    _handed(seen, want, RH, RW)
    cells = M.cells_with_a_pixel(RH, RW)
    assert rd["tnr"] == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4, "subpel": 4}
    assert rd["frame_tnr_held"] == [R.totals(w, RH, RW)[0] / (RH * RW) for w in want]
    assert rd["frame_tnr_mad"] == [R.totals(w, RH, RW)[1] / (RH * RW) for w in want]
    assert rd["frame_tnr_moved"] == [R.totals(w, RH, RW)[2] / cells for w in want]
    assert rd["frame_tnr_mad_zero"] == [R.totals(w, RH, RW)[3] / (RH * RW) for w in want]
    assert rd["frame_tnr_subpel"] == [R.totals(w, RH, RW)[4] / cells for w in want]
    assert all((rd["frame_tnr_subpel"][t] == 0.0) == (t in INTRA) for t in range(N_FRAMES))
    assert json.loads((tmp / "sub.json").read_text()) == rd
    assert set(rd) - set(whole_rd) == {"frame_tnr_subpel"} and set(whole_rd) <= set(rd) and "subpel" not in whole_rd["tnr"]
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "sub2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, tnr=SETTING)
    assert U.bins(tmp / "sub2") == U.bins(tmp / "sub")
    for key in ("tnr", "frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero", "frame_tnr_subpel", "frame_bpp"):
        assert rd2[key] == rd[key], key
