"""Vectors per 8 x 8 sub-cell on a real MI355X: dcvc_me_split and dcvc_me_compensate_split bit for bit against the numpy
restatement (tests/mesplit_ref.py) in tests/test_gpu_me.py's strided, offset, NaN-surrounded layouts with guarded outputs,
repeated cell vectors against dcvc_me_compensate_sub on the device, TnrFilter(split=True) with and without the refinement
and the look-ahead, and the file loops end to end: the pictures the codec is handed, an unchanged decoder, the report, two
GOP streams, the command line."""
import json

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import me_ref as M
from tests import mesplit_ref as R
from tests import mesub_ref as S
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from tests.test_gpu_me import LAYOUTS, SENT16, SENT32, _cells, _handed, _padded, _spy, _tensors
from vcm_ts_amd import lib
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
RADIUS = 8


def _split(cur, ref, lam, unit, mv_in, H, W, layout, want, where):
    """One dcvc_me_split in `layout`, held against want = (mv8, cost8)."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kc, vc, crs, cps, mask = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)
    kr, vr, rrs, rps, _ = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
    mv[m0:m0 + 2 * n] = torch.from_numpy(np.asarray(mv_in).astype(np.int16).reshape(-1)).to(DEV)
    mv8, q0 = U.guarded(8 * n, shift, np.uint16, SENT16, DEV)  # (fresh sentinels every time: every sub-cell is WRITTEN)
    cost8, c0 = U.guarded(4 * n, shift, np.uint32, SENT32, DEV)
    lib.check(lib.hip().dcvc_me_split(vc.data_ptr(), crs, cps, vr.data_ptr(), rrs, rps, H, W, lam, unit, mv.data_ptr() + 2 * m0,
                                      mv8.data_ptr() + 2 * q0, cost8.data_ptr() + 4 * c0, U.stream(DEV)), "me_split")
    _cells(mv8, q0, 8 * n, want[0], SENT16, where)
    _cells(cost8, c0, 4 * n, want[1], SENT32, where)
    _cells(mv, m0, 2 * n, mv_in, SENT16, where)  # the inputs are only read, and nothing beside them is written
    for k, pic in ((kc, cur), (kr, ref)):
        got = k.cpu().numpy()
        assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(pic).reshape(-1).view(np.uint32)), where
        assert np.isnan(got[~mask]).all(), where


def _compensate(ref, mv8, H, W, layout, where, cells=None):
    """One dcvc_me_compensate_split in `layout`, held against the restatement on the bits the device holds; cells: mv8 is
    these cells' vectors repeated, and dcvc_me_compensate_sub with them gives the same bits ON THE DEVICE."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kr, vr, rrs, rps, mask = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(8 * n, shift, np.uint16, SENT16, DEV)
    mv[m0:m0 + 8 * n] = torch.from_numpy(np.asarray(mv8).astype(np.int16).reshape(-1)).to(DEV)
    before = kr.cpu().numpy()
    held = before[mask].reshape(3, H, W)  # (the bits as the device holds them)
    lib.check(lib.hip().dcvc_me_compensate_split(vr.data_ptr(), rrs, rps, vo.data_ptr(), ors, ops, H, W, mv.data_ptr() + 2 * m0,
                                                 U.stream(DEV)), "me_compensate_split")
    got = ko.cpu().numpy()
    want = R.compensate_split(held, mv8)
    assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32)), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    assert np.array_equal(kr.cpu().numpy().view(np.uint32), before.view(np.uint32)), where
    _cells(mv, m0, 8 * n, mv8, SENT16, where)
    if cells is not None:
        assert np.array_equal(R.repeated(cells), mv8)
        k2, v2, _, _, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
        mvq, z0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
        mvq[z0:z0 + 2 * n] = torch.from_numpy(np.asarray(cells).astype(np.int16).reshape(-1)).to(DEV)
        lib.check(lib.hip().dcvc_me_compensate_sub(vr.data_ptr(), rrs, rps, v2.data_ptr(), ors, ops, H, W, mvq.data_ptr() + 2 * z0, U.stream(DEV)),
                  "me_compensate_sub")
        assert np.array_equal(k2.cpu().numpy()[mask].view(np.uint32), got[mask].view(np.uint32)), where
    return want


def _split_pairs(H, W):
    """name -> [(cur, ref)]: tests/me_ref.py's pairs, and pairs whose cur is ref moved by a fraction of a pixel."""
    pairs = dict(M.pairs(H, W, RADIUS))
    pairs["shifted"] = [S.shifted_pair(H, W, (0, 2)), S.shifted_pair(H, W, (-7, 13))]
    return pairs


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_equals_the_restatement(size):
    H, W = size
    left = 0
    for name, todo in _split_pairs(H, W).items():
        for n, (cur, ref) in enumerate(todo):
            found = M.search(cur, ref, RADIUS, 4)[0]
            fields = {"search": (found, 1)}
            if name in ("clip", "shifted"):  # (the refinement's vectors, and words far outside the clamps)
                fields.update(refine=(S.refine(cur, ref, 4, found)[0], 4), wild=(M.wild_vectors(H, W), 1),
                              random=(S.random_quarters(H, W), 4), far=(S.far_quarters(H, W), 4))
            for kind, (mv_in, unit) in fields.items():
                table = R.sad8_table(cur, ref, mv_in, unit)
                for lam in M.LAMBDAS:
                    want = R.split(cur, ref, lam, mv_in, unit, table)
                    for k, layout in enumerate(LAYOUTS):
                        if (name != "clip" or kind not in ("search", "refine")) and k not in (0, 1 + (lam + n + len(name) + len(kind)) % 3):
                            continue  # (every layout on the clip's own vectors, two on the others)
                        _split(cur, ref, lam, unit, mv_in, H, W, layout, want, (name, n, kind, lam, layout))
                    mv8, cost8 = want
                    left += R.left(mv8, R.quarters(mv_in, unit), H, W)
                    assert not mv8[-(-H // 8):].any() and not mv8[:, -(-W // 8):].any() and not cost8[-(-H // 8):].any()
                    if name == "flat" and kind == "search":  # every candidate is (0, 0)
                        assert not mv8.any() and not cost8.any()
    assert left or H * W <= 256  # (and some sub-cell left its cell's vector)


def test_nine_equal_and_nine_different_candidates():
    """70 x 100.  One vector everywhere, whole (nothing is staged) or fractional (one candidate is): every sub-cell that holds
    a pixel returns it.  No two cells alike: every cell inside the grid weighs nine distinct candidates."""
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    noisy = S.subpel_clip((2.25, 5.5), size=(H, W))[0]
    cur, ref = noisy[4], noisy[3]
    for v, unit in (((0, 0), 1), ((3, -2), 1), ((-32, 32), 1), ((12, -8), 4), ((5, -6), 4), ((-131, 130), 4), ((0, 2), 4)):
        mv_in = np.broadcast_to(np.array(v), (hc, wc, 2))
        for lam, layout in zip(M.LAMBDAS, LAYOUTS):
            want = R.split(cur, ref, lam, mv_in, unit)
            assert (want[0][:-(-H // 8), :-(-W // 8)] == np.array(v) * (4 // unit)).all()
            _split(cur, ref, lam, unit, mv_in, H, W, layout, want, (v, unit, lam))
    mv_in = R.distinct_vectors(H, W)
    assert len({tuple(v) for v in mv_in.reshape(-1, 2).tolist()}) == hc * wc
    table = R.sad8_table(cur, ref, mv_in, 4)
    assert max(len(t) for t in table.values()) == 9
    for lam, layout in zip(M.LAMBDAS + (17,), LAYOUTS):
        _split(cur, ref, lam, 4, mv_in, H, W, layout, R.split(cur, ref, lam, mv_in, 4, table), ("distinct", lam))


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compensation_equals_the_restatement(size):
    H, W = size
    g = np.random.default_rng(H + 1000 * W)
    pics = {"arbitrary": g.uniform(-0.1, 1.1, (3, H, W)).astype(F32), "8 bit": g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0),
            "odd bits": M.odd_bits(H, W)}
    fields = {"random": R.sub_vectors(H, W), "half whole": R.sub_vectors(H, W, seed=31, whole=0.5), "whole": R.sub_vectors(H, W, seed=37, whole=1.0),
              "still": np.zeros(R.sub_grid(H, W) + (2,), dtype=np.int64)}
    assert {-32768, 32767} <= set(fields["random"].reshape(-1).tolist())  # (the far words are in every field, also the whole one)
    for name, mv8 in fields.items():
        for k, layout in enumerate(LAYOUTS):
            for kind, pic in pics.items():
                if name in ("whole", "still") and kind == "8 bit":  # (bits are copied: the arbitrary and the odd samples say it all)
                    continue
                want = _compensate(pic, mv8, H, W, layout, (name, kind, layout))
                if name == "still" and kind == "arbitrary":
                    assert np.array_equal(want.view(np.uint32), pic.view(np.uint32))
    # every cell's vector repeated: the cell's own path, and dcvc_me_compensate_sub's bits on the device
    for name, mvq in (("random", S.random_quarters(H, W)), ("far", S.far_quarters(H, W)), ("whole", 4 * M.wild_vectors(H, W).clip(-8000, 8000))):
        for k, layout in enumerate(LAYOUTS):
            _compensate(pics["odd bits" if k % 2 else "arbitrary"], R.repeated(mvq), H, W, layout, ("repeated", name, layout), cells=mvq)
    # the re-selected vectors of the clip, as TnrFilter hands them over
    noisy = M.clip(H, W)[0]
    mvq = S.refine(noisy[5], noisy[4], 4, M.search(noisy[5], noisy[4], RADIUS, 4)[0])[0]
    _compensate(noisy[4], R.split(noisy[5], noisy[4], 4, mvq, 4)[0], H, W, LAYOUTS[0], "clip")


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
    mv8, q0 = U.guarded(8 * n, 0, np.uint16, SENT16, DEV)
    cost8, c0 = U.guarded(4 * n, 0, np.uint32, SENT32, DEV)
    good = dict(cur=vc.data_ptr(), crs=crs, cps=cps, ref=vr.data_ptr(), rrs=rrs, rps=rps, H=H, W=W, lam=4, unit=1, mv=mv.data_ptr() + 2 * m0,
                mv8=mv8.data_ptr() + 2 * q0, cost=cost8.data_ptr() + 4 * c0)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "lam", "unit", "mv", "mv8", "cost")
    bad = [{k: None} for k in ("cur", "ref", "mv", "mv8", "cost")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"lam": -1}, {"lam": 256}] + [{"unit": u} for u in (0, 2, 3, 8, -1)] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * crs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost")] + [{"mv": good["mv"] + 1}, {"mv8": good["mv8"] + 1}] + \
          [{"mv8": good["mv"]}, {"mv8": good["mv"] + 4 * n - 2}, {"mv8": good["mv"] - 16 * n + 2}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_split(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(mv8) == SENT16).all() and (U.words(cost8) == SENT32).all()
    _cells(mv, m0, 2 * n, found, SENT16, "refused")
    assert lib.hip().dcvc_me_split(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.split(noisy[5], noisy[4], 4, found, 1)
    _cells(mv8, q0, 8 * n, want[0], SENT16, "good")
    _cells(cost8, c0, 4 * n, want[1], SENT32, "good")

    span = 4 * (2 * rps + (H - 1) * rrs + W)
    good = dict(ref=vr.data_ptr(), rrs=rrs, rps=rps, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W, mv=mv8.data_ptr() + 2 * q0)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rrs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"ref": good["out"] + 4 * ops},
           {"ref": good["out"] + 4 * (H - 1) * ors}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate_split(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_me_compensate_split(*[good[k] for k in order], U.stream(DEV)) == 0
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), R.compensate_split(noisy[4], want[0]).reshape(-1).view(np.uint32))
    assert np.array_equal(kr.cpu().numpy()[mask].view(np.uint32), noisy[4].reshape(-1).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ TnrFilter
STEP = (2.25, 5.5)  # what the object of the clip moves by, pixels a picture
PLAIN = ["bufs", "wtab", "sad", "held", "_rows", "comp", "mv", "cost", "zero"]


def _bytes(f):
    """The device memory the filter's attributes hold (views of another attribute's memory counted once)."""
    seen = {}
    for v in vars(f).values():
        for t in (v if isinstance(v, list) else [v]):
            if torch.is_tensor(t):
                seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
    return sum(seen.values())


@pytest.mark.parametrize("subpel", [True, False], ids=["subpel", "whole"])
def test_filter_with_split_equals_the_restatement(subpel):
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = list(S.subpel_clip(STEP, size=(H, W))[0]), S.SETTING, {0, 4}
    want = R.run(pics, setting, intra, RADIUS, 4, subpel)
    f = N.TnrFilter(N.TNR(*setting, search=RADIUS, subpel=subpel, split=True), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.grid == R.grid(H, W) and f.launches == 0 and f.untouched == (0,) * (6 if subpel else 5)
    assert _tensors(f) == sorted(PLAIN + ["mv8", "cost8"] + (["mvq", "costq"] if subpel else []))
    assert f.mv8.shape == (8 * 64,) and f.cost8.shape == (4 * 64,)
    got, launches = [], []
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        y = f.step(x, t in intra)
        assert (y is x) == (t in intra), t
        launches.append(f.launches)
        got.append(y.cpu().numpy())
        assert torch.equal(x, torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV))  # the source is only read
        if t not in intra:  # the sub-cells of the step, and a moved picture whose padding stays zero
            assert np.array_equal(f.mv8.cpu().numpy().astype(np.int64), want[t][6].reshape(-1)), t
            assert np.array_equal(U.words(f.cost8), want[t][7].reshape(-1)) and np.array_equal(U.words(f.zero), want[t][5].reshape(-1)), t
            cells = f.mvq.cpu().numpy().astype(np.int64) if subpel else 4 * f.mv.cpu().numpy().astype(np.int64)
            assert np.array_equal(cells, want[t][3].reshape(-1)), t
            comp = _padded(R.compensate_split(want[t - 1][0], want[t][6]), Hp, Wp)
            assert np.array_equal(f.comp.cpu().numpy().view(np.uint32), comp.view(np.uint32)), t
    per = 5 if subpel else 4  # a P picture: search, [refine,] split, compensate_split, step
    assert launches == [0, per, 2 * per, 3 * per, 3 * per, 4 * per, 5 * per, 6 * per]
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [R.totals(w, H, W, subpel) for w in want]
    assert f.totals()[4] == (0,) * (6 if subpel else 5) and any(row[-1] > 0 for row in f.totals()) and not f._done
    bare = N.TnrFilter(N.TNR(*setting, search=RADIUS, subpel=subpel, split=True), (H, W), DEV, totals=False)
    for t, pic in enumerate(pics[:3]):
        y = bare.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == 2 * per and bare._rows is None


def test_filter_without_split_owns_and_launches_what_it_did():
    H, W, Hp, Wp = 70, 100, 128, 128
    picture, cells = 3 * Hp * Wp * 4, 64
    base = 2 * picture + 256 * 2 + cells * 4 + cells * 2  # bufs, wtab, sad, held
    for subpel in (False, True):
        f = N.TnrFilter(N.TNR(*S.SETTING, search=RADIUS, subpel=subpel), (H, W), DEV)
        row = 5 if subpel else 4
        assert _tensors(f) == sorted(PLAIN + (["mvq", "costq"] if subpel else [])) and f.untouched == (0,) * row
        assert not any(hasattr(f, k) for k in ("mv8", "cost8", "mv8s", "cost8s"))
        want = base + 64 * row * 8 + picture + cells * (4 + 4 + 4) + (cells * (4 + 4) if subpel else 0)  # _rows, comp, mv / cost / zero, mvq / costq
        assert _bytes(f) == want, (subpel, _bytes(f), want)
        pics = S.subpel_clip(STEP, size=(H, W))[0][:3]
        for t, pic in enumerate(pics):
            f.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t == 0)
        assert f.launches == 2 * (4 if subpel else 3)
        assert len(f.totals()[1]) == row
    g = N.TnrFilter(N.TNR(*S.SETTING, search=RADIUS, subpel=True, split=True), (H, W), DEV)
    assert _bytes(g) == base + 64 * 6 * 8 + picture + cells * 12 + cells * 8 + cells * (16 + 16)  # (and mv8 / cost8 are what split adds)


@pytest.mark.parametrize("subpel", [True, False], ids=["subpel", "whole"])
def test_filter_with_split_and_look_ahead_equals_the_restatement(subpel):
    H, W, Hp, Wp, K = 70, 100, 128, 128, 2
    pics, setting, intra = list(S.subpel_clip(STEP, size=(H, W))[0]), S.SETTING, {0, 4}
    want = R.run_intra(pics, setting, intra, K, RADIUS, 4, subpel)
    f = N.TnrFilter(N.TNR(*setting, search=RADIUS, intra=K, subpel=subpel, split=True), (H, W), DEV)
    assert f.mv8s.shape == (4, 8 * 64) and f.cost8s.shape == (4, 4 * 64) and f.untouched == (0,) * (7 if subpel else 6)
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
    assert launches == [(4 if subpel else 3) * w[3] + 1 for w in want]  # per reference search, [refine,] split, compensate_split; ONE blend
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum())) + tuple(w[4:]) + (w[3],) for w in want]
    assert any(w[-1] for w in want)


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW, RH, RW = 4, 8, 96, 128, 176, 192
SETTING = N.TNR(*S.SETTING, search=RADIUS, subpel=True, split=True)
INTRA = {0, 4}


def _write_pngs(folder, size):
    """The noisy clip as PNGs -> what u8_to_unit_float uploads of them, (3, H, W) float32 each."""
    u8 = np.rint(S.subpel_clip(STEP, size=size)[0] * 255).astype(np.uint8)
    U.write_pngs(folder, u8.transpose(0, 2, 3, 1))
    return [a.astype(F32) / F32(255.0) for a in u8]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the 96 x 128 clip as PNGs, coded with the refinement alone and with the re-selection behind it"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("mesplit_e2e")
    pics = _write_pngs(tmp / "png", (FH, FW))
    RC.encode_folder(str(tmp / "png"), str(tmp / "sub"), gop=GOP, nets=file_nets, tnr=N.TNR(*S.SETTING, search=RADIUS, subpel=True))
    with _spy() as seen:
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "split"), str(tmp / "split_rec"), gop=GOP, nets=file_nets, picture_hash=True,
                                      tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, seen=seen, want=R.run(pics, S.SETTING, INTRA, RADIUS, 4))


def test_the_codec_is_handed_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    assert any(R.left(w[6], w[3], FH, FW) for w in e2e["want"])  # (and sub-cells left their cells' vectors: the test is about them)
    alone = S.run(e2e["pics"], S.SETTING, INTRA, RADIUS, 4)
    assert any(not np.array_equal(alone[t][0], e2e["want"][t][0]) for t in range(N_FRAMES))


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert U.others(tmp / "split") == ["hashes.json"]  # no side file of the filter, the search, the refinement or the re-selection
    split, sub = U.bins(tmp / "split"), U.bins(tmp / "sub")
    assert list(split) == list(sub) and split != sub
    for t in INTRA:  # I pictures are handed over as they are
        assert split[f"im{t + 1:05d}.bin"] == sub[f"im{t + 1:05d}.bin"], t
    assert RC.decode_folder(str(tmp / "split"), str(tmp / "split_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "split_dec", tmp / "split_rec", N_FRAMES)


def test_two_gop_streams_and_the_command_line_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spy() as seen:
        RC.encode_folder(str(tmp / "png"), str(tmp / "split2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "split2") == U.bins(tmp / "split")
    _handed(seen, e2e["want"], FH, FW)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "12", "--tnr-search", "8",
             "--tnr-subpel", "--tnr-split", "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "split")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "split_rec", N_FRAMES)


def test_report_speaks_of_the_re_selection(tmp_path, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path
    pics = _write_pngs(tmp / "png", (RH, RW))
    want = R.run(pics, S.SETTING, INTRA, RADIUS, 4)
    _, _, sub_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "sub"), gop=GOP, nets=file_nets, report=True,
                                    tnr=N.TNR(*S.SETTING, search=RADIUS, subpel=True))
    with _spy() as seen:
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "split"), gop=GOP, nets=file_nets, report=str(tmp / "split.json"), tnr=SETTING)
    assert size == (RH, RW)
    _handed(seen, want, RH, RW)
    cells, subs = M.cells_with_a_pixel(RH, RW), (RH // 8) * (RW // 8)
    assert rd["tnr"] == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4, "subpel": 4, "split": 8}
    assert rd["frame_tnr_held"] == [R.totals(w, RH, RW)[0] / (RH * RW) for w in want]
    assert rd["frame_tnr_mad"] == [R.totals(w, RH, RW)[1] / (RH * RW) for w in want]
    assert rd["frame_tnr_moved"] == [R.totals(w, RH, RW)[2] / cells for w in want]
    assert rd["frame_tnr_mad_zero"] == [R.totals(w, RH, RW)[3] / (RH * RW) for w in want]
    assert rd["frame_tnr_subpel"] == [R.totals(w, RH, RW)[4] / cells for w in want]
    assert rd["frame_tnr_split"] == [R.totals(w, RH, RW)[5] / subs for w in want]
    assert all(rd["frame_tnr_split"][t] == 0.0 for t in INTRA) and any(v > 0.0 for v in rd["frame_tnr_split"])  # (a P picture may have none)
    assert json.loads((tmp / "split.json").read_text()) == rd
    assert set(rd) - set(sub_rd) == {"frame_tnr_split"} and set(sub_rd) <= set(rd) and "split" not in sub_rd["tnr"]
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "split2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, tnr=SETTING)
    assert U.bins(tmp / "split2") == U.bins(tmp / "split")
    for key in ("tnr", "frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero", "frame_tnr_subpel", "frame_tnr_split", "frame_bpp"):
        assert rd2[key] == rd[key], key
