"""The motion search and compensation on a real MI355X: both kernels bit for bit against the numpy restatement
(tests/me_ref.py) in strided, offset, NaN-surrounded layouts with guarded outputs, their refusals, TnrFilter with and
without `search`, and the file loops end to end: the pictures the codec is handed, an unchanged decoder, the report, two GOP
streams, a Y4M file, the command line."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import me_ref as R
from tests import tnr_ref as T
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from vcm_ts_amd import lib
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
SENT16, SENT32 = 0xABCD, 0xABCD1234
# (row pad, plane pad, offset of the pictures, shift of mv / cost / zero): the four layouts of tests/test_gpu_tnr.py --
# 16-byte accesses; an odd offset, an odd row stride, an odd plane stride -> 4-byte accesses
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]


def _cells(buf, at, n, want, sentinel, where):
    got = U.words(buf)
    mask = (1 << (8 * buf.element_size())) - 1
    assert np.array_equal(got[at:at + n], np.asarray(want, dtype=np.int64).reshape(-1) & mask), where
    assert U.guards_intact(buf, at, n, sentinel), where


def _bits_of(buf, mask):
    return buf.cpu().numpy()[mask].view(np.uint32)


def _search(cur, ref, radius, lam, H, W, layout, want, where):
    """One dcvc_me_search in `layout`, held against want = (mv, cost, zero)."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kc, vc, crs, cps, mask = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)
    kr, vr, rrs, rps, _ = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)  # (fresh sentinels every time: every cell is WRITTEN)
    cost, c0 = U.guarded(n, shift, np.uint32, SENT32, DEV)
    zero, z0 = U.guarded(n, shift, np.uint32, SENT32, DEV)
    lib.check(lib.hip().dcvc_me_search(vc.data_ptr(), crs, cps, vr.data_ptr(), rrs, rps, H, W, radius, lam, mv.data_ptr() + 2 * m0,
                                       cost.data_ptr() + 4 * c0, zero.data_ptr() + 4 * z0, U.stream(DEV)), "me_search")
    _cells(mv, m0, 2 * n, want[0], SENT16, where)
    _cells(cost, c0, n, want[1], SENT32, where)
    _cells(zero, z0, n, want[2], SENT32, where)
    for k, pic in ((kc, cur), (kr, ref)):  # the inputs are only read, and nothing beside them is written
        got = k.cpu().numpy()
        assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(pic).reshape(-1).view(np.uint32)), where
        assert np.isnan(got[~mask]).all(), where


def _compensate(ref, vectors, H, W, layout, where):
    """One dcvc_me_compensate in `layout`, held against the restatement on the bits the device holds."""
    row_pad, plane_pad, offset, shift = layout
    n = int(np.prod(R.grid(H, W)))
    kr, vr, rrs, rps, mask = U.strided(ref, H, W, row_pad, plane_pad, offset, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
    mv[m0:m0 + 2 * n] = torch.from_numpy(np.asarray(vectors).astype(np.int16).reshape(-1)).to(DEV)
    before = kr.cpu().numpy()
    held = before[mask].reshape(3, H, W)  # (the bits as the device holds them: what the upload made of a signalling NaN is not at issue)
    lib.check(lib.hip().dcvc_me_compensate(vr.data_ptr(), rrs, rps, vo.data_ptr(), ors, ops, H, W, mv.data_ptr() + 2 * m0, U.stream(DEV)),
              "me_compensate")
    got = ko.cpu().numpy()
    want = R.compensate(held, vectors)
    assert np.array_equal(got[mask].view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32)), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    assert np.array_equal(kr.cpu().numpy().view(np.uint32), before.view(np.uint32)), where
    _cells(mv, m0, 2 * n, vectors, SENT16, where)
    return want


def _radii(size):
    return (1, 8, 32) if size == (70, 100) else (1, 8)


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_search_equals_the_restatement(size):
    H, W = size
    for radius in _radii(size):
        pairs = R.pairs(H, W, radius)
        if radius == 32:  # (the brute force over 4225 candidates: one pair of each kind that differs at this radius)
            pairs = {name: pairs[name][:1] for name in ("clip", "quadrants", "flip", "corner")}
        for name, todo in pairs.items():
            for n, (cur, ref) in enumerate(todo):
                table = R.sads(cur, ref, radius)
                for lam in R.LAMBDAS:
                    want = R.search(cur, ref, radius, lam, table)
                    for k, layout in enumerate(LAYOUTS):
                        if name != "clip" and k not in (0, 1 + (lam + n + len(name)) % 3):  # (every layout on the clip, two on the others)
                            continue
                        _search(cur, ref, radius, lam, H, W, layout, want, (name, n, radius, lam, layout))
                    mv, cost, zero = want
                    assert not mv[(H + 15) // 16:].any() and not mv[:, (W + 15) // 16:].any() and not zero[(H + 15) // 16:].any()
                    if name == "flat":  # every candidate matches: the shortest
                        assert not mv.any() and not cost.any()
                    if name == "flip":  # every candidate differs by 255 codes in every pixel: the shortest again
                        assert not mv.any() and int(cost.sum()) == 255 * H * W and np.array_equal(cost, zero)
                    if name == "period4" and lam == 0 and radius >= 2 and H >= 48 and W >= 48:
                        assert (mv[:(H // 16), 1:(W // 16) - 1, 1] == -2).all() and not mv[..., 0].any()
                    if name == "quadrants" and lam == 0 and radius == 8:
                        _quadrant_cells(H, W, radius, mv, cost)


def _quadrant_cells(H, W, radius, mv, cost):
    """A cell inside one quadrant whose moved copy lies inside the picture returns the quadrant's vector at cost 0."""
    _, _, vectors = R.quadrants(H, W, radius)
    seen = 0
    for i in range(H // 16):
        for j in range(W // 16):
            for q, (y0, y1, x0, x1) in enumerate(((0, (H + 1) // 2, 0, (W + 1) // 2), (0, (H + 1) // 2, (W + 1) // 2, W),
                                                  ((H + 1) // 2, H, 0, (W + 1) // 2), ((H + 1) // 2, H, (W + 1) // 2, W))):
                dy, dx = vectors[q]
                if y0 <= 16 * i and 16 * i + 16 <= y1 and x0 <= 16 * j and 16 * j + 16 <= x1 and \
                        0 <= 16 * i + dy and 16 * i + 16 + dy <= H and 0 <= 16 * j + dx and 16 * j + 16 + dx <= W:
                    assert tuple(mv[i, j]) == (dy, dx) and cost[i, j] == 0, (i, j, q)
                    seen += 1
    assert seen or H < 64 or W < 64


def test_period4_tie_and_quadrants_at_a_size_with_inner_cells():
    """64 x 96: cells two columns or more from the edges take (0, -2), not (0, +2); each quadrant's inner cells return its vector."""
    H, W = 64, 96
    cur, ref = R.period4(H, W)
    want = R.search(cur, ref, 8, 0)
    assert (want[0][:4, 1:5, 1] == -2).all() and not want[0][..., 0].any() and not want[1][:4, 1:5].any()
    _search(cur, ref, 8, 0, H, W, LAYOUTS[0], want, "period4")
    cur, ref, _ = R.quadrants(H, W, 8)
    want = R.search(cur, ref, 8, 0)
    _quadrant_cells(H, W, 8, want[0], want[1])
    _search(cur, ref, 8, 0, H, W, LAYOUTS[1], want, "quadrants")


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compensation_equals_the_restatement(size):
    H, W = size
    g = np.random.default_rng(H + 1000 * W)
    plain = g.uniform(-0.1, 1.1, (3, H, W)).astype(F32)
    fields = {"wild": R.wild_vectors(H, W), "fours": 4 * R.wild_vectors(H, W, seed=5).clip(-8, 8),  # (dx a multiple of 4: 16-byte reads)
              "still": np.zeros(R.grid(H, W) + (2,), dtype=np.int64)}
    for name, vectors in fields.items():
        for layout in LAYOUTS:
            for kind, pic in (("plain", plain), ("odd bits", R.odd_bits(H, W))):
                want = _compensate(pic, vectors, H, W, layout, (name, kind, layout))
                if name == "still" and kind == "plain":
                    assert np.array_equal(want.view(np.uint32), plain.view(np.uint32))
    assert (np.abs(fields["wild"]) > R.MAX_R).any()  # words far outside the search range: only the clamp keeps them inside
    # the found vectors of the clip, as TnrFilter hands them over
    noisy = R.clip(H, W)[0]
    _compensate(noisy[4], R.search(noisy[5], noisy[4], 8, 4)[0], H, W, LAYOUTS[0], "clip")


def test_the_step_on_the_compensated_picture_measures_the_searchs_cost():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    noisy = R.clip(H, W)[0]
    cur, ref = U.to_dev(noisy[5], DEV), U.to_dev(noisy[4], DEV)
    comp, out = torch.zeros_like(ref), torch.zeros_like(ref)
    mv = torch.zeros(2 * hc * wc, dtype=torch.int16, device=DEV)
    cost, zero, sad = (torch.zeros(hc * wc, dtype=torch.int32, device=DEV) for _ in range(3))
    held = torch.zeros(hc * wc, dtype=torch.int16, device=DEV)
    tab = torch.from_numpy(T.table(12, 64).view(np.int16)).to(DEV)
    hip, st = lib.hip(), U.stream(DEV)
    for radius, lam in ((8, 4), (32, 0)):
        lib.check(hip.dcvc_me_search(cur.data_ptr(), W, H * W, ref.data_ptr(), W, H * W, H, W, radius, lam, mv.data_ptr(), cost.data_ptr(),
                                     zero.data_ptr(), st), "me_search")
        lib.check(hip.dcvc_me_compensate(ref.data_ptr(), W, H * W, comp.data_ptr(), W, H * W, H, W, mv.data_ptr(), st), "me_compensate")
        lib.check(hip.dcvc_tnr_step(cur.data_ptr(), W, H * W, comp.data_ptr(), W, H * W, out.data_ptr(), W, H * W, H, W, tab.data_ptr(), 36,
                                    sad.data_ptr(), held.data_ptr(), st), "tnr_step")
        assert torch.equal(sad, cost) and int(cost.sum()) > 0 and (mv != 0).any()
        assert int(cost.sum()) <= int(zero.sum())
        # cur and ref may be the same picture: every cell stays where it is at cost 0
        lib.check(hip.dcvc_me_search(cur.data_ptr(), W, H * W, cur.data_ptr(), W, H * W, H, W, radius, lam, mv.data_ptr(), cost.data_ptr(),
                                     zero.data_ptr(), st), "me_search")
        assert not mv.any() and not cost.any() and not zero.any()


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    n = int(np.prod(R.grid(H, W)))
    noisy = R.clip(H, W)[0]
    kc, vc, crs, cps, mask = U.strided(noisy[5], H, W, 8, 24, 12, DEV)
    kr, vr, rrs, rps, _ = U.strided(noisy[4], H, W, 8, 24, 12, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, 8, 24, 12, DEV)
    mv, m0 = U.guarded(2 * n, 0, np.uint16, SENT16, DEV)
    cost, c0 = U.guarded(n, 0, np.uint32, SENT32, DEV)
    zero, z0 = U.guarded(n, 0, np.uint32, SENT32, DEV)
    good = dict(cur=vc.data_ptr(), crs=crs, cps=cps, ref=vr.data_ptr(), rrs=rrs, rps=rps, H=H, W=W, R=8, lam=4, mv=mv.data_ptr() + 2 * m0,
                cost=cost.data_ptr() + 4 * c0, zero=zero.data_ptr() + 4 * z0)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "R", "lam", "mv", "cost", "zero")
    bad = [{k: None} for k in ("cur", "ref", "mv", "cost", "zero")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"R": 0}, {"R": 33}, {"lam": -1}, {"lam": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * crs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost", "zero")] + [{"mv": good["mv"] + 1}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_search(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(mv) == SENT16).all() and (U.words(cost) == SENT32).all() and (U.words(zero) == SENT32).all()
    assert lib.hip().dcvc_me_search(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.search(noisy[5], noisy[4], 8, 4)
    _cells(mv, m0, 2 * n, want[0], SENT16, "good")
    _cells(cost, c0, n, want[1], SENT32, "good")
    _cells(zero, z0, n, want[2], SENT32, "good")

    span = 4 * (2 * rps + (H - 1) * rrs + W)
    good = dict(ref=vr.data_ptr(), rrs=rrs, rps=rps, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W, mv=mv.data_ptr() + 2 * m0)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rrs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"ref": good["out"] + 4 * ops},
           {"ref": good["out"] + 4 * (H - 1) * ors}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_me_compensate(*[good[k] for k in order], U.stream(DEV)) == 0
    assert np.array_equal(_bits_of(ko, mask), R.compensate(noisy[4], want[0]).reshape(-1).view(np.uint32))
    assert np.array_equal(_bits_of(kr, mask), noisy[4].reshape(-1).view(np.uint32))


def _padded(pic, Hp, Wp):
    out = np.zeros((1, 3, Hp, Wp), F32)
    out[0, :, :pic.shape[1], :pic.shape[2]] = pic
    return out


def _tensors(f):
    """The names of the filter's attributes that hold device memory."""
    return sorted(k for k, v in vars(f).items() if torch.is_tensor(v) or (isinstance(v, list) and v and torch.is_tensor(v[0])))


def test_filter_with_search_equals_the_restatement():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = list(R.clip(H, W)[0]), (12, 64, 36), {0, 4}
    want = R.run(pics, setting, intra, 8, 4)
    f = N.TnrFilter(N.TNR(*setting, search=8), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.grid == R.grid(H, W) and f.launches == 0
    assert _tensors(f) == sorted(["bufs", "wtab", "sad", "held", "_rows", "comp", "mv", "cost", "zero"]) and len(f.bufs) == 2
    got, launches = [], []
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        y = f.step(x, t in intra)
        assert (y is x) == (t in intra), t
        launches.append(f.launches)
        got.append(y.cpu().numpy())
        assert torch.equal(x, torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV))  # the source is only read
        if t not in intra:  # the cells of the step, and a compensated picture whose padding stays zero
            assert np.array_equal(f.mv.cpu().numpy().astype(np.int64), want[t][3].reshape(-1)), t
            assert np.array_equal(U.words(f.cost), want[t][4].reshape(-1)) and np.array_equal(U.words(f.zero), want[t][5].reshape(-1)), t
            assert np.array_equal(U.words(f.sad), want[t][4].reshape(-1)), t
            comp = _padded(R.compensate(want[t - 1][0], want[t][3]), Hp, Wp)
            assert np.array_equal(f.comp.cpu().numpy().view(np.uint32), comp.view(np.uint32)), t
    assert launches == [0, 3, 6, 9, 9, 12, 15, 18]  # an I picture launches nothing, a P picture search, compensate, step
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [R.totals(w, H, W) for w in want]
    assert f.totals()[4] == (0, 0, 0, 0) and f.totals()[5][2] > 0 and f.totals()[5][3] >= f.totals()[5][1] and not f._done
    assert any(tuple(v) != (0, 0) for w in want for v in w[3].reshape(-1, 2))  # (something moved)
    bare = N.TnrFilter(N.TNR(*setting, search=8), (H, W), DEV, totals=False)  # the same pictures without the bookkeeping
    for t, pic in enumerate(pics[:3]):
        y = bare.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == 6 and not bare._done and bare._rows is None and not bare._log.keys  # no pinned memory, no event
    with pytest.raises(ValueError, match="totals=False"):
        bare.totals()
    with pytest.raises(ValueError, match="first picture of a stream is an I picture"):
        N.TnrFilter(N.TNR(12, search=8), (H, W), DEV).step(torch.zeros((1, 3, Hp, Wp), device=DEV), False)


def test_filter_without_search_launches_and_allocates_what_it_did():
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting = list(R.clip(H, W)[0][:4]), (12, 64, 36)
    want = T.run(pics, setting, {0})
    torch.cuda.synchronize(DEV)
    before = torch.cuda.memory_allocated(DEV)
    f = N.TnrFilter(N.TNR(*setting), (H, W), DEV)
    cells = f.grid[0] * f.grid[1]
    own = 2 * 3 * Hp * Wp * 4 + 256 * 2 + cells * 4 + cells * 2 + N.ROWS * 2 * 8  # two pictures, the table, sad, held, the rows
    assert _tensors(f) == sorted(["bufs", "wtab", "sad", "held", "_rows"]) and len(f.bufs) == 2 and f._rows.shape == (N.ROWS, 2)
    assert not any(hasattr(f, name) for name in ("comp", "mv", "cost", "zero"))
    assert own <= torch.cuda.memory_allocated(DEV) - before < own + 4096  # (each rounded up to the allocator's granule; a third picture is 196608)
    for t, pic in enumerate(pics):
        y = f.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t == 0)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.launches == 3 and f.untouched == (0, 0)  # one launch a P picture
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum())) for w in want]


# -------------------------------------------------------------------------------------------------------- file loops
# As tests/test_gpu_tnr.py: at 128 x 192 no report exists (MS-SSIM needs sides above 160): there the handed pictures, the
# decoder, the hashes, the GOP streams and the command line are checked; everything about --report on a 176 x 192 clip.
GOP, N_FRAMES, FH, FW, RH = 4, 8, 128, 192, 176
SETTING = N.TNR(12, 64, 36, search=8)
INTRA = {0, 4}


def _write_pngs(folder, H, W):
    """The noisy clip as PNGs -> what u8_to_unit_float uploads of them, (3, H, W) float32 each."""
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
def _spy():
    """The padded picture the codec was handed, by frame number, of the encodes run inside."""
    from vcm_ts_amd import run_codec as RC

    seen = {}
    encode = RC._EncodeRun.encode

    def spy_encode(self, frames, *a, **kw):
        def wrapped(k):
            for t, x in enumerate(frames(k)):
                seen[self.global_index(k, t)] = x.cpu().numpy()
                yield x
        return encode(self, wrapped, *a, **kw)

    RC._EncodeRun.encode = spy_encode
    try:
        yield seen
    finally:
        RC._EncodeRun.encode = encode


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the noisy clip as PNGs, coded with the plain prefilter and with the search in front of it"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("me_e2e")
    pics = _write_pngs(tmp / "png", FH, FW)
    RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), gop=GOP, nets=file_nets, tnr=N.TNR(12, 64, 36))
    with _spy() as seen:
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "me"), str(tmp / "me_rec"), gop=GOP, nets=file_nets, picture_hash=True,
                                      tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, seen=seen, want=R.run(pics, (12, 64, 36), INTRA, 8, 4))


def test_the_codec_is_handed_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    for t in range(N_FRAMES):  # an I picture is the source itself, a P picture is not
        assert np.array_equal(e2e["seen"][t][0], e2e["pics"][t]) == (t in INTRA), t
    assert any(w[3].any() for w in e2e["want"])  # (and the search found the object: the test is about compensated pictures)
    plain = T.run(e2e["pics"], (12, 64, 36), INTRA)
    assert any(not np.array_equal(plain[t][0], e2e["want"][t][0]) for t in range(N_FRAMES))


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert U.others(tmp / "me") == ["hashes.json"]  # no side file of the filter or the search
    me, tnr = U.bins(tmp / "me"), U.bins(tmp / "tnr")
    assert list(me) == list(tnr) and me != tnr
    for t in INTRA:  # I pictures are handed over as they are
        assert me[f"im{t + 1:05d}.bin"] == tnr[f"im{t + 1:05d}.bin"], t
    assert RC.decode_folder(str(tmp / "me"), str(tmp / "me_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "me_dec", tmp / "me_rec", N_FRAMES)


def test_two_gop_streams_and_the_command_line_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spy() as seen:
        RC.encode_folder(str(tmp / "png"), str(tmp / "me2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "me2") == U.bins(tmp / "me")
    _handed(seen, e2e["want"], FH, FW)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "12", "--tnr-search", "8",
             "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "me")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "me_rec", N_FRAMES)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli2"), "--gop", str(GOP), "--tnr", "12", "--tnr-search", "4",
             "--tnr-penalty", "0"])
    with _spy() as seen:
        RC.encode_folder(str(tmp / "png"), str(tmp / "api2"), gop=GOP, nets=file_nets, tnr=N.TNR(12, search=4, penalty=0))
    assert U.bins(tmp / "cli2") == U.bins(tmp / "api2")
    _handed(seen, R.run(e2e["pics"], (12, 64, 36), INTRA, 4, 0), FH, FW)


def _report_keys(rd, want, H, W):
    cells = R.cells_with_a_pixel(H, W)
    assert rd["tnr"] == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4}
    assert rd["frame_tnr_held"] == [R.totals(w, H, W)[0] / (H * W) for w in want]
    assert rd["frame_tnr_mad"] == [R.totals(w, H, W)[1] / (H * W) for w in want]
    assert rd["frame_tnr_moved"] == [R.totals(w, H, W)[2] / cells for w in want]
    assert rd["frame_tnr_mad_zero"] == [R.totals(w, H, W)[3] / (H * W) for w in want]
    for key in ("frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero"):
        assert all((rd[key][t] == 0.0) == (t in INTRA) for t in range(N_FRAMES)), key


def test_report_speaks_of_the_search(tmp_path, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path
    pics = _write_pngs(tmp / "png", RH, FW)
    want = R.run(pics, (12, 64, 36), INTRA, 8, 4)
    _, _, plain_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), gop=GOP, nets=file_nets, report=True, tnr=N.TNR(12, 64, 36))
    with _spy() as seen:
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "me"), gop=GOP, nets=file_nets, report=str(tmp / "me.json"), tnr=SETTING)
    assert size == (RH, FW)
    _handed(seen, want, RH, FW)
    _report_keys(rd, want, RH, FW)
    assert json.loads((tmp / "me.json").read_text()) == rd
    assert set(rd) - set(plain_rd) == {"frame_tnr_moved", "frame_tnr_mad_zero"} and set(plain_rd) <= set(rd)
    assert sorted(os.listdir(tmp / "me")) == sorted(U.bins(tmp / "me"))
    # two GOP streams: the same bytes and the same figures
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "me2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, tnr=SETTING)
    assert U.bins(tmp / "me2") == U.bins(tmp / "me")
    for key in ("tnr", "frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero", "frame_bpp"):
        assert rd2[key] == rd[key], key


def test_y4m_file(tmp_path, file_nets):
    """A Y4M source: the same mechanism on the pictures the conversion gives."""
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp = tmp_path
    pics = [a.astype(F32) / F32(255.0) for a in np.rint(R.clip(RH, FW)[0][:N_FRAMES] * 255).astype(np.uint8)]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(pic, dtype=np.float64)) for pic in pics]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, RH, fps="30:1")
    with Y.open_video(str(tmp / "src.y4m")) as reader:
        src = [x.cpu().numpy()[0, :, :RH, :FW] for x, _ in RC._video_pictures(reader, range(N_FRAMES), reader.spec(), False, DEV)]
    want = R.run(src, (12, 64, 36), INTRA, 8, 4)
    with _spy() as seen:
        _, _, rd = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), gop=GOP, nets=file_nets, gop_streams=2,
                                   report=True, tnr=SETTING)
    _handed(seen, want, RH, FW)
    _report_keys(rd, want, RH, FW)
    assert "tnr" not in RC.read_sequence_info(str(tmp / "vbins")) and U.others(tmp / "vbins") == ["sequence.json"]
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vseq"), gop=GOP, nets=file_nets, tnr=SETTING)
    assert U.bins(tmp / "vseq") == U.bins(tmp / "vbins")  # one stream and two give the same bytes
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()
