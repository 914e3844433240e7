"""The camera-shake registration on a real MI355X: the three kernels bit for bit against the numpy restatement
(tests/shake_ref.py) through the C ABI -- contiguous and strided, offset, NaN-surrounded pictures with guarded outputs --
their refusals, the Registrar, and the file loops: boxes --shake, noise --shake, encode --tnr-auto --shake and run_codec shake
write what the restatement says, from a PNG folder and from a Y4M file."""
import json
import pickle

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import me_ref as ME
from tests import motion_ref as MR
from tests import noise_ref as NR
from tests import shake_ref as R
from tests import yuv_ref as Y
from tests.gpu_util import file_nets  # noqa: F401 (a fixture)
from vcm_ts_amd import lib
from vcm_ts_amd import shake as SH
from vcm_ts_amd import tnr as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
WORD, BYTE, HALF = 0xABCD1234, 0xA5, 0x7B7B


def _views(pic, H, W):
    """The picture three ways: contiguous (16-byte loads); strided and offset by an odd count inside NaN (4-byte loads);
    strided with multiples of four.  (view, row stride, plane stride)"""
    return [U.strided(pic, H, W, *pads, DEV)[1:4] for pads in ((0, 0, 0), (5, 23, 13), (8, 24, 12))]


def _random(H, W, seed=0):
    """Samples beyond [0, 1] and NaNs among them."""
    g = np.random.default_rng(1000 * H + W + seed)
    a = g.uniform(-0.05, 1.05, (3, H, W)).astype(F32)
    a[g.integers(0, 3), g.integers(0, H), g.integers(0, W)] = np.nan
    a[:, H // 2, W // 2] = np.nan
    return a


# ------------------------------------------------------------------------------------------------- dcvc_shake_plane
def _plane(view, rs, ps, H, W, slack=4, shift=0):
    ys = -(-W // 4) * 4 + slack
    buf, y0 = U.guarded(H * ys, 4 * shift, np.uint8, BYTE, DEV)
    lib.check(lib.hip().dcvc_shake_plane(view.data_ptr(), rs, ps, H, W, buf.data_ptr() + y0, ys, U.stream(DEV)), "shake_plane")
    rows = U.words(buf)[y0:y0 + H * ys].reshape(H, ys)
    assert (rows[:, W:] == BYTE).all() and U.guards_intact(buf, y0, H * ys, BYTE)  # the bytes from column W on; the guards
    return rows[:, :W]


@pytest.mark.parametrize("size", [(1, 1), (64, 64), (70, 100), (128, 192), (48, 517)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    pic = _random(H, W)
    want = R.plane(pic)
    assert want[H // 2, W // 2] == 0  # a NaN codes as 0
    for n, (view, rs, ps) in enumerate(_views(pic, H, W)):
        assert np.array_equal(_plane(view, rs, ps, H, W, slack=4 * (n % 2), shift=n), want), (size, n)
    ones = U.to_dev(np.ones((3, H, W), F32), DEV)
    assert (_plane(ones, W, H * W, H, W) == 255).all()


# ------------------------------------------------------------------------------------------------- dcvc_shake_tiles
def _anchor_buffer(plane, slack=4):
    """The anchor plane on the device with `slack` foreign bytes behind every row (never read: they differ from run to run
    of the restatement's answer if they were)."""
    H, W = plane.shape
    ys = -(-W // 4) * 4 + slack
    a = np.full((H, ys), 0x5A, dtype=np.uint8)
    a[:, :W] = plane
    return U.to_dev(a, DEV), ys


def _tiles(view, rs, ps, H, W, plane, R_, shift=0, slack=4):
    n = (H // 64) * (W // 64)
    abuf, ys = _anchor_buffer(plane, slack)
    tbuf, t0 = U.guarded(max(5 * n, 1), shift, np.uint32, WORD, DEV)
    lib.check(lib.hip().dcvc_shake_tiles(view.data_ptr(), rs, ps, H, W, abuf.data_ptr(), ys, R_, tbuf.data_ptr() + 4 * t0, U.stream(DEV)),
              "shake_tiles")
    assert U.guards_intact(tbuf, t0, 5 * n, WORD)  # (with no tile: every word)
    assert np.array_equal(abuf.cpu().numpy()[:, :W], plane) and (abuf.cpu().numpy()[:, W:] == 0x5A).all()  # (only read)
    return U.words(tbuf)[t0:t0 + 5 * n].astype(np.uint32).view(np.int32).astype(np.int64).reshape(n, 5)


def _shifted_pair(H, W, move, seed=2):
    """(cur, the anchor's plane): a random grey world seen from (0, 0) and from `move`."""
    world = np.random.default_rng(seed + H + W).integers(0, 256, (H + 32, W + 32))
    return ME.grey(world[16 + move[0]:16 + move[0] + H, 16 + move[1]:16 + move[1] + W]), world[16:16 + H, 16:16 + W]


def _tile_cases(H, W, R_):
    m = min(R_, 6)
    cases = {"shift": _shifted_pair(H, W, (m, -m + 1)), "shift2": _shifted_pair(H, W, (-m, m), 5),
             "noise": (_random(H, W, 3), R.plane(_random(H, W, 4))),
             "equal": (ME.grey(np.full((H, W), 77)), np.full((H, W), 77)),
             "flip": (np.ones((3, H, W), F32), np.zeros((H, W), np.int64))}
    cur, ref = ME.period4(H, W)
    cases["period4"] = (cur, R.luma(ref))
    return cases


@pytest.mark.parametrize("size,R_", [((64, 64), 1), ((64, 64), 16), ((70, 100), 5), ((128, 192), 8), ((64, 192), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"R{v}")
def test_tiles_kernel_equals_the_restatement_bit_for_bit(size, R_):
    H, W = size
    for name, (cur, plane) in _tile_cases(H, W, R_).items():
        want = R.tiles(cur, plane, R_)
        if name == "flip":
            assert (want == [0, 0, 261120, 261120, 261120]).all()
        if name == "equal":
            assert (want == 0).all()
        if name == "period4" and size == (64, 192):
            assert want[1, :3].tolist() == [0, -2, 0]  # the tie the key order decides
        if name == "shift" and R_ > 1 and size == (128, 192):
            assert (want[:, 0] == min(R_, 6)).all() and (want[:, 1] == 1 - min(R_, 6)).all()
        for n, (view, rs, ps) in enumerate(_views(cur, H, W)):
            got = _tiles(view, rs, ps, H, W, plane.astype(np.uint8), R_, shift=n, slack=4 * (n % 2))
            assert np.array_equal(got, want), (size, R_, name, n, got.tolist(), want.tolist())


def test_tiles_kernel_writes_nothing_without_a_tile():
    H, W = 63, 200
    cur, plane = _shifted_pair(H, W, (1, 1))
    assert _tiles(U.to_dev(cur, DEV), W, H * W, H, W, plane.astype(np.uint8), 8).shape == (0, 5)  # (answer 0, every word intact)


# -------------------------------------------------------------------------------------------------- dcvc_shake_vote
def _vote(tile_words, R_, min_votes, H=70, W=100, shift=0):
    t = np.asarray(tile_words, dtype=np.int64).reshape(-1, 5)
    hc, wc = R.grid(H, W)
    dev = U.to_dev(t.astype(np.int32) if len(t) else np.zeros((1, 5), np.int32), DEV)
    rbuf, r0 = U.guarded(8, shift, np.uint32, WORD, DEV)
    mbuf, m0 = U.guarded(2 * hc * wc, shift, np.uint16, HALF, DEV)
    lib.check(lib.hip().dcvc_shake_vote(dev.data_ptr(), len(t), R_, min_votes, H, W, rbuf.data_ptr() + 4 * r0, mbuf.data_ptr() + 2 * m0,
                                        U.stream(DEV)), "shake_vote")
    assert U.guards_intact(rbuf, r0, 8, WORD) and U.guards_intact(mbuf, m0, 2 * hc * wc, HALF)
    rec = U.words(rbuf)[r0:r0 + 8].astype(np.uint32).view(np.int32).astype(np.int64).tolist()
    mv = U.words(mbuf)[m0:m0 + 2 * hc * wc].astype(np.uint16).view(np.int16).astype(np.int64).reshape(hc, wc, 2)
    assert np.array_equal(mv, R.field(rec, H, W))  # every cell of the padded grid holds (-dy, -dx)
    return rec


def _rec(dy, dx, s=10, top=100):
    return [dy, dx, s, top, 50]


VOTES = {
    "no tiles": ([], 8, 1),
    "none voting": ([_rec(1, 1, 0, 0), _rec(2, 2, 60, 100), _rec(0, 0, 0, 0)], 8, 1),
    "below min_votes": ([_rec(2, -3), _rec(2, -3), _rec(5, 5, 0, 0), _rec(5, 5, 51, 100)], 8, 3),
    "even": ([_rec(1, 5), _rec(2, 6), _rec(3, 7), _rec(4, 8)], 8, 1),
    "two tiles": ([_rec(0, 3), _rec(1, 0), _rec(2, 1)], 8, 1),
    "median at -R": ([_rec(-8, 1)] * 3 + [_rec(0, 0)], 8, 1),
    "median at +R": ([_rec(1, 16)] * 3, 16, 4),
    "beyond the range": ([_rec(9, 0), _rec(0, -9), _rec(-3, 4)], 8, 1),
    "equality votes": ([_rec(5, -5, 50, 100), _rec(1, 1, 51, 101)], 8, 1),
    "large sads": ([_rec(-1, 2, 130560, 261120), _rec(7, 7, 2 ** 31 - 1, 2 ** 31 - 1)], 8, 1),
}


@pytest.mark.parametrize("name", list(VOTES))
def test_vote_kernel_equals_the_restatement(name):
    t, R_, min_votes = VOTES[name]
    want = R.vote(t, R_, min_votes)
    for shift, size in enumerate(((70, 100), (16, 16), (128, 192))):
        assert _vote(t, R_, min_votes, *size, shift=shift) == want, (name, size)
    if name == "two tiles":
        assert want[3] == 0 and want[5] == 0
    if name == "none voting":
        assert want == [0, 0, 0, 0, 3, R.FEW, 0, 0]


def test_vote_kernel_on_16384_tiles():
    g = np.random.default_rng(9)
    t = np.stack([g.integers(-16, 17, 16384), g.integers(-16, 17, 16384), g.integers(0, 200, 16384), g.integers(0, 300, 16384),
                  g.integers(0, 300, 16384)], axis=1)
    t[::5] = 0  # tiles of exact zeros: they must not vote
    want = R.vote(t, 16, 100)
    assert 100 < want[2] < 16384 - 16384 // 5 and want[4] == 16384
    assert _vote(t, 16, 100) == want
    same = np.tile(np.array([[3, -4, 10, 100, 50]]), (16384, 1))  # every tile into one bin
    assert _vote(same, 8, 16384, 64, 64) == R.vote(same, 8, 16384) == [3, -4, 16384, 16384, 16384, 0, 3, -4]


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_alone():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    keep, view, rs, ps = U.strided(_random(H, W), H, W, 8, 24, 12, DEV)[:4]
    ybuf, y0 = U.guarded(H * 100, 0, np.uint8, BYTE, DEV)
    tbuf, t0 = U.guarded(5, 0, np.uint32, WORD, DEV)
    rbuf, r0 = U.guarded(8, 0, np.uint32, WORD, DEV)
    mbuf, m0 = U.guarded(2 * hc * wc, 0, np.uint16, HALF, DEV)
    L, st = lib.hip(), U.stream(DEV)
    plane = dict(rgb=view.data_ptr(), rs=rs, ps=ps, H=H, W=W, y=ybuf.data_ptr() + y0, ys=100)
    order = ("rgb", "rs", "ps", "H", "W", "y", "ys")
    for bad in ({"rgb": None}, {"y": None}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"rs": W - 1}, {"ps": (H - 1) * rs + W - 1},
                {"ys": 96}, {"ys": 102}, {"rgb": plane["rgb"] + 2}, {"y": plane["y"] + 1}, {"y": plane["y"] + 2}):
        v = dict(plane, **bad)
        assert L.dcvc_shake_plane(*[v[k] for k in order], st) == -1, bad
    tiles = dict(rgb=view.data_ptr(), rs=rs, ps=ps, H=H, W=W, anchor=ybuf.data_ptr() + y0, ys=100, R=8, tiles=tbuf.data_ptr() + 4 * t0)
    order_t = ("rgb", "rs", "ps", "H", "W", "anchor", "ys", "R", "tiles")
    for bad in ({"rgb": None}, {"anchor": None}, {"tiles": None}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"rs": W - 1},
                {"ps": (H - 1) * rs + W - 1}, {"ys": 96}, {"ys": 102}, {"R": 0}, {"R": 17}, {"R": -1}, {"rgb": tiles["rgb"] + 2},
                {"anchor": tiles["anchor"] + 2}, {"tiles": tiles["tiles"] + 2}):
        v = dict(tiles, **bad)
        assert L.dcvc_shake_tiles(*[v[k] for k in order_t], st) == -1, bad
    vote = dict(tiles=tbuf.data_ptr() + 4 * t0, n=1, R=8, min_votes=1, H=H, W=W, record=rbuf.data_ptr() + 4 * r0, mv=mbuf.data_ptr() + 2 * m0)
    order_v = ("tiles", "n", "R", "min_votes", "H", "W", "record", "mv")
    for bad in ({"tiles": None}, {"record": None}, {"mv": None}, {"n": -1}, {"n": 16385}, {"R": 0}, {"R": 17}, {"min_votes": 0},
                {"min_votes": 16385}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"tiles": vote["tiles"] + 2},
                {"record": vote["record"] + 2}, {"mv": vote["mv"] + 1}):
        v = dict(vote, **bad)
        assert L.dcvc_shake_vote(*[v[k] for k in order_v], st) == -1, bad
    torch.cuda.synchronize(DEV)
    assert (U.words(ybuf) == BYTE).all() and (U.words(tbuf) == WORD).all() and (U.words(rbuf) == WORD).all() and (U.words(mbuf) == HALF).all()
    # (and the arguments were good ones)
    assert L.dcvc_shake_plane(*[plane[k] for k in order], st) == 0 and L.dcvc_shake_tiles(*[tiles[k] for k in order_t], st) == 0
    assert L.dcvc_shake_vote(*[vote[k] for k in order_v], st) == 0
    torch.cuda.synchronize(DEV)
    assert (U.words(tbuf)[t0:t0 + 5] != WORD).all() and U.guards_intact(tbuf, t0, 5, WORD) and U.guards_intact(rbuf, r0, 8, WORD)


# ------------------------------------------------------------------------------------------------------- Registrar
H, W, FRAMES, GOP, RADIUS, VOTES_MIN = 128, 192, 5, 4, 8, 3
MOVES = [(0, 0), (3, -2), (-4, 5), (1, 6), (-6, -1)]


def _clip():
    return R.clip(H, W, MOVES, s=2.0, obj=(24, 32))


@pytest.fixture(scope="module")
def want():
    """The restatement's answers for the clip, computed once: from the PNG folder's pictures and from the Y4M file's."""
    pics = _clip()
    planes = [tuple(p.astype(np.uint8) for p in Y.from_rgb(pic)) for pic in pics]
    out = {"pics": pics, "planes": planes}
    for name, seq in (("png", list(pics)), ("y4m", [Y.to_rgb(*p) for p in planes])):
        log, reg = R.run(seq, RADIUS, VOTES_MIN)
        out[name] = dict(seq=seq, log=log, reg=reg, doc=R.document(log, RADIUS, VOTES_MIN, 25, H, W))
    assert [tuple(r[:2]) for r in out["png"]["log"].tolist()] == MOVES and (out["png"]["log"][:, 5] == 0).all()
    return out


def test_registrar_equals_the_restatement(want):
    w = want["png"]
    params = SH.ShakeParams(RADIUS, VOTES_MIN)

    def run():
        reg, got = SH.Registrar(DEV, H, W, FRAMES, params), []
        for t, p in enumerate(w["seq"]):
            wide = torch.full((1, 3, 192, 256), float("nan"), device=DEV)  # (the padding is never read: a NaN there would show)
            wide[0, :, :H, :W] = U.to_dev(p, DEV)
            out = reg.add(wide)
            assert (out is wide) == (t == 0)
            got.append(out[0, :, :H, :W].cpu().numpy())
        return reg, got

    reg, got = run()
    assert np.array_equal(reg.log(), w["log"]) and reg.log().dtype == np.int64 and (reg.n, reg.n_tiles, reg.grid) == (5, 6, (8, 12))
    for t in range(FRAMES):
        assert np.array_equal(U.f32_bits(got[t]), U.f32_bits(w["reg"][t])), t
    assert SH.summary(reg.log()) == R.summary(w["log"]) == w["doc"]["summary"]
    assert SH.document(reg.log(), params, H, W) == w["doc"]
    with torch.cuda.stream(torch.cuda.Stream(DEV)):  # made on one stream and used on another
        other, _ = run()
    assert np.array_equal(other.log(), w["log"])
    with pytest.raises(ValueError, match="picture 5 of a scan of 5"):
        reg.add(torch.zeros(1, 3, H, W, device=DEV))
    fresh = SH.Registrar("cuda", H, W, 2, SH.ShakeParams(8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        fresh.add(torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="expected a"):
        fresh.add(torch.zeros(1, 3, H - 1, W, device=DEV))
    with pytest.raises(ValueError, match="ShakeParams"):
        SH.Registrar(DEV, H, W, 2, 8)
    # the default min_votes of 8 exceeds this picture's 6 tiles: every picture is lost and passed on unmoved
    lost = SH.Registrar(DEV, H, W, 2, SH.ShakeParams(8))
    lost.add(U.to_dev(w["seq"][0], DEV)[None])
    out = lost.add(U.to_dev(w["seq"][1], DEV)[None])
    assert np.array_equal(U.f32_bits(out[0].cpu().numpy()), U.f32_bits(w["seq"][1]))
    assert lost.log().tolist() == R.run(w["seq"][:2], 8, 8)[0].tolist() and lost.log()[1, 5] == R.FEW


# -------------------------------------------------------------------------------------------------------- file loops
@pytest.fixture(scope="module")
def files(tmp_path_factory, want):
    tmp = tmp_path_factory.mktemp("shake")
    U.write_pngs(str(tmp / "png"), want["pics"])
    Y.write_y4m(str(tmp / "src.y4m"), want["planes"], W, H)
    return tmp


MOTION = dict(threshold=12, min_pixels=8)


def _want_boxes(w):
    counts = np.stack([c for _, c in MR.run(w["reg"], MOTION["threshold"], 4, 8)])
    masked = R.masked_counts(counts, w["log"], H, W)
    return [np.zeros((0, 4), np.int32) if t == 0 else MR.boxes(c, H, W, min_pixels=8) for t, c in enumerate(masked)]


def _read_boxes(root, n):
    return [np.asarray(pickle.load(open(root / "motion_coords" / ("%05d" % (t + 1)), "rb"))).astype(np.int32).reshape(-1, 4) for t in range(n)]


@pytest.mark.parametrize("kind", ["png", "y4m"])
def test_boxes_shake_writes_the_restatements_boxes(kind, files, want, capsys):
    from vcm_ts_amd import motionroi as M
    from vcm_ts_amd import run_codec as RC

    w, root, plain = want[kind], files / f"boxes_{kind}", files / f"boxes_plain_{kind}"
    src = ["--frames", str(files / "png")] if kind == "png" else ["--video", str(files / "src.y4m")]
    RC.main(["boxes", *src, "--out", str(root), "--threshold", "12", "--shake", str(RADIUS), "--shake-min-votes", str(VOTES_MIN)])
    expect = _want_boxes(w)
    got = _read_boxes(root, FRAMES)
    assert all(np.array_equal(a, b) for a, b in zip(got, expect)), (got, expect)
    assert json.loads((root / "shake.json").read_text()) == w["doc"]
    info = json.loads((root / "motion.json").read_text())
    assert info["shake"] == dict(w["doc"]["params"], **w["doc"]["summary"])
    assert M.read_info(str(root)) == (M.MotionParams(12), H, W, FRAMES)
    # without the option: no shake.json, no "shake" key, and the shaken clip's boxes are other (larger) ones
    RC.main(["boxes", *src, "--out", str(plain), "--threshold", "12"])
    assert not (plain / "shake.json").exists() and "shake" not in json.loads((plain / "motion.json").read_text())
    assert M.read_info(str(plain)) == (M.MotionParams(12), H, W, FRAMES)
    unregistered = MR.clip_boxes(w["seq"], 12, min_pixels=8)
    assert all(np.array_equal(a, b) for a, b in zip(_read_boxes(plain, FRAMES), unregistered))
    area = lambda bs: sum(int((b[:, 2] - b[:, 0]) @ (b[:, 3] - b[:, 1])) for b in bs)  # noqa: E731
    assert area(unregistered) > 2 * area(expect)


def _noise_record(w, scale=3.0):
    return dict(NR.record(w["reg"], scale, 16), shake=w["doc"]["summary"])


@pytest.mark.parametrize("kind", ["png", "y4m"])
def test_noise_shake_and_the_shake_command_print_the_restatements_json(kind, files, want, capsys):
    from vcm_ts_amd import run_codec as RC

    w = want[kind]
    src = ["--frames", str(files / "png")] if kind == "png" else ["--video", str(files / "src.y4m")]
    capsys.readouterr()
    RC.main(["noise", *src, "--min-cells", "16", "--shake", str(RADIUS), "--shake-min-votes", str(VOTES_MIN)])
    assert json.loads(capsys.readouterr().out) == _noise_record(w)
    RC.main(["noise", *src, "--min-cells", "16"])
    plain = json.loads(capsys.readouterr().out)
    assert "shake" not in plain and plain == NR.record(w["seq"], 3.0, 16) and plain["mad32"] > 3 * _noise_record(w)["mad32"]
    RC.main(["shake", *src, "--radius", str(RADIUS), "--min-votes", str(VOTES_MIN), "--out", str(files / f"shake_{kind}.json")])
    assert json.loads(capsys.readouterr().out) == w["doc"] == json.loads((files / f"shake_{kind}.json").read_text())
    RC.main(["shake", *src, "--radius", "4", "--max-frames", "3"])  # six tiles against the default min_votes of 8, and (-4, 5) beyond a radius of 4
    short = json.loads(capsys.readouterr().out)
    assert short == R.document(R.run(w["seq"][:3], 4, 8)[0], 4, 8, 25, H, W) and short["summary"]["lost"] == 2
    # a source whose pictures are lost is refused by name, with the advice: the default min_votes of 8 exceeds its 6 tiles
    with pytest.raises((SystemExit, ValueError)) as ex:
        RC.main(["noise", *src, "--min-cells", "16", "--shake", str(RADIUS)])
    text = capsys.readouterr().err + str(ex.value)
    assert "4 of 5 pictures" in text and "the camera moves" in text and "--tnr T" in text and getattr(ex.value, "code", 2) != 0
    for argv in (["encode", *src, "--bins", str(files / "refused"), "--shake", "8"],
                 ["encode", *src, "--bins", str(files / "refused"), "--tnr", "4", "--shake", "8"],
                 ["noise", *src, "--shake-min-votes", "3"], ["noise", *src, "--shake", "17"], ["shake", *src, "--radius", "0"]):
        with pytest.raises(SystemExit):
            RC.main(argv)
    capsys.readouterr()
    assert not (files / "refused").exists()


def test_encode_tnr_auto_shake_codes_the_bytes_of_the_restatements_threshold(files, want, file_nets, monkeypatch):
    from vcm_ts_amd import run_codec as RC

    w = want["png"]
    rec = _noise_record(w)
    T = rec["threshold"]
    assert 1 < T < 64 and NR.record(w["seq"], 3.0, 16)["threshold"] > T  # the unregistered scan would have chosen a higher one
    params, auto = SH.ShakeParams(RADIUS, VOTES_MIN), N.AutoTNR(min_cells=16)
    plain, size = RC.encode_folder(str(files / "png"), str(files / "given"), gop=GOP, nets=file_nets, tnr=N.TNR(T))
    bits, _ = RC.encode_folder(str(files / "png"), str(files / "auto"), gop=GOP, nets=file_nets, tnr=auto, shake=params, scenecut=0.99)
    assert size == (H, W) and bits == plain and len(bits) == FRAMES and U.bins(files / "auto") == U.bins(files / "given")
    assert json.loads((files / "auto" / "noise.json").read_text()) == rec
    assert json.loads((files / "auto" / "shake.json").read_text()) == w["doc"]
    assert U.others(files / "auto") == ["gops.json", "noise.json", "shake.json"] and U.others(files / "given") == []
    # the scene scan saw the unregistered pictures: its plan is that of the same encode without the option
    gops = json.loads((files / "auto" / "gops.json").read_text())
    RC.encode_folder(str(files / "png"), str(files / "auto"), gop=GOP, nets=file_nets, tnr=auto, scenecut=0.99)
    assert json.loads((files / "auto" / "gops.json").read_text()) == gops
    assert U.others(files / "auto") == ["gops.json", "noise.json"]  # (the stale shake.json is gone)
    assert "shake" not in json.loads((files / "auto" / "noise.json").read_text())
    for bad, match in ((dict(tnr=N.TNR(4), shake=params), "belongs to a tnr.AutoTNR"), (dict(tnr=auto, shake=8), "ShakeParams")):
        with pytest.raises(ValueError, match=match):
            RC.encode_folder(str(files / "png"), str(files / "bad"), gop=GOP, nets=file_nets, **bad)
    assert not (files / "bad").exists() or U.bins(files / "bad") == {}
    # the command line, from the Y4M file
    v = want["y4m"]
    monkeypatch.setattr(RC, "_nets", lambda *a, **k: file_nets[0])
    RC.main(["encode", "--video", str(files / "src.y4m"), "--bins", str(files / "cli"), "--gop", str(GOP), "--tnr-auto",
             "--tnr-auto-min-cells", "16", "--shake", str(RADIUS), "--shake-min-votes", str(VOTES_MIN)])
    vrec = _noise_record(v)
    RC.encode_video(str(files / "src.y4m"), str(files / "cli_given"), gop=GOP, nets=file_nets, tnr=N.TNR(vrec["threshold"]))
    assert U.bins(files / "cli") == U.bins(files / "cli_given")
    assert json.loads((files / "cli" / "noise.json").read_text()) == vrec and json.loads((files / "cli" / "shake.json").read_text()) == v["doc"]
    assert U.others(files / "cli") == ["noise.json", "sequence.json", "shake.json"] and U.others(files / "cli_given") == ["sequence.json"]
