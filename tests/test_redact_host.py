"""ROI redaction without a GPU: the properties of the numpy restatement (tests/redact_ref.py) that the header states, the
host half of vcm_ts_amd/redact.py (Redact, held_boxes), the entry point's refusals (which return before anything is
launched) and every refusal of the command line."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import gpu_util as U
from tests import redact_ref as R
from vcm_ts_amd import redact as D
from vcm_ts_amd import roi as X

F32 = np.float32


def test_table_is_the_hosts_division_and_codes_back():
    assert R.T.dtype == F32 and np.array_equal(R.T, np.array([F32(k) / F32(255.0) for k in range(256)], F32))
    assert np.array_equal(R.code(R.T), np.arange(256))
    assert R.code(F32(np.nan)) == 0 and R.code(F32(-3)) == 0 and R.code(F32(np.inf)) == 255 and R.code(F32(0.5)) == 128


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_properties(size):
    H, W = size
    pic = R.picture(H, W)
    assert np.isnan(pic).any() or H * W < 8
    for name, boxes, grow in R.cases(H, W):
        Rg = R.region(boxes, H, W, R.MASK, grow)
        for tile, fill in R.MODES:
            out, count = R.expected(H, W, name, grow, tile, fill)
            assert out.dtype == F32 and count.shape == R.grid(H, W)
            assert np.array_equal(U.f32_bits(out)[:, ~Rg], U.f32_bits(pic)[:, ~Rg])  # outside R: the bits, NaN payloads included
            inside = out[:, Rg]
            k = R.code(inside)
            assert np.array_equal(U.f32_bits(inside), U.f32_bits(R.T[k])) and np.array_equal(np.rint(F32(255.0) * R.T[k]).astype(np.int64), k)
            assert int(count.sum()) == int(Rg.sum()) and count.max(initial=0) <= 256
            assert not count[(H + 15) // 16:].any() and not count[:, (W + 15) // 16:].any()
            if tile == 0:
                assert (k == fill).all()
        if name == "none":
            assert not Rg.any()
        if name == "whole":
            assert Rg.all()


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiles_inside_r_show_their_rounded_mean(size):
    """Every tile of the grid, the clipped ones at the right and lower edge with n_t < tile^2 included, is constant and
    holds the mean of its own pixels' codes rounded half up -- in exact rational arithmetic here."""
    from fractions import Fraction

    H, W = size
    pic = R.picture(H, W)
    codes = R.code(pic)
    for tile in R.TILES:
        out, _ = R.expected(H, W, "whole", R.GROW, tile, -1)
        clipped = 0
        for y in range(0, H, tile):
            for x in range(0, W, tile):
                block = codes[:, y:y + tile, x:x + tile]
                n = block.shape[1] * block.shape[2]
                clipped += n < tile * tile
                for c in range(3):
                    m = int(np.floor(Fraction(int(block[c].sum()), n) + Fraction(1, 2)))
                    assert (out[c, y:y + tile, x:x + tile] == R.T[m]).all(), (tile, y, x, c)
        assert clipped > 0 or (H % tile == 0 and W % tile == 0)
    # a mean of exactly k + 1/2 rounds up
    half = np.zeros((3, 2, 2), F32)
    half[:, 0, 0] = R.T[2]
    assert (R.redact(half, [[0, 0, 2, 2, 0]], 1, 0, 2, -1)[0] == R.T[1]).all()
    half[:, 0, 1] = R.T[255]
    assert (R.redact(half, [[0, 0, 2, 2, 0]], 1, 0, 2, -1)[0] == R.T[64]).all()  # 257 / 4 = 64.25


def test_the_grid_does_not_move_with_the_boxes():
    H, W = 70, 100
    pic = R.picture(H, W)
    whole = R.expected(H, W, "whole", R.GROW, 16, -1)[0]
    for box in ([3, 5, 40, 33, 0], [17, 1, 99, 70, 2], [50, 50, 51, 51, 0]):
        out, _ = R.redact(pic, [box], R.MASK, 0, 16, -1)
        Rg = R.region([box], H, W, R.MASK, 0)
        assert np.array_equal(U.f32_bits(out)[:, Rg], U.f32_bits(whole)[:, Rg])  # a tile's value comes from ALL its pixels, in R or not


def test_grow_clips_and_empty_or_unselected_boxes_change_nothing():
    H, W = 70, 100
    pic = R.picture(H, W)
    Rg = R.region([[2, 3, 4, 5, 0], [97, 66, 100, 70, 2]], H, W, R.MASK, 5)
    want = np.zeros((H, W), bool)
    want[0:10, 0:9] = True
    want[61:70, 92:100] = True
    assert np.array_equal(Rg, want)
    for boxes in ([[5, 5, 5, 40, 0]], [[5, 40, 30, 40, 2]], [[30, 30, 10, 10, 0]], [[5, 5, 60, 60, 1]], [[5, 5, 60, 60, 3]]):
        for grow in (0, 200):
            out, count = R.redact(pic, boxes, R.MASK, grow, 8, -1)
            assert np.array_equal(U.f32_bits(out), U.f32_bits(pic)) and not count.any(), (boxes, grow)
    # an unselected box neither adds to R nor shields what a selected one covers
    a = R.redact(pic, [[10, 10, 50, 50, 0]], R.MASK, 2, 0, 9)
    b = R.redact(pic, [[0, 0, 100, 70, 1], [10, 10, 50, 50, 0], [20, 20, 30, 30, 1]], R.MASK, 2, 0, 9)
    assert np.array_equal(U.f32_bits(a[0]), U.f32_bits(b[0])) and np.array_equal(a[1], b[1]) and int(a[1].sum()) == 44 * 44


def test_list_order_does_not_matter():
    H, W = 130, 200
    pic, boxes = R.picture(H, W), R.box_sets(H, W)["random300"]
    assert len(boxes) == 300 and len(R.box_sets(H, W)["full1024"]) == R.MAX_BOXES == X.MAX_BOXES
    g = np.random.default_rng(3)
    for tile, fill in ((4, -1), (32, -1), (0, 77)):
        want = R.redact(pic, boxes, R.MASK, 3, tile, fill)
        for _ in range(3):
            got = R.redact(pic, boxes[g.permutation(len(boxes))], R.MASK, 3, tile, fill)
            assert np.array_equal(U.f32_bits(got[0]), U.f32_bits(want[0])) and np.array_equal(got[1], want[1])


def test_held_boxes_at_the_ends_and_across_gops():
    frames = R.clip_boxes(128, 192)
    assert len(frames) == 8 and not any(b[4] == 2 for b in frames[0].tolist())
    for mask in (0b001, 0b100, 0b101, 0b111):
        for hold in (0, 1, 2, 32):
            for g in range(len(frames)):
                got = D.held_boxes([X.FrameBoxes(f) for f in frames], g, mask, hold)
                want = R.held_boxes(frames, g, mask, hold)
                assert isinstance(got, X.FrameBoxes) and np.array_equal(got.array, want), (mask, hold, g)
                assert all((mask >> c) & 1 for c in got.array[:, 4].tolist())
    # the sequence's ends: only pictures that exist; a GOP boundary (GOP 4: pictures 3 | 4) is no boundary for the lists
    assert len(D.held_boxes(frames, 0, 0b100, 0)) == 0 and len(D.held_boxes(frames, 0, 0b100, 2)) == 2
    assert np.array_equal(D.held_boxes(frames, 7, 0b100, 2).array[:, 0], [9 * t + 4 for t in (5, 6, 7)])
    assert np.array_equal(D.held_boxes(frames, 4, 0b100, 2).array[:, 0], [9 * t + 4 for t in (2, 3, 4, 5, 6)])
    # the plate the detector misses in pictures 3 and 4 is still covered there with hold >= 2, from both sides
    assert len(D.held_boxes(frames, 3, 0b001, 0)) == 0 and len(D.held_boxes(frames, 3, 0b001, 1)) == 1
    assert np.array_equal(D.held_boxes(frames, 4, 0b001, 2).array[:, 0], [62, 65, 66])
    # raw arrays and an empty sequence are taken too
    assert len(D.held_boxes([], 0, 1, 3)) == 0
    # more than 1024 after merging: refused by naming the picture, on the host
    many = [R.random_boxes(128, 192, 400, s) for s in range(4)]
    assert len(D.held_boxes(many, 0, 0b111, 1)) == 800
    with pytest.raises(ValueError, match="picture 1 .*1200 boxes"):
        D.held_boxes(many, 1, 0b111, 1)
    with pytest.raises(ValueError, match="picture 1"):
        R.held_boxes(many, 1, 0b111, 1)
    assert len(D.held_boxes(many, 1, 0b001, 1)) == sum(int((m[:, 4] == 0).sum()) for m in many[:3]) <= 1024


def test_redact_validation_and_json():
    r = D.Redact(["liplates", "motion"], tile=8, grow=3, hold=2)
    assert r.classes == ("liplates", "motion") and r.mode() == (8, -1) and r.mask(R.NAMES) == 0b101 and r.mask(("motion", "liplates")) == 0b11
    assert r.to_json() == {"classes": ["liplates", "motion"], "tile": 8, "fill": None, "grow": 3, "hold": 2, "restorable": False}
    assert json.loads(json.dumps(r.to_json())) == r.to_json()
    s = D.Redact("faces", fill=0, restorable=True)
    assert s.classes == ("faces",) and s.mode() == (0, 0) and s.to_json()["restorable"] is True and s.to_json()["tile"] is None
    assert D.Redact(("faces",), tile=np.int64(64)).tile == 64 and D.Redact(("faces",), fill=255).mode() == (0, 255)
    with pytest.raises(Exception):
        r.tile = 4  # frozen
    for kw, name in ((dict(classes=("faces",)), "exactly one of tile"), (dict(classes=("faces",), tile=8, fill=0), "exactly one of tile"),
                     (dict(classes=("faces",), tile=3), "tile"), (dict(classes=("faces",), tile=1), "tile"),
                     (dict(classes=("faces",), tile=128), "tile"), (dict(classes=("faces",), tile=8.0), "tile"),
                     (dict(classes=("faces",), tile=True), "tile"), (dict(classes=("faces",), fill=-1), "fill"),
                     (dict(classes=("faces",), fill=256), "fill"), (dict(classes=("faces",), fill=1.5), "fill"),
                     (dict(classes=("faces",), tile=8, grow=-1), "grow"), (dict(classes=("faces",), tile=8, grow=256), "grow"),
                     (dict(classes=("faces",), tile=8, hold=-1), "hold"), (dict(classes=("faces",), tile=8, hold=33), "hold"),
                     (dict(classes=("faces",), tile=8, restorable=1), "restorable"), (dict(classes=(), tile=8), "classes"),
                     (dict(classes=("faces", "faces"), tile=8), "'faces' is named twice"), (dict(classes=(0,), tile=8), "classes"),
                     (dict(classes=3, tile=8), "classes")):
        with pytest.raises(ValueError, match=name):
            D.Redact(**kw)
    with pytest.raises(TypeError):
        D.Redact()  # (no default classes)
    with pytest.raises(ValueError, match="no class 'plates' among the roi's classes"):
        D.Redact(("plates",), tile=8).mask(R.NAMES)
    with pytest.raises(ValueError, match="no class 'motion'"):
        r.mask(("liplates", "faces"))  # a root without motion_coords
    with pytest.raises(ValueError, match="redact.Redact"):
        D.Redactor((("faces",), 8), None, (70, 100), "cuda:0")
    roi = X.Roi(lambda g: X.FrameBoxes(), (X.RoiClass(0),) * 3, R.NAMES)
    with pytest.raises(ValueError, match="no CPU fallback"):
        D.Redactor(r, roi, (70, 100), "cpu")


def test_entry_point_refuses_on_the_host():
    """Every refusal of include/dcvc_hip_redact.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU.  (The box list is real host memory: it is validated.)"""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)
    keep = np.ascontiguousarray(R.box_sets(H, W)["classes"], dtype=np.int32)

    def with_box(row):
        a = keep.copy()
        a[-1] = row
        return a

    lists = [with_box(r) for r in ([-1, 0, 5, 5, 0], [0, 0, W + 1, 5, 0], [0, -1, 5, 5, 0], [0, 0, 5, H + 1, 0], [0, 0, 5, 5, -1], [0, 0, 5, 5, 4])]
    good = dict(src=0x10000000, srs=rs, sps=ps, out=0x30000000, ors=rs, ops=ps, H=H, W=W, host=keep.ctypes.data, dev=0x70000000,
                n=len(keep), mask=0b101, grow=5, tile=8, fill=-1, count=0x60000000)
    order = ("src", "srs", "sps", "out", "ors", "ops", "H", "W", "host", "dev", "n", "mask", "grow", "tile", "fill", "count")
    bad = [{k: None} for k in ("src", "out", "count", "host", "dev")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"srs": W - 1}, {"ors": W - 1}, {"sps": (H - 1) * rs + W - 1},
           {"ops": (H - 1) * rs + W - 1}, {"src": good["src"] + 2}, {"out": good["out"] + 2}, {"count": good["count"] + 1},
           {"n": -1}, {"n": 1025}, {"grow": -1}, {"grow": 256}, {"mask": 0}, {"mask": 16}, {"mask": -1},
           {"tile": 0, "fill": -1}, {"tile": 8, "fill": 0}, {"tile": 64, "fill": 255}, {"tile": 0, "fill": 256}, {"tile": 0, "fill": -2},
           {"tile": 1}, {"tile": 3}, {"tile": 24}, {"tile": 128}, {"tile": -8},
           {"out": good["src"]}, {"out": good["src"] + span - 4}, {"out": good["src"] - span + 4}, {"out": good["src"] + 4 * ps}] + \
          [{"host": a.ctypes.data} for a in lists]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_redact(*[v[k] for k in order], None) == -1, b


def _root(path, frames, names=R.NAMES):
    """A PickleBoxes root holding `frames` ((n, 5) arrays), one folder per class name."""
    for cls, name in enumerate(names):
        folder = path / f"{name}_coords"
        os.makedirs(folder)
        for t, a in enumerate(frames):
            with open(folder / ("%05d" % (t + 1)), "wb") as f:
                pickle.dump(np.asarray(a)[np.asarray(a)[:, 4] == cls][:, :4].astype(np.uint16), f)
    return str(path)


def test_cli_refusals(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    two = _root(tmp_path / "two", R.clip_boxes(128, 192), ("liplates", "faces"))
    three = _root(tmp_path / "three", R.clip_boxes(128, 192))
    assert X.PickleBoxes(three).names == R.NAMES and X.PickleBoxes(two).names == ("liplates", "faces")
    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    cases = [
        (["--redact-tile", "8"], "belong to --redact"), (["--redact-fill", "0"], "belong to --redact"),
        (["--redact-grow", "2"], "belong to --redact"), (["--redact-hold", "1"], "belong to --redact"),
        (["--redact-restorable"], "belong to --redact"), (["--roi-root", three, "--redact-hold", "0"], "belong to --redact"),
        (["--redact", "faces", "--redact-tile", "8"], "--redact needs --roi-root"),
        (["--roi-root", three, "--redact", "faces"], "exactly one of tile"),
        (["--roi-root", three, "--redact", "faces", "--redact-tile", "8", "--redact-fill", "0"], "exactly one of tile"),
        (["--roi-root", three, "--redact", "faces", "--redact-tile", "12"], "tile must be one of"),
        (["--roi-root", three, "--redact", "faces", "--redact-fill", "256"], "fill"),
        (["--roi-root", three, "--redact", "faces", "--redact-fill", "-1"], "fill"),
        (["--roi-root", three, "--redact", "faces", "--redact-tile", "8", "--redact-grow", "256"], "grow"),
        (["--roi-root", three, "--redact", "faces", "--redact-tile", "8", "--redact-hold", "33"], "hold"),
        (["--roi-root", three, "--redact", "faces", "faces", "--redact-tile", "8"], "named twice"),
        (["--roi-root", three, "--redact", "plates", "--redact-tile", "8"], "no class 'plates'"),
        (["--roi-root", two, "--redact", "motion", "--redact-tile", "8"], "no class 'motion'"),
        (["--roi-root", three, "--redact", "faces", "--redact-tile", "8", "--residual-bins", str(tmp_path / "rl")], "--redact-restorable"),
        (["--roi-root", three, "--redact", "faces", "--redact-fill", "0", "--residuals", str(tmp_path / "res.gbrp")], "--redact-restorable"),
    ]
    for extra, name in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and name in err, (extra, err)
    assert not (tmp_path / "bins").exists() and not (tmp_path / "rl").exists()


def test_api_refusals_come_before_any_gpu_work(tmp_path):
    """The loops refuse by name before they look at a file or at the device: the folders do not exist."""
    from vcm_ts_amd import run_codec as RC

    roi = X.Roi(lambda g: X.FrameBoxes(), (X.RoiClass(0),) * 3, R.NAMES)
    r = D.Redact(("faces",), tile=8)
    for kw, name in ((dict(redact=r), "needs roi="), (dict(redact=(("faces",), 8), roi=roi), "redact.Redact"),
                     (dict(redact=D.Redact(("plates",), tile=8), roi=roi), "no class 'plates'"),
                     (dict(redact=r, roi=roi, residual_bins=str(tmp_path / "rl")), "restorable=True"),
                     (dict(redact=r, roi=roi, residuals=str(tmp_path / "r.gbrp")), "restorable=True")):
        with pytest.raises(ValueError, match=name):
            RC._redact_args(kw.get("redact"), kw.get("roi"), kw.get("residuals"), kw.get("residual_bins"))
    RC._redact_args(D.Redact(("faces",), tile=8, restorable=True), roi, None, str(tmp_path / "rl"))
    RC._redact_args(None, None, "x", "y")
    assert not (tmp_path / "rl").exists()
    # the setting's file: written for a redacted encode, a stale one removed without
    RC._write_redact(str(tmp_path), r)
    assert json.loads((tmp_path / RC.REDACT_JSON).read_text()) == r.to_json()
    RC._write_redact(str(tmp_path), None)
    assert not (tmp_path / RC.REDACT_JSON).exists()
