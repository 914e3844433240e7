"""Motion ROI boxes without a GPU: motionroi.boxes_from_counts against the numpy restatement (tests/motion_ref.py, which
restates include/dcvc_hip_motion.h and the seven steps of the box rule with scipy.ndimage), hand-made grids, the properties
of the background model on the restatement, the coordinate files through roi.PickleBoxes, motion.json, and the refusals
by name."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import motion_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import motionroi as M
from vcm_ts_amd import roi as X


def _same(a, b):
    return a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)


def test_header_symbols_and_build_wiring():
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "motion.hip" in mk and "dcvc_hip_motion.h" in mk
    src = open(os.path.join(lib.CSRC, "motion.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include")[-1]
    # the code and the luma are those the other kernels use, written once
    assert "luma8(code8(" in src and "rintf" not in src


# ------------------------------------------------------------------------------------------------------------ the boxes
GRIDS = [((64, 64), (4, 4)), ((128, 192), (8, 12)), ((1080, 1920), (68, 120)), ((70, 100), (8, 8))]


def test_boxes_equal_the_restatement_on_random_grids():
    g = np.random.default_rng(5)
    n = ran = capped = kept_all = 0
    for (H, W), cells in GRIDS:
        assert X.grid_of(H, W) == R.grid(H, W) == cells
        for density in (0.01, 0.03, 0.08, 0.15, 0.3, 0.5, 0.8, 1.0):
            for grow in range(4):
                for min_cells in (1, 3):
                    for max_boxes in (2, 5, 64):
                        if (n + grow) % 3 and cells[0] > 8:  # (a third of the large grids: they are the slow ones)
                            n += 1
                            continue
                        counts = g.integers(0, 257, cells) * (g.random(cells) < density)
                        p = M.MotionParams(24, min_pixels=8, grow=grow, min_cells=min_cells, max_boxes=max_boxes)
                        got = M.boxes_from_counts(counts, H, W, p)
                        want = R.boxes(counts, H, W, 8, grow, min_cells, max_boxes)
                        assert _same(got, want), (H, W, density, grow, min_cells, max_boxes)
                        free = R.boxes(counts, H, W, 8, grow, min_cells, 10 ** 6)
                        capped += len(free) > max_boxes
                        kept_all += 0 < len(free) <= max_boxes
                        assert len(got) == min(len(free), max_boxes)
                        n += 1
                        ran += 1
    assert ran >= 200 and capped >= 20 and kept_all >= 20, (ran, capped, kept_all)


def _grid(H, W, cells):
    c = np.zeros(X.grid_of(H, W), dtype=np.int32)
    for (i, j), v in cells.items():
        c[i, j] = v
    return c


def test_hand_made_grids():
    P = M.MotionParams
    # two diagonal cells are one 8-connected region
    assert M.boxes_from_counts(_grid(128, 192, {(1, 1): 9, (2, 2): 9}), 128, 192, P(24, grow=0)).tolist() == [[16, 16, 48, 48]]
    # two cells two apart: two boxes at grow 0, one at grow 1 (the dilations touch)
    far = _grid(128, 192, {(1, 1): 9, (1, 4): 9})
    assert M.boxes_from_counts(far, 128, 192, P(24, grow=0)).tolist() == [[16, 16, 32, 32], [64, 16, 80, 32]]
    assert M.boxes_from_counts(far, 128, 192, P(24, grow=1)).tolist() == [[0, 0, 96, 48]]
    # 70 x 100: the last cell row and column with pixels are clipped to the picture
    assert X.grid_of(70, 100) == (8, 8)
    assert M.boxes_from_counts(_grid(70, 100, {(4, 6): 200}), 70, 100, P(24, grow=0)).tolist() == [[96, 64, 100, 70]]
    assert M.boxes_from_counts(_grid(70, 100, {(4, 6): 200}), 70, 100, P(24, grow=1)).tolist() == [[80, 48, 100, 70]]
    # a region of padding cells alone (the kernel writes 0 there, so only a foreign grid holds one) has an empty box
    assert len(M.boxes_from_counts(_grid(70, 100, {(6, 7): 200}), 70, 100, P(24, grow=0))) == 0
    assert _same(M.boxes_from_counts(_grid(70, 100, {(6, 7): 200}), 70, 100, P(24, grow=0)), R.boxes(_grid(70, 100, {(6, 7): 200}), 70, 100, grow=0))
    # min_pixels is inclusive
    edge = _grid(64, 64, {(0, 0): 7, (2, 2): 8})
    assert M.boxes_from_counts(edge, 64, 64, P(24, grow=0)).tolist() == [[32, 32, 48, 48]]
    assert M.boxes_from_counts(edge, 64, 64, P(24, grow=0, min_pixels=7)).tolist() == [[0, 0, 16, 16], [32, 32, 48, 48]]
    # min_cells counts ACTIVE cells, not dilated ones
    assert len(M.boxes_from_counts(edge, 64, 64, P(24, grow=1, min_cells=2))) == 0
    assert len(M.boxes_from_counts(_grid(64, 64, {(0, 0): 9, (1, 1): 9}), 64, 64, P(24, grow=1, min_cells=2))) == 1
    # the cap keeps the largest sums; equal sums go to the smaller (y1, x1, y2, x2); the output is sorted by position
    tie = _grid(128, 192, {(0, 0): 50, (0, 4): 90, (4, 0): 50, (4, 4): 50, (6, 8): 20})
    assert M.boxes_from_counts(tie, 128, 192, P(24, grow=0, max_boxes=3)).tolist() == \
        [[0, 0, 16, 16], [64, 0, 80, 16], [0, 64, 16, 80]]
    assert M.boxes_from_counts(tie, 128, 192, P(24, grow=0, max_boxes=1)).tolist() == [[64, 0, 80, 16]]
    assert _same(M.boxes_from_counts(tie, 128, 192, P(24, grow=0, max_boxes=3)), R.boxes(tie, 128, 192, grow=0, max_boxes=3))
    # nothing active, and the output's type
    none = M.boxes_from_counts(_grid(64, 64, {}), 64, 64, P(24))
    assert none.shape == (0, 4) and none.dtype == np.int32
    # what it refuses
    with pytest.raises(ValueError, match="grid of"):
        M.boxes_from_counts(np.zeros((4, 5), np.int32), 64, 64, P(24))
    with pytest.raises(ValueError, match="grid of"):
        M.boxes_from_counts(np.zeros((4, 4), np.float32), 64, 64, P(24))
    with pytest.raises(ValueError, match="MotionParams"):
        M.boxes_from_counts(np.zeros((4, 4), np.int32), 64, 64, {"threshold": 24})
    assert [len(b) for b in M.boxes_of_scan(np.stack([tie, tie]), 128, 192, P(24, grow=0))] == [0, 5]


# ------------------------------------------------------------------------------------------------------------ the model
def test_model_properties_on_the_restatement():
    H, W = 48, 80
    g = np.random.default_rng(9)
    pics = [(g.standard_normal((3, H, W)) * 0.5 + 0.5).astype(np.float32) for _ in range(50)]
    for T, k_bg, k_fg in R.SETTINGS + [(24, 1, 2)]:
        bg, counts = R.init(pics[0])
        assert counts.shape == R.grid(H, W) and not counts.any()
        for pic in pics[1:]:
            bg, counts = R.step(pic, bg, T, k_bg, k_fg)
            assert bg.min() >= 0 and bg.max() <= 65280
            assert counts.min() >= 0 and counts.max() <= 256 and not counts[3:].any() and not counts[:, 5:].any()
    start = R.init(pics[0])[0]
    assert np.array_equal(R.step(pics[1], start, 24, 16, 16)[0], start)                    # k = 16 never moves the model
    assert np.array_equal(R.step(pics[1], start, 24, 0, 0)[0], R.luma(pics[1]) << 8)       # k = 0 lands on Y << 8
    # |delta| = 1 .. 2^k - 1 moves nothing, 2^k moves by one, whatever the sign
    grey = np.full((3, 1, 1), np.float32(100.0 / 255.0))
    for k in (1, 4, 8):
        for d in (1, 2 ** k - 1):
            for sign in (1, -1):
                b = np.array([[(100 << 8) + sign * d]])
                assert R.step(grey, b, 254, k, k)[0][0, 0] == b[0, 0]
        assert R.step(grey, np.array([[(100 << 8) + 2 ** k]]), 254, k, k)[0][0, 0] == (100 << 8) + 2 ** k - 1
        assert R.step(grey, np.array([[(100 << 8) - 2 ** k]]), 254, k, k)[0][0, 0] == (100 << 8) - 2 ** k + 1
    # a == T << 8 is background, a == (T << 8) + 1 foreground
    for T in (1, 24, 254):
        b, pic = R.edge_case(16, 16, T)
        new, counts = R.step(pic, b, T, 16, 16)
        assert counts[0, 0] == 128 and counts.sum() == 128
        new, counts = R.step(pic, b, T, 0, 16)  # (the background half follows the picture, the foreground half stays)
        assert np.array_equal(new[:, 0::2], (R.luma(pic) << 8)[:, 0::2]) and np.array_equal(new[:, 1::2], b[:, 1::2])


def test_the_clip_yields_the_boxes_the_issue_asks_for():
    """The end-to-end conditions of tests/test_gpu_motion.py on the restatement alone: what the GPU test then demands of
    the kernel is demanded of a clip that can meet it."""
    for H, W in ((128, 192), (70, 100)):
        pics, rects = R.clip(H, W)
        per = R.clip_boxes(pics, 24)
        assert len(per) == R.CLIP_FRAMES and len(per[0]) == 0
        for t in range(1, R.CLIP_FRAMES):
            assert len(per[t]) >= 1 and R.covered(rects[t], per[t]), (H, W, t, per[t].tolist())
        assert all(len(b) == 0 for b in R.clip_boxes(R.clip(H, W, rectangle=False)[0], 24))


# ------------------------------------------------------------------------------------------------------------ the files
def test_written_boxes_come_back_through_pickleboxes(tmp_path):
    root = str(tmp_path / "root")
    per = [np.zeros((0, 4), np.int32), np.array([[16, 0, 64, 48], [0, 64, 32, 70]], np.int32), np.zeros((0, 4), np.int32)]
    p = M.MotionParams(24, learn=(3, 9), grow=2)
    M.write_boxes(root, per, p, 70, 100)
    assert sorted(os.listdir(os.path.join(root, "motion_coords"))) == ["00001", "00002", "00003"]
    with open(os.path.join(root, "motion_coords", "00002"), "rb") as f:
        raw = pickle.load(f)
    assert raw.dtype == np.uint16 and raw.tolist() == per[1].tolist()
    src = X.PickleBoxes(root)
    assert src.names == ("liplates", "faces", "motion") and len(src.classes) == 3
    assert [src(t).array.tolist() for t in range(3)] == [[], [[16, 0, 64, 48, 2], [0, 64, 32, 70, 2]], []]
    roi = X.Roi(src, src.classes)
    assert roi.names[2] == "motion" and len(roi.frame(1, 70, 100)) == 2
    with pytest.raises(ValueError, match="three classes"):
        X.PickleBoxes(root, (X.RoiClass(0), X.RoiClass(0)))
    # beside plates: plates first, motion last
    os.makedirs(os.path.join(root, "liplates_coords"))
    for t in range(3):
        with open(os.path.join(root, "liplates_coords", "%05d" % (t + 1)), "wb") as f:
            pickle.dump(np.array([[1, 2, 3, 4]], np.uint16), f)
    assert X.PickleBoxes(root, (X.RoiClass(1), X.RoiClass(2), X.RoiClass(3)))(1).array.tolist() == \
        [[1, 2, 3, 4, 0], [16, 0, 64, 48, 2], [0, 64, 32, 70, 2]]
    # motion.json round-trips
    assert M.read_info(root) == (p, 70, 100, 3)
    info = json.load(open(os.path.join(root, "motion.json")))
    assert info["version"] == 1 and info["frames"] == 3 and info["params"]["learn"] == [3, 9]
    assert M.MotionParams.from_json(info["params"]) == p
    assert M.read_info(str(tmp_path)) is None
    # the same run again is fine; another frame count or size is refused and nothing is touched
    M.write_boxes(root, per, p, 70, 100)
    for bad_per, h, w in ((per[:2], 70, 100), (per, 70, 104), (per, 72, 100)):
        with pytest.raises(ValueError, match="another run"):
            M.write_boxes(root, bad_per, p, h, w)
    assert sorted(os.listdir(os.path.join(root, "motion_coords"))) == ["00001", "00002", "00003"]
    os.remove(os.path.join(root, "motion.json"))
    with pytest.raises(ValueError, match="does not say whose"):
        M.write_boxes(root, per, p, 70, 100)
    with pytest.raises(ValueError, match="out of range"):
        M.write_boxes(str(tmp_path / "x"), [np.array([[0, 0, 101, 10]])], p, 70, 100)
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        M.write_boxes(str(tmp_path / "x"), [np.zeros((1, 5), np.int32)], p, 70, 100)
    assert not os.path.exists(str(tmp_path / "x"))
    bad = dict(info, version=2)
    os.makedirs(tmp_path / "v2")
    json.dump(bad, open(tmp_path / "v2" / "motion.json", "w"))
    with pytest.raises(ValueError, match="version"):
        M.read_info(str(tmp_path / "v2"))


def test_a_root_without_motion_coords_is_what_it_was(tmp_path):
    root = tmp_path / "old"
    os.makedirs(root / "faces_coords")
    with open(root / "faces_coords" / "00001", "wb") as f:
        pickle.dump(np.array([[1, 1, 2, 2]], np.uint16), f)
    src = X.PickleBoxes(str(root))
    assert src.names == ("liplates", "faces") and len(src.classes) == 2 and src(0).array.tolist() == [[1, 1, 2, 2, 1]]
    assert not X.PickleBoxes.has_motion(str(root))
    with pytest.raises(ValueError, match="two classes"):
        X.PickleBoxes(str(root), (X.RoiClass(0),) * 3)
    os.makedirs(tmp_path / "nothing")
    with pytest.raises(FileNotFoundError, match="neither liplates_coords nor faces_coords"):
        X.PickleBoxes(str(tmp_path / "nothing"))


def test_params_refuse_by_name():
    p = M.MotionParams(24)
    assert (p.learn, p.min_pixels, p.grow, p.min_cells, p.max_boxes) == ((4, 8), 8, 1, 1, 64)
    with pytest.raises(TypeError):
        M.MotionParams()  # no default threshold
    with pytest.raises(Exception):
        p.threshold = 3  # frozen
    for kw, name in (({"threshold": 0}, "threshold"), ({"threshold": 255}, "threshold"), ({"threshold": 24.0}, "threshold"),
                     ({"threshold": True}, "threshold"), ({"learn": (17, 8)}, "k_bg"), ({"learn": (4, -1)}, "k_fg"),
                     ({"learn": 4}, "learn"), ({"learn": (4, 8, 2)}, "learn"), ({"min_pixels": 0}, "min_pixels"),
                     ({"min_pixels": 257}, "min_pixels"), ({"grow": -1}, "grow"), ({"grow": 9}, "grow"),
                     ({"min_cells": 0}, "min_cells"), ({"min_cells": 65536}, "min_cells"), ({"max_boxes": 0}, "max_boxes"),
                     ({"max_boxes": X.MAX_BOXES + 1}, "max_boxes")):
        with pytest.raises(ValueError, match=name):
            M.MotionParams(**dict({"threshold": 24}, **kw))
    assert M.MotionParams(254, learn=[0, 16], min_pixels=256, grow=8, min_cells=65535, max_boxes=X.MAX_BOXES).learn == (0, 16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.MotionScan("cpu", 64, 64, 2, p)


def test_entry_point_refuses_before_any_launch():
    """Host-only: a refused call launches nothing and dereferences nothing (the pointers are aligned dummies)."""
    L = lib.hip()
    good = dict(rgb=0x10000, rs=100, ps=7000, H=70, W=100, bg=0x20000, init=0, T=24, k_bg=4, k_fg=8, counts=0x30000)

    def call(**kw):
        v = dict(good, **kw)
        return L.dcvc_motion_step(*[v[k] for k in ("rgb", "rs", "ps", "H", "W", "bg", "init", "T", "k_bg", "k_fg", "counts")], None)

    for bad in ({"rgb": None}, {"bg": None}, {"counts": None}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1},
                {"rs": 99}, {"ps": 69 * 100 + 99}, {"T": 0}, {"T": 255}, {"k_bg": -1}, {"k_bg": 17}, {"k_fg": -1},
                {"k_fg": 17}, {"rgb": 0x10002}, {"bg": 0x20001}, {"counts": 0x30001},
                {"init": 1, "T": 0}, {"init": 1, "k_bg": 17}, {"init": 1, "k_fg": 17}):
        assert call(**bad) == -1, bad


def test_command_line_threads_the_motion_class(tmp_path, monkeypatch, capsys):
    """--motion-q and --motion-border go where the plates' options go, only for a root that holds motion_coords; the option
    errors of `boxes` go through ap.error before anything touches a GPU."""
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    M.write_boxes("ROOT", [np.zeros((0, 4), np.int32)], M.MotionParams(24), 64, 96)
    os.makedirs("OLD/faces_coords")
    seen = {}

    def fake_encode(*args, **kw):
        seen.update(kw)
        return [8], (64, 96)

    def fake_decode(*args, **kw):
        seen.update(kw)
        return 1

    monkeypatch.setattr(RC, "encode_folder", fake_encode)
    monkeypatch.setattr(RC, "decode_folder", fake_decode)
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--motion-q", "0.5", "--background-q", "2.0", "--motion-border", "6"])
    assert seen["roi_q"] == X.RoiQ(200, (100, 100, 50), 0) and seen["roi"].names == ("liplates", "faces", "motion")
    assert [c.border for c in seen["roi"].classes] == [0, 0, 6]
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--plate-q", "0.6"])
    assert seen["roi_q"] == X.RoiQ(100, (60, 100, 100), 0)
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT"])
    assert seen["roi_q"] is None and len(seen["roi"].classes) == 3
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "OLD", "--plate-q", "0.6"])
    assert seen["roi_q"] == X.RoiQ(100, (60, 100), 0) and seen["roi"].names == ("liplates", "faces")
    os.makedirs("Q")
    RC.write_roiq("Q", X.RoiQ(200, (100, 100, 50)), ("liplates", "faces", "motion"))
    seen.clear()
    RC.main(["decode", "--bins", "Q", "--recon", "R", "--height", "64", "--width", "96", "--roi-root", "ROOT", "--motion-border", "3"])
    assert seen["roi"].names[2] == "motion" and seen["roi"].classes[2].border == 3
    assert RC.read_roiq("Q", seen["roi"]) == X.RoiQ(200, (100, 100, 50))
    for argv in (["encode", "--frames", "F", "--bins", "B", "--motion-q", "0.5"],
                 ["encode", "--frames", "F", "--bins", "B", "--roi-root", "OLD", "--motion-q", "0.5"],
                 ["encode", "--frames", "F", "--bins", "B", "--roi-root", "OLD", "--motion-border", "2"],
                 ["decode", "--bins", "Q", "--recon", "R", "--height", "64", "--width", "96", "--roi-root", "OLD", "--motion-border", "2"],
                 ["decode", "--bins", "Q", "--recon", "R", "--height", "64", "--width", "96", "--roi-root", "ROOT", "--motion-q", "0.5"],
                 ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--motion-q", "0.05"],
                 ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--motion-border", "65"],
                 ["boxes", "--frames", "F", "--out", "O"],
                 ["boxes", "--out", "O", "--threshold", "24"],
                 ["boxes", "--frames", "F", "--video", "v.y4m", "--out", "O", "--threshold", "24"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "255"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "24", "--learn", "4", "17"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "24", "--grow", "9"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "24", "--min-pixels", "0"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "24", "--max-boxes", "0"],
                 ["boxes", "--frames", "F", "--out", "O", "--threshold", "24", "--size", "64x64"],
                 ["boxes", "--video", "v.mp4", "--out", "O", "--threshold", "24"],
                 ["boxes", "--video", "v.yuv", "--out", "O", "--threshold", "24"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(argv)
        assert ex.value.code == 2 and "error:" in capsys.readouterr().err, argv
    assert not os.path.exists("O")
