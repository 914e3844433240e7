"""ROI-weighted quantisation without a GPU: the restatement the GPU tests compare with (tests/roiq_ref.py: the literal
procedure) checked against the header's closed-form "touches" rule, RoiQ and its JSON form, the roiq.json side file,
the entry points' refusals (a refused call launches nothing) and the command line's."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import roiq_ref as R
from tests.test_roi_host import _write_coords
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_literal_procedure_is_the_touches_rule(size):
    H, W = size
    f = R.factors()
    lists = R.box_lists(H, W)
    assert len(lists["1024"]) == len(lists["1024-large"]) == 1024
    for name, boxes in lists.items():
        assert (boxes[:, :4] >= 0).all() and (boxes[:, [0, 2]] <= W).all() and (boxes[:, [1, 3]] <= H).all(), name
        for grow in R.GROWS:
            a, b = R.q_map(boxes, H, W, grow, f), R.q_map_touches(boxes, H, W, grow, f)
            assert a.shape == R.grid(H, W) and _same(a, b), (name, grow)
            assert _same(a, R.q_map(boxes[::-1], H, W, grow, f)), (name, grow)  # independent of list order


def test_edges_at_15_16_17():
    f = R.factors(100, (60,))
    one = lambda x1, y1, x2, y2, grow=0, H=64, W=64: R.q_map(np.array([[x1, y1, x2, y2, 0]]), H, W, grow, f)
    lo, bg = f[1], f[0]
    assert (one(0, 0, 15, 15) == lo).sum() == 1 and (one(0, 0, 16, 16) == lo).sum() == 1 and (one(0, 0, 17, 17) == lo).sum() == 4
    assert one(15, 15, 16, 16)[0, 0] == lo and one(16, 16, 17, 17)[1, 1] == lo and (one(16, 16, 17, 17) == lo).sum() == 1
    assert (one(15, 15, 17, 17) == lo).sum() == 4
    assert (one(16, 16, 32, 32, grow=0) == lo).sum() == 1 and (one(16, 16, 32, 32, grow=1) == lo).sum() == 9
    assert (one(16, 16, 32, 32, grow=16) == lo).sum() == 9 and (one(20, 20, 21, 21, grow=255) == lo).all()
    # empty boxes paint nothing, grown or not; the padding keeps the background
    assert (one(5, 5, 5, 9, grow=255) == bg).all() and (one(9, 9, 3, 12, grow=16) == bg).all()
    m = one(0, 0, 65, 63, grow=255, H=65, W=63)  # (grid 8 x 4: rows 5.. and no column lie wholly in the padding)
    assert m.shape == (8, 4) and (m[:5] == lo).all() and (m[5:] == bg).all()
    m = one(0, 0, 17, 33, grow=255, H=17, W=33)
    assert m.shape == (4, 4) and (m[:2, :3] == lo).all() and (m[2:] == bg).all() and (m[:, 3] == bg).all()
    # the minimum over the boxes, not with the background: a class above the background wins where only it touches
    f2 = R.factors(100, (60, 140))
    m = R.q_map(np.array([[0, 0, 40, 16, 1], [16, 0, 32, 16, 0]]), 64, 64, 0, f2)
    assert m[0].tolist() == [f2[2], f2[1], f2[2], f2[0]]


def test_factors_are_the_hosts_quotients():
    q = X.RoiQ(100, (60, 140, 10, 1000))
    want = np.array([np.float32(k) / np.float32(100) for k in (100, 60, 140, 10, 1000)], dtype=np.float32)
    assert _same(q.factors(), want) and _same(R.factors(100, (60, 140, 10, 1000)), want)
    assert q.factors()[0] == 1.0 and q.factors()[3] == np.float32(0.1) and q.factors()[4] == 10.0
    assert X.RoiQ().is_neutral() and X.RoiQ(100, (100, 100)).is_neutral() and not q.is_neutral()
    assert X.grid_of(1080, 1920) == (68, 120) and X.grid_of(1, 1) == (4, 4) and X.grid_of(65, 63) == (8, 4)
    assert X.RoiQ.hundredths(0.6) == 60 and X.RoiQ.hundredths(1.4) == 140 and X.RoiQ.hundredths(0.299) == 30


# ------------------------------------------------------------------------------------------------------------ RoiQ
def test_roiq_validates_by_name():
    q = X.RoiQ(background=140, classes=[60, np.int32(80)], grow=3)
    assert (q.background, q.classes, q.grow) == (140, (60, 80), 3) and all(type(v) is int for v in q.classes)
    for kw, match in ((dict(background=9), "background"), (dict(background=1001), "background"), (dict(background=1.0), "background"),
                      (dict(background=True), "background"), (dict(classes=(100, 5)), r"classes\[1\]"),
                      (dict(classes=(0.6,)), r"classes\[0\]"), (dict(classes=(100,) * 5), "at most 4"), (dict(classes=7), "classes"),
                      (dict(grow=-1), "grow"), (dict(grow=256), "grow"), (dict(grow=1.5), "grow")):
        with pytest.raises(ValueError, match=match):
            X.RoiQ(**kw)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            X.RoiQ.hundredths(bad)


def test_roiq_json_round_trip():
    q = X.RoiQ(140, (60, 80), 3)
    info = q.to_json(("liplates", "faces"))
    assert info == {"cell": 16, "background": 140, "classes": {"liplates": 60, "faces": 80}, "grow": 3}
    info = json.loads(json.dumps(info))
    assert X.RoiQ.from_json(info) == q and X.RoiQ.from_json(info, ("liplates", "faces")) == q
    with pytest.raises(ValueError, match="class names"):
        X.RoiQ.from_json(info, ("faces", "liplates"))
    with pytest.raises(ValueError, match="class names"):
        X.RoiQ.from_json(info, ("liplates",))
    with pytest.raises(ValueError, match="class names"):
        q.to_json(("liplates",))
    for bad, match in ((dict(info, cell=8), "cell"), (dict(info, background=5), "background"), (dict(info, grow=300), "grow"),
                       (dict(info, classes={"liplates": 60, "faces": 2000}), r"classes\[1\]"),
                       (dict(info, classes=[60, 80]), "keys"), ({k: v for k, v in info.items() if k != "grow"}, "keys"),
                       (dict(info, more=1), "keys")):
        with pytest.raises(ValueError, match=match):
            X.RoiQ.from_json(bad)


# ------------------------------------------------------------------------------------------------------- side file
def test_side_file_writer_reader_and_stale_removal(tmp_path):
    from vcm_ts_amd import run_codec as RC

    roi = X.Roi(lambda t: X.FrameBoxes(), (X.RoiClass(0), X.RoiClass(0)), ("liplates", "faces"))
    q = X.RoiQ(140, (60, 80), 5)
    bins = str(tmp_path)
    assert RC.read_roiq(bins) is None and RC.read_roiq(bins, roi) is None
    RC.write_roiq(bins, q, roi.names)
    path = tmp_path / RC.ROIQ_JSON
    assert RC.ROIQ_JSON == "roiq.json"
    assert json.loads(path.read_text()) == {"cell": 16, "background": 140, "classes": {"liplates": 60, "faces": 80}, "grow": 5}
    assert RC.read_roiq(bins, roi) == q
    with pytest.raises(ValueError, match=r"roiq\.json.*boxes"):
        RC.read_roiq(bins)
    other = X.Roi(lambda t: X.FrameBoxes(), (X.RoiClass(0), X.RoiClass(0)), ("cars", "faces"))
    with pytest.raises(ValueError, match=r"roiq\.json.*class names"):
        RC.read_roiq(bins, other)
    path.write_text(json.dumps({"cell": 16, "background": 1, "classes": {"liplates": 60, "faces": 80}, "grow": 5}))
    with pytest.raises(ValueError, match=r"roiq\.json.*background"):
        RC.read_roiq(bins, roi)
    RC.write_roiq(bins, None)  # an encode without the feature into the same folder: the stale file goes
    assert not path.exists()
    RC.write_roiq(bins, None)
    assert os.listdir(bins) == []


def test_file_loops_refuse_by_name_before_any_gpu_work(tmp_path):
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S

    h, w = 64, 96
    bins = tmp_path / "bins"
    bins.mkdir()
    for t in range(4):  # (headers only: every refusal comes before a picture is decoded)
        S.encode_i(h, w, 0, b"", str(bins / f"im{t + 1:05d}.bin"))
    roi = X.Roi(lambda t: X.FrameBoxes([[1, 2, 30, 40, 0]]), (X.RoiClass(0), X.RoiClass(0)), ("liplates", "faces"))
    RC.write_roiq(str(bins), X.RoiQ(140, (60, 80)), roi.names)
    renamed = X.Roi(roi.boxes, roi.classes, ("plates", "faces"))
    beyond = X.Roi(lambda t: X.FrameBoxes([[1, 2, 300, 40, 0]]), roi.classes, roi.names)
    for kw, match in ((dict(), r"roiq\.json.*boxes"), (dict(roi=renamed), "class names"), (dict(roi=beyond), "coordinates out of range")):
        with pytest.raises(ValueError, match=match):
            RC.decode_folder(str(bins), str(tmp_path / "out"), h, w, gop=2, **kw)
        with pytest.raises(ValueError, match=match):
            RC.decode_video(str(bins), str(tmp_path / "out.y4m"), height=h, width=w, gop=2, **kw)
    # encode: the option without boxes, something that is no RoiQ, factors that do not fit the classes
    from PIL import Image

    (tmp_path / "png").mkdir()
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(tmp_path / "png" / "im00001.png")
    for kw, match in ((dict(roi_q=X.RoiQ(140, (60, 80))), "roi_q= needs roi="), (dict(roi=roi, roi_q=(140, 60, 80)), "RoiQ"),
                      (dict(roi=roi, roi_q=X.RoiQ(140, (60,))), "class factors")):
        with pytest.raises(ValueError, match=match):
            RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "never"), **kw)
    assert not (tmp_path / "never").exists()


# ------------------------------------------------------------------------------------------------- the C entry points
P = 0x100000  # an aligned dummy: a refused call returns before anything is launched or dereferenced


def _qmap_call(H=64, W=96, n=2, grow=3, n_classes=2, f=(1.0, 0.6, 1.4), **over):
    boxes = (lib.RoiBox * 1025)()
    for i in range(1025):
        boxes[i].x1, boxes[i].y1, boxes[i].x2, boxes[i].y2, boxes[i].cls = 1, 1, W, H, i % 2
    fac = (C.c_float * 5)(*f)
    a = dict(H=H, W=W, bh=C.addressof(boxes), bd=P, n=n, grow=grow, fp=C.addressof(fac), n_classes=n_classes, map=P)
    a.update(over)
    return [a[k] for k in ("H", "W", "bh", "bd", "n", "grow", "fp", "n_classes", "map")] + [None], (boxes, fac)


def test_qmap_entry_point_refuses_bad_arguments_without_a_gpu():
    L = lib.hip()
    bad = {"null factors": dict(fp=None), "null map": dict(map=None), "null boxes on the host": dict(bh=None),
           "null boxes on the device": dict(bd=None), "zero height": dict(H=0), "zero width": dict(W=0),
           "height beyond the limit": dict(H=32769), "negative grow": dict(grow=-1), "grow 256": dict(grow=256),
           "1025 boxes": dict(n=1025), "negative count": dict(n=-1), "five classes": dict(n_classes=5),
           "negative classes": dict(n_classes=-1), "class of a box unknown": dict(n_classes=1)}
    for what, over in bad.items():
        args, keep = _qmap_call(**over)
        assert L.dcvc_roi_qmap(*args) == -1, what
    for f in ((0.09, 1, 1), (1, 10.5, 1), (1, 1, float("nan")), (float("inf"), 1, 1), (1, -1.0, 1), (1, 1, 0.0)):
        args, keep = _qmap_call(f=f)
        assert L.dcvc_roi_qmap(*args) == -1, f
    for field, value in (("x1", -1), ("y1", -1), ("x2", 97), ("y2", 65), ("cls", 2), ("cls", -1)):
        args, keep = _qmap_call()
        setattr(keep[0][1], field, value)
        assert L.dcvc_roi_qmap(*args) == -1, (field, value)


def test_scale_channels_map_refuses_sizes_that_do_not_fit():
    L = lib.hip()
    ok = dict(src=P, src_cs=8, out=P, out_cs=8, q_basic=P, q_scale=P, mode=0, N=2, HW=24, C=8, q_map=P, H=4, W=6)
    order = "src src_cs out out_cs q_basic q_scale mode N HW C q_map H W".split()
    assert len(order) + 1 == len(lib._SIGS["dcvc_scale_channels_map"])
    for over in (dict(H=4, W=5), dict(H=0, W=6), dict(H=-4, W=-6), dict(H=24, W=0), dict(src=None), dict(q_scale=None), dict(N=0),
                 dict(HW=0, H=0, W=0), dict(C=0), dict(src_cs=7), dict(out_cs=7)):
        vals = dict(ok, **over)
        assert L.dcvc_scale_channels_map(*[vals[k] for k in order], None) == -1, over


def test_bindings_follow_the_headers():
    assert lib.DualPriorArgs._fields_[-1] == ("q_map", C.c_void_p)
    hdr = open(os.path.join(ROOT, "include", "dcvc_hip.h")).read()
    body = hdr[hdr.index("typedef struct {\n    const float *y;"):hdr.index("} dcvc_dual_prior_args;")]
    decls = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1].split(";")[:-1]
    members = [re.findall(r"\w+", part)[-1] for d in decls for part in d.split(",")]
    assert members[-1] == "q_map" and members == [n for n, _ in lib.DualPriorArgs._fields_]  # the last member, same order
    assert "dcvc_roi_qmap" in lib.ROI_SYMBOLS and "dcvc_scale_channels_map" in lib.HIP_SYMBOLS
    roi_hdr = open(os.path.join(ROOT, "include", "dcvc_hip_roi.h")).read()
    assert "#define DCVC_ROI_CELL 16" in roi_hdr and X.CELL == 16 and X.MAX_GROW == 255


# ----------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("argv", [
    ["encode", "--frames", "F", "--bins", "B", "--plate-q", "0.6"],
    ["encode", "--frames", "F", "--bins", "B", "--face-q", "0.6"],
    ["encode", "--frames", "F", "--bins", "B", "--background-q", "1.4"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-q-grow", "4"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--roi-q-grow", "4"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--plate-q", "0.05"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--face-q", "10.5"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--background-q", "nan"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--plate-q", "0.6", "--roi-q-grow", "256"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--plate-q", "0.6", "--roi-q-grow", "-1"],
    ["decode", "--bins", "Q", "--recon", "R", "--height", "64", "--width", "96"],
    ["decode", "--bins", "B", "--recon", "R", "--height", "64", "--width", "96", "--plate-q", "0.6"],
], ids=lambda a: " ".join(a[0:1] + a[-2:]))
def test_command_line_refuses_q_options_that_do_not_fit(argv, tmp_path, monkeypatch, capsys):
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    _write_coords(tmp_path / "ROOT" / "faces_coords", 1, [[1, 1, 2, 2]])
    (tmp_path / "Q").mkdir()
    RC.write_roiq("Q", X.RoiQ(140, (60, 80)), ("liplates", "faces"))  # bins that were coded with maps: decode needs --roi-root
    with pytest.raises(SystemExit) as ex:
        RC.main(argv)
    assert ex.value.code == 2 and "error:" in capsys.readouterr().err


def test_command_line_builds_the_options(tmp_path, monkeypatch):
    """--plate-q 0.6 alone switches the feature on with the others at 1.00; decode --roi-root without --residuals is
    taken when a roiq.json lies beside the .bin files."""
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    _write_coords(tmp_path / "ROOT" / "liplates_coords", 1, [[1, 1, 2, 2]])
    seen = {}

    def fake_encode(*args, **kw):
        seen.update(kw)
        return [8], (64, 64)

    def fake_decode(*args, **kw):
        seen.update(kw)
        return 1

    monkeypatch.setattr(RC, "encode_folder", fake_encode)
    monkeypatch.setattr(RC, "decode_folder", fake_decode)
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--plate-q", "0.6"])
    assert seen["roi_q"] == X.RoiQ(100, (60, 100), 0) and seen["roi"].names == ("liplates", "faces")
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--face-q", "0.799", "--background-q", "1.4", "--roi-q-grow", "8"])
    assert seen["roi_q"] == X.RoiQ(140, (100, 80), 8)
    RC.main(["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT"])
    assert seen["roi_q"] is None
    (tmp_path / "Q").mkdir()
    RC.write_roiq("Q", X.RoiQ(140, (60, 80)), ("liplates", "faces"))
    seen.clear()
    RC.main(["decode", "--bins", "Q", "--recon", "R", "--height", "64", "--width", "96", "--roi-root", "ROOT"])
    assert seen["roi"].names == ("liplates", "faces") and seen["residuals"] is None
