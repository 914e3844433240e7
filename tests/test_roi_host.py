"""The ROI enhancement layer without a GPU: the restatement the GPU tests compare with (tests/roi_ref.py) checked against
the reference's literal procedure, the host side of vcm_ts_amd/roi.py, and the entry points' refusals (a refused call
launches nothing and dereferences no device pointer)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from tests import roi_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("size", R.SIZES + [(40, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_closed_form_feather_mask_is_the_literal_procedure(size):
    H, W = size
    for name, boxes in R.box_lists(H, W).items():
        for borders in (R.BORDERS, (0, 1, 2, 25)):
            a, b = R.feather_mask(boxes, borders, H, W), R.feather_mask_literal(boxes, borders, H, W)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, borders)


def test_order_of_overlapping_boxes_changes_the_mask():
    lists = R.box_lists(64, 64)
    a = R.feather_mask(lists["overlap"], R.BORDERS, 64, 64)
    b = R.feather_mask(lists["overlap-reversed"], R.BORDERS, 64, 64)
    assert not np.array_equal(a, b)


def test_code_returns_the_byte_of_an_eight_bit_picture():
    assert np.array_equal(R.code(R.T), np.arange(256))
    assert R.code(np.float32(-3.0)) == 0 and R.code(np.float32(7.0)) == 255


def test_feather_table():
    for border in (0, 1, 2, 3, 10, 25, 64):
        want = np.array([np.float32(1.0 - v) for v in np.linspace(0.9, 0.0, border)], dtype=np.float32)
        got = X.feather_table(border)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(X.feather_table(0)) == 0
    assert X.feather_table(1).tolist() == [np.float32(0.1)]       # the reference's quirk: 0.1 over the whole box
    assert X.feather_table(10)[-1] == 1.0 and X.feather_table(10)[0] == np.float32(0.1)
    assert np.array_equal(R.feather_mask(np.array([[1, 1, 6, 5, 0]]), (1,), 8, 8)[1:5, 1:6], np.full((4, 5), np.float32(0.1)))
    assert np.array_equal(R.feather_mask(np.array([[1, 1, 6, 5, 0]]), (0,), 8, 8)[1:5, 1:6], np.ones((4, 5), np.float32))
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            X.feather_table(bad)
    rec = X.RoiClass(10).record()
    assert (rec.border, rec.shrink) == (10, 10) and list(rec.feather)[:10] == X.feather_table(10).tolist()
    assert X.RoiClass(10, 0).shrink == 0
    with pytest.raises(ValueError):
        X.RoiClass(65)


def test_fuse_inputs_tell_a_fused_multiply_add_apart():
    """The bit comparison of the GPU fuse tests is sensitive to contraction only where m * e + b rounded once truncates
    to another code than multiply-then-add: the shared inputs must hold such samples."""
    table = R.feather_table(10)
    m, e, b = np.meshgrid(table, np.arange(256, dtype=np.float32) - 128, np.arange(256, dtype=np.float32), indexing="ij")
    assert int(R.fma_sensitive(m, e, b).sum()) == 1480
    total = 0
    for seed, (H, W) in enumerate(R.SIZES):
        base = R.pictures(seed, H, W)[1]
        res = R.residual_picture(seed, H, W)
        for name, boxes in R.box_lists(H, W).items():
            mask = np.broadcast_to(R.feather_mask(boxes, R.BORDERS, H, W)[None], res.shape)
            total += int(R.fma_sensitive(mask, res.astype(np.float32) - 128, R.code(base).astype(np.float32)).sum())
    print("samples where a fused multiply-add would give another code:", total)
    assert total >= 10


# ------------------------------------------------------------------------------------------------------- box sources
def test_frame_boxes_validate_by_name():
    fb = X.FrameBoxes([[0, 0, 10, 10, 0], [5, 5, 2, 2, 1]])
    assert len(fb) == 2 and fb.array.dtype == np.int32 and fb.validate(10, 10, 2) is fb
    assert len(X.FrameBoxes()) == 0 and len(X.FrameBoxes(np.zeros((0, 5))).validate(1, 1, 0)) == 0
    with pytest.raises(ValueError, match="too many boxes"):
        X.FrameBoxes(np.zeros((1025, 5), np.int32))
    with pytest.raises(ValueError, match="coordinates out of range"):
        fb.validate(9, 10, 2)
    with pytest.raises(ValueError, match="coordinates out of range"):
        X.FrameBoxes([[-1, 0, 3, 3, 0]]).validate(10, 10, 1)
    with pytest.raises(ValueError, match="unknown class"):
        fb.validate(10, 10, 1)
    with pytest.raises(ValueError, match=r"\(n, 5\)"):
        X.FrameBoxes([[0, 0, 1, 1]])


def _write_coords(folder, index, rows):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "%05d" % index), "wb") as f:
        pickle.dump(np.array(rows, dtype=np.uint16), f)


class _Other:
    pass


def test_pickle_boxes(tmp_path):
    root = tmp_path / "encoded"
    _write_coords(root / "liplates_coords", 1, [[1, 2, 30, 40], [5, 6, 7, 8]])
    _write_coords(root / "liplates_coords", 2, [])
    _write_coords(root / "faces_coords", 1, [[10, 20, 50, 60]])
    _write_coords(root / "faces_coords", 2, [[0, 0, 3, 3]])
    src = X.PickleBoxes(str(root), (X.RoiClass(10), X.RoiClass(3)))
    assert src(0).array.tolist() == [[1, 2, 30, 40, 0], [5, 6, 7, 8, 0], [10, 20, 50, 60, 1]]  # plates before faces
    assert src(1).array.tolist() == [[0, 0, 3, 3, 1]]
    with pytest.raises(FileNotFoundError, match="00003"):
        src(2)
    roi = X.Roi(src, src.classes)
    assert roi.names == ("liplates", "faces") and roi.to_json()["classes"][1] == {"name": "faces", "border": 3, "shrink": 3}
    with pytest.raises(ValueError, match="coordinates out of range"):
        roi.frame(0, 50, 50)
    # one folder only
    only = tmp_path / "only"
    _write_coords(only / "faces_coords", 1, [[1, 1, 2, 2]])
    assert X.PickleBoxes(str(only))(0).array.tolist() == [[1, 1, 2, 2, 1]]
    with pytest.raises(FileNotFoundError):
        X.PickleBoxes(str(tmp_path / "nothing"))
    # anything else inside a file
    bad = tmp_path / "bad"
    os.makedirs(bad / "faces_coords")
    with open(bad / "faces_coords" / "00001", "wb") as f:
        pickle.dump(_Other(), f)
    with open(bad / "faces_coords" / "00002", "wb") as f:
        pickle.dump({"os": os.getcwd}, f)
    with open(bad / "faces_coords" / "00003", "wb") as f:
        pickle.dump(np.zeros((2, 4), np.int64), f)
    with open(bad / "faces_coords" / "00004", "wb") as f:
        f.write(b"not a pickle")
    _write_coords(bad / "faces_coords", 5, np.zeros((1025, 4)))
    for k, match in ((0, "_Other"), (1, "getcwd"), (2, "uint16"), (3, "not a pickled"), (4, "too many boxes")):
        with pytest.raises(ValueError, match=match):
            X.PickleBoxes(str(bad))(k)


def test_raw_planar_round_trip_with_out_of_order_writes(tmp_path):
    H, W, n = 5, 7, 4
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (3, H, W), dtype=np.uint8) for _ in range(n)]
    path = str(tmp_path / "r.gbrp")
    with X.RawPlanarWriter(path, W, H) as w:
        for k in (2, 0, 3, 1):
            w.write(k, frames[k])
        assert w.n_frames == n and w.frame_bytes == 3 * H * W
        with pytest.raises(ValueError):
            w.write(0, frames[0][:2])
    assert open(path, "rb").read() == b"".join(f.tobytes() for f in frames)  # display order, no header
    with X.RawPlanarReader(path, W, H) as r:
        assert r.n_frames == n
        buf = np.empty((3, H, W), np.uint8)
        for k in (3, 1, 0, 2):
            r.read_into(k, buf)
            assert np.array_equal(buf, frames[k])
        with pytest.raises(IndexError):
            r.read_into(n, buf)
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError, match="truncated"):
        X.RawPlanarReader(path, W, H)


def test_region_psnr_in_both_divisor_modes():
    H, W = 12, 20
    for sums in ([5000, 70000, 40], [0, 70000, 40], [5000, 0, 240], [0, 123, 0]):
        for mode in ("samples", "reference"):
            got, want = X.region_psnr(sums, H, W, mode), R.psnr(sums, H, W, mode)
            for g, w in zip(got, want):
                assert (np.isnan(g) and np.isnan(w)) or g == pytest.approx(w, rel=1e-14), (sums, mode)
    s = [5000, 70000, 40]
    samples, ref = X.region_psnr(s, H, W), X.region_psnr(s, H, W, "reference")
    assert samples[0] == ref[0]
    assert samples[2] - ref[2] == pytest.approx(10 * np.log10(3), rel=1e-12)  # the reference divides three channels' sum by pixels
    assert samples[2] == pytest.approx(10 * np.log10(255.0 ** 2 / (5000 / 120)), rel=1e-14)
    assert ref[1] == pytest.approx(10 * np.log10(255.0 ** 2 / (70000 / (720 - 40))), rel=1e-14)
    with pytest.raises(ValueError):
        X.region_psnr(s, H, W, "pixels")


# ------------------------------------------------------------------------------------------------- the C entry points
def test_library_exports_what_the_roi_header_declares():
    mk = open(os.path.join(ROOT, "vcm_ts_amd", "csrc", "Makefile")).read()
    assert "roi.hip" in [ln for ln in mk.splitlines() if ln.startswith("HIPSRC")][0].split()
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "vcm_ts_amd", "csrc", "roi.hip")).read()


P = 0x100000  # an aligned dummy: a refused call returns before anything is launched or dereferenced


def _calls(H=16, W=24, n=2, n_classes=2, **over):
    """Argument lists of the three entry points that pass every check, with named overrides."""
    boxes = (lib.RoiBox * 1025)()
    for i in range(1025):
        boxes[i].x1, boxes[i].y1, boxes[i].x2, boxes[i].y2, boxes[i].cls = 1, 1, W, H, i % 2
    classes = (lib.RoiClassRec * 4)()
    for c in range(4):
        classes[c].border = classes[c].shrink = 3
    a = dict(src=P, rs=W, ps=H * W, rec=P, H=H, W=W, bh=C.addressof(boxes), bd=P, n=n, u8=P, cs=H * W, urs=W, px=1,
             order=(0, 1, 2), classes=C.addressof(classes), n_classes=n_classes, out=P, sums=P, keep=(boxes, classes))
    a.update(over)
    residual = [a["src"], a["rs"], a["ps"], a["rec"], a["rs"], a["ps"], a["H"], a["W"], a["bh"], a["bd"], a["n"], a["u8"], a["cs"],
                a["urs"], a["px"], *a["order"], None]
    fuse = [a["src"], a["rs"], a["ps"], a["u8"], a["cs"], a["urs"], a["px"], *a["order"], a["H"], a["W"], a["bh"], a["bd"], a["n"],
            a["classes"], a["n_classes"], a["out"], a["rs"], a["ps"], None]
    sse = [a["src"], a["rs"], a["ps"], a["rec"], a["rs"], a["ps"], a["H"], a["W"], a["bh"], a["bd"], a["n"], a["classes"],
           a["n_classes"], a["sums"], None]
    return {"dcvc_roi_residual": residual, "dcvc_roi_fuse": fuse, "dcvc_roi_sse": sse}, a


BAD = {
    "null picture": dict(src=None), "null boxes on the host": dict(bh=None), "null boxes on the device": dict(bd=None),
    "zero height": dict(H=0), "width beyond the limit": dict(W=32769, rs=32769, urs=32769), "row stride below the width": dict(rs=23),
    "plane stride too small": dict(ps=16 * 24 - 1), "1025 boxes": dict(n=1025), "negative count": dict(n=-1),
}
BAD_U8 = {"null 8-bit picture": dict(u8=None), "pixel stride 2": dict(px=2), "pixel stride 3 with planes": dict(px=3),
          "interleaved row too short": dict(px=3, cs=1, urs=71), "planar row too short": dict(urs=23),
          "order repeats a channel": dict(order=(0, 1, 1)), "order out of range": dict(order=(0, 1, 3))}
BAD_CLASSES = {"class of a box unknown": dict(n_classes=1), "five classes": dict(n_classes=5), "null classes": dict(classes=None)}


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = lib.hip()
    for what, over in {**BAD, **BAD_U8, **BAD_CLASSES}.items():
        calls, _ = _calls(**over)
        for name, args in calls.items():
            if what in BAD_U8 and name == "dcvc_roi_sse":
                continue
            if what in BAD_CLASSES and name == "dcvc_roi_residual":
                continue
            assert getattr(L, name)(*args) == -1, (what, name)
    # class records out of range (fuse and sse read them)
    for field, value in (("border", 65), ("border", -1), ("shrink", 65), ("shrink", -1)):
        calls, a = _calls()
        setattr(a["keep"][1][1], field, value)
        assert L.dcvc_roi_fuse(*calls["dcvc_roi_fuse"]) == -1 and L.dcvc_roi_sse(*calls["dcvc_roi_sse"]) == -1, (field, value)
    # a class the residual kernel could not index, a negative coordinate, unaligned sums, a null output
    calls, a = _calls()
    a["keep"][0][1].cls = 4
    assert L.dcvc_roi_residual(*calls["dcvc_roi_residual"]) == -1
    for field, value in (("x1", -1), ("y1", -1), ("x2", 25), ("y2", 17)):
        calls, a = _calls()
        setattr(a["keep"][0][0], field, value)
        assert all(getattr(L, name)(*args) == -1 for name, args in calls.items()), (field, value)
    assert L.dcvc_roi_sse(*_calls(sums=P + 4)[0]["dcvc_roi_sse"]) == -1
    assert L.dcvc_roi_sse(*_calls(sums=None)[0]["dcvc_roi_sse"]) == -1
    assert L.dcvc_roi_fuse(*_calls(out=None)[0]["dcvc_roi_fuse"]) == -1


# ------------------------------------------------------------------------------------------------------- file loops
def test_decode_loops_refuse_by_name_before_any_gpu_work(tmp_path):
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S

    h, w = 64, 96
    bins = tmp_path / "bins"
    bins.mkdir()
    for t in range(6):  # (headers only: every refusal comes before a picture is decoded)
        S.encode_i(h, w, 0, b"", str(bins / f"im{t + 1:05d}.bin"))
    roi = X.Roi(lambda t: X.FrameBoxes([[1, 2, 30, 40, 0]]), (X.RoiClass(3), X.RoiClass(10)))
    short = tmp_path / "short.gbrp"
    short.write_bytes(bytes(3 * h * w * 2))
    (tmp_path / "pngs").mkdir()
    beyond = X.Roi(lambda t: X.FrameBoxes([[1, 2, 300, 40, 0]]), (X.RoiClass(3),))
    for kw, match in ((dict(roi=roi), "residuals"), (dict(residuals=str(short)), "roi"),
                      (dict(roi=roi, residuals=str(short)), "2 residual frames for 6 pictures"),
                      (dict(roi=roi, residuals=str(tmp_path / "pngs")), "no residual picture im00001.png"),
                      (dict(roi=beyond, residuals=str(short)), "coordinates out of range")):
        with pytest.raises(ValueError, match=match):
            RC.decode_folder(str(bins), str(tmp_path / "out"), h, w, gop=3, **kw)
        with pytest.raises(ValueError, match=match):
            RC.decode_video(str(bins), str(tmp_path / "out.y4m"), height=h, width=w, gop=3, **kw)


@pytest.mark.parametrize("argv", [
    ["decode", "--bins", "B", "--recon", "R", "--height", "64", "--width", "96", "--roi-root", "X"],
    ["encode", "--frames", "F", "--bins", "B", "--residuals", "r.gbrp"],
    ["encode", "--frames", "F", "--bins", "B", "--plate-border", "3"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "nothing-here"],
    ["encode", "--frames", "F", "--bins", "B", "--roi-root", "ROOT", "--face-border", "65"],
], ids=lambda a: " ".join(a[-2:]))
def test_command_line_refuses_roi_options_that_do_not_fit(argv, tmp_path, monkeypatch, capsys):
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    _write_coords(tmp_path / "ROOT" / "faces_coords", 1, [[1, 1, 2, 2]])
    with pytest.raises(SystemExit) as ex:
        RC.main(argv)
    assert ex.value.code == 2 and "error:" in capsys.readouterr().err
