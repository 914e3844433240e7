"""The deinterlacer without a GPU: tests/deint_ref.py (the numpy restatement of include/dcvc_hip_deint.h the kernel is
pinned to) against an independent per-sample statement of the header, what the rule does to a static and to a moving clip,
the host side of vcm_ts_amd/deint.py, the readers' opt-in and the command line's refusals.

The moving clip (deint_ref.MOVING: 96 x 128, 8 field times, a 32 x 40 textured box over a static textured ground), squared
error of the luma inside the object's box against the progressive truth, summed over the 8 output pictures of "field" mode,
as a ratio to weaving the frame's two fields -- measured on the committed clip (DESIGN.md has the same figures):

    step (dy, dx) a field      (1, 3)     (3, 8)     (0.5, 0.75)
    rule / weave               0.096      0.140      0.148

Each leaves more than the margin of 1.5 that "below half of weave's" asks for (the largest, 0.148 * 1.5 = 0.22 < 0.5), so
that is what is asserted for all three.  Nothing is asserted against line averaging.
"""
import json
import os

import numpy as np
import pytest

from tests import deint_ref as D
from tests import yuv_ref as YR
from vcm_ts_amd import deint as DI
from vcm_ts_amd import yuv as Y


# ------------------------------------------------------------------------------- the header, a sample at a time
def _row(q, PH):
    """The nearest row inside 0 .. PH - 1 with q's parity, by search."""
    if 0 <= q < PH:
        return q
    return min((k for k in range(PH) if (k - q) % 2 == 0), key=lambda k: abs(k - q))


def _by_the_header(prev, cur, nxt, parity, second, depth):
    """One plane, as the header reads: Python integers, one sample at a time."""
    PH, PW = cur.shape
    peak = (1 << depth) - 1
    out, moved = [[0] * PW for _ in range(PH)], [[False] * PW for _ in range(PH)]
    A, B = (prev, cur) if second == 0 else (cur, nxt)
    for r in range(PH):
        for x in range(PW):
            if r % 2 == parity:
                out[r][x] = int(cur[r][x])
                continue
            c, e = int(cur[_row(r - 1, PH)][x]), int(cur[_row(r + 1, PH)][x])
            c3, e3 = int(cur[_row(r - 3, PH)][x]), int(cur[_row(r + 3, PH)][x])
            a, b = int(A[r][x]), int(B[r][x])
            d = (a + b) // 2
            td0 = abs(a - b)
            td1 = (abs(int(prev[_row(r - 1, PH)][x]) - c) + abs(int(prev[_row(r + 1, PH)][x]) - e)) // 2
            td2 = (abs(int(nxt[_row(r - 1, PH)][x]) - c) + abs(int(nxt[_row(r + 1, PH)][x]) - e)) // 2
            diff = max(td0 // 2, td1, td2)
            pred = min(max((9 * (c + e) - (c3 + e3) + 8) // 16, 0), peak)  # (// floors, as an arithmetic shift does)
            out[r][x] = min(max(pred, d - diff), d + diff)
            moved[r][x] = diff > 0
    return np.array(out), np.array(moved)


@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", [(4, 2), (8, 6), (20, 14)])
def test_the_restatement_is_the_header(H, W, depth, order):
    rng = np.random.default_rng(1000 * H + 10 * depth + (order == "bff"))
    frames = [D.random_frame(rng, H, W, depth) for _ in range(3)]
    for g in range(6):  # "field" mode: both fields of a first, a middle and a last frame
        (a, n, b), second = D.needs(g, 3, "field")
        assert (a, n, b) == (max(n - 1, 0), g // 2, min(n + 1, 2)) and second == g % 2
        parity = D.parity_of(order, second)
        assert parity == (second if order == "tff" else 1 - second)
        got, moved = D.picture(frames, g, "field", order, depth)
        luma_moved = None
        for k in range(3):
            want, mask = _by_the_header(frames[a][k], frames[n][k], frames[b][k], parity, second, depth)
            assert got[k].dtype == frames[n][k].dtype and np.array_equal(got[k], want), (g, k)
            luma_moved = mask if k == 0 else luma_moved
        assert moved.tolist() == [int(luma_moved[r:r + 8].sum()) for r in range(0, H, 8)], g
        if g % 2 == 0:  # "frame" mode keeps the earlier field
            again, moved1 = D.picture(frames, g // 2, "frame", order, depth)
            assert all(np.array_equal(x, y) for x, y in zip(again, got)) and np.array_equal(moved1, moved)


def test_the_stripes_drive_the_predictor_outside_the_range():
    for depth in (8, 10):
        cur = D.striped_frame(16, 8, depth)[0].astype(np.int64)
        r = np.arange(3, 13, 2)
        raw = (9 * (cur[r - 1] + cur[r + 1]) - (cur[r - 3] + cur[r + 3]) + 8) >> 4
        assert raw.max() > (1 << depth) - 1 and raw.min() < 0


# ------------------------------------------------------------------------------------------------------- what it does
@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("depth", [8, 10])
def test_a_static_clip_comes_back_bit_for_bit(depth, mode, order):
    pics = D.static_clip(24, 32, 8, depth)
    frames = D.interlace(pics, order)
    assert len(frames) == 4 and D.pictures_of(4, mode) == (4 if mode == "frame" else 8)
    for g in range(D.pictures_of(4, mode)):
        got, moved = D.picture(frames, g, mode, order, depth)
        assert all(np.array_equal(x, y) for x, y in zip(got, pics[0])), g
        assert not moved.any(), g


def _box_errors(step, order="tff"):
    """(the rule's, weave's) squared luma error inside the object's box against the truth, over the 8 pictures of "field"
    mode; and the checks of the ground on the way."""
    pics, boxes = D.moving_clip(step)
    frames = D.interlace(pics, order)
    H, W = D.MOVING["size"]
    rows = np.zeros(H, dtype=bool)   # rows and columns the object ever touches
    cols = np.zeros(W, dtype=bool)
    for y1, x1, y2, x2 in boxes:
        rows[y1:y2], cols[x1:x2] = True, True
    near = np.convolve(rows, np.ones(9), "same") > 0  # (the rule reaches 3 rows; 4 are allowed for)
    assert (~near).sum() >= 16 and (~cols).sum() >= 16
    ours = weave = 0
    for f in range(len(pics)):
        got, moved = D.picture(frames, f, "field", order, 8)
        truth = pics[f]
        # the ground is exact: every column the object never touches (the rule is vertical only), every row far from it
        for k, sub in enumerate((1, 2, 2)):
            far_c, far_r = ~cols[::sub] & ~cols[sub - 1::sub], ~near[::sub] & ~near[sub - 1::sub]
            assert np.array_equal(got[k][:, far_c], truth[k][:, far_c]), (f, k)
            assert np.array_equal(got[k][far_r], truth[k][far_r]), (f, k)
        for b in range(H // 8):
            if not near[8 * b:8 * b + 8].any():
                assert moved[b] == 0, (f, b)
        assert moved.sum() > 0, f
        y1, x1, y2, x2 = boxes[f]
        t = truth[0][y1:y2, x1:x2].astype(np.int64)
        ours += int(((got[0][y1:y2, x1:x2].astype(np.int64) - t) ** 2).sum())
        weave += int(((frames[f // 2][0][y1:y2, x1:x2].astype(np.int64) - t) ** 2).sum())
    return ours, weave


@pytest.mark.parametrize("step,margin", [((1, 3), 2), ((3, 8), 2), ((0.5, 0.75), 2)])
def test_a_moving_object_is_closer_to_the_truth_than_weaving_and_the_ground_stays_exact(step, margin):
    ours, weave = _box_errors(step)
    print(f"step {step}: rule {ours}, weave {weave}, ratio {ours / weave:.3f}")
    assert weave > 0 and margin * ours < weave, (ours, weave)


# --------------------------------------------------------------------------------------------------------- host side
def test_deinterlace_setting_numbers_pictures_as_the_restatement_does():
    for mode in D.MODES:
        for order in D.ORDERS:
            di = DI.Deinterlace(mode, order)
            assert di.to_json() == {"mode": mode, "order": order}
            for n in (1, 2, 5):
                assert di.pictures_of(n) == D.pictures_of(n, mode)
                for g in range(di.pictures_of(n)):
                    assert di.needs(g, n) == D.needs(g, n, mode), (mode, n, g)
                    assert di.parity(di.needs(g, n)[1]) == D.parity_of(order, D.needs(g, n, mode)[1])
                with pytest.raises(IndexError):
                    di.needs(di.pictures_of(n), n)
    assert DI.Deinterlace("frame", "tff").needs(0, 3) == ((0, 0, 1), 0)    # frame 0: its own past
    assert DI.Deinterlace("frame", "tff").needs(2, 3) == ((1, 2, 2), 0)    # the last frame: its own future
    assert DI.Deinterlace("field", "bff").needs(5, 3) == ((1, 2, 2), 1)
    assert DI.Deinterlace("field", "bff").needs(1, 1) == ((0, 0, 0), 1)
    assert DI.BAND == D.BAND
    for bad in (("weave", "tff"), ("frame", "top"), (None, "tff"), ("field", None)):
        with pytest.raises(ValueError):
            DI.Deinterlace(*bad)
    with pytest.raises(ValueError, match="multiple of 4"):
        DI.check_height(6)
    with pytest.raises(ValueError, match="GPU"):
        import torch

        t = torch.zeros(4 * 4 * 3 // 2, dtype=torch.uint8)
        DI.Deinterlace("frame", "tff").step(t, t, t, 4, 4, 8, 0)


def _y4m(path, n, h, w, **kw):
    YR.write_y4m(path, [YR.random_planes(5 + t, h, w, 8) for t in range(n)], w, h, **kw)


def test_the_readers_take_interlaced_files_only_when_asked(tmp_path):
    path = str(tmp_path / "a.y4m")
    for mark, order in (("t", "tff"), ("b", "bff")):
        _y4m(path, 3, 8, 6, interlace=mark)
        for opened in (lambda: Y.Y4MReader(path), lambda: Y.open_video(path)):
            with pytest.raises(ValueError, match="interlaced"):
                opened()
        with Y.Y4MReader(path, interlaced=True) as r:
            assert r.field_order == order and r.interlace == mark and r.n_frames == 3
        with Y.open_video(path, interlaced=True) as r:
            assert r.field_order == order
        with Y.open_video(path, interlaced=True, field_order="tff") as r:  # the option overrides the header
            assert r.field_order == "tff"
    _y4m(path, 3, 8, 6, interlace="m")
    with pytest.raises(ValueError, match="Im"):
        Y.Y4MReader(path, interlaced=True)
    with Y.Y4MReader(path, interlaced=True, field_order="bff") as r:
        assert r.field_order == "bff"
    _y4m(path, 3, 8, 6)  # a header that says progressive: accepted, and names no order
    with Y.Y4MReader(path, interlaced=True) as r:
        assert r.field_order is None
    with Y.Y4MReader(path) as r:
        assert r.field_order is None
    with pytest.raises(ValueError, match="field_order"):
        Y.Y4MReader(path, field_order="tff")
    with pytest.raises(ValueError, match="field_order"):
        Y.Y4MReader(path, interlaced=True, field_order="top")
    _y4m(path, 3, 8, 6, interlace="t", chroma="422")  # other chroma formats stay refused
    with pytest.raises(ValueError, match="C422"):
        Y.Y4MReader(path, interlaced=True)
    raw = str(tmp_path / "a.yuv")
    open(raw, "wb").write(bytes(3 * 8 * 6 * 3 // 2))
    with Y.open_video(raw, (6, 8)) as r:
        assert r.field_order is None
    with Y.open_video(raw, (6, 8), interlaced=True, field_order="bff") as r:
        assert r.field_order == "bff" and r.n_frames == 3


def test_sequence_json_records_the_setting_only_when_there_is_one(tmp_path):
    from vcm_ts_amd import run_codec as RC

    RC.write_sequence_info(str(tmp_path), 8, 8, 6, 8, (50, 1), Y.ColorSpec(), "y4m", chroma="420", interlace="p",
                           deinterlace=DI.Deinterlace("field", "bff"))
    info = RC.read_sequence_info(str(tmp_path))
    assert info["deinterlace"] == {"mode": "field", "order": "bff"} and info["interlace"] == "p" and info["fps"] == (50, 1)
    RC.write_sequence_info(str(tmp_path), 8, 8, 6, 8, (50, 1), Y.ColorSpec(), "y4m", chroma="420", interlace="p")
    assert "deinterlace" not in json.load(open(os.path.join(str(tmp_path), RC.SEQUENCE_JSON)))


def _cases(tmp_path):
    six, mixed, prog, ok = (str(tmp_path / n) for n in ("six.y4m", "mixed.y4m", "prog.y4m", "ok.y4m"))
    _y4m(six, 2, 6, 8, interlace="t")
    _y4m(mixed, 2, 8, 8, interlace="m")
    _y4m(prog, 2, 8, 8)
    _y4m(ok, 2, 8, 8, interlace="t")
    raw = str(tmp_path / "raw.yuv")
    open(raw, "wb").write(bytes(2 * 8 * 8 * 3 // 2))
    os.makedirs(str(tmp_path / "pngs"))
    return {
        "height 6": (["--video", six, "--deinterlace", "frame"], "multiple of 4"),
        "Im without an order": (["--video", mixed, "--deinterlace", "field"], "Im"),
        "Ip without an order": (["--video", prog, "--deinterlace", "frame"], "--field-order"),
        "yuv without an order": (["--video", raw, "--size", "8x8", "--deinterlace", "frame"], "--field-order"),
        "PNG source": (["--frames", str(tmp_path / "pngs"), "--deinterlace", "frame"], "PNG folder"),
        "order without the option": (["--video", ok, "--field-order", "tff"], "belongs to --deinterlace"),
    }


@pytest.mark.parametrize("cmd", ["encode", "boxes"])
@pytest.mark.parametrize("case", ["height 6", "Im without an order", "Ip without an order", "yuv without an order", "PNG source",
                                  "order without the option"])
def test_command_line_refusals_by_name_before_any_gpu_work(tmp_path, capsys, cmd, case):
    from vcm_ts_amd import run_codec as RC

    argv, word = _cases(tmp_path)[case]
    tail = ["--bins", str(tmp_path / "bins")] if cmd == "encode" else ["--out", str(tmp_path / "boxes"), "--threshold", "12"]
    with pytest.raises(SystemExit) as ex:
        RC.main([cmd] + argv + tail + ["--device", "cuda:0"])
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and word in err, err
    assert not os.path.exists(str(tmp_path / "bins")) and not os.path.exists(str(tmp_path / "boxes"))
