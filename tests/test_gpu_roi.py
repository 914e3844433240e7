"""The ROI enhancement layer on the device (vcm_ts_amd/roi.py, csrc/roi.hip) and the file loops built on it.

Every comparison is array_equal against tests/roi_ref.py, the numpy restatement of include/dcvc_hip_roi.h: the
arithmetic is integer apart from fuse's one multiply and one add, which the header pins, so nothing needs a tolerance
(tests/test_roi_host.py checks that the inputs here tell a fused multiply-add apart).

The end-to-end tests run at 64x96, 6 pictures, GOP 3, two GOP streams.  The report test alone runs at 192x320: a report
carries MS-SSIM, which takes no picture side below 161 (vcm_ts_amd/metrics.py), with or without a ROI.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import roi_ref as R
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from vcm_ts_amd import roi as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CLASSES = tuple(X.RoiClass(b) for b in R.BORDERS)
CASES = [(seed, H, W, False) for seed, (H, W) in enumerate(R.SIZES)] + [(9, 40, 130, True)]
IDS = [f"{H}x{W}" + ("-crop" if crop else "") for _, H, W, crop in CASES]
SLOTS = {"rgb": [0, 1, 2], "gbr": [1, 2, 0]}


def _dev_u8(a, layout, crop):
    """an 8-bit picture (3, H, W) in slot order, as the layout's device tensor"""
    H, W = a.shape[1:]
    if layout == "hwc":
        a = a.transpose(1, 2, 0)
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if not crop:
        return t
    big = torch.full((3, 64, 192) if layout == "planar" else (64, 192, 3), 99, dtype=torch.uint8, device=DEV)
    view = big[:, 1:1 + H, 1:1 + W] if layout == "planar" else big[1:1 + H, 1:1 + W]
    view.copy_(t)
    return view


def _planes(t, layout):
    a = t.cpu().numpy()
    return a if layout == "planar" else a.transpose(2, 0, 1)


@pytest.fixture(scope="module")
def refs():
    """per case: pictures, residual picture, box lists and the restatement's answers, computed once"""
    out = {}
    for seed, H, W, crop in CASES:
        src, rec = R.pictures(seed, H, W)
        res = R.residual_picture(seed, H, W)
        lists = R.box_lists(H, W)
        out[(H, W)] = dict(src=src, rec=rec, res=res, lists=lists,
                           residual={n: R.residual(src, rec, b) for n, b in lists.items()},
                           fuse={n: R.fuse(rec, res, b, R.BORDERS) for n, b in lists.items()},
                           sse={(n, s): R.sse(src, rec, b, sh) for n, b in lists.items() for s, sh in R.SHRINKS.items()})
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_residual_in_both_layouts_and_orders(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    src, rec = U.picture(ref["src"], crop, DEV), U.picture(ref["rec"], crop, DEV)
    for name, boxes in ref["lists"].items():
        for layout in X.LAYOUTS:
            for order, slots in SLOTS.items():
                got = X.residual_layer(src, rec, X.FrameBoxes(boxes), layout=layout, order=order)
                assert got.dtype == torch.uint8 and tuple(got.shape) == ((3, H, W) if layout == "planar" else (H, W, 3))
                assert np.array_equal(_planes(got, layout), ref["residual"][name][slots]), (name, layout, order)
    if crop:  # an output inside a larger buffer: unaligned rows, and nothing written around it
        for layout in X.LAYOUTS:
            out = _dev_u8(np.zeros((3, H, W), np.uint8), layout, True)
            X.residual_layer(src, rec, X.FrameBoxes(ref["lists"]["edges"]), layout=layout, out=out)
            assert np.array_equal(_planes(out, layout), ref["residual"]["edges"]), layout
            whole = out._base if out._base is not None else out
            around = whole.clone()
            (around[:, 1:1 + H, 1:1 + W] if layout == "planar" else around[1:1 + H, 1:1 + W]).fill_(99)
            assert bool((around == 99).all())
    assert (H, W) == (1, 1) or not np.array_equal(ref["residual"]["none"], ref["residual"]["whole"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fuse_from_both_residual_layouts(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    base = U.picture(ref["rec"], crop, DEV)
    table = R.T.view(np.uint32)
    for name, boxes in ref["lists"].items():
        want = ref["fuse"][name].view(np.uint32)
        for layout in X.LAYOUTS:
            for order, slots in SLOTS.items():
                res = _dev_u8(ref["res"][slots], layout, crop)
                got = X.fuse(base, res, X.FrameBoxes(boxes), CLASSES, layout=layout, order=order)
                assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, H, W)
                bits = got.cpu().numpy()[0].view(np.uint32)
                assert np.array_equal(bits, want), (name, layout, order, int((bits != want).sum()))
        assert np.isin(want, table).all()
    # the order of overlapping boxes decides: the reversed list gives another, also matching, picture
    if min(H, W) >= 37:
        assert not np.array_equal(ref["fuse"]["overlap"], ref["fuse"]["overlap-reversed"])
    # outside every box the result is T[code(base)]
    assert np.array_equal(ref["fuse"]["none"].view(np.uint32), R.T[R.code(ref["rec"])].view(np.uint32))
    # the layout is taken from the residual's shape; fusing a residual_layer output in place of a file
    r = X.residual_layer(U.picture(ref["src"], crop, DEV), base, X.FrameBoxes(ref["lists"]["whole"]), layout="hwc")
    if (H, W, 3) != (3, H, W):
        got = X.fuse(base, r, X.FrameBoxes(ref["lists"]["whole"]), CLASSES)
        want = R.fuse(ref["rec"], R.residual(ref["src"], ref["rec"], ref["lists"]["whole"]), ref["lists"]["whole"], R.BORDERS)
        assert np.array_equal(got.cpu().numpy()[0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_region_sums_added_onto_starting_values(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    a, b = U.picture(ref["src"], crop, DEV), U.picture(ref["rec"], crop, DEV)
    start = [7, 2 ** 40 + 11, 13]
    for name, boxes in ref["lists"].items():
        for sname, shrinks in R.SHRINKS.items():
            classes = tuple(X.RoiClass(bd, sh) for bd, sh in zip(R.BORDERS, shrinks))
            sums = torch.tensor(start, dtype=torch.int64, device=DEV)
            got = X.region_sse(a, b, X.FrameBoxes(boxes), classes, sums=sums)
            assert got is sums
            want = ref["sse"][(name, sname)]
            assert got.tolist() == [s + w for s, w in zip(start, want)], (name, sname)
            assert want[2] <= H * W
    fresh = X.region_sse(a, b, X.FrameBoxes(ref["lists"]["whole"]), CLASSES[2:3] * 4)  # shrink 0: everything inside
    assert fresh.dtype == torch.int64 and fresh.tolist() == ref["sse"][("whole", "shrink0")] and fresh.tolist()[1:] == [0, H * W]
    if (H, W) == (38, 518):  # shrinking takes pixels out of the mask, down to none of a box
        assert 0 < ref["sse"][("overlap", "shrink3")][2] < ref["sse"][("overlap", "shrink0")][2]
        assert ref["sse"][("whole", "emptying")][2] == 0 < ref["sse"][("whole", "shrink3")][2]


def test_python_layer_refuses_by_name():
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="coordinates out of range"):
        X.residual_layer(x, x, X.FrameBoxes([[0, 0, 9, 8, 0]]))
    with pytest.raises(ValueError, match="unknown class"):
        X.fuse(x, torch.zeros(3, 8, 8, dtype=torch.uint8, device=DEV), X.FrameBoxes([[0, 0, 8, 8, 1]]), CLASSES[:1])
    with pytest.raises(ValueError, match="layout"):
        X.residual_layer(x, x, X.FrameBoxes(), layout="chw")
    with pytest.raises(ValueError, match="order"):
        X.residual_layer(x, x, X.FrameBoxes(), order="bgr")
    with pytest.raises(ValueError, match="does not match"):
        X.residual_layer(x, x[..., :7], X.FrameBoxes())
    with pytest.raises(ValueError, match="GPU"):
        X.region_sse(x.cpu(), x.cpu(), X.FrameBoxes(), CLASSES)
    with pytest.raises(ValueError, match="float32"):
        X.region_sse(x.half(), x.half(), X.FrameBoxes(), CLASSES)


def test_run_to_run_identical_also_beside_convolutions_on_another_stream(refs):
    from vcm_ts_amd.dmc import DMC
    from vcm_ts_amd.synthetic import frames

    H, W = 38, 518
    ref = refs[(H, W)]
    src, rec = U.picture(ref["src"], False, DEV), U.picture(ref["rec"], False, DEV)
    res = _dev_u8(ref["res"], "planar", False)
    boxes = X.FrameBoxes(ref["lists"]["many150"])
    boxes.on_device(DEV)

    def once():
        return (X.residual_layer(src, rec, boxes, order="gbr"), X.fuse(rec, res, boxes, CLASSES),
                X.region_sse(src, rec, boxes, CLASSES))

    first = once()
    m = DMC().to(DEV).eval()
    clip = torch.from_numpy(frames(3, 2, 128, 128)).to(DEV)
    dpb = {"ref_frame": clip[0:1], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    with torch.no_grad():
        m.forward_one_frame(clip[1:2], dpb, 1.0, 1.0)  # (packs the filters, allocates the workspace)
        work, side = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(work):
            for _ in range(2):
                m.forward_one_frame(clip[1:2], dpb, 1.0, 1.0)
        with torch.cuda.stream(side):
            busy = [once() for _ in range(2)]
    torch.cuda.synchronize(DEV)
    for run in busy:
        for a, b in zip(first, run):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- end to end
E2E_BORDERS = (3, 10)  # plates, faces


def _e2e_boxes(h, w):
    """frame_index -> boxes: overlapping boxes of both classes (the order matters), a box on the picture's edge, an
    empty one, and a frame without any"""
    def boxes(t):
        if t == 4:
            return X.FrameBoxes()
        return X.FrameBoxes([[4 + t, 6, 40 + t, 40, 1], [20, 2 + t, 70, 30, 0], [30, 20, 60, 50 + t, 1], [w - 9, h - 11, w, h, 0],
                             [8, 8, 8, 20, 1]])
    return boxes


def _source(path, seed, n, h, w):
    """a seeded Y4M; returns the float32 RGB pictures the encoder is given (the restatement of the colour conversion,
    which tests/test_gpu_yuv.py holds the device to bit for bit)"""
    from tests import yuv_ref as YR

    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(f, dtype=np.float64)) for f in YR.gamut_rgb(seed, n, h, w)]
    YR.write_y4m(str(path), planes, w, h, fps="30:1")
    return [YR.to_rgb(*p, dtype=np.float32) for p in planes]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("roi_e2e")
    n, h, w, gop = 6, 64, 96, 3
    src = _source(tmp / "src.y4m", 51, n, h, w)
    roi = X.Roi(_e2e_boxes(h, w), tuple(X.RoiClass(b) for b in E2E_BORDERS), ("liplates", "faces"))
    kw = dict(gop=gop, gop_streams=2, nets=file_nets)
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "plain"), **kw)
    bits, size = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "bins"), roi=roi, residuals=str(tmp / "res.gbrp"), **kw)
    assert size == (h, w) and len(bits) == n
    assert RC.decode_folder(str(tmp / "plain"), str(tmp / "rec"), h, w, gop=gop) == n
    rec = [U.png(tmp / "rec" / f"im{t + 1:05d}.png", planar=True) for t in range(n)]  # code(reconstruction), as save_torch_image rounds it
    raw = np.frombuffer((tmp / "res.gbrp").read_bytes(), np.uint8).reshape(n, 3, h, w)
    return dict(tmp=tmp, n=n, h=h, w=w, gop=gop, src=src, rec=rec, roi=roi, raw=raw, kw=kw)


def test_end_to_end_same_bins_and_residual_file_in_display_order(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w = e2e["tmp"], e2e["n"], e2e["h"], e2e["w"]
    assert U.bins(tmp / "bins") == U.bins(tmp / "plain") and len(U.bins(tmp / "bins")) == n
    assert sorted(os.listdir(tmp / "bins")) == sorted(os.listdir(tmp / "plain"))
    info = RC.read_sequence_info(str(tmp / "bins"))
    assert info["roi"] == {"classes": [{"name": "liplates", "border": 3, "shrink": 3}, {"name": "faces", "border": 10, "shrink": 10}]}
    assert "roi" not in RC.read_sequence_info(str(tmp / "plain"))
    assert (tmp / "res.gbrp").stat().st_size == n * 3 * h * w
    for t in range(n):
        want = R.residual(e2e["src"][t], R.T[e2e["rec"][t]], e2e["roi"].boxes(t).array)
        assert np.array_equal(e2e["raw"][t], want[[1, 2, 0]]), t  # G, B, R planes
        assert want.any() == (t != 4)


def test_end_to_end_decoders_write_the_fused_picture(e2e):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp, n, h, w, gop, roi = (e2e[k] for k in ("tmp", "n", "h", "w", "gop", "roi"))
    res = str(tmp / "res.gbrp")
    assert RC.decode_folder(str(tmp / "bins"), str(tmp / "fused"), h, w, gop=gop, roi=roi, residuals=res) == n
    assert RC.decode_video(str(tmp / "bins"), str(tmp / "fused.y4m"), roi=roi, residuals=res) == n
    _, frames = YR.read_y4m(str(tmp / "fused.y4m"))
    changed = 0
    for t in range(n):
        want = R.fuse(R.T[e2e["rec"][t]], e2e["raw"][t][[2, 0, 1]], roi.boxes(t).array, E2E_BORDERS)
        codes = np.rint(want * np.float32(255.0)).astype(np.uint8)
        assert np.array_equal(U.png(tmp / "fused" / f"im{t + 1:05d}.png", planar=True), codes), t
        changed += int((codes != e2e["rec"][t]).sum())
        samples = Y.rgb_to_yuv420(torch.from_numpy(want)[None].to(DEV), h, w)
        assert np.array_equal(samples.cpu().numpy(), np.asarray(frames[t]).reshape(-1)), t
    assert changed > 100  # the enhancement layer did something
    # the decoder refuses by name before it decodes
    with pytest.raises(ValueError, match="residuals"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, roi=roi)
    with pytest.raises(ValueError, match="roi"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, residuals=res)
    short = tmp / "short.gbrp"
    short.write_bytes((tmp / "res.gbrp").read_bytes()[:3 * h * w * 2])
    with pytest.raises(ValueError, match="residual frames"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, roi=roi, residuals=str(short))


def test_end_to_end_png_residuals_agree_with_the_raw_file(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w, gop, roi = (e2e[k] for k in ("tmp", "n", "h", "w", "gop", "roi"))
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "bins_png"), roi=roi, residuals=str(tmp / "res_png"), **e2e["kw"])
    assert U.bins(tmp / "bins_png") == U.bins(tmp / "plain")
    assert sorted(os.listdir(tmp / "res_png")) == [f"im{t + 1:05d}.png" for t in range(n)]
    for t in range(n):
        assert np.array_equal(U.png(tmp / "res_png" / f"im{t + 1:05d}.png", planar=True), e2e["raw"][t][[2, 0, 1]]), t
    assert RC.decode_folder(str(tmp / "bins"), str(tmp / "fused_png"), h, w, gop=gop, roi=roi, residuals=str(tmp / "res_png")) == n
    if (tmp / "fused").exists():
        for t in range(n):
            name = f"im{t + 1:05d}.png"
            assert np.array_equal(U.png(tmp / "fused_png" / name, planar=True), U.png(tmp / "fused" / name, planar=True)), t


def test_report_gains_region_psnr(tmp_path, file_nets):
    """At 192x320 (see the module's docstring), otherwise the end-to-end setting."""
    from vcm_ts_amd import run_codec as RC

    n, h, w, gop = 6, 192, 320, 3
    src = _source(tmp_path / "src.y4m", 53, n, h, w)
    roi = X.Roi(_e2e_boxes(h, w), tuple(X.RoiClass(b) for b in E2E_BORDERS))
    kw = dict(gop=gop, gop_streams=2, nets=file_nets)
    _, _, plain = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "plain"), report=True, **kw)
    _, _, rd = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "bins"), report=str(tmp_path / "rd.json"), roi=roi,
                               residuals=str(tmp_path / "res.gbrp"), **kw)
    assert U.bins(tmp_path / "bins") == U.bins(tmp_path / "plain")
    new = {"frame_psnr_roi", "frame_psnr_bg", "frame_roi_pixels"}
    assert set(rd) - set(plain) == new and not new & set(plain)
    for key in plain:  # what was there is what it was
        assert rd[key] == plain[key], key
    assert RC.decode_folder(str(tmp_path / "plain"), str(tmp_path / "rec"), h, w, gop=gop) == n
    for t in range(n):
        rec = R.T[U.png(tmp_path / "rec" / f"im{t + 1:05d}.png", planar=True)]
        sums = R.sse(rec, src[t], roi.boxes(t).array, E2E_BORDERS)
        total, bg, inside = R.psnr(sums, h, w, "samples")
        assert rd["frame_roi_pixels"][t] == sums[2] and (sums[2] > 0) == (t != 4)
        assert rd["frame_psnr_bg"][t] == pytest.approx(bg, rel=1e-13)
        if t == 4:
            assert np.isnan(rd["frame_psnr_roi"][t])
        else:
            assert rd["frame_psnr_roi"][t] == pytest.approx(inside, rel=1e-13)
    assert json.loads((tmp_path / "rd.json").read_text())["frame_roi_pixels"] == rd["frame_roi_pixels"]
    # the PNG path reports the same keys
    from PIL import Image

    png = tmp_path / "png"
    png.mkdir()
    for t in range(n):
        Image.fromarray(R.code(src[t]).astype(np.uint8).transpose(1, 2, 0)).save(png / f"im{t + 1:05d}.png")
    _, _, rf = RC.encode_folder(str(png), str(tmp_path / "bf"), report=True, roi=roi, residuals=str(tmp_path / "rf.gbrp"), **kw)
    assert new <= set(rf) and len(rf["frame_psnr_roi"]) == n and rf["frame_roi_pixels"] == rd["frame_roi_pixels"]
    assert (tmp_path / "rf.gbrp").stat().st_size == n * 3 * h * w
