"""Scene-cut I pictures on the device: the histogram kernel (csrc/scene.hip) bit for bit against tests/scenecut_ref.py, the
numpy restatement of include/dcvc_hip_scene.h, and the file loops that place, record, code and decode the I pictures.

Everything the kernel computes is an integer sum, so every comparison is array_equal.

The end-to-end tests run at 64x64, 16 pictures (five of a bright scene, eleven of a dark one), longest GOP 8, threshold
0.5, min_gop 2: the plan is [0, 5, 13] (tests/test_scenecut_host.py holds the margins of that threshold).  The report test
alone runs at 192x192: a report carries MS-SSIM, which takes no picture side below 161 (vcm_ts_amd/metrics.py).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import scenecut_ref as R
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from vcm_ts_amd import lib
from vcm_ts_amd import scenecut as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [(1, 1), (3, 5), (65, 63), (64, 96), (135, 241)]
IDS = [f"{h}x{w}" for h, w in SIZES]
NAN = float("nan")


def _view(a, layout):
    """the (3, H, W) picture as a (1, 3, H, W) strided view inside a larger NaN-filled buffer, with its strides.
    "offset": at an odd element offset with odd strides (no row is 16-byte aligned: the scalar path, a NaN read in place
    of a pixel would move a count).  "aligned": rows and planes padded to multiples of 4 elements from an aligned base
    (the 16-byte path, with the scalar quads at the cells' edges)."""
    _, H, W = a.shape
    if layout == "offset":
        off, rs = 3, W + 5 + (W + 5) % 2 + 1
        ps = (H + 2) * rs + 1
    else:
        off, rs = 0, (W + 3) // 4 * 4 + 4
        ps = (H + 1) * rs
    buf = torch.full((off + 3 * ps + 7,), NAN, dtype=torch.float32, device=DEV)
    v = buf.as_strided((1, 3, H, W), (3 * ps, ps, rs, 1), off)
    v.copy_(torch.from_numpy(a)[None])
    assert (v.data_ptr() % 16 == 0) == (layout == "aligned")
    return v, rs, ps


def _kernel(v, rs, ps, hist=None):
    """dcvc_scene_hist itself, on the view's own strides"""
    H, W = v.shape[2:]
    if hist is None:
        hist = torch.zeros(512, dtype=torch.int32, device=DEV)
    lib.check(lib.hip().dcvc_scene_hist(v.data_ptr(), rs, ps, H, W, hist.data_ptr(), U.stream(DEV)), "scene_hist")
    return hist


@pytest.mark.parametrize("layout", ["offset", "aligned"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_kernel_equals_the_restatement_bit_for_bit(size, layout):
    H, W = size
    a = R.wide_picture(11 + H, H, W)  # values over [-0.5, 1.5]: both clamps act
    assert a.min() < 0 and a.max() > 1 or H * W < 4
    want = R.hist(a)
    v, rs, ps = _view(a, layout)
    got = _kernel(v, rs, ps).cpu().numpy().astype(np.int64)
    assert got.sum() == H * W
    assert np.array_equal(got, want), int((got != want).sum())
    if size == (3, 5):
        assert (want.reshape(16, 32).sum(axis=1) == 0).any()  # empty cells


@pytest.mark.parametrize("layout", ["offset", "aligned"])
@pytest.mark.parametrize("size", [(64, 96), (135, 241)], ids=["64x96", "135x241"])
def test_result_does_not_depend_on_how_the_counts_collide(size, layout):
    """a constant picture (one counter per cell takes everything), a two-valued checkerboard, a horizontal ramp"""
    H, W = size
    for name, a in R.content_pictures(H, W).items():
        want = R.hist(a)
        v, rs, ps = _view(a, layout)
        got = _kernel(v, rs, ps).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), name
        if name == "constant":
            assert (want > 0).sum() == 16 and np.array_equal(want[want > 0], R.cell_pixels(H, W))


def test_kernel_adds_onto_the_counters_it_is_given():
    H, W = 65, 63
    a = R.wide_picture(2, H, W)
    v, rs, ps = _view(a, "offset")
    hist = _kernel(v, rs, ps)
    _kernel(v, rs, ps, hist)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), 2 * R.hist(a))
    scan = SC.SceneScan(DEV, H, W, 2)
    scan.add(v)
    scan.add(v, row=0)
    scan.add(v)
    assert np.array_equal(scan.histograms(), np.stack([2 * R.hist(a), R.hist(a)]))


def test_scan_on_another_stream_through_padded_pictures():
    """SceneScan.add on a non-default stream, nothing synchronised before distances(); the 65 x 63 crop of padded
    (1, 3, 128, 128) pictures is read in place and the padding (here: values that would land in other bins) ignored."""
    H, W, n = 65, 63, 4
    pics = [R.wide_picture(20 + t, H, W) for t in range(n)]
    pics[2] = pics[1].copy()  # a repeated picture: distance 0
    padded = []
    for p in pics:
        big = torch.full((1, 3, 128, 128), 0.999, device=DEV)
        big[..., :H, :W] = torch.from_numpy(p).to(DEV)
        padded.append(big)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(DEV)
    scan = SC.SceneScan(DEV, H, W, n)  # (zeroed on the default stream: the side stream's first add is ordered behind it)
    with torch.cuda.stream(side):
        for big in padded:
            scan.add(big)
        d = scan.distances()
    want = R.distances(pics)
    assert d.dtype == np.float64 and d.shape == (n,) and d[0] == 0.0 and d[2] == 0.0
    assert np.array_equal(d, want)
    assert np.array_equal(scan.histograms(), np.stack([R.hist(p) for p in pics]))
    with pytest.raises(ValueError, match="GPU"):
        scan.add(padded[0].cpu())
    with pytest.raises(ValueError, match="row 4"):
        scan.add(padded[0])


# ------------------------------------------------------------------------------------------------------- end to end
GOP, T, MIN_GOP, PLAN = 8, 0.5, 2, [0, 5, 13]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the clip as PNGs; a plain encode (the baseline) and the scene-cut encode with its reconstructions"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("scenecut_e2e")
    clip = R.cut_clip(64, 64)
    U.write_pngs(tmp / "png", clip)
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    return dict(tmp=tmp, clip=clip, n=len(clip))


@pytest.fixture(scope="module")
def cut(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "cut"), str(tmp / "cut_rec"), gop=GOP, nets=file_nets, scenecut=T,
                                  min_gop=MIN_GOP)
    assert size == (64, 64) and len(bits) == e2e["n"]
    return tmp / "cut"


def test_folder_plan_is_recorded_and_the_cut_pictures_are_i_files(e2e, cut):
    from vcm_ts_amd import stream as S

    floats = [a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0) for a in e2e["clip"]]
    assert R.plan(R.distances(floats), GOP, T, MIN_GOP) == PLAN  # the restatement is the judge of the inputs
    assert json.loads((cut / "gops.json").read_text()) == {"frames": 16, "gop": GOP, "min_gop": MIN_GOP, "scenecut": T,
                                                           "i_pictures": PLAN}
    assert sorted(n for n in os.listdir(cut) if not n.endswith(".bin")) == ["gops.json"]
    for g in PLAN:
        h, w, _, payload = S.decode_i(str(cut / f"im{g + 1:05d}.bin"))
        assert (h, w) == (64, 64) and len(payload) > 0
    plain = U.bins(e2e["tmp"] / "plain")
    ours = U.bins(cut)
    assert list(ours) == list(plain) and len(ours) == 16
    assert all(ours[f"im{t + 1:05d}.bin"] == plain[f"im{t + 1:05d}.bin"] for t in range(5))  # the first GOP is the same
    assert ours["im00006.bin"] != plain["im00006.bin"]


def test_folder_decodes_to_the_encoders_reconstruction(e2e, cut):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert RC.decode_folder(str(cut), str(tmp / "cut_dec"), 64, 64) == 16  # (the plan's gop, not the default 32)
    assert RC.decode_folder(str(cut), str(tmp / "cut_dec8"), 64, 64, gop=GOP) == 16
    for t in range(16):
        name = f"im{t + 1:05d}.png"
        want = (tmp / "cut_rec" / name).read_bytes()
        assert (tmp / "cut_dec" / name).read_bytes() == want, t
        assert (tmp / "cut_dec8" / name).read_bytes() == want, t
    with pytest.raises(ValueError, match="gop 8, not 4"):
        RC.decode_folder(str(cut), str(tmp / "x"), 64, 64, gop=4)


def test_two_gop_streams_write_the_same_bins(e2e, cut, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "cut2"), gop=GOP, nets=file_nets, gop_streams=2, scenecut=T, min_gop=MIN_GOP)
    assert U.bins(tmp / "cut2") == U.bins(cut)
    assert (tmp / "cut2" / "gops.json").read_text() == (cut / "gops.json").read_text()


def test_feature_off_is_free(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    plain = U.bins(tmp / "plain")
    assert sorted(os.listdir(tmp / "plain")) == sorted(plain)  # no gops.json, nothing but the .bin files
    RC.encode_folder(str(tmp / "png"), str(tmp / "never"), gop=GOP, nets=file_nets, scenecut=1.0)  # d > 1.0 cannot happen
    assert U.bins(tmp / "never") == plain
    info = json.loads((tmp / "never" / "gops.json").read_text())
    assert SC.GopPlan.from_json(info) == SC.GopPlan.fixed(16, GOP) and info["scenecut"] == 1.0 and info["min_gop"] == 1
    for bad in (dict(scenecut=0.0), dict(scenecut=1.5), dict(scenecut=0.5, min_gop=9), dict(scenecut=0.5, min_gop=0)):
        with pytest.raises(ValueError, match="threshold|min_gop"):
            RC.encode_folder(str(tmp / "png"), str(tmp / "bad"), gop=GOP, nets=file_nets, **bad)
    assert not (tmp / "bad").exists()


def test_report_marks_the_i_pictures(tmp_path, file_nets):
    """At 192x192 (see the module's docstring), otherwise the end-to-end clip and options."""
    from vcm_ts_amd import run_codec as RC

    clip = R.cut_clip(192, 192)
    floats = [a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0) for a in clip]
    assert R.plan(R.distances(floats), GOP, T, MIN_GOP) == PLAN
    U.write_pngs(tmp_path / "png", clip)
    _, _, rd = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), gop=GOP, nets=file_nets, gop_streams=2, report=True,
                                scenecut=T, min_gop=MIN_GOP)
    assert [t for t, k in enumerate(rd["frame_type"]) if k == 0] == PLAN and len(rd["frame_type"]) == 16
    assert rd["i_frame_num"] == 3 and rd["p_frame_num"] == 13
    assert len(rd["frame_psnr"]) == 16 and all(np.isfinite(rd["frame_psnr"])) and all(np.isfinite(rd["frame_msssim"]))
    assert json.loads((tmp_path / "bins" / "gops.json").read_text())["i_pictures"] == PLAN


def test_y4m_plan_and_decoder_output(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0), dtype=np.float64))
              for a in e2e["clip"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, 64, 64, fps="30:1")
    # the restatement on the CONVERTED pictures is the judge of what the scan sees
    converted = [YR.to_rgb(*p, dtype=np.float32) for p in planes]
    assert R.plan(R.distances(converted), GOP, T, MIN_GOP) == PLAN
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), gop=GOP, nets=file_nets, gop_streams=2,
                    scenecut=T, min_gop=MIN_GOP)
    assert json.loads((tmp / "vbins" / "gops.json").read_text())["i_pictures"] == PLAN
    info = RC.read_sequence_info(str(tmp / "vbins"))
    assert info["gop"] == GOP and info["frames"] == 16 and "i_pictures" not in info and "scenecut" not in info
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == 16
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()
    assert (tmp / "dec.y4m").stat().st_size > 16 * 64 * 64 * 3 // 2


def test_roi_layer_either_side_of_the_cut(e2e, file_nets):
    """Boxes on frames 4, 5 and 6 (the cut is at 5; with two GOP streams frames 4 and 5 are coded on different streams):
    the residual file and the decoder's fused pictures are what tests/test_gpu_roi.py checks for fixed GOPs."""
    from tests import roi_ref as RR
    from vcm_ts_amd import roi as X
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w = e2e["tmp"], e2e["n"], 64, 64
    borders = (3, 10)

    def boxes(t):
        if t not in (4, 5, 6):
            return X.FrameBoxes()
        return X.FrameBoxes([[4 + t, 6, 40 + t, 40, 1], [20, 2 + t, 60, 30, 0], [w - 9, h - 11, w, h, 0]])

    roi = X.Roi(boxes, tuple(X.RoiClass(b) for b in borders), ("liplates", "faces"))
    res = str(tmp / "res.gbrp")
    RC.encode_folder(str(tmp / "png"), str(tmp / "rbins"), gop=GOP, nets=file_nets, gop_streams=2, roi=roi, residuals=res,
                     scenecut=T, min_gop=MIN_GOP)
    assert json.loads((tmp / "rbins" / "gops.json").read_text())["i_pictures"] == PLAN
    assert RC.decode_folder(str(tmp / "rbins"), str(tmp / "rrec"), h, w) == n
    assert RC.decode_folder(str(tmp / "rbins"), str(tmp / "rfused"), h, w, roi=roi, residuals=res) == n
    raw = np.frombuffer(open(res, "rb").read(), np.uint8).reshape(n, 3, h, w)
    changed = 0
    for t in range(n):
        rec = U.png(tmp / "rrec" / f"im{t + 1:05d}.png", planar=True)
        src = RR.T[e2e["clip"][t].transpose(2, 0, 1)]
        want_res = RR.residual(src, RR.T[rec], boxes(t).array)
        assert np.array_equal(raw[t], want_res[[1, 2, 0]]), t  # G, B, R planes
        assert want_res.any() == (t in (4, 5, 6))
        want = RR.fuse(RR.T[rec], raw[t][[2, 0, 1]], boxes(t).array, borders)
        codes = np.rint(want * np.float32(255.0)).astype(np.uint8)
        assert np.array_equal(U.png(tmp / "rfused" / f"im{t + 1:05d}.png", planar=True), codes), t
        changed += int((codes != rec).sum())
    assert changed > 100
