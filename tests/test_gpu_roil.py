"""The ROI residual layer on the device (vcm_ts_amd/roilayer.py, csrc/roil.hip) and the file loops built on it.

Every comparison is equality of bytes against tests/roil_ref.py, the restatement of include/dcvc_hip_roil.h: after code()
the layer is integer arithmetic and a fixed format, so nothing needs a tolerance.  The cases are those of
tests/test_gpu_roi.py (its four sizes, and 40x130 as an offset view inside a 64x192 buffer with foreign values around it)
on pictures whose cells have residual spreads from exact to uniform (roil_ref.pictures), steps 1 and 7.

The end-to-end tests run at 64x96, 6 pictures, GOP 3, two GOP streams; the report test alone at 192x320, the smallest
size MS-SSIM admits.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import roi_ref as R
from tests import roil_ref as RL
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from vcm_ts_amd import roi as X
from vcm_ts_amd import roilayer as Y

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(seed, H, W, False) for seed, (H, W) in enumerate(R.SIZES)] + [(9, 40, 130, True)]
IDS = [f"{H}x{W}" + ("-crop" if crop else "") for _, H, W, crop in CASES]
SLOTS = {"rgb": [0, 1, 2], "gbr": [1, 2, 0]}
STEPS = (1, 7)


def _guarded(layout, H, W):
    """(buffer, view): an output picture of the layout one element inside a larger buffer of 99s"""
    if layout == "planar":
        big = torch.full((3, H + 2, W + 3), 99, dtype=torch.uint8, device=DEV)
        return big, big[:, 1:1 + H, 1:1 + W]
    big = torch.full((H + 2, W + 3, 3), 99, dtype=torch.uint8, device=DEV)
    return big, big[1:1 + H, 1:1 + W]


def _guards_intact(big, layout, H, W):
    around = big.clone()
    (around[:, 1:1 + H, 1:1 + W] if layout == "planar" else around[1:1 + H, 1:1 + W]).fill_(99)
    return bool((around == 99).all())


def _planes(t, layout):
    a = t.cpu().numpy()
    return a if layout == "planar" else a.transpose(2, 0, 1)


@pytest.fixture(scope="module")
def refs():
    """per case: pictures, box lists and the restatement's records and decoded pictures, computed once"""
    out = {}
    for seed, H, W, crop in CASES:
        src, rec = RL.pictures(seed, H, W)
        lists = R.box_lists(H, W)
        res = {n: R.residual(src, rec, b) for n, b in lists.items()}
        out[(H, W)] = dict(src=src, rec=rec, lists=lists, res=res,
                           coded={(n, S): RL.encode_record(res[n], b, S) for n, b in lists.items() for S in STEPS})
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_record_is_the_restatements_bytes(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    src, rec = U.picture(ref["src"], crop, DEV), U.picture(ref["rec"], crop, DEV)
    pending = {(n, S): Y.encode_layer(src, rec, X.FrameBoxes(b), step=S) for n, b in ref["lists"].items() for S in STEPS}
    seen = set()
    for key, p in pending.items():
        got, (want, modes, _) = p.bytes(), ref["coded"][key]
        assert got == want, (key, len(got), len(want), Y.parse_record(got)["modes"].reshape(-1).tolist()[:12], modes[:12])
        seen.update(modes)
    assert (H, W) == (1, 1) or len(seen) >= 5  # several modes per case; all nine over the cases: tests/test_roil_host.py
    assert pending[("none", 1)].bytes() == b"RL\x01\x01\x00\x00\x00\x00"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_decodes_the_restatements_record_in_both_layouts_and_orders(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    for (name, S), (record, _, want) in ref["coded"].items():
        boxes = X.FrameBoxes(ref["lists"][name])
        for layout in X.LAYOUTS:
            for order, slots in SLOTS.items():
                if name not in ("edges", "overlap", "none") and (layout, order) not in (("planar", "gbr"), ("hwc", "rgb")):
                    continue  # (every list in the two combinations the file loops use, three lists in all four)
                got = Y.decode_layer(record, boxes, H, W, layout=layout, order=order)
                assert got.dtype == torch.uint8 and tuple(got.shape) == ((3, H, W) if layout == "planar" else (H, W, 3))
                assert np.array_equal(_planes(got, layout), want[slots]), (name, S, layout, order)
    for layout in X.LAYOUTS:  # an output inside a larger buffer: every element written, nothing around it
        record, _, want = ref["coded"][("edges", 7)]
        big, view = _guarded(layout, H, W)
        assert Y.decode_layer(record, X.FrameBoxes(ref["lists"]["edges"]), H, W, layout=layout, out=view) is view
        assert np.array_equal(_planes(view, layout), want) and _guards_intact(big, layout, H, W), layout
    if (H, W) == (37, 131):  # mode 7, which no encoder chooses and every decoder accepts (roil_ref.REACHABLE_MODES)
        boxes = ref["lists"]["whole"]
        record, modes, want = RL.encode_record(ref["res"]["whole"], boxes, 1, force7=True)
        assert 7 in modes
        assert np.array_equal(Y.decode_layer(record, X.FrameBoxes(boxes), H, W).cpu().numpy(), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decode_of_the_devices_own_record_is_the_quantised_residual(case, refs):
    _, H, W, crop = case
    ref = refs[(H, W)]
    src, rec = U.picture(ref["src"], crop, DEV), U.picture(ref["rec"], crop, DEV)
    for name in ("edges", "overlap", "whole", "max1024"):
        boxes = X.FrameBoxes(ref["lists"][name])
        for S in STEPS:
            record = Y.encode_layer(src, rec, boxes, step=S).bytes()
            got = Y.decode_layer(record, boxes, H, W)
            assert np.array_equal(got.cpu().numpy(), ref["coded"][(name, S)][2]), (name, S)
            if S == 1:
                assert torch.equal(got, X.residual_layer(src, rec, boxes))


def test_a_zeroed_payload_sets_the_status_word_and_stays_inside_the_picture(refs):
    """Decoded ONCE.  The table is valid, so the launch happens; the unary sections have no set bit.  Safe by construction:
    reads are bounded by the validated lengths, writes by the cell."""
    H, W = 38, 518
    ref = refs[(H, W)]
    record, modes, _ = ref["coded"][("whole", 1)]
    A = Y.parse_record(record)["cells"]
    assert any(m < 8 for m in modes)
    zeroed = record[:8 + 6 * A] + bytes(len(record) - 8 - 6 * A)
    big, view = _guarded("planar", H, W)
    with pytest.raises(Y.RoiLayerError, match="BAD_STREAM") as err:
        Y.decode_layer(zeroed, X.FrameBoxes(ref["lists"]["whole"]), H, W, out=view)
    assert err.value.status & Y.BAD_STREAM
    assert _guards_intact(big, "planar", H, W)


def test_python_layer_refuses_by_name(refs):
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="residual step"):
        Y.encode_layer(x, x, X.FrameBoxes(), step=0)
    with pytest.raises(ValueError, match="coordinates out of range"):
        Y.encode_layer(x, x, X.FrameBoxes([[0, 0, 9, 8, 0]]))
    with pytest.raises(ValueError, match="does not match"):
        Y.encode_layer(x, x[..., :7], X.FrameBoxes())
    with pytest.raises(ValueError, match="GPU"):
        Y.encode_layer(x.cpu(), x.cpu(), X.FrameBoxes())
    record = Y.encode_layer(x, x, X.FrameBoxes([[0, 0, 8, 8, 0]]), step=3).bytes()
    assert record == b"RL\x01\x03\x01\x00\x00\x00" + (9 << 12).to_bytes(2, "little") * 3  # an exact cell: three empty segments
    with pytest.raises(Y.RoiLayerError, match="wrong number of active cells"):
        Y.decode_layer(record, X.FrameBoxes(), 8, 8)
    with pytest.raises(Y.RoiLayerError, match="truncated"):
        Y.decode_layer(record[:-1], X.FrameBoxes([[0, 0, 8, 8, 0]]), 8, 8)
    with pytest.raises(ValueError, match="layout"):
        Y.decode_layer(record, X.FrameBoxes([[0, 0, 8, 8, 0]]), 8, 8, layout="chw")
    with pytest.raises(ValueError, match="order"):
        Y.decode_layer(record, X.FrameBoxes([[0, 0, 8, 8, 0]]), 8, 8, order="bgr")
    out = Y.decode_layer(record, X.FrameBoxes([[0, 0, 8, 8, 0]]), 8, 8)
    assert bool((out == 128).all())


# ------------------------------------------------------------------------------------------------------- end to end
from tests import test_gpu_roi as G  # noqa: E402  (its seeded source and boxes: the same loop setting)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """encode without the layer, and with --residuals x.gbrp and --residual-bins (into the --bins folder) together"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("roil_e2e")
    n, h, w, gop = 6, 64, 96, 3
    G._source(tmp / "src.y4m", 51, n, h, w)
    roi = X.Roi(G._e2e_boxes(h, w), tuple(X.RoiClass(b) for b in G.E2E_BORDERS), ("liplates", "faces"))
    kw = dict(gop=gop, gop_streams=2, nets=file_nets)
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "plain"), **kw)
    bits, size = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "bins"), roi=roi, residuals=str(tmp / "res.gbrp"),
                                 residual_bins=str(tmp / "bins"), **kw)
    assert size == (h, w) and len(bits) == n
    raw = np.frombuffer((tmp / "res.gbrp").read_bytes(), np.uint8).reshape(n, 3, h, w)
    return dict(tmp=tmp, n=n, h=h, w=w, gop=gop, roi=roi, raw=raw, kw=kw)


def _records(folder, n):
    return [open(os.path.join(folder, f"im{t + 1:05d}.rl"), "rb").read() for t in range(n)]


def test_end_to_end_same_bins_and_records_of_the_raw_residual(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w, roi = (e2e[k] for k in ("tmp", "n", "h", "w", "roi"))
    assert U.bins(tmp / "bins") == U.bins(tmp / "plain") and len(U.bins(tmp / "bins")) == n
    assert sorted(set(os.listdir(tmp / "bins")) - set(os.listdir(tmp / "plain"))) == [f"im{t + 1:05d}.rl" for t in range(n)]
    assert RC.read_sequence_info(str(tmp / "bins"))["residual_step"] == 1
    assert "residual_step" not in RC.read_sequence_info(str(tmp / "plain"))
    for t, record in enumerate(_records(tmp / "bins", n)):  # in display order whatever order the GOP streams finished in
        boxes, res = roi.boxes(t).array, e2e["raw"][t][[2, 0, 1]]  # the .gbrp planes are G, B, R
        assert record == RL.encode_record(res, boxes, 1)[0], t
        assert np.array_equal(RL.decode_record(record, boxes, h, w), res), t
        assert (len(record) == 8) == (t == 4)
        cells, counts, _ = RL.active_cells(boxes, h, w)
        assert len(record) <= 8 + 6 * len(cells) + 3 * int(counts.sum())  # L <= n: never more than the raw samples and the table


def test_end_to_end_decoding_the_records_writes_the_pngs_of_the_raw_file(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w, gop, roi = (e2e[k] for k in ("tmp", "n", "h", "w", "gop", "roi"))
    assert RC.decode_folder(str(tmp / "bins"), str(tmp / "fused_raw"), h, w, gop=gop, roi=roi, residuals=str(tmp / "res.gbrp")) == n
    assert RC.decode_folder(str(tmp / "bins"), str(tmp / "fused_rl"), h, w, gop=gop, roi=roi, residual_bins=str(tmp / "bins")) == n
    changed = 0
    for t in range(n):
        name = f"im{t + 1:05d}.png"
        assert (tmp / "fused_rl" / name).read_bytes() == (tmp / "fused_raw" / name).read_bytes(), t
    assert RC.decode_folder(str(tmp / "plain"), str(tmp / "rec"), h, w, gop=gop) == n
    for t in range(n):
        name = f"im{t + 1:05d}.png"
        changed += int((U.png(tmp / "fused_rl" / name, planar=True) != U.png(tmp / "rec" / name, planar=True)).sum())
    assert changed > 100  # the enhancement layer did something
    assert RC.decode_video(str(tmp / "bins"), str(tmp / "fused_rl.y4m"), roi=roi, residual_bins=str(tmp / "bins")) == n
    assert RC.decode_video(str(tmp / "bins"), str(tmp / "fused_raw.y4m"), roi=roi, residuals=str(tmp / "res.gbrp")) == n
    assert (tmp / "fused_rl.y4m").read_bytes() == (tmp / "fused_raw.y4m").read_bytes()
    # refused by name before anything is decoded
    with pytest.raises(ValueError, match="not both"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, roi=roi, residuals=str(tmp / "res.gbrp"),
                         residual_bins=str(tmp / "bins"))
    with pytest.raises(ValueError, match="roi"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, residual_bins=str(tmp / "bins"))
    holed = tmp / "holed"
    holed.mkdir()
    for t, record in enumerate(_records(tmp / "bins", n)):
        if t != 2:
            (holed / f"im{t + 1:05d}.rl").write_bytes(record)
    with pytest.raises(ValueError, match="im00003.rl"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, roi=roi, residual_bins=str(holed))
    (holed / "im00003.rl").write_bytes(_records(tmp / "bins", n)[4])  # the record of the frame without boxes
    with pytest.raises(Y.RoiLayerError, match="im00003.rl.*wrong number of active cells"):
        RC.decode_folder(str(tmp / "bins"), str(tmp / "x"), h, w, gop=gop, roi=roi, residual_bins=str(holed))


def test_end_to_end_step_seven_is_recorded_and_coded(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, n, h, w, roi = (e2e[k] for k in ("tmp", "n", "h", "w", "roi"))
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "bins7"), roi=roi, residual_bins=str(tmp / "rl7"), residual_step=7, **e2e["kw"])
    assert U.bins(tmp / "bins7") == U.bins(tmp / "plain")
    assert RC.read_sequence_info(str(tmp / "bins7"))["residual_step"] == 7
    assert sorted(os.listdir(tmp / "rl7")) == [f"im{t + 1:05d}.rl" for t in range(n)]
    for t, record in enumerate(_records(tmp / "rl7", n)):
        assert record == RL.encode_record(e2e["raw"][t][[2, 0, 1]], roi.boxes(t).array, 7)[0], t
    with pytest.raises(ValueError, match="residual_step"):
        RC.encode_video(str(tmp / "src.y4m"), str(tmp / "x"), roi=roi, residual_step=7, **e2e["kw"])
    with pytest.raises(ValueError, match="residual step"):
        RC.encode_video(str(tmp / "src.y4m"), str(tmp / "x"), roi=roi, residual_bins=str(tmp / "x"), residual_step=65, **e2e["kw"])
    with pytest.raises(ValueError, match="roi"):
        RC.encode_video(str(tmp / "src.y4m"), str(tmp / "x"), residual_bins=str(tmp / "x"), **e2e["kw"])


def test_report_gains_the_enhancement_layers_bits(tmp_path, file_nets):
    """At 192x320, the smallest size MS-SSIM admits; otherwise the end-to-end setting."""
    from vcm_ts_amd import run_codec as RC

    n, h, w, gop = 6, 192, 320, 3
    G._source(tmp_path / "src.y4m", 53, n, h, w)
    roi = X.Roi(G._e2e_boxes(h, w), tuple(X.RoiClass(b) for b in G.E2E_BORDERS))
    kw = dict(gop=gop, gop_streams=2, nets=file_nets, roi=roi)
    _, _, base = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "base"), report=True, **kw)
    _, _, rd = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "bins"), report=str(tmp_path / "rd.json"),
                               residual_bins=str(tmp_path / "bins"), **kw)
    assert U.bins(tmp_path / "bins") == U.bins(tmp_path / "base")
    new = {"frame_bits_enh", "frame_bpp_enh", "ave_all_frame_bpp_enh", "ave_all_frame_bpp_total"}
    assert set(rd) - set(base) == new and not new & set(base)
    for key in base:  # what was there is what it was
        assert json.dumps(rd[key]) == json.dumps(base[key]), key  # (as text: frame_psnr_roi of the frame without boxes is nan)
    sizes = [os.path.getsize(tmp_path / "bins" / f"im{t + 1:05d}.rl") for t in range(n)]
    assert rd["frame_bits_enh"] == [8 * s for s in sizes] and sizes[4] == 8 and min(sizes[:4]) > 8
    assert rd["frame_bpp_enh"] == [8 * s / (h * w) for s in sizes]
    assert rd["ave_all_frame_bpp_enh"] == pytest.approx(8 * sum(sizes) / (n * h * w), rel=1e-12)
    assert rd["ave_all_frame_bpp_total"] == rd["ave_all_frame_bpp"] + rd["ave_all_frame_bpp_enh"]
    assert json.loads((tmp_path / "rd.json").read_text())["frame_bits_enh"] == rd["frame_bits_enh"]
