"""Motion ROI boxes on a real MI355X: the background-model kernel bit for bit against the numpy restatement
(tests/motion_ref.py) in strided, offset, NaN-surrounded layouts with guarded outputs, its refusals, MotionScan, a
static-camera clip end to end, and the command line: `boxes`, then encode and decode with the third box class."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import motion_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import motionroi as M
from vcm_ts_amd import roi as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
SENTINEL = 0xABCD


def _ptr(buf, at):
    return buf.data_ptr() + 2 * at


def _check(buf, at, n, want, where):
    got = U.words(buf)
    assert np.array_equal(got[at:at + n], np.asarray(want, dtype=np.int64).reshape(-1)), where
    assert U.guards_intact(buf, at, n, SENTINEL), where


# (row pad, plane pad, picture offset, model / counts shift): 16-byte picture loads and 8-byte model accesses; an odd
# offset, an odd row stride, an odd plane stride -> 4-byte loads; a model that is only 2-, 4- or 6-byte aligned -> 2-byte accesses
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    hc, wc = R.grid(H, W)
    assert X.grid_of(H, W) == (hc, wc)
    L = lib.hip()
    seqs = R.sequences(H, W)
    full_cells = 0
    for T, k_bg, k_fg in R.SETTINGS:
        edge_bg, edge_pic = R.edge_case(H, W, T)
        edge_want = R.step(edge_pic, edge_bg, T, k_bg, k_fg)
        for name, pics in seqs.items():
            want = R.run(pics, T, k_bg, k_fg)
            full_cells += sum(int((c == 256).sum()) for _, c in want)
            for n, (row_pad, plane_pad, offset, shift) in enumerate(LAYOUTS):
                if name != "random" and n not in (0, 1 + (T + len(name)) % 3):  # (every layout on one sequence, two on the others)
                    continue
                bg, b0 = U.guarded(H * W, shift, np.uint16, SENTINEL, DEV)
                for t, pic in enumerate(pics):
                    where = (name, T, k_bg, k_fg, row_pad, plane_pad, offset, shift, t)
                    keep, view, rs, ps = U.strided(pic, H, W, row_pad, plane_pad, offset, DEV)[:4]
                    counts, c0 = U.guarded(hc * wc, shift, np.uint16, SENTINEL, DEV)  # (fresh sentinels every step: every cell is WRITTEN)
                    lib.check(L.dcvc_motion_step(view.data_ptr(), rs, ps, H, W, _ptr(bg, b0), int(t == 0), T, k_bg, k_fg,
                                                 _ptr(counts, c0), U.stream(DEV)), "motion_step")
                    _check(bg, b0, H * W, want[t][0], where)
                    _check(counts, c0, hc * wc, want[t][1], where)
                    assert not want[t][1][(H + 15) // 16:].any() and not want[t][1][:, (W + 15) // 16:].any()  # the padding cells
                # one more step from a model written by the host: |delta| on both sides of the threshold, side by side
                bg[b0:b0 + H * W] = torch.from_numpy(edge_bg.astype(np.uint16).view(np.int16).reshape(-1)).to(DEV)
                keep, view, rs, ps = U.strided(edge_pic, H, W, row_pad, plane_pad, offset, DEV)[:4]
                counts, c0 = U.guarded(hc * wc, shift, np.uint16, SENTINEL, DEV)
                lib.check(L.dcvc_motion_step(view.data_ptr(), rs, ps, H, W, _ptr(bg, b0), 0, T, k_bg, k_fg, _ptr(counts, c0),
                                             U.stream(DEV)), "motion_step")
                _check(bg, b0, H * W, edge_want[0], ("edge", T, n))
                _check(counts, c0, hc * wc, edge_want[1], ("edge", T, n))
        assert int(edge_want[1].sum()) == H * (W // 2)  # exactly the odd columns are foreground
    assert full_cells > 0 or H * W < 256  # zeros against ones: cells with all 256 pixels foreground


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    keep, view, rs, ps = U.strided(R.pictures(H, W)["random0"], H, W, 8, 24, 12, DEV)[:4]
    bg, b0 = U.guarded(H * W, 0, np.uint16, SENTINEL, DEV)
    counts, c0 = U.guarded(hc * wc, 0, np.uint16, SENTINEL, DEV)
    good = dict(rgb=view.data_ptr(), rs=rs, ps=ps, H=H, W=W, bg=_ptr(bg, b0), init=1, T=24, k_bg=4, k_fg=8, counts=_ptr(counts, c0))
    order = ("rgb", "rs", "ps", "H", "W", "bg", "init", "T", "k_bg", "k_fg", "counts")
    for bad in ({"rgb": None}, {"bg": None}, {"counts": None}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769},
                {"rs": W - 1}, {"ps": (H - 1) * rs + W - 1}, {"T": 0}, {"T": 255}, {"k_bg": -1}, {"k_bg": 17}, {"k_fg": -1},
                {"k_fg": 17}, {"rgb": view.data_ptr() + 2}, {"bg": _ptr(bg, b0) + 1}, {"counts": _ptr(counts, c0) + 1},
                {"init": 0, "T": 0}, {"init": 0, "k_fg": 17}):
        v = dict(good, **bad)
        assert lib.hip().dcvc_motion_step(*[v[k] for k in order], U.stream(DEV)) == -1, bad
    torch.cuda.synchronize(DEV)
    assert (U.words(bg) == SENTINEL).all() and (U.words(counts) == SENTINEL).all()
    assert lib.hip().dcvc_motion_step(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    _check(bg, b0, H * W, R.init(R.pictures(H, W)["random0"])[0], "init")


def test_motion_scan_reads_a_crop_in_place_and_keeps_the_order():
    H, W = 70, 100
    pics = R.sequences(H, W)["random"]
    p = M.MotionParams(24, learn=(4, 8))
    scan = M.MotionScan(DEV, H, W, len(pics), p)
    assert scan.grid == R.grid(H, W) and scan.bg.dtype == torch.uint16 and tuple(scan.cells.shape) == (4, 64)
    for pic in pics:
        wide = torch.full((1, 3, 128, 256), float("nan"), device=DEV)  # (the padding is never read: a NaN there would show)
        wide[0, :, :H, :W] = torch.from_numpy(pic).to(DEV)
        scan.add(wide)
    want = R.run(pics, 24, 4, 8)
    got = scan.counts()
    assert got.shape == (4, 8, 8) and got.dtype == np.int32
    assert np.array_equal(got, np.stack([c for _, c in want])) and not got[0].any() and got[1:].any()
    assert np.array_equal(scan.bg.cpu().numpy().astype(np.int64), want[-1][0])
    with pytest.raises(ValueError, match="of a scan of 4 pictures"):
        scan.add(wide)
    fresh = M.MotionScan("cuda", H, W, 2, p)
    with pytest.raises(ValueError, match="no CPU fallback"):
        fresh.add(wide.cpu())
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.MotionScan("cpu", H, W, 2, p)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="the scan on"):
            fresh.add(wide.to("cuda:1"))
    else:
        with pytest.raises(ValueError, match="the scan on"):  # (the check itself, with the scan's device swapped for another)
            other = M.MotionScan(DEV, H, W, 2, p)
            other.device = torch.device("cuda", 1)
            other.add(wide)
    for bad in (wide[0], wide[:, :2], wide.double(), wide[..., :H - 1, :], wide[..., :W - 1]):
        with pytest.raises(ValueError, match="expected a"):
            fresh.add(bad)
    assert fresh.n == 0
    with pytest.raises(ValueError, match="MotionParams"):
        M.MotionScan(DEV, H, W, 2, (24, 4, 8))


# -------------------------------------------------------------------------------------------------------- end to end
def _on_device(pics):
    return (torch.from_numpy(np.ascontiguousarray(p[None])).to(DEV) for p in pics)


@pytest.mark.parametrize("size", [(128, 192), (70, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_static_camera_clip_end_to_end(size):
    H, W = size
    p = M.MotionParams(threshold=24)
    pics, rects = R.clip(H, W)
    got = M.scan(_on_device(pics), len(pics), (H, W), DEV, p)
    want = R.clip_boxes(pics, 24)
    assert len(got) == len(want) == R.CLIP_FRAMES
    for t in range(R.CLIP_FRAMES):
        assert got[t].dtype == np.int32 and np.array_equal(got[t], want[t]), (t, got[t].tolist(), want[t].tolist())
    assert len(got[0]) == 0
    for t in range(1, R.CLIP_FRAMES):
        assert R.covered(rects[t], got[t]), (t, rects[t], got[t].tolist())
    still = M.scan(_on_device(R.clip(H, W, rectangle=False)[0]), R.CLIP_FRAMES, (H, W), DEV, p)
    assert all(len(b) == 0 for b in still)
    with pytest.raises(ValueError, match="saw 3 pictures of 6"):
        M.scan(_on_device(pics[:3]), R.CLIP_FRAMES, (H, W), DEV, p)


# ------------------------------------------------------------------------------------------------------- command line
CH, CW, GOP = 70, 100, 3


def _coords(folder, per_frame):
    os.makedirs(folder)
    for t, rows in enumerate(per_frame):
        with open(os.path.join(folder, "%05d" % (t + 1)), "wb") as f:
            pickle.dump(np.array(rows, dtype=np.uint16).reshape(-1, 4), f)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """the clip as PNGs, and the root `run_codec boxes` makes of it"""
    from PIL import Image

    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("motion_cli")
    u8 = np.rint(R.clip(CH, CW)[0] * 255).astype(np.uint8)
    os.makedirs(tmp / "png")
    for t, a in enumerate(u8):
        Image.fromarray(a.transpose(1, 2, 0)).save(tmp / "png" / f"im{t + 1:05d}.png")
    RC.main(["boxes", "--frames", str(tmp / "png"), "--out", str(tmp / "root"), "--threshold", "24"])
    return dict(tmp=tmp, pics=u8.astype(F32) / F32(255.0))


def test_boxes_command_writes_the_boxes_of_the_api(cli, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp, pics = cli["tmp"], cli["pics"]
    p = M.MotionParams(24)
    api = M.scan(_on_device(pics), len(pics), (CH, CW), DEV, p)
    assert [b.tolist() for b in api] == [b.tolist() for b in R.clip_boxes(pics, 24)] and sum(len(b) for b in api) >= 5
    src = X.PickleBoxes(str(tmp / "root"))
    assert src.names == ("liplates", "faces", "motion")
    for t, b in enumerate(api):
        with open(tmp / "root" / "motion_coords" / ("%05d" % (t + 1)), "rb") as f:
            raw = pickle.load(f)
        assert raw.dtype == np.uint16 and raw.reshape(-1, 4).tolist() == b.tolist(), t
        assert src(t).array.tolist() == [row + [2] for row in b.tolist()]
    assert M.read_info(str(tmp / "root")) == (p, CH, CW, len(pics))
    # other parameters reach the scan; the printed line counts frames and boxes
    capsys.readouterr()
    RC.main(["boxes", "--frames", str(tmp / "png"), "--out", str(tmp / "root2"), "--threshold", "24", "--learn", "0", "16",
             "--min-pixels", "150", "--grow", "0", "--min-cells", "1", "--max-boxes", "1"])
    p2 = M.MotionParams(24, learn=(0, 16), min_pixels=150, grow=0, max_boxes=1)
    want = R.clip_boxes(pics, 24, learn=(0, 16), min_pixels=150, grow=0, max_boxes=1)
    assert M.read_info(str(tmp / "root2"))[0] == p2 and all(len(b) <= 1 for b in want) and any(len(b) for b in want)
    assert [X.PickleBoxes(str(tmp / "root2"))(t).array[:, :4].tolist() for t in range(len(pics))] == [b.tolist() for b in want]
    assert f"{len(pics)} pictures, {sum(len(b) for b in want)} boxes" in capsys.readouterr().out
    # a rerun with another clip length is refused through ap.error
    os.makedirs(tmp / "short")
    for t in range(2):
        os.link(tmp / "png" / f"im{t + 1:05d}.png", tmp / "short" / f"im{t + 1:05d}.png")
    with pytest.raises(SystemExit) as ex:
        RC.main(["boxes", "--frames", str(tmp / "short"), "--out", str(tmp / "root"), "--threshold", "24"])
    assert ex.value.code == 2 and "another run" in capsys.readouterr().err


def test_encode_and_decode_with_the_motion_class(cli, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = cli["tmp"]
    common = ["--gop", str(GOP), "--roi-root", str(tmp / "root")]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "bins"), "--recon", str(tmp / "rec"), "--motion-q", "0.5",
             "--background-q", "2.0"] + common)
    assert json.loads((tmp / "bins" / "roiq.json").read_text()) == \
        {"cell": 16, "background": 200, "classes": {"liplates": 100, "faces": 100, "motion": 50}, "grow": 0}
    RC.main(["decode", "--bins", str(tmp / "bins"), "--recon", str(tmp / "dec"), "--height", str(CH), "--width", str(CW)] + common)
    names = sorted(os.listdir(tmp / "rec"))
    assert len(names) == R.CLIP_FRAMES and sorted(os.listdir(tmp / "dec")) == names
    for name in names:
        assert (tmp / "dec" / name).read_bytes() == (tmp / "rec" / name).read_bytes(), name
    # the boxes decide bits: the same factors on a root whose motion boxes are all empty code other bytes
    _coords(tmp / "empty" / "motion_coords", [[]] * R.CLIP_FRAMES)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "flat"), "--motion-q", "0.5", "--background-q", "2.0",
             "--gop", str(GOP), "--roi-root", str(tmp / "empty")])
    assert list(U.bins(tmp / "flat")) == list(U.bins(tmp / "bins")) and U.bins(tmp / "flat") != U.bins(tmp / "bins")


def test_a_root_without_motion_coords_codes_the_bytes_it_did(cli, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = cli["tmp"]
    plates = [[[8 + 4 * t, 10, 60 + 4 * t, 40]] for t in range(R.CLIP_FRAMES)]
    _coords(tmp / "old" / "liplates_coords", plates)
    _coords(tmp / "new" / "liplates_coords", plates)
    _coords(tmp / "new" / "motion_coords", [[]] * R.CLIP_FRAMES)
    base = ["encode", "--frames", str(tmp / "png"), "--gop", str(GOP), "--plate-q", "0.6"]
    RC.main(base + ["--bins", str(tmp / "old_bins"), "--roi-root", str(tmp / "old")])
    RC.main(base + ["--bins", str(tmp / "new_bins"), "--roi-root", str(tmp / "new"), "--motion-q", "1.0"])
    assert U.bins(tmp / "old_bins") == U.bins(tmp / "new_bins") and len(U.bins(tmp / "old_bins")) == R.CLIP_FRAMES
    assert json.loads((tmp / "old_bins" / "roiq.json").read_text())["classes"] == {"liplates": 60, "faces": 100}
    assert json.loads((tmp / "new_bins" / "roiq.json").read_text())["classes"] == {"liplates": 60, "faces": 100, "motion": 100}
    assert sorted(os.listdir(tmp / "old_bins")) == sorted(os.listdir(tmp / "new_bins"))
    for argv in (base + ["--bins", str(tmp / "x"), "--roi-root", str(tmp / "old"), "--motion-q", "0.5"],
                 base + ["--bins", str(tmp / "x"), "--roi-root", str(tmp / "old"), "--motion-border", "4"],
                 ["decode", "--bins", str(tmp / "old_bins"), "--recon", str(tmp / "x"), "--height", str(CH), "--width", str(CW),
                  "--roi-root", str(tmp / "old"), "--motion-border", "4"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(argv)
        assert ex.value.code == 2 and "--motion-q" in capsys.readouterr().err
    assert not (tmp / "x").exists()
