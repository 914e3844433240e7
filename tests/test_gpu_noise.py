"""The noise estimate on a real MI355X: both kernels bit for bit against the numpy restatement (tests/noise_ref.py) through
the C ABI -- contiguous and strided, offset, NaN-surrounded pictures with guarded outputs -- their refusals, NoiseScan, and
the file loops: encode --tnr-auto codes the bytes of encode --tnr T with the restatement's T."""
import json

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import noise_ref as R
from tests import yuv_ref as Y
from tests.gpu_util import file_nets  # noqa: F401 (a fixture)
from vcm_ts_amd import lib
from vcm_ts_amd import noise as NS
from vcm_ts_amd import tnr as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
WORD, BYTE = 0xABCD1234, 0xA5


def _pictures(H, W, seed=0):
    """Two pictures a little apart, values beyond [0, 1] among them."""
    g = np.random.default_rng(1000 * H + W + seed)
    a = g.uniform(-0.05, 1.05, (3, H, W)).astype(F32)
    return a, (a + g.normal(0.0, 0.03, (3, H, W))).astype(F32)


def _cells(view, rs, ps, H, W, yprev, slack=4, shift=0):
    """One dcvc_noise_cells call into guarded outputs -> (ycur (H, W), the words (hc, wc)), everything around them checked."""
    hc, wc = R.grid(H, W)
    ys = -(-W // 4) * 4 + slack
    ybuf, y0 = U.guarded(H * ys, 4 * shift, np.uint8, BYTE, DEV)
    cbuf, c0 = U.guarded(hc * wc, shift, np.uint32, WORD, DEV)
    pbuf = None
    if yprev is not None:  # the previous picture's plane, with the same stride
        plane = np.full((H, ys), 0x5A, dtype=np.uint8)
        plane[:, :W] = yprev
        pbuf = U.to_dev(plane, DEV)
    lib.check(lib.hip().dcvc_noise_cells(view.data_ptr(), rs, ps, H, W, pbuf.data_ptr() if pbuf is not None else None,
                                         ybuf.data_ptr() + y0, ys, cbuf.data_ptr() + 4 * c0, U.stream(DEV)), "noise_cells")
    rows = U.words(ybuf)[y0:y0 + H * ys].reshape(H, ys)
    assert (rows[:, W:] == BYTE).all() and U.guards_intact(ybuf, y0, H * ys, BYTE)  # the slack bytes beyond column W; the guards
    assert U.guards_intact(cbuf, c0, hc * wc, WORD)  # the words beyond hc * wc
    if pbuf is not None:
        assert np.array_equal(pbuf.cpu().numpy()[:, :W], yprev) and (pbuf.cpu().numpy()[:, W:] == 0x5A).all()  # (only read)
    return rows[:, :W], U.words(cbuf)[c0:c0 + hc * wc].reshape(hc, wc)


# ------------------------------------------------------------------------------------------------- dcvc_noise_cells
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cells_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    prev, cur = _pictures(H, W)
    yprev, none = R.cell_words(prev, None)
    want_y, want = R.cell_words(cur, yprev)
    assert ((want != R.NONE).sum() == (H // 16) * (W // 16)) and (none == R.NONE).all()
    # contiguous (16-byte loads); strided and offset by an odd count inside NaN (4-byte loads), another output alignment
    for n, (row_pad, plane_pad, offset, shift) in enumerate([(0, 0, 0, 0), (5, 23, 13, 1), (8, 24, 12, 3)]):
        view, rs, ps = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)[1:4]
        got_y, got = _cells(view, rs, ps, H, W, yprev.astype(np.uint8), slack=4 * (n % 2), shift=shift)
        assert np.array_equal(got_y, want_y), (size, n)
        assert np.array_equal(got, want), (size, n)
        first_y, first = _cells(view, rs, ps, H, W, None, slack=4, shift=shift)  # yprev = NULL: all NONE, a correct ycur
        assert np.array_equal(first_y, want_y) and (first == R.NONE).all(), (size, n)


def test_cells_kernel_codes_a_nan_as_zero_and_reaches_the_extremes():
    H, W = 64, 96
    prev, cur = _pictures(H, W, 1)
    cur[:, 5, 7] = np.nan
    cur[1, 40, 90] = np.nan
    yprev = R.luma(prev)
    want_y, want = R.cell_words(cur, yprev)
    assert want_y[5, 7] == 0
    got_y, got = _cells(U.to_dev(cur, DEV), W, H * W, H, W, yprev.astype(np.uint8))
    assert np.array_equal(got_y, want_y) and np.array_equal(got, want)
    # cur = 1 against prev = 0: m = l = 65280 in every full cell; cur == prev: m = 0
    H, W = 48, 80
    ones = np.ones((3, H, W), dtype=F32)
    got_y, got = _cells(U.to_dev(ones, DEV), W, H * W, H, W, np.zeros((H, W), dtype=np.uint8))
    assert (got_y == 255).all() and (got[:3, :5] == ((65280 >> 12) << 16 | 65280)).all() and (got[3:] == R.NONE).all() and \
        (got[:, 5:] == R.NONE).all()
    assert np.array_equal(got, R.cell_words(ones, np.zeros((H, W), dtype=np.int64))[1])
    got_y, got = _cells(U.to_dev(ones, DEV), W, H * W, H, W, np.full((H, W), 255, dtype=np.uint8))
    assert (got[:3, :5] == (15 << 16)).all()


def test_two_consecutive_calls_ping_pong_the_planes():
    H, W = 33, 50
    hc, wc = R.grid(H, W)
    g = np.random.default_rng(5)
    pics = [g.uniform(0, 1, (3, H, W)).astype(F32) for _ in range(3)]
    want = R.run(pics)
    ys = 52
    planes = [torch.full((H, ys), BYTE, dtype=torch.uint8, device=DEV) for _ in range(2)]
    cells = torch.zeros((3, hc * wc), dtype=torch.int32, device=DEV)
    for t, p in enumerate(pics):
        x = U.to_dev(p, DEV)
        lib.check(lib.hip().dcvc_noise_cells(x.data_ptr(), W, H * W, H, W, planes[(t - 1) % 2].data_ptr() if t else None,
                                             planes[t % 2].data_ptr(), ys, cells[t].data_ptr(), U.stream(DEV)), "noise_cells")
    assert np.array_equal(U.words(cells).reshape(3, hc, wc), np.stack([w for _, w in want]))
    assert np.array_equal(planes[0].cpu().numpy()[:, :W], want[2][0]) and np.array_equal(planes[1].cpu().numpy()[:, :W], want[1][0])


def test_cells_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    keep, view, rs, ps = U.strided(_pictures(H, W)[0], H, W, 8, 24, 12, DEV)[:4]
    ybuf, y0 = U.guarded(H * 100, 0, np.uint8, BYTE, DEV)
    pbuf, p0 = U.guarded(H * 100, 0, np.uint8, BYTE, DEV)
    cbuf, c0 = U.guarded(hc * wc, 0, np.uint32, WORD, DEV)
    good = dict(rgb=view.data_ptr(), rs=rs, ps=ps, H=H, W=W, yprev=pbuf.data_ptr() + p0, ycur=ybuf.data_ptr() + y0, ys=100,
                cells=cbuf.data_ptr() + 4 * c0)
    order = ("rgb", "rs", "ps", "H", "W", "yprev", "ycur", "ys", "cells")
    for bad in ({"rgb": None}, {"ycur": None}, {"cells": None}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"rs": W - 1},
                {"ps": (H - 1) * rs + W - 1}, {"ys": 96}, {"ys": 102}, {"rgb": good["rgb"] + 2}, {"ycur": good["ycur"] + 1},
                {"ycur": good["ycur"] + 2}, {"yprev": good["yprev"] + 2}, {"cells": good["cells"] + 2}, {"ycur": good["yprev"]}):
        v = dict(good, **bad)
        assert lib.hip().dcvc_noise_cells(*[v[k] for k in order], U.stream(DEV)) == -1, bad
    torch.cuda.synchronize(DEV)
    assert (U.words(ybuf) == BYTE).all() and (U.words(pbuf) == BYTE).all() and (U.words(cbuf) == WORD).all()
    assert lib.hip().dcvc_noise_cells(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    torch.cuda.synchronize(DEV)
    assert (U.words(cbuf)[c0:c0 + hc * wc] != WORD).all() and U.guards_intact(cbuf, c0, hc * wc, WORD)


# -------------------------------------------------------------------------------------------------- dcvc_noise_hist
GUARD = 256  # counters around the histogram


def _hist_buffer():
    return torch.full((GUARD + NS.COUNTERS + GUARD,), 7, dtype=torch.int32, device=DEV)


def _add(buf, words):
    w = U.to_dev(np.asarray(words, dtype=np.uint32).view(np.int32), DEV) if len(words) else torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(lib.hip().dcvc_noise_hist(w.data_ptr(), len(words), buf.data_ptr() + 4 * GUARD, U.stream(DEV)), "noise_hist")


def _counters(buf):
    got = U.words(buf)
    assert (got[:GUARD] == 7).all() and (got[GUARD + NS.COUNTERS:] == 7).all()  # the guard band around the 8192 counters
    return got[GUARD:GUARD + NS.COUNTERS].reshape(16, 512) - 7


@pytest.mark.parametrize("n", [0, 1, 255, 257, 8192])
def test_hist_kernel_counts_equal_words_into_one_bin(n):
    buf = _hist_buffer()
    _add(buf, [(9 << 16) | 325] * n)
    want = np.zeros((16, 512), dtype=np.int64)
    want[9, 20] = n
    assert np.array_equal(_counters(buf), want)


def test_hist_kernel_skips_adds_and_saturates_the_column():
    g = np.random.default_rng(11)
    words = ((g.integers(0, 16, 5000) << 16) | g.integers(0, 9000, 5000)).astype(np.int64)
    words[::7] = R.NONE
    words[3::11] = (16 << 16) | 40          # an upper half of 16: skipped
    words[5::13] = (0xFFFE << 16) | 40      # ... and of 0xFFFE
    words[1::17] = (4 << 16) | 33           # many cells in few bins, beside the spread-out ones
    words[:3] = [(2 << 16) | 8175, (2 << 16) | 8176, (2 << 16) | 65280]  # column 510, and twice column 511
    want = R.hist_add(np.zeros((16, 512), dtype=np.int64), words)
    assert want[2, 511] >= 2 and want[2, 510] >= 1 and want.sum() < 5000 and (want > 0).sum() > 1000
    buf = _hist_buffer()
    _add(buf, words)
    assert np.array_equal(_counters(buf), want)
    more = words[::-1][:1234]
    _add(buf, more)  # a second launch adds to the first
    assert np.array_equal(_counters(buf), R.hist_add(want.copy(), more))
    buf = _hist_buffer()
    _add(buf, [R.NONE] * 300)
    assert not _counters(buf).any()
    # more words than one round of all workgroups takes: 256 workgroups x 256 threads
    many = ((g.integers(1, 15, 200000) << 16) | g.integers(0, 64, 200000)).astype(np.int64)
    buf = _hist_buffer()
    _add(buf, many)
    assert np.array_equal(_counters(buf), R.hist_add(np.zeros((16, 512), dtype=np.int64), many))


def test_hist_refusals_leave_the_counters_alone():
    buf = _hist_buffer()
    w = torch.zeros(64, dtype=torch.int32, device=DEV)
    good = (w.data_ptr(), 64, buf.data_ptr() + 4 * GUARD)
    for bad in ((None, 64, good[2]), (good[0], 64, None), (good[0], -1, good[2]), (good[0], (1 << 28) + 1, good[2]),
                (good[0] + 2, 60, good[2]), (good[0], 64, good[2] + 2)):
        assert lib.hip().dcvc_noise_hist(*bad, U.stream(DEV)) == -1, bad
    torch.cuda.synchronize(DEV)
    assert (U.words(buf) == 7).all()
    assert lib.hip().dcvc_noise_hist(*good, U.stream(DEV)) == 0
    assert _counters(buf)[0, 0] == 64 and _counters(buf).sum() == 64


# ---------------------------------------------------------------------------------------------------------- NoiseScan
H, W, FRAMES, GOP = 64, 96, 5, 4
BH, BW, BN = 164, 176, 3  # the report's clip: MS-SSIM's five levels need sides beyond 160


def _clip(h=H, w=W, n=FRAMES, s=2.0):
    return R.clip(h, w, n, s, obj=(12, 12))


def test_noise_scan_equals_the_restatements_histogram():
    pics = _clip()
    want = R.histogram(pics)
    assert want.sum() == 4 * 24

    def scan_of(batch, fold_at=None):
        scan = NS.NoiseScan(DEV, H, W, batch=batch)
        if fold_at is not None:
            scan._fold_at = fold_at
        for p in pics:
            wide = torch.full((1, 3, 128, 128), float("nan"), device=DEV)  # (the padding is never read: a NaN there would show)
            wide[0, :, :H, :W] = U.to_dev(p, DEV)
            scan.add(wide)
        return scan

    scan = scan_of(2)
    got = scan.histogram()
    assert got.shape == (16, 512) and got.dtype == np.int64 and np.array_equal(got, want)
    assert (scan.n, scan.pairs, scan.filled, scan.grid, scan.y_stride) == (5, 4, 0, (4, 8), 96) and np.array_equal(scan.histogram(), want)
    assert np.array_equal(scan_of(64).histogram(), want) and np.array_equal(scan_of(1).histogram(), want)
    assert np.array_equal(scan_of(2, fold_at=2).histogram(), want)  # the device counters folded into the host's on the way
    with torch.cuda.stream(torch.cuda.Stream(DEV)):  # a scan made on one stream and used on another
        other = scan_of(2)
    assert np.array_equal(other.histogram(), want)
    est = NS.estimate(got, 16, scan.pairs)
    assert est.to_json() == R.estimate(want, 16, 4) and est.mad32 is not None
    fresh = NS.NoiseScan("cuda", H, W)
    with pytest.raises(ValueError, match="no CPU fallback"):
        fresh.add(torch.zeros(1, 3, H, W))
    for bad in (torch.zeros(3, H, W, device=DEV), torch.zeros(1, 3, H - 1, W, device=DEV), torch.zeros(1, 3, H, W, device=DEV).double()):
        with pytest.raises(ValueError, match="expected a"):
            fresh.add(bad)
    with pytest.raises(ValueError, match="batch"):
        NS.NoiseScan(DEV, H, W, batch=0)
    assert fresh.n == 0 and not fresh.histogram().any()


# --------------------------------------------------------------------------------------------------------- file loops
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The noisy clip as a PNG folder and, through the restatement's RGB -> 4:2:0, as a Y4M file whose pictures the
    restatement converts back; a noise-free folder; the larger clip of the report."""
    tmp = tmp_path_factory.mktemp("noise")
    pics = _clip()
    U.write_pngs(str(tmp / "png"), pics)
    U.write_pngs(str(tmp / "clean"), R.clip(H, W, FRAMES, 0.0, obj=None))
    planes = [tuple(p.astype(np.uint8) for p in Y.from_rgb(pic)) for pic in pics]
    Y.write_y4m(str(tmp / "src.y4m"), planes, W, H)
    big = _clip(BH, BW, BN)
    U.write_pngs(str(tmp / "big"), big)
    return dict(tmp=tmp, png=R.record(pics, 3.0, 16), y4m=R.record([Y.to_rgb(*p) for p in planes], 3.0, 16), big=R.record(big, 3.0, 16))


def test_encode_tnr_auto_codes_the_bytes_of_the_restatements_threshold(clip, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, want = clip["tmp"], clip["png"]
    T = want["threshold"]
    assert 1 < T < 64 and want["mad32"] is not None and want["cells"] == 96 and want["pairs"] == 4
    auto = N.AutoTNR(min_cells=16, search=4)
    plain, size = RC.encode_folder(str(tmp / "png"), str(tmp / "given"), gop=GOP, nets=file_nets, tnr=N.TNR(T, search=4))
    bits, _ = RC.encode_folder(str(tmp / "png"), str(tmp / "auto"), gop=GOP, nets=file_nets, tnr=auto)
    two, _ = RC.encode_folder(str(tmp / "png"), str(tmp / "two"), gop=GOP, nets=file_nets, tnr=auto, gop_streams=2, scenecut=0.99)
    assert size == (H, W) and bits == plain == two and len(bits) == FRAMES
    assert U.bins(tmp / "auto") == U.bins(tmp / "given") == U.bins(tmp / "two")
    assert json.loads((tmp / "auto" / "noise.json").read_text()) == want == json.loads((tmp / "two" / "noise.json").read_text())
    assert U.others(tmp / "auto") == ["noise.json"] and U.others(tmp / "two") == ["gops.json", "noise.json"]
    assert U.others(tmp / "given") == []  # an encode with neither option writes no noise.json
    # another scale resolves to another threshold and other bytes
    other = R.record(_clip(), 8.0, 16)
    assert other["threshold"] > T
    RC.encode_folder(str(tmp / "png"), str(tmp / "auto"), gop=GOP, nets=file_nets, tnr=N.AutoTNR(8.0, min_cells=16, search=4))
    assert json.loads((tmp / "auto" / "noise.json").read_text()) == other and U.bins(tmp / "auto") != U.bins(tmp / "given")


def test_encode_video_tnr_auto_measures_the_converted_pictures(clip, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, want = clip["tmp"], clip["y4m"]
    assert want["mad32"] is not None
    plain, size = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "v_given"), gop=GOP, nets=file_nets, tnr=N.TNR(want["threshold"]))
    bits, _ = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "v_auto"), gop=GOP, nets=file_nets, tnr=N.AutoTNR(min_cells=16))
    assert size == (H, W) and bits == plain and U.bins(tmp / "v_auto") == U.bins(tmp / "v_given")
    assert json.loads((tmp / "v_auto" / "noise.json").read_text()) == want
    assert U.others(tmp / "v_auto") == ["noise.json", "sequence.json"] and U.others(tmp / "v_given") == ["sequence.json"]


def test_report_carries_the_estimate_and_the_resolved_setting(clip, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, want = clip["tmp"], clip["big"]
    bits, size, rd = RC.encode_folder(str(tmp / "big"), str(tmp / "big_auto"), gop=GOP, nets=file_nets, report=str(tmp / "big.json"),
                                      tnr=N.AutoTNR(2.0, min_cells=16, pixel=9))
    assert size == (BH, BW) and len(bits) == BN
    want = dict(want, scale=2.0, threshold=R.auto_threshold(want["mad32"], 2.0), pixel=9)
    assert rd["noise"] == want and rd["tnr"] == N.TNR(want["threshold"], pixel=9).to_json()
    assert json.loads((tmp / "big.json").read_text())["noise"] == want == json.loads((tmp / "big_auto" / "noise.json").read_text())
    assert len(rd["frame_tnr_held"]) == BN and rd["frame_tnr_held"][1] > 0


def test_command_line(clip, file_nets, monkeypatch, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = clip["tmp"]
    monkeypatch.setattr(RC, "_nets", lambda *a, **k: file_nets[0])
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr-auto",
             "--tnr-auto-min-cells", "16"])
    RC.encode_folder(str(tmp / "png"), str(tmp / "cli_given"), gop=GOP, nets=file_nets, tnr=N.TNR(clip["png"]["threshold"]))
    assert U.bins(tmp / "cli") == U.bins(tmp / "cli_given") and json.loads((tmp / "cli" / "noise.json").read_text()) == clip["png"]
    # run_codec noise prints the same estimate, from the folder and from the file
    capsys.readouterr()
    RC.main(["noise", "--frames", str(tmp / "png"), "--min-cells", "16", "--out", str(tmp / "noise_out.json")])
    assert json.loads(capsys.readouterr().out) == clip["png"] == json.loads((tmp / "noise_out.json").read_text())
    RC.main(["noise", "--video", str(tmp / "src.y4m"), "--min-cells", "16"])
    assert json.loads(capsys.readouterr().out) == clip["y4m"]
    RC.main(["noise", "--frames", str(tmp / "png"), "--min-cells", "16", "--scale", "8", "--max-frames", "3"])
    assert json.loads(capsys.readouterr().out) == R.record(_clip()[:3], 8.0, 16)
    # a noise-free clip is refused by name: by the command, by encode, and by the file loop
    for argv in (["noise", "--frames", str(tmp / "clean"), "--min-cells", "16"],
                 ["encode", "--frames", str(tmp / "clean"), "--bins", str(tmp / "refused"), "--tnr-auto", "--tnr-auto-min-cells", "16"]):
        with pytest.raises((SystemExit, ValueError)) as ex:
            RC.main(argv)
        text = capsys.readouterr().err + str(ex.value)
        assert "too few counted cells: 0 of 16" in text and "--tnr T" in text and getattr(ex.value, "code", 2) != 0, argv
    assert not (tmp / "refused").exists() or U.bins(tmp / "refused") == {}
