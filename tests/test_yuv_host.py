"""Y4M / raw YUV files and the colour description without a GPU: the readers and writers, sequence.json, the command
line's refusals, the host-only coefficient entry point -- and the check that the caps tests/test_gpu_yuv.py grants the
kernels against the float64 restatement can be met by correct fp32 code at all: the float32 restatement
(tests/yuv_ref.py), on the very inputs the GPU tests use, stays within HALF of each."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import yuv_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import yuv as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# caps of the GPU tests (kernel against the float64 restatement); here the fp32 restatement must stay within half
CAP_RGB = 1e-6       # unrounded RGB, absolute
CAP_CODES = 1e-4     # share of quantize8 codes that may differ (by 1)
CAP_SAMPLES = 2e-4   # share of the samples of each plane that may differ (by 1)


def _frames(n, h, w, depth=8, seed=5):
    return [R.random_planes(seed + t, h, w, depth) for t in range(n)]


# ------------------------------------------------------------------------------------------------------------ files
@pytest.mark.parametrize("chroma,depth,siting", [("420", 8, "left"), ("420jpeg", 8, "center"), ("420mpeg2", 8, "left"),
                                                 ("420paldv", 8, "left"), ("420p10", 10, "left")])
def test_y4m_reader_accepts_every_supported_chroma_tag_and_reads_by_index(tmp_path, chroma, depth, siting):
    frames = _frames(5, 6, 10, depth)
    path = str(tmp_path / "a.y4m")
    R.write_y4m(path, frames, 10, 6, chroma=chroma, fps="30000:1001")
    with Y.Y4MReader(path) as r:
        assert (r.width, r.height, r.n_frames, r.bit_depth, r.siting, r.fps) == (10, 6, 5, depth, siting, (30000, 1001))
        assert r.full_range is None and r.spec() == Y.ColorSpec("bt709", False, siting, depth)
        assert r.spec("bt601", True, "center") == Y.ColorSpec("bt601", True, "center", depth)
        buf = np.empty(r.frame_bytes, np.uint8)
        for k in (3, 0, 4, 1, 2):  # any order: frames sit at a fixed stride
            r.read_into(k, buf)
            want = R.to_i420(frames[k]).astype("<u2" if depth == 10 else np.uint8).tobytes()
            assert buf.tobytes() == want, k
        with pytest.raises(IndexError):
            r.read_into(5, buf)
        with pytest.raises(ValueError):
            r.read_into(0, np.empty(r.frame_bytes - 1, np.uint8))


def test_y4m_reader_fills_a_torch_tensor_in_place(tmp_path):
    frames = _frames(2, 4, 4)
    path = str(tmp_path / "a.y4m")
    R.write_y4m(path, frames, 4, 4)
    with Y.Y4MReader(path) as r:
        t = torch.zeros(r.frame_bytes, dtype=torch.uint8)
        r.read_into(1, t.numpy())
        assert np.array_equal(t.numpy(), R.to_i420(frames[1]))


@pytest.mark.parametrize("extra,full", [("XCOLORRANGE=FULL", True), ("XCOLORRANGE=LIMITED", False), ("XYSCSS=420JPEG", None)])
def test_y4m_colour_range_extension(tmp_path, extra, full):
    path = str(tmp_path / "a.y4m")
    R.write_y4m(path, _frames(1, 4, 4), 4, 4, extra=extra)
    with Y.Y4MReader(path) as r:
        assert r.full_range is full
        assert r.spec().full_range is bool(full)


@pytest.mark.parametrize("kw,word", [
    (dict(chroma="422"), "C422"), (dict(chroma="444"), "C444"), (dict(chroma="mono"), "Cmono"), (dict(chroma="420p12"), "C420p12"),
    (dict(chroma="444p10"), "C444p10"), (dict(interlace="t"), "interlaced"), (dict(interlace="b"), "interlaced"),
    (dict(interlace="m"), "interlaced"), (dict(frame_line=b"FRAME Ip\n"), "FRAME line with parameters"),
    (dict(extra="XCOLORRANGE=WIDE"), "XCOLORRANGE"),
])
def test_y4m_reader_refuses_what_it_does_not_handle_and_names_it(tmp_path, kw, word):
    path = str(tmp_path / "a.y4m")
    R.write_y4m(path, _frames(3, 4, 6), 6, 4, **kw)
    with pytest.raises(ValueError, match=re.escape(word)):
        Y.Y4MReader(path)


def test_y4m_reader_refuses_odd_sizes_truncation_and_other_files(tmp_path):
    path = str(tmp_path / "a.y4m")
    open(path, "wb").write(b"YUV4MPEG2 W5 H4 F25:1 Ip C420\nFRAME\n" + bytes(30))
    with pytest.raises(ValueError, match="even"):
        Y.Y4MReader(path)
    R.write_y4m(path, _frames(3, 4, 6), 6, 4)
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-5])
    with pytest.raises(ValueError, match="truncated"):
        Y.Y4MReader(path)
    open(path, "wb").write(data[:-36 + 3])  # cut inside the last FRAME line's frame
    with pytest.raises(ValueError, match="truncated"):
        Y.Y4MReader(path)
    open(path, "wb").write(b"RIFF....AVI " + bytes(100))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        Y.Y4MReader(path)
    open(path, "wb").write(b"YUV4MPEG2 H4 F25:1\nFRAME\n")
    with pytest.raises(ValueError, match="W or H"):
        Y.Y4MReader(path)


@pytest.mark.parametrize("depth", [8, 10])
def test_writers_round_trip_through_the_readers_in_any_order(tmp_path, depth):
    frames = _frames(4, 6, 8, depth)
    spec = Y.ColorSpec("bt601", True, "center" if depth == 8 else "left", depth)
    flat = [R.to_i420(f).astype("<u2" if depth == 10 else np.uint8) for f in frames]
    y4m, raw = str(tmp_path / "o.y4m"), str(tmp_path / "o.yuv")
    with Y.create_video(y4m, 8, 6, spec, fps=(50, 1)) as wy, Y.create_video(raw, 8, 6, spec) as wr:
        for k in (2, 0, 3, 1):  # GOP streams finish out of order; the file is in display order
            wy.write(k, flat[k])
            wr.write(k, flat[k])
        with pytest.raises(ValueError):
            wy.write(0, flat[0][:-1])
    fields, got = R.read_y4m(y4m)  # (the tests' own reader)
    assert (fields["W"], fields["H"], fields["F"], fields["I"]) == ("8", "6", "50:1", "p")
    assert fields["C"] == ("420p10" if depth == 10 else "420jpeg") and fields["X"] == ["COLORRANGE=FULL"]
    assert all(np.array_equal(a, b) for a, b in zip(got, flat)) and len(got) == 4
    with Y.open_video(y4m) as r:
        assert r.n_frames == 4 and r.spec("bt601") == spec and r.fps == (50, 1)
    assert open(raw, "rb").read() == b"".join(f.tobytes() for f in flat)
    with Y.open_video(raw, size=(8, 6), bit_depth=depth, fps=(50, 1)) as r:
        assert (r.n_frames, r.width, r.height, r.fps) == (4, 8, 6, (50, 1))
        buf = np.empty(r.frame_bytes, np.uint8)
        r.read_into(2, buf)
        assert buf.tobytes() == flat[2].tobytes()


def test_raw_reader_refuses_a_truncated_file_odd_sizes_and_missing_size(tmp_path):
    raw = str(tmp_path / "o.yuv")
    open(raw, "wb").write(bytes(6 * 8 * 3 // 2 * 2 - 1))
    with pytest.raises(ValueError, match="truncated"):
        Y.RawYUVReader(raw, 8, 6)
    with pytest.raises(ValueError, match="even"):
        Y.RawYUVReader(raw, 7, 6)
    with pytest.raises(ValueError, match="size"):
        Y.open_video(raw)
    with pytest.raises(ValueError, match="extension"):
        Y.open_video(str(tmp_path / "o.mp4"))
    with pytest.raises(ValueError, match="chroma tag"):
        Y.Y4MWriter(str(tmp_path / "x.y4m"), 8, 6, Y.ColorSpec(bit_depth=10), chroma="420jpeg")


def test_color_spec_refuses_unknown_values():
    for kw in (dict(matrix="bt2020"), dict(siting="top"), dict(bit_depth=12)):
        with pytest.raises(ValueError):
            Y.ColorSpec(**kw)
    assert Y.ColorSpec.from_json(json.loads(json.dumps(Y.ColorSpec("bt601", True, "center", 10).to_json()))) == \
        Y.ColorSpec("bt601", True, "center", 10)


def test_sequence_json_round_trip(tmp_path):
    from vcm_ts_amd import run_codec as RC

    assert RC.read_sequence_info(str(tmp_path)) is None
    spec = Y.ColorSpec("bt601", True, "center", 8)
    RC.write_sequence_info(str(tmp_path), 322, 180, 17, 8, (30000, 1001), spec, "y4m", chroma="420jpeg", interlace="p", aspect="1:1")
    info = RC.read_sequence_info(str(tmp_path))
    assert (info["width"], info["height"], info["frames"], info["gop"], info["fps"]) == (322, 180, 17, 8, (30000, 1001))
    assert info["color"] == spec and info["container"] == "y4m" and info["chroma"] == "420jpeg"
    assert json.load(open(tmp_path / "sequence.json"))["color"] == {"matrix": "bt601", "full_range": True, "siting": "center", "bit_depth": 8}


@pytest.mark.parametrize("argv", [
    ["encode", "--bins", "b"],                                                   # neither --frames nor --video
    ["encode", "--bins", "b", "--frames", "f", "--video", "x.y4m"],              # both
    ["encode", "--bins", "b", "--video", "x.yuv"],                               # raw file without --size
    ["encode", "--bins", "b", "--video", "x.yuv", "--size", "1920"],             # malformed size
    ["encode", "--bins", "b", "--video", "x.mkv"],                               # a container
    ["encode", "--bins", "b", "--frames", "f", "--recon-video", "r.y4m"],        # video output of the PNG path
    ["encode", "--bins", "b", "--video", "x.y4m", "--matrix", "bt2020"],
    ["decode", "--bins", "b"],                                                   # neither output
    ["decode", "--bins", "b", "--recon", "r", "--recon-video", "r.y4m"],         # both
    ["decode", "--bins", "b", "--recon-video", "r.y4m"],                         # no sequence.json, no size
    ["decode", "--bins", "b", "--recon", "r"],                                   # as before: size required
])
def test_command_line_refusals(tmp_path, monkeypatch, argv, capsys):
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ex:
        RC.main(argv)
    assert ex.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_video_path_does_not_import_pil():
    import subprocess
    import sys

    code = "import sys; import vcm_ts_amd.run_codec, vcm_ts_amd.yuv; sys.exit(int(any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules)))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ------------------------------------------------------------------------------------------------- the C entry points
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("depth", [8, 10])
def test_color_coeffs_are_the_double_precision_values_rounded_once(matrix, full, depth):
    cc = Y.ColorSpec(matrix, full, "center", depth).coeffs()
    kr, kb = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}[matrix]
    kg = 1.0 - kr - kb
    s, mx = 2.0 ** (depth - 8), 2.0 ** depth - 1
    y_off, y_range, c_range = (0.0, mx, mx) if full else (16 * s, 219 * s, 224 * s)
    want = dict(y_off=y_off, c_off=128 * s, y_scale=1 / y_range, c_scale=1 / c_range, crr=2 * (1 - kr), cbb=2 * (1 - kb),
                cgb=2 * kb * (1 - kb) / kg, cgr=2 * kr * (1 - kr) / kg, kr=kr, kg=kg, kb=kb, icb=1 / (2 * (1 - kb)),
                icr=1 / (2 * (1 - kr)), y_range=y_range, c_range=c_range)
    for name, v in want.items():
        got = np.float32(getattr(cc, name))
        # correctly rounded from (an evaluation of) the double value: within half an fp32 ulp of it, and exactly the
        # restatement's constant
        assert abs(float(got) - v) <= 0.5 * float(np.spacing(np.float32(v))) * (1 + 1e-9), (name, got, v)
        assert got == R.constants(matrix, full, depth, np.float32)[name], name
    assert (cc.max_code, cc.bit_depth, cc.siting, cc.matrix, cc.range) == (int(mx), depth, 1, Y.MATRICES[matrix], int(full))
    # luma weights sum to one and the matrices invert each other in double precision
    assert abs(kr + kg + kb - 1) < 1e-15 and abs(want["crr"] * want["icr"] - 1) < 1e-15


def test_entry_points_refuse_bad_codes_and_shapes_without_a_gpu():
    L = lib.hip()
    cc = lib.ColorCoeffs()
    for args in ((2, 0, 8, 0), (0, 2, 8, 0), (0, 0, 12, 0), (0, 0, 8, 2), (8, 8, 8, 8), (-1, 0, 8, 0)):
        assert L.dcvc_color_coeffs(*args, C.byref(cc)) == -1, args
    assert L.dcvc_color_coeffs(0, 0, 8, 0, None) == -1
    assert L.dcvc_color_coeffs(0, 0, 8, 0, C.byref(cc)) == 0
    p = 0x10000  # an aligned dummy: a refused call returns before anything is launched or dereferenced
    ok = dict(H=64, W=64, ys=64, cs=32, oh=64, ow=64, rs=64, ps=64 * 64)

    def to_rgb(cc_=cc, y=p, rgb=p, **kw):
        a = dict(ok, **kw)
        return L.dcvc_yuv420_to_rgb(y, p, p, a["H"], a["W"], a["ys"], a["cs"], C.byref(cc_) if cc_ is not None else None, rgb,
                                    a["oh"], a["ow"], a["rs"], a["ps"], 0, None)

    def from_rgb(cc_=cc, y=p, sse=None, src=None, **kw):
        a = dict(ok, **kw)
        return L.dcvc_rgb_to_yuv420(p, a["H"], a["W"], a["rs"], a["ps"], C.byref(cc_) if cc_ is not None else None, y, p, p,
                                    a["ys"], a["cs"], src, src, src, a["ys"], a["cs"], sse, None)

    bad = [dict(H=63), dict(W=62 + 1), dict(H=0), dict(W=-2), dict(H=32770, oh=32770), dict(ys=62), dict(cs=31),
           dict(rs=60), dict(ps=64 * 63)]
    for kw in bad:
        assert to_rgb(**kw) == -1, kw
        assert from_rgb(**kw) == -1, kw
    for kw in (dict(oh=62), dict(ow=60), dict(ow=40000, rs=40000, ps=40000 * 64)):
        assert to_rgb(**kw) == -1, kw
    assert to_rgb(cc_=None) == -1 and from_rgb(cc_=None) == -1 and to_rgb(y=None) == -1 and to_rgb(rgb=None) == -1
    assert from_rgb(y=None) == -1
    assert to_rgb(cc_=lib.ColorCoeffs()) == -1 and from_rgb(cc_=lib.ColorCoeffs()) == -1  # a struct nobody filled
    assert from_rgb(sse=p) == -1 and from_rgb(src=p) == -1  # source planes and sums: all or none


def test_python_surface_refuses_without_a_gpu():
    frame = torch.zeros(64 * 64 * 3 // 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        Y.yuv420_to_rgb(frame, 64, 64)
    with pytest.raises(ValueError, match="GPU"):
        Y.rgb_to_yuv420(torch.zeros(1, 3, 64, 64), 64, 64)
    with pytest.raises(ValueError, match="even"):
        Y.yuv420_to_rgb(frame, 63, 64)
    assert Y.psnr_yuv([0, 4, 16], 2, 2, 8)[0] == float("inf")


def test_psnr_yuv_is_the_float64_formula():
    g = np.random.default_rng(3)
    for depth in (8, 10):
        a, b = R.random_planes(1, 8, 12, depth), R.random_planes(2, 8, 12, depth)
        sums, want = R.psnr_yuv(a, b, depth)
        assert Y.psnr_yuv(sums, 8, 12, depth) == pytest.approx(want, rel=1e-14)
    py, pu, pv, pyuv = Y.psnr_yuv([96 * 1, 24 * 4, 24 * 16], 8, 12, 8)
    assert py == pytest.approx(10 * np.log10(255 ** 2 / 1.0)) and pv == pytest.approx(10 * np.log10(255 ** 2 / 16.0))
    assert pyuv == pytest.approx((6 * py + pu + pv) / 8)
    del g


# ------------------------------------------------------------------- the caps can be met: fp32 against fp64 restatement
@pytest.mark.parametrize("kind", ["gamut", "random"])
@pytest.mark.parametrize("case", R.cases(), ids=[c[0] for c in R.cases()])
def test_float32_restatement_stays_within_half_of_each_cap(case, kind):
    name, h, w, col = case
    y, u, v = R.case_planes(name, h, w, col, kind)
    a32, a64 = R.to_rgb(y, u, v, dtype=np.float32, **col), R.to_rgb(y, u, v, dtype=np.float64, **col)
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert float(np.abs(a32.astype(np.float64) - a64).max()) <= CAP_RGB / 2
    q32 = np.rint(R.to_rgb(y, u, v, dtype=np.float32, quantize8=True, **col).astype(np.float64) * 255.0)
    q64 = R.to_rgb(y, u, v, dtype=np.float64, quantize8=True, **col)
    d = np.abs(q32 - q64)
    assert d.max() <= 1 and (d != 0).sum() <= CAP_CODES / 2 * d.size, ((d != 0).sum(), d.size)
    rgb = R.case_rgb(name, h, w, kind)
    for p32, p64 in zip(R.from_rgb(rgb, dtype=np.float32, **col), R.from_rgb(rgb, dtype=np.float64, **col)):
        d = np.abs(p32 - p64)
        assert d.max() <= 1 and (d != 0).sum() <= CAP_SAMPLES / 2 * d.size, ((d != 0).sum(), d.size)


@pytest.mark.parametrize("col", [c[3] for c in R.cases() if c[1:3] == R.MID], ids=[c[0] for c in R.cases() if c[1:3] == R.MID])
def test_luma_round_trips_through_the_float32_restatement(col):
    """samples -> RGB (unrounded) -> samples reproduces every luma sample whose RGB triple was not clamped."""
    h, w = R.MID
    y, u, v = R.gamut_planes(11, h, w, **col)
    back = R.from_rgb(R.to_rgb(y, u, v, dtype=np.float32, **col), dtype=np.float32, **col)[0]
    keep = R.unclamped_mask(y, u, v, **col)
    assert keep.mean() > 0.5
    assert np.array_equal(back[keep], y.astype(np.int64)[keep])


def test_restatements_agree_with_first_principles():
    """A grey ramp has no chroma: R = G = B = (y - 16) / 219, and white / black map to the ends, in both matrices."""
    y = np.arange(16, 236, dtype=np.uint8).reshape(2, 110)
    c = np.full((1, 55), 128, np.uint8)
    for m in ("bt709", "bt601"):
        rgb = R.to_rgb(y, c, c, matrix=m, dtype=np.float64)
        assert np.allclose(rgb, ((y.astype(np.float64) - 16) / 219)[None], atol=1e-15)
        yy, uu, vv = R.from_rgb(np.stack([np.ones((2, 2)), np.zeros((2, 2)), np.zeros((2, 2))]), matrix=m, dtype=np.float64)
        kr = R.MATRIX[m][0]
        assert yy[0, 0] == round(16 + 219 * kr) and vv[0, 0] == 240 and uu[0, 0] == round(128 - 224 * kr / (2 * (1 - R.MATRIX[m][1])))
    # siting: a chroma step between columns 0 and 1 reaches luma column 1 at half (left) or a quarter (center) height
    u = np.array([[0, 160]], np.uint8)
    assert R.upsample16(u, "left")[0].tolist() == [0, 16 * 80, 16 * 160, 16 * 160]
    assert R.upsample16(u, "center")[0].tolist() == [0, 16 * 40, 16 * 120, 16 * 160]
