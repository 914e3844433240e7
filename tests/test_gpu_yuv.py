"""4:2:0 <-> RGB on the device (vcm_ts_amd/yuv.py, csrc/color.hip) and the video path of run_codec built on it.

Kernel tests (K1-K6) compare with tests/yuv_ref.py: BIT equality with the float32 restatement of the header's formulas
is the primary assertion; the float64 restatement guards against the kernel and that restatement sharing a mistake.
Bounds against float64 (from the arithmetic, checked without a GPU by tests/test_yuv_host.py on these very inputs):
unrounded RGB 1e-6 (at most 8 roundings of 2^-23 on magnitudes below 2); quantize8 codes at most 1 apart in at most 1e-4
of the samples; RGB -> samples at most 1 apart in at most 2e-4 of the samples of each plane.

End-to-end tests (E1-E5): the video path codes byte-identical .bin files to the PNG path given the same pictures, its
encoder-side and decoder-side reconstruction files are identical, and the sample-domain PSNR of the report equals
numpy's on the files.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import yuv_ref as R
from vcm_ts_amd import yuv as Y

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP_RGB, CAP_CODES, CAP_SAMPLES = 1e-6, 1e-4, 2e-4
CASES = R.cases()
IDS = [c[0] for c in CASES]


def _spec(col):
    return Y.ColorSpec(col["matrix"], col["full_range"], col["siting"], col["depth"])


def _dev_frame(planes, depth):
    flat = R.to_i420(planes)
    return torch.from_numpy(flat.astype(np.int16) if depth == 10 else flat).to(DEV)


def _host_planes(frame, h, w):
    a = frame.cpu().numpy()
    return R.from_i420(a.view(np.uint16) if a.dtype == np.int16 else a, h, w)


# ------------------------------------------------------------------------------------------------------------ K1, K2
@pytest.mark.parametrize("kind", ["gamut", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_k1_yuv420_to_rgb_unrounded(case, kind):
    from vcm_ts_amd.pipeline import pad_frame

    name, h, w, col = case
    planes = R.case_planes(name, h, w, col, kind)
    out = Y.yuv420_to_rgb(_dev_frame(planes, col["depth"]), h, w, _spec(col))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(pad_frame(torch.empty(1, 3, h, w)).shape)
    got = out.cpu().numpy()[0]
    want32, want64 = R.to_rgb(*planes, dtype=np.float32, **col), R.to_rgb(*planes, dtype=np.float64, **col)
    err = float(np.abs(got[:, :h, :w].astype(np.float64) - want64).max())
    print(name, kind, "max |gpu - fp64|", err, " fp32 restatement", float(np.abs(want32.astype(np.float64) - want64).max()),
          " bit mismatches", int((U.f32_bits(got[:, :h, :w]) != U.f32_bits(want32)).sum()))
    assert np.array_equal(U.f32_bits(got[:, :h, :w]), U.f32_bits(want32))
    assert err <= CAP_RGB
    pad = got.copy()
    pad[:, :h, :w] = 0
    assert not U.f32_bits(pad).any()  # the padding is exactly +0.0
    plain = Y.yuv420_to_rgb(_dev_frame(planes, col["depth"]), h, w, _spec(col), pad=False)
    assert tuple(plain.shape) == (1, 3, h, w) and np.array_equal(U.f32_bits(plain.cpu().numpy()[0]), U.f32_bits(want32))


@pytest.mark.parametrize("kind", ["gamut", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_k2_quantize8(case, kind):
    name, h, w, col = case
    planes = R.case_planes(name, h, w, col, kind)
    got = Y.yuv420_to_rgb(_dev_frame(planes, col["depth"]), h, w, _spec(col), quantize8=True).cpu().numpy()[0]
    want32 = R.to_rgb(*planes, dtype=np.float32, quantize8=True, **col)
    assert np.array_equal(U.f32_bits(got[:, :h, :w]), U.f32_bits(want32))
    table = np.arange(256, dtype=np.float32) / 255.0
    assert np.isin(U.f32_bits(got), U.f32_bits(table)).all()  # padding included: 0.0 is T[0]
    codes = np.rint(got[:, :h, :w].astype(np.float64) * 255.0)
    assert np.array_equal(U.f32_bits(table[codes.astype(np.int64)]), U.f32_bits(got[:, :h, :w]))
    d = np.abs(codes - R.to_rgb(*planes, dtype=np.float64, quantize8=True, **col))
    print(name, kind, "codes differing from fp64", int((d != 0).sum()), "of", d.size)
    assert d.max() <= 1 and (d != 0).sum() <= CAP_CODES * d.size


def test_k1_strided_planes_and_odd_output_sizes():
    h, w = 66, 130
    planes = R.random_planes(9, h, w, 8)
    big = [torch.full((p.shape[0] + 3, p.shape[1] + 7), 77, dtype=torch.uint8, device=DEV) for p in planes]
    big[2] = torch.full_like(big[1], 78)
    views = []
    for b, p, off in zip(big, planes, (3, 1, 1)):  # offsets that break the 4-byte alignment of the rows
        b[1:1 + p.shape[0], off:off + p.shape[1]] = torch.from_numpy(p).to(DEV)
        views.append(b[1:1 + p.shape[0], off:off + p.shape[1]])
    want = R.to_rgb(*planes, dtype=np.float32)
    for size in (None, (67, 131), (70, 133), (128, 192)):
        got = Y.planes_to_rgb(*views, Y.ColorSpec(), size).cpu().numpy()[0]
        assert got.shape[1:] == (size or (h, w))
        assert np.array_equal(U.f32_bits(got[:, :h, :w]), U.f32_bits(want))
        got[:, :h, :w] = 0
        assert not U.f32_bits(got).any()
    with pytest.raises(ValueError):
        Y.planes_to_rgb(views[0], views[1], views[2][:, ::2], Y.ColorSpec())
    with pytest.raises(ValueError):
        Y.planes_to_rgb(*views, Y.ColorSpec(), (64, 130))
    with pytest.raises(ValueError):
        Y.planes_to_rgb(*views, Y.ColorSpec(bit_depth=10))


# ---------------------------------------------------------------------------------------------------------------- K3
@pytest.mark.parametrize("kind", ["gamut", "random"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_k3_rgb_to_yuv420(case, kind):
    name, h, w, col = case
    rgb = R.case_rgb(name, h, w, kind)  # "random" reaches beyond [0, 1]
    x = torch.from_numpy(rgb)[None].to(DEV)
    frame = Y.rgb_to_yuv420(x, h, w, _spec(col))
    assert frame.dtype == (torch.uint8 if col["depth"] == 8 else torch.int16) and frame.numel() == h * w * 3 // 2
    got = _host_planes(frame, h, w)
    want32, want64 = R.from_rgb(rgb, dtype=np.float32, **col), R.from_rgb(rgb, dtype=np.float64, **col)
    for g, a, b, plane in zip(got, want32, want64, "yuv"):
        d = np.abs(g.astype(np.int64) - b)
        print(name, kind, plane, "samples differing from fp32", int((g != a).sum()), "from fp64", int((d != 0).sum()), "of", d.size)
        assert np.array_equal(g.astype(np.int64), a), plane
        assert d.max() <= 1 and (d != 0).sum() <= CAP_SAMPLES * d.size, plane
    # reconstructions are clamped on load: the samples of an out-of-range input are those of its clamped self
    assert torch.equal(Y.rgb_to_yuv420(x.clamp(0.0, 1.0), h, w, _spec(col)), frame)


def test_k3_cropped_rgb_input_is_read_in_place():
    h, w = 270, 482
    rgb = R.case_rgb("crop", h, w, "gamut")
    padded = torch.full((1, 3, 320, 512), 0.77, device=DEV)
    padded[..., :h, :w] = torch.from_numpy(rgb).to(DEV)
    want = R.from_rgb(rgb, dtype=np.float32)
    for src in (padded, padded[..., :h, :w], padded[..., 2:, 1:][..., :h, :w]):  # the last: rows not 16-byte aligned
        ref = want if src.data_ptr() == padded.data_ptr() else R.from_rgb(src[0, :, :h, :w].cpu().numpy(), dtype=np.float32)
        got = _host_planes(Y.rgb_to_yuv420(src, h, w), h, w)
        assert all(np.array_equal(g.astype(np.int64), a) for g, a in zip(got, ref))
    with pytest.raises(ValueError):
        Y.rgb_to_yuv420(padded, 322, 482)
    with pytest.raises(ValueError):
        Y.rgb_to_yuv420(padded.half(), h, w)
    with pytest.raises(ValueError):
        Y.rgb_to_yuv420(padded, h, w, source=torch.zeros(5, dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- K4
@pytest.mark.parametrize("case", [c for c in CASES if c[1:3] == R.MID], ids=[c[0] for c in CASES if c[1:3] == R.MID])
def test_k4_luma_round_trip(case):
    name, h, w, col = case
    planes = R.gamut_planes(11, h, w, **col)
    rgb = Y.yuv420_to_rgb(_dev_frame(planes, col["depth"]), h, w, _spec(col))
    back = _host_planes(Y.rgb_to_yuv420(rgb, h, w, _spec(col)), h, w)[0]
    keep = R.unclamped_mask(*planes, **col)
    assert keep.mean() > 0.5
    assert np.array_equal(back[keep], planes[0][keep])


# ---------------------------------------------------------------------------------------------------------------- K5
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", [(2, 2), (66, 130), (1080, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_k5_integer_sums_and_psnr(size, depth):
    h, w = size
    spec = Y.ColorSpec(bit_depth=depth)
    src = R.random_planes(21, h, w, depth)  # far from the picture: large differences, sums beyond 32 bits at 1080p
    rgb = torch.from_numpy(R.case_rgb(f"k5-{h}", h, w, "random"))[None].to(DEV)
    frame, sums = Y.rgb_to_yuv420(rgb, h, w, spec, source=_dev_frame(src, depth))
    assert torch.equal(frame, Y.rgb_to_yuv420(rgb, h, w, spec))
    assert sums.dtype == torch.int64 and sums.shape == (3,)
    want_sums, want_psnr = R.psnr_yuv(src, _host_planes(frame, h, w), depth)
    assert sums.tolist() == want_sums
    assert (h, w) != (1080, 1920) or want_sums[0] > 2 ** 32
    assert Y.psnr_yuv(sums, h, w, depth) == pytest.approx(want_psnr, rel=1e-14)
    same, zero = Y.rgb_to_yuv420(rgb, h, w, spec, source=frame)
    assert zero.tolist() == [0, 0, 0] and torch.equal(same, frame)


# ---------------------------------------------------------------------------------------------------------------- K6
def test_k6_run_to_run_identical_also_beside_other_work():
    from vcm_ts_amd.dmc import DMC
    from vcm_ts_amd.synthetic import frames

    h, w = 1080, 1920
    spec = Y.ColorSpec()
    src = _dev_frame(R.gamut_planes(4, h, w), 8)

    def once():
        rgb = Y.yuv420_to_rgb(src, h, w, spec)
        back, sums = Y.rgb_to_yuv420(rgb, h, w, spec, source=src)
        return rgb, Y.yuv420_to_rgb(src, h, w, spec, quantize8=True), back, sums

    first = once()
    for a, b in zip(first, once()):
        assert torch.equal(a, b)
    # the same on a side stream while the codec's convolutions (split-fp16 MFMA kernels) run on another
    m = DMC().to(DEV).eval()
    clip = torch.from_numpy(frames(3, 2, 256, 256)).to(DEV)
    dpb = {"ref_frame": clip[0:1], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    with torch.no_grad():
        m.forward_one_frame(clip[1:2], dpb, 1.0, 1.0)  # (packs the filters, allocates the workspace)
        work, side = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        torch.cuda.synchronize(DEV)
        with torch.cuda.stream(work):
            for _ in range(4):
                m.forward_one_frame(clip[1:2], dpb, 1.0, 1.0)
        with torch.cuda.stream(side):
            busy = [once() for _ in range(3)]
    torch.cuda.synchronize(DEV)
    for run in busy:
        for a, b in zip(first, run):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- end to end
def _write_source(path, seed, n, h, w, depth=8, chroma=None, **col):
    """A seeded Y4M of in-gamut content, written by the tests' own writer; returns the list of plane triples."""
    col = dict(dict(matrix="bt709", full_range=False, siting="left"), **col)
    frames = [tuple(p.astype(R.sample_dtype(depth)) for p in R.from_rgb(f, depth=depth, dtype=np.float64, **col))
              for f in R.gamut_rgb(seed, n, h, w)]
    R.write_y4m(str(path), frames, w, h, chroma=chroma or ("420p10" if depth == 10 else "420mpeg2"), fps="30:1")
    return frames


def test_e1_video_path_codes_the_same_bytes_as_the_png_path(tmp_path):
    from PIL import Image

    from vcm_ts_amd import run_codec as RC

    n, h, w, gop = 8, 128, 192, 4
    planes = _write_source(tmp_path / "src.y4m", 31, n, h, w)
    bits_v, size_v = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "bv"), quantize8=True, gop=gop, gop_streams=2)
    # the device's own converted pictures as 8-bit RGB PNGs, coded by the tested PNG path with the same settings
    png = tmp_path / "png"
    png.mkdir()
    for t, p in enumerate(planes):
        x = Y.yuv420_to_rgb(_dev_frame(p, 8), h, w, Y.ColorSpec(), pad=False, quantize8=True)
        u8 = torch.round(x[0] * 255.0).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(U.f32_bits(u8.astype(np.float32) / 255.0), U.f32_bits(x[0].permute(1, 2, 0).cpu().numpy()))
        Image.fromarray(u8).save(png / f"im{t + 1:05d}.png")
    bits_f, size_f = RC.encode_folder(str(png), str(tmp_path / "bf"), gop=gop, gop_streams=2)
    assert size_v == size_f == (h, w) and bits_v == bits_f and len(bits_v) == n
    a, b = U.bins(tmp_path / "bv"), U.bins(tmp_path / "bf")
    assert sorted(a) == sorted(b) == [f"im{t + 1:05d}.bin" for t in range(n)]
    for name in a:
        assert a[name] == b[name], name
    # without quantize8 the codec sees the unrounded floats: other pictures, other bytes
    bits_u, _ = RC.encode_video(str(tmp_path / "src.y4m"), str(tmp_path / "bu"), gop=gop, gop_streams=2)
    assert U.bins(tmp_path / "bu") != a and len(bits_u) == n


def _round_trip(tmp_path, h, w, n=6, gop=4, depth=8, chroma=None, coder="host", **col):
    from vcm_ts_amd import run_codec as RC

    src = tmp_path / "src.y4m"
    _write_source(src, 37, n, h, w, depth=depth, chroma=chroma, **col)
    bins = tmp_path / "bins"
    bits, size = RC.encode_video(str(src), str(bins), recon_video=str(tmp_path / "a.y4m"), gop=gop, gop_streams=2, coder=coder)
    assert size == (h, w) and len(bits) == n
    # nothing but the .bin files and sequence.json reaches the decoder
    assert sorted(os.listdir(bins)) == [f"im{t + 1:05d}.bin" for t in range(n)] + ["sequence.json"]
    assert RC.decode_video(str(bins), str(tmp_path / "b.y4m")) == n
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes()
    f_src, fr_src = R.read_y4m(str(src))
    f_out, fr_out = R.read_y4m(str(tmp_path / "a.y4m"))
    assert len(fr_out) == len(fr_src) == n
    for key in ("W", "H", "F", "I", "A", "C"):
        assert f_out[key] == f_src[key], key
    assert all(int(b.max()) <= (1 << depth) - 1 and not np.array_equal(a, b) for a, b in zip(fr_src, fr_out))  # a reconstruction
    return bins


def test_e2_encoder_and_decoder_write_identical_video_and_the_bins_serve_the_png_decoder(tmp_path):
    from PIL import Image

    from vcm_ts_amd import run_codec as RC

    h, w, n = 128, 192, 6
    bins = _round_trip(tmp_path, h, w, n=n)
    info = RC.read_sequence_info(str(bins))
    assert (info["width"], info["height"], info["frames"], info["gop"], info["fps"], info["container"]) == (w, h, n, 4, (30, 1), "y4m")
    assert info["color"] == Y.ColorSpec()
    # format interoperability: the unchanged decode_folder reads the same .bin files into PNGs
    assert RC.decode_folder(str(bins), str(tmp_path / "png"), h, w, gop=4) == n
    _, fr = R.read_y4m(str(tmp_path / "a.y4m"))
    for t in range(n):
        img = np.asarray(Image.open(tmp_path / "png" / f"im{t + 1:05d}.png"))
        assert img.shape == (h, w, 3)
        # the same reconstruction in both outputs: rounding R, G, B to 8 bits moves Y' by at most 0.5 / 255, i.e. the
        # luma sample by at most 0.43 codes before its own rounding -- so the two lumas are at most 1 apart
        y = R.from_rgb(img.transpose(2, 0, 1).astype(np.float64) / 255.0, dtype=np.float64)[0]
        assert np.abs(y.reshape(-1) - fr[t][:h * w].astype(np.int64)).max() <= 1
    # explicit arguments override sequence.json; a raw .yuv output holds the same samples
    assert RC.decode_video(str(bins), str(tmp_path / "c.yuv")) == n
    assert (tmp_path / "c.yuv").read_bytes() == b"".join(f.tobytes() for f in fr)
    with pytest.raises(ValueError):
        RC.decode_video(str(bins), str(tmp_path / "d.y4m"), height=64, width=64)
    os.remove(bins / "sequence.json")
    with pytest.raises(ValueError, match="height and width"):
        RC.decode_video(str(bins), str(tmp_path / "d.y4m"))
    assert RC.decode_video(str(bins), str(tmp_path / "d.yuv"), height=h, width=w, gop=4) == n
    assert (tmp_path / "d.yuv").read_bytes() == (tmp_path / "c.yuv").read_bytes()


def test_e3_sizes_that_need_padding(tmp_path):
    _round_trip(tmp_path, 180, 322, chroma="420jpeg", siting="center")


def test_e3_ten_bit_source(tmp_path):
    from vcm_ts_amd import run_codec as RC

    bins = _round_trip(tmp_path, 128, 192, depth=10)
    assert RC.read_sequence_info(str(bins))["color"].bit_depth == 10


def test_e4_report_has_sample_domain_psnr(tmp_path):
    from vcm_ts_amd import run_codec as RC

    n, h, w, gop = 6, 192, 320, 4
    src = tmp_path / "src.y4m"
    _write_source(src, 41, n, h, w)
    plain_bits, _ = RC.encode_video(str(src), str(tmp_path / "plain"), gop=gop, gop_streams=2)
    bits, size, rd = RC.encode_video(str(src), str(tmp_path / "rep"), recon_video=str(tmp_path / "r.y4m"), gop=gop, gop_streams=2,
                                     report=str(tmp_path / "rd.json"))
    assert bits == plain_bits and U.bins(tmp_path / "rep") == U.bins(tmp_path / "plain")
    assert json.loads((tmp_path / "rd.json").read_text()) == json.loads(json.dumps(rd))
    _, fr_src = R.read_y4m(str(src))
    _, fr_rec = R.read_y4m(str(tmp_path / "r.y4m"))
    want = [R.psnr_yuv(R.from_i420(a, h, w), R.from_i420(b, h, w), 8)[1] for a, b in zip(fr_src, fr_rec)]
    for k, name in enumerate(("y", "u", "v", "yuv")):
        assert rd[f"frame_psnr_{name}"] == pytest.approx([p[k] for p in want], rel=1e-13), name
    types = [0 if t % gop == 0 else 1 for t in range(n)]
    for kind, keep in (("i", [t for t in range(n) if types[t] == 0]), ("p", [t for t in range(n) if types[t]]), ("all", list(range(n)))):
        assert rd[f"ave_{kind}_frame_psnr_yuv"] == pytest.approx(np.mean([want[t][3] for t in keep]), rel=1e-13)
    for key in ("frame_pixel_num", "i_frame_num", "p_frame_num", "ave_all_frame_bpp", "ave_all_frame_psnr", "ave_all_frame_msssim",
                "ave_i_frame_psnr", "ave_p_frame_msssim", "frame_bpp", "frame_psnr", "frame_msssim", "frame_type"):
        assert key in rd, key
    assert rd["frame_type"] == types and len(rd["frame_psnr"]) == n
    assert np.isfinite(rd["frame_psnr"]).all() and np.isfinite(rd["frame_msssim"]).all() and np.isfinite(rd["frame_psnr_yuv"]).all()
    # report without a reconstruction file gives the same numbers
    _, _, rd2 = RC.encode_video(str(src), str(tmp_path / "rep2"), gop=gop, gop_streams=1, report=True)
    assert rd2["frame_psnr_yuv"] == rd["frame_psnr_yuv"] and rd2["frame_psnr"] == rd["frame_psnr"]


def test_e5_device_coder(tmp_path):
    _round_trip(tmp_path, 128, 192, coder="device")


def test_command_line_round_trip_without_pil(tmp_path):
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, h, w = 5, 192, 320
    planes = _write_source(tmp_path / "x.y4m", 43, n, h, w)
    guard = ("import sys, runpy; sys.argv = ['run_codec'] + sys.argv[1:]\n"
             "try:\n    runpy.run_module('vcm_ts_amd.run_codec', run_name='__main__')\n"
             "finally:\n    assert not any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules), 'PIL was imported'\n")
    run = lambda *a: subprocess.run([sys.executable, "-c", guard, *a], cwd=root, capture_output=True, text=True, timeout=900)
    r = run("encode", "--video", str(tmp_path / "x.y4m"), "--bins", str(tmp_path / "B"), "--recon-video", str(tmp_path / "r.y4m"),
            "--report", str(tmp_path / "r.json"), "--gop", "4", "--gop-streams", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PSNR-YUV" in r.stdout and "ave_all_frame_psnr_yuv" in json.loads((tmp_path / "r.json").read_text())
    r = run("decode", "--bins", str(tmp_path / "B"), "--recon-video", str(tmp_path / "d.y4m"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "r.y4m").read_bytes() == (tmp_path / "d.y4m").read_bytes()
    # a raw .yuv file of the same samples with --size codes the same pictures
    (tmp_path / "x.yuv").write_bytes(b"".join(R.to_i420(p).tobytes() for p in planes))
    r = run("encode", "--video", str(tmp_path / "x.yuv"), "--size", f"{w}x{h}", "--fps", "30", "--bins", str(tmp_path / "B2"),
            "--gop", "4")
    assert r.returncode == 0, r.stdout + r.stderr
    assert U.bins(tmp_path / "B2") == U.bins(tmp_path / "B")
