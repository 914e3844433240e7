"""The file loops of run_codec as functions of their source: a PNG folder and a Y4M file of the same 8-bit pixels go through
encode_folder / encode_video and decode_folder / decode_video with every option of the codec switched on together.

The two encode loops must write the same .bin and .rl files, the same sidecars (sequence.json is the video path's one extra)
and the same report but for the video path's sample-domain keys; the two decode loops must run to the end under
verify="strict" and give the encoders' own reconstructions.  Everything is an equality of bytes or of values: there is no
tolerance.  The clip is 4 pictures of 176x208 (both sides need padding and are above the 160 MS-SSIM refuses): three of a
bright scene and one of a dark one, so that GOP 2 with scene cuts gives I pictures at 0, 2 and 3, coded on two GOP streams.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import scenecut_ref as SR
from tests import yuv_ref as YR
from tests.gpu_util import file_nets  # noqa: F401 (fixture)
from vcm_ts_amd import yuv as Y

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, H, W, GOP, T, PLAN = 4, 208, 176, 2, 0.5, [0, 2, 3]
YUV_KEYS = {f"frame_psnr_{c}" for c in ("y", "u", "v", "yuv")} | {f"ave_{k}_frame_psnr_yuv" for k in ("i", "p", "all")}


def _boxes(t):
    from vcm_ts_amd import roi as X

    return X.FrameBoxes([[20 + 3 * t, 30, 75 + 3 * t, 90 + t, 0], [W - 61, H - 50 - t, W, H, 1]])


def _options(case, tmp, side):
    """The keyword arguments of one encode call; `side` names the outputs of the folder / video call."""
    from vcm_ts_amd import aq as A
    from vcm_ts_amd import redact as D
    from vcm_ts_amd import roi as X
    from vcm_ts_amd import tnr as TN

    roi = X.Roi(_boxes, (X.RoiClass(3), X.RoiClass(5)), ("liplates", "faces"))
    kw = dict(gop=GOP, gop_streams=2, report=True, picture_hash=True, aq=A.AQ(100), tnr=TN.TNR(12, 64, 36), target_bpp=0.5,
              scenecut=T)
    with_roi = dict(roi=roi, residual_bins=str(tmp / f"{case}_{side}_rl"), redact=D.Redact(("liplates",), tile=8, restorable=True))
    if case == "maps":
        kw.update(with_roi, roi_q=X.RoiQ(140, (60, 80), 0), bit_map=True)
    elif case == "base":  # (base_scale= with bit_map= and roi= is refused: the bit maps go without the boxes)
        kw.update(base_scale="1/2", bit_map=True)
    else:  # "base-roi": the boxes and what hangs on them, without the bit maps
        kw.update(with_roi, base_scale="1/2")
    return kw


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """src.y4m, and png/: the device's own 8-bit conversion of its pictures (what quantize8=True hands the codec)"""
    from PIL import Image

    tmp = tmp_path_factory.mktemp("file_loops")
    rgb = SR.cut_clip(H, W, n_a=3, n_b=1).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(f, dtype=np.float64)) for f in rgb]
    YR.write_y4m(str(tmp / "src.y4m"), planes, W, H, fps="30:1")
    os.makedirs(tmp / "png")
    for t, p in enumerate(planes):
        x = Y.yuv420_to_rgb(torch.from_numpy(YR.to_i420(p)).to(DEV), H, W, Y.ColorSpec(), pad=False, quantize8=True)
        Image.fromarray(torch.round(x[0] * 255.0).to(torch.uint8).permute(1, 2, 0).cpu().numpy()).save(tmp / "png" / f"im{t + 1:05d}.png")
    return tmp


def _files(folder, keep):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder)) if keep(n)}


@pytest.mark.parametrize("case", ["maps", "base", "base-roi"])
def test_both_sources_code_and_decode_alike(clip, file_nets, case):
    from vcm_ts_amd import run_codec as RC

    tmp = clip
    bf, bv = tmp / f"{case}_f", tmp / f"{case}_v"
    kw_f, kw_v = _options(case, tmp, "f"), _options(case, tmp, "v")
    bits_f, size_f, rd_f = RC.encode_folder(str(tmp / "png"), str(bf), str(tmp / f"{case}_f_rec"), nets=file_nets, **kw_f)
    bits_v, size_v, rd_v = RC.encode_video(str(tmp / "src.y4m"), str(bv), str(tmp / f"{case}_v_rec.y4m"), quantize8=True,
                                           nets=file_nets, **kw_v)
    # ---- encode: the same .bin and .rl files, sidecars and report
    assert size_f == size_v == (H, W) and bits_f == bits_v and len(bits_f) == N
    bins = _files(bf, lambda n: n.endswith(".bin"))
    assert sorted(bins) == [f"im{t + 1:05d}.bin" for t in range(N)] and bins == _files(bv, lambda n: n.endswith(".bin"))
    if "roi" in kw_f:
        records = _files(kw_f["residual_bins"], lambda n: True)
        assert sorted(records) == [f"im{t + 1:05d}.rl" for t in range(N)] and records == _files(kw_v["residual_bins"], lambda n: True)
    side_f, side_v = (_files(b, lambda n: not n.endswith(".bin")) for b in (bf, bv))
    want = {"gops.json", "hashes.json", "aq.json"} | ({"redact.json"} if "roi" in kw_f else set()) | \
        ({"roiq.json"} if case == "maps" else {"scale.json"})
    assert set(side_f) == want and set(side_v) == want | {"sequence.json"}
    for name in side_f:
        assert side_f[name] == side_v[name], name
    assert json.loads(side_f["gops.json"])["i_pictures"] == PLAN
    extra = set(rd_v) - set(rd_f)
    assert extra == YUV_KEYS and not set(rd_f) - set(rd_v)
    assert [k for k in rd_v if k not in extra] == list(rd_f)
    for key in rd_f:
        assert rd_f[key] == rd_v[key], key
    assert rd_f["frame_type"] == [0, 1, 0, 0] and ("frame_bits_y" in rd_f) == ("bit_map" in kw_f)
    assert ("frame_redacted" in rd_f) == ("frame_bits_enh" in rd_f) == ("frame_psnr_roi" in rd_f) == ("roi" in kw_f)
    assert "frame_tnr_held" in rd_f and "frame_q_y" in rd_f
    # ---- decode: both loops reach the end under the strict check and give the encoders' own reconstructions
    roi = dict(roi=kw_f["roi"]) if case == "maps" else {}  # (a roiq.json is followed with the boxes; nothing is fused)
    assert RC.decode_folder(str(bf), str(tmp / f"{case}_f_dec"), H, W, verify="strict", **roi) == N
    assert RC.decode_video(str(bv), str(tmp / f"{case}_v_dec.y4m"), verify="strict", **roi) == N
    assert (tmp / f"{case}_v_dec.y4m").read_bytes() == (tmp / f"{case}_v_rec.y4m").read_bytes()
    assert (tmp / f"{case}_v_dec.y4m").stat().st_size > N * H * W * 3 // 2
    for t in range(N):
        name = f"im{t + 1:05d}.png"
        got = U.png(tmp / f"{case}_f_dec" / name)
        assert got.shape == (H, W, 3) and np.array_equal(got, U.png(tmp / f"{case}_f_rec" / name)), t


def test_base_scale_with_bit_map_and_roi_stays_refused(clip, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = clip
    kw = dict(_options("base-roi", tmp, "never"), bit_map=True)
    with pytest.raises(NotImplementedError, match="bit_map= and roi="):
        RC.encode_folder(str(tmp / "png"), str(tmp / "never_f"), nets=file_nets, **kw)
    with pytest.raises(NotImplementedError, match="bit_map= and roi="):
        RC.encode_video(str(tmp / "src.y4m"), str(tmp / "never_v"), quantize8=True, nets=file_nets, **kw)
    assert not (tmp / "never_f").exists() and not (tmp / "never_v").exists() and not (tmp / "base-roi_never_rl").exists()
