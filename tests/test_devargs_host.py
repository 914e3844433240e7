"""The feature modules' device boundary without a GPU: every public entry refuses a CPU tensor (and every constructor a
CPU device) with a ValueError before any GPU work, and vcm_ts_amd/devargs.py's own functions -- the integer and
hundredths validators, the stride helper on CPU tensors, the first refusals of picture() -- and stream.read_sidecar."""
import json

import numpy as np
import pytest
import torch

from vcm_ts_amd import aq as A
from vcm_ts_amd import metrics as MT
from vcm_ts_amd import motionroi as M
from vcm_ts_amd import picturehash as PH
from vcm_ts_amd import redact as D
from vcm_ts_amd import roi as X
from vcm_ts_amd import roilayer as RL
from vcm_ts_amd import scale as SC
from vcm_ts_amd import scenecut as SN
from vcm_ts_amd import tnr as N
from vcm_ts_amd import yuv as Y

CLASSES = (X.RoiClass(0),)
FILL = D.Redact(("faces",), fill=0)


def _roi():
    return X.Roi(lambda index: X.FrameBoxes(), CLASSES, ("faces",))


def _cpu():
    return torch.zeros((1, 3, 176, 176))


ENTRIES = {
    "crc32_pixels": lambda x: PH.crc32_pixels(x),
    "crc32_f32": lambda x: PH.crc32_f32(x),
    "roi.residual_layer": lambda x: X.residual_layer(x, x, X.FrameBoxes()),
    "roi.fuse": lambda x: X.fuse(x, torch.zeros((3, 176, 176), dtype=torch.uint8), X.FrameBoxes(), CLASSES),
    "roi.region_sse": lambda x: X.region_sse(x, x, X.FrameBoxes(), CLASSES),
    "roilayer.encode_layer": lambda x: RL.encode_layer(x, x, X.FrameBoxes()),
    "scale.scale_planes": lambda x: SC.scale_planes(x, (88, 88), None, None),
    "yuv.rgb_to_yuv420": lambda x: Y.rgb_to_yuv420(x, 176, 176),
    "yuv.yuv420_to_rgb": lambda x: Y.yuv420_to_rgb(torch.zeros(176 * 176 * 3 // 2, dtype=torch.uint8), 176, 176),
    "metrics.ms_ssim": lambda x: MT.ms_ssim(x, x),
    "metrics.psnr": lambda x: MT.psnr(x, x),
    "redact.redact_picture": lambda x: D.redact_picture(x, X.FrameBoxes(), FILL, ("faces",)),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_cpu_tensor_is_a_value_error(name):
    with pytest.raises(ValueError, match="no CPU fallback"):
        ENTRIES[name](_cpu())


CONSTRUCTORS = {
    "AqMaps": lambda dev: A.AqMaps(A.AQ(100), dev),
    "SceneScan": lambda dev: SN.SceneScan(dev, 8, 8, 1),
    "MotionScan": lambda dev: M.MotionScan(dev, 8, 8, 1, M.MotionParams(24)),
    "Scale": lambda dev: SC.Scale((40, 52), "1/2", dev),
    "TnrFilter": lambda dev: N.TnrFilter(N.TNR(12), (8, 8), dev),
    "Redactor": lambda dev: D.Redactor(FILL, _roi(), (8, 8), dev),
}


@pytest.mark.parametrize("name", sorted(CONSTRUCTORS))
def test_a_cpu_device_is_a_value_error(name):
    for dev in ("cpu", torch.device("cpu")):
        with pytest.raises(ValueError, match="no CPU fallback"):
            CONSTRUCTORS[name](dev)


def test_the_names_the_modules_export_are_one_constant():
    for mod in (A, SN, PH, SC, X, Y):
        assert mod.MAX_SIDE == 32768


# ---------------------------------------------------------------------------------------------------- the new module
def test_devargs_whole():
    from vcm_ts_amd import devargs as V

    assert V.whole("k", 3, 1, 8) == 3 and V.whole("k", 1, 1, 8) == 1 and V.whole("k", 8, 1, 8) == 8
    got = V.whole("k", np.int64(5), 1, 8)
    assert got == 5 and type(got) is int
    for bad in (True, False, 1.0, 0, 9, "3", None, np.float32(2)):
        with pytest.raises(ValueError, match=r"k must be an integer within 1\.\.8, got"):
            V.whole("k", bad, 1, 8)
    with pytest.raises(ValueError, match=r"k must be an integer within 1\.\.8 \(pixels\), got 9"):
        V.whole("k", 9, 1, 8, "pixels")
    assert V.MAX_SIDE == 32768


def test_devargs_hundredths():
    from vcm_ts_amd import devargs as V

    assert V.hundredths(0.6, "f") == 60 and V.hundredths(1, "f") == 100 and V.hundredths(np.float32(2.5), "f") == 250
    for bad in (float("nan"), float("inf"), -float("inf"), True, "1.0", None):
        with pytest.raises(ValueError, match="f must be a finite number"):
            V.hundredths(bad, "f")
    # the two names that stay call it
    assert A.AQ.hundredths(0.6) == 60 and X.RoiQ.hundredths(0.6) == 60
    for fn in (A.AQ.hundredths, X.RoiQ.hundredths):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                fn(bad)


def test_devargs_cuda_device_refuses_everything_else():
    from vcm_ts_amd import devargs as V

    for bad in ("cpu", torch.device("cpu"), "meta", "no such device", 1.5):
        with pytest.raises(ValueError, match="Who: .*no CPU fallback"):
            V.cuda_device(bad, "Who")
    assert V.cuda_device("cuda:3", "Who") == torch.device("cuda", 3)  # (an explicit index asks the runtime nothing)


def test_devargs_planar_reads_a_dense_crop_in_place():
    from vcm_ts_amd import devargs as V

    base = torch.arange(2 * 3 * 8 * 10, dtype=torch.float32).reshape(2, 3, 8, 10)
    for t in (base[:1], base, base[:1, :, 2:, 3:], base[1:, 1:2], base[:, :1]):  # (whole, batch, offset crop, C == 1 twice)
        crop = t[..., :5, :7]
        got, rs, ps = V.planar(crop)
        assert got.data_ptr() == crop.data_ptr() and got.shape == crop.shape and rs == 10
        if t.shape[1] > 1:
            assert ps == 80
        elif t.shape[0] > 1:
            assert ps == t.stride(0)  # (planes of a one-channel batch are one sample apart)
    one = torch.zeros((1, 1, 8, 10))[..., :5, :7]
    assert V.planar(one)[0].data_ptr() == one.data_ptr() and V.planar(one)[1] == 10


def test_devargs_planar_copies_what_is_not_planar_rows():
    from vcm_ts_amd import devargs as V

    base = torch.arange(3 * 8 * 10, dtype=torch.float32).reshape(1, 3, 8, 10)
    for t in (base.transpose(2, 3), base[..., ::2], base.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2),
              torch.zeros((2, 3, 8, 10))[:, :2]):  # (transposed, strided columns, channels last, unevenly spaced samples)
        got, rs, ps = V.planar(t)
        H, W = t.shape[2:]
        assert got.data_ptr() != t.data_ptr() and got.is_contiguous() and (rs, ps) == (W, H * W) and torch.equal(got, t)


def test_devargs_picture_refuses_what_is_not_on_the_gpu_first():
    from vcm_ts_amd import devargs as V

    for bad in (_cpu(), _cpu().double()[0], np.zeros((1, 3, 8, 8), np.float32), None):  # (wrong in other ways too)
        for fn in (V.picture, V.checked):
            with pytest.raises(ValueError, match="Caller.add: .*no CPU fallback"):
                fn(bad, "Caller.add", exact=(4, 4))
        with pytest.raises(ValueError, match="Caller.add: the operand .*no CPU fallback"):
            V.on_gpu(bad, "Caller.add", noun="operand")


SIDECARS = {
    "aq.json": lambda d: A.read_aq(d),
    "scale.json": lambda d: SC.read_scale(d),
    "hashes.json": lambda d: PH.read_hashes(d),
    "motion.json": lambda d: M.read_info(d),
    "roiq.json": lambda d: _run_codec().read_roiq(d, _roi()),
    "gops.json": lambda d: _run_codec().read_gop_plan(d),
    "sequence.json": lambda d: _run_codec().read_sequence_info(d),
}


def _run_codec():
    from vcm_ts_amd import run_codec

    return run_codec


@pytest.mark.parametrize("name", sorted(SIDECARS))
def test_read_sidecar_and_its_seven_readers(tmp_path, name):
    from vcm_ts_amd.stream import read_sidecar, write_sidecar

    folder, path = str(tmp_path), str(tmp_path / name)
    assert read_sidecar(folder, name) is None
    if name != "gops.json":  # (without the file read_gop_plan answers with the fixed plan)
        assert SIDECARS[name](folder) is None
    write_sidecar(folder, name, {"version": 1, "list": [1, 2, 3]})
    assert read_sidecar(folder, name) == (path, {"version": 1, "list": [1, 2, 3]})
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(text[:len(text) // 2])  # truncated
    for call in (lambda: read_sidecar(folder, name), lambda: SIDECARS[name](folder)):
        with pytest.raises(ValueError, match="not JSON") as ex:
            call()
        assert path in str(ex.value) and not isinstance(ex.value, json.JSONDecodeError)
