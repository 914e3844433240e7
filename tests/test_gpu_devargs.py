"""vcm_ts_amd/devargs.py on a real MI355X: picture() reads a padded picture's crop in place and copies what is not planar
rows, refuses in its stated order, launch() enqueues on the current stream of the device, cuda_device() names it."""
import pytest
import torch

from tests import scenecut_ref as R
from vcm_ts_amd import devargs as V
from vcm_ts_amd import scenecut as SN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W, HP, WP = 70, 130, 128, 192


@pytest.fixture(scope="module")
def padded():
    x = torch.zeros((1, 3, HP, WP), device=DEV)
    x[..., :H, :W] = torch.from_numpy(R.wide_picture(3, H, W)).to(DEV)
    return x


def test_a_crop_of_a_padded_picture_is_read_in_place(padded):
    got, rs, ps = V.picture(padded, "Caller.add", device=DEV, at_least=(H, W))
    assert got.data_ptr() == padded.data_ptr() and tuple(got.shape) == (1, 3, H, W) and (rs, ps) == (WP, HP * WP)
    whole, rs, ps = V.picture(padded, "Caller.add", exact=(HP, WP))
    assert whole.data_ptr() == padded.data_ptr() and (rs, ps) == (WP, HP * WP)
    grad = padded.clone().requires_grad_()
    assert not V.picture(grad, "Caller.add")[0].requires_grad


def test_a_channels_last_view_comes_back_as_a_copy(padded):
    last = padded.contiguous(memory_format=torch.channels_last)
    assert last.stride(3) == 3 and torch.equal(last, padded)
    got, rs, ps = V.picture(last, "Caller.add", at_least=(H, W))
    assert got.data_ptr() != last.data_ptr() and got.is_contiguous() and (rs, ps) == (W, H * W)
    assert torch.equal(got, padded[..., :H, :W])


def test_picture_refuses_in_its_stated_order(padded):
    other = torch.device("cuda", 1)  # (the check itself: no second device is touched)
    half, big = padded.half(), torch.zeros((1, 3, 1, V.MAX_SIDE + 1), device=DEV)
    cases = [
        (dict(t=padded.cpu().half(), device=other, exact=(1, 1)), "no CPU fallback"),
        (dict(t=half, device=other, exact=(1, 1), owner="scan"), f"is on {DEV}, the scan on {other}"),
        (dict(t=half, device=DEV), r"expected a \(1, 3, H, W\) float32 picture, got .*float16"),
        (dict(t=padded[0], noun="reference picture"), "float32 reference picture"),
        (dict(t=padded[:, :2]), "expected a"),
        (dict(t=padded.expand(2, -1, -1, -1)), "expected a"),
        (dict(t=padded[..., :0, :]), "expected a"),
        (dict(t=padded, exact=(H, W), like=half), rf"expected a \(1, 3, {H}, {W}\) float32 picture"),
        (dict(t=padded, at_least=(HP + 1, W), like=half), "crop"),
        (dict(t=padded, at_least=(0, W)), "crop"),
        (dict(t=big, like=padded), "does not match"),
        (dict(t=padded, like=padded[..., :H, :W]), "does not match"),
        (dict(t=big, like=big), f"sides must be within 1..{V.MAX_SIDE}"),
    ]
    for kw, match in cases:
        t = kw.pop("t")
        for fn in (V.picture, V.checked):
            with pytest.raises(ValueError, match="Caller.add: .*" + match):
                fn(t, "Caller.add", **kw)


def test_launch_enqueues_on_the_current_stream_of_the_device(padded):
    side = torch.cuda.Stream(DEV)
    scan = SN.SceneScan(DEV, H, W, 1)
    hist = torch.zeros(SN.COUNTERS, dtype=torch.uint32, device=DEV)
    host = torch.zeros((2, SN.COUNTERS), dtype=torch.uint32).pin_memory()
    busy = torch.zeros(1 << 28, device=DEV)
    torch.cuda.synchronize(DEV)
    for _ in range(64):  # (tens of milliseconds on the DEFAULT stream: a launch that went there would still be queued below)
        busy.add_(1.0)
    with torch.cuda.stream(side):
        assert V.stream(DEV).value == side.cuda_stream
        scan.add(padded)
        x, rs, ps = V.picture(padded, "test", device=DEV, at_least=(H, W))
        V.launch("dcvc_scene_hist", DEV, x.data_ptr(), rs, ps, H, W, hist.data_ptr())
        host[0].copy_(hist, non_blocking=True)
        host[1].copy_(scan.hist[0], non_blocking=True)
    side.synchronize()  # this stream only
    got = host.numpy().astype("int64")
    assert got[0].sum() == H * W and (got[0] == got[1]).all()
    assert (got[0] == R.hist(R.wide_picture(3, H, W)).reshape(-1)).all()
    torch.cuda.synchronize(DEV)


def test_cuda_device_names_the_current_device():
    assert V.cuda_device("cuda", "Who") == torch.device("cuda", torch.cuda.current_device())
    assert V.cuda_device(torch.device("cuda"), "Who").index == torch.cuda.current_device()
    assert V.cuda_device(DEV, "Who") == DEV
    with pytest.raises(ValueError, match="Who: .*no CPU fallback"):
        V.cuda_device("cpu", "Who")
