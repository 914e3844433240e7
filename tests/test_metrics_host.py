"""Host-only checks of the MS-SSIM work: the float64 restatement the GPU tests are measured against
(tests/msssim_ref.py) is sane by itself, the C ABI of include/dcvc_hip_metrics.h refuses bad arguments before it
touches anything (no GPU is needed for a refused call), and run_codec's report has the reference's key layout."""
import ctypes as C

import pytest
import torch

from tests import msssim_ref as R


def test_window_sums_to_one_and_is_symmetric():
    for dtype in (torch.float64, torch.float32):
        g = R.window(dtype)
        assert g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-6
        assert torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    assert float(R.window()[4] / R.window()[5]) == pytest.approx(float(torch.exp(torch.tensor(-1 / 4.5, dtype=torch.float64))))


def test_level_sizes():
    assert R.level_sizes(1080) == [1080, 540, 270, 135, 68]
    assert R.level_sizes(161) == [161, 81, 41, 21, 11]
    assert R.level_sizes(270) == [270, 135, 68, 34, 17]
    x = torch.rand(1, 1, 161, 270, dtype=torch.float64)
    for _ in range(4):
        x = torch.nn.functional.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])
    assert tuple(x.shape[2:]) == (11, 17)


def test_identity_gives_one_and_noise_gives_less():
    x, y = R.smooth_pair(1, 2, 3, 176, 200, 0.03)
    one = R.ms_ssim(x.double(), x.double())
    assert one.shape == (2,) and float((one - 1).abs().max()) < 1e-12
    val = R.ms_ssim(x.double(), y.double())
    assert 0.9 < float(val.min()) and float(val.max()) < 0.9999
    assert torch.equal(y[..., 134:], x[..., 134:]) and not torch.equal(y, x)  # a third of the picture is exactly equal
    assert float(R.ms_ssim(x.double(), y.double(), size_average=True)) == pytest.approx(float(val.mean()))
    kept = R.ms_ssim_levels(x.double(), y.double())
    assert kept.shape == (5, 2, 3) and float(kept.min()) > 0.5


def test_restatement_refuses_small_pictures_and_clips():
    with pytest.raises(ValueError):
        R.ms_ssim(torch.rand(1, 3, 160, 300), torch.rand(1, 3, 160, 300))
    x = torch.rand(1, 3, 200, 200, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    assert float(R.ms_ssim(x, 1 - x)) == 0.0


def test_restatement_gradient_is_symmetric():
    x, y = R.smooth_pair(2, 1, 3, 161, 176, 0.03)
    a, b = x.double().requires_grad_(), y.double().requires_grad_()
    R.ms_ssim(a, b).sum().backward()
    c, d = y.double().requires_grad_(), x.double().requires_grad_()
    R.ms_ssim(c, d).sum().backward()
    torch.testing.assert_close(a.grad, d.grad, rtol=1e-9, atol=1e-15)
    torch.testing.assert_close(b.grad, c.grad, rtol=1e-9, atol=1e-15)


def test_c_abi_refuses_bad_arguments_on_the_host():
    """NULL pointers, empty and too small shapes, bad strides: DCVC_E_ARG before anything is dereferenced or launched
    (the pointers below are host addresses -- a call that got past its checks would not survive them)."""
    from vcm_ts_amd import lib

    L = lib.hip()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p = (p + 15) // 16 * 16

    def fwd(x=p, y=p, N=1, C_=3, H=176, W=176, rs=None, ps=None, L_=1.0, ws=p, out=p):
        rs = W if rs is None else rs
        ps = H * rs if ps is None else ps
        return L.dcvc_ms_ssim(x, y, N, C_, H, W, rs, ps, rs, ps, L_, 0, ws, out, None, None, None)

    def grad(x=p, y=p, H=176, W=176, clamp=0, ws=p, g=p, gx=p):
        return L.dcvc_ms_ssim_grad(x, y, 1, 3, H, W, W, H * W, W, H * W, 1.0, clamp, ws, g, gx, None)

    for kw in (dict(x=None), dict(y=None), dict(ws=None), dict(out=None), dict(N=0), dict(C_=0), dict(H=0, W=0),
               dict(H=160), dict(W=160), dict(H=160, W=160), dict(H=40000), dict(N=300, C_=300), dict(rs=175), dict(ps=175),
               dict(L_=0.0), dict(L_=float("nan")), dict(ws=p + 4)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(x=None), dict(y=None), dict(ws=None), dict(g=None), dict(gx=None), dict(H=160), dict(W=160), dict(clamp=1)):
        assert grad(**kw) == -1, kw
    assert L.dcvc_ms_ssim_workspace_bytes(1, 3, 160, 1920, 0) == 0
    assert L.dcvc_ms_ssim_workspace_bytes(0, 3, 1080, 1920, 0) == 0
    small, big = L.dcvc_ms_ssim_workspace_bytes(1, 3, 1080, 1920, 0), L.dcvc_ms_ssim_workspace_bytes(1, 3, 1080, 1920, 1)
    # pyramid of both pictures (a third of each) + a little; with the gradient three maps and a pyramid more
    assert 2 * 3 * 1080 * 1920 * 4 // 3 < small < 2 * 3 * 1080 * 1920 * 4 // 2
    assert big > small + 3 * 3 * 1070 * 1910 * 4


def test_python_surface_refuses_without_a_gpu():
    from vcm_ts_amd import metrics as M

    x = torch.rand(1, 3, 176, 176)
    for fn in (M.ms_ssim, M.psnr, M.MS_SSIM(data_range=1.0, size_average=False)):
        with pytest.raises(ValueError):
            fn(x, x)


def test_report_key_layout():
    from vcm_ts_amd.run_codec import rd_report

    rd = rd_report([0, 1, 1, 0, 1], [400, 40, 60, 800, 100], [30.0, 31.0, 33.0, 34.0, 35.0], [0.9, 0.91, 0.93, 0.94, 0.95], 100)
    assert list(rd)[:3] == ["frame_pixel_num", "i_frame_num", "p_frame_num"]
    assert (rd["i_frame_num"], rd["p_frame_num"]) == (2, 3)
    assert rd["ave_i_frame_bpp"] == pytest.approx(6.0) and rd["ave_p_frame_bpp"] == pytest.approx(200 / 300)
    assert rd["ave_all_frame_bpp"] == pytest.approx(1400 / 500)
    assert rd["ave_i_frame_psnr"] == pytest.approx(32.0) and rd["ave_p_frame_psnr"] == pytest.approx(33.0)
    assert rd["ave_all_frame_msssim"] == pytest.approx(0.926)
    assert rd["frame_bpp"] == [4.0, 0.4, 0.6, 8.0, 1.0] and rd["frame_type"] == [0, 1, 1, 0, 1]
    only_i = rd_report([0], [100], [30.0], [0.9], 100)
    assert only_i["ave_p_frame_bpp"] == 0 and only_i["ave_p_frame_psnr"] == 0 and only_i["ave_p_frame_msssim"] == 0
