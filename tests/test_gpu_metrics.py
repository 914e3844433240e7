"""MS-SSIM and PSNR on the device (vcm_ts_amd/metrics.py, csrc/metrics.hip) against tests/msssim_ref.py, the float64
torch-CPU restatement of pytorch_msssim.ms_ssim: values, per-level values, gradients in both arguments, strided crops,
clipped levels, determinism, refusals, and the three places the metric surfaces: the codecs' opt-in "ssim" /
"ssim_dist" keys (with their gradient through the picture's autograd node), the DCVC_HEM wrapper's loss_dist_key, and
run_codec's --report.

Bounds.  Values and per-level values: 2e-6 absolute, ten times the 2.3e-7 the restatement's own float32 evaluation
deviates from float64 on these inputs.  Gradients: 1e-3 of the norm, ten times its 1.0e-4.  PSNR: 1e-4 dB.  Each value
test prints the device's and the float32 restatement's deviation side by side.
"""
import json

import numpy as np
import pytest
import torch

from tests import msssim_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = ((1080, 1920), (256, 256), (270, 486), (161, 176))
SIGMAS = (0.005, 0.03, 0.15)
VALUE_TOL, GRAD_TOL, PSNR_TOL_DB = 2e-6, 1e-3, 1e-4


def _pair(H, W, sigma):
    return R.smooth_pair(1000 * H + W + int(sigma * 1000), 2, 3, H, W, sigma)


def _on_device(x, H):
    """1080 rows: as the crop view of a 1088-row tensor (the reconstruction of a padded picture), else a plain copy."""
    if H != 1080:
        return x.to(DEV)
    full = torch.full((x.shape[0], x.shape[1], 1088, x.shape[3]), 0.5, device=DEV)
    full[..., :1080, :] = x.to(DEV)
    return full[..., :1080, :]


def _rel(got, want):
    return float((got.detach().cpu().double() - want).norm() / want.norm())


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_value_levels_and_gradient_match_the_float64_restatement(size, sigma):
    from vcm_ts_amd import metrics as M

    H, W = size
    x, y = _pair(H, W, sigma)
    xd, yd = _on_device(x, H), _on_device(y, H)
    assert (H != 1080) or not xd.is_contiguous()
    x64, y64 = x.double().requires_grad_(), y.double().requires_grad_()
    kept64 = R.ms_ssim_levels(x64, y64)
    w = torch.tensor(R.WEIGHTS, dtype=torch.float64).view(-1, 1, 1)
    ref = torch.prod(kept64 ** w, dim=0).mean(1)
    g_ms = torch.rand(2, generator=torch.Generator().manual_seed(5), dtype=torch.float64) + 0.5
    (ref * g_ms).sum().backward()
    cpu32 = R.ms_ssim(x, y).double()
    for order in ("xy", "yx"):
        a, b = (xd, yd) if order == "xy" else (yd, xd)
        ms, levels, _ = M.measure(a, b, want_levels=True)
        dev_val = float((ms.cpu().double() - ref.detach()).abs().max())
        dev_lvl = float((levels.cpu().double() - kept64.detach()).abs().max())
        print(f"{H}x{W} sigma {sigma} {order}: ms-ssim {ref.tolist()}  |gpu - ref64| {dev_val:.3e}  "
              f"|cpu32 - ref64| {float((cpu32 - ref.detach()).abs().max()):.3e}  levels |gpu - ref64| {dev_lvl:.3e}  "
              f"smallest kept {float(kept64.detach().min()):.3f}")
        assert dev_val <= VALUE_TOL
        assert dev_lvl <= VALUE_TOL
    # gradient: size_average=False with a random upstream gradient, then the mean
    xg, yg = xd.detach().requires_grad_(), yd.detach().requires_grad_()
    out = M.ms_ssim(xg, yg, size_average=False)
    assert out.shape == (2,)
    (out * g_ms.float().to(DEV)).sum().backward()
    ex, ey = _rel(xg.grad, x64.grad), _rel(yg.grad, y64.grad)
    print(f"{H}x{W} sigma {sigma}: gradient relative error x {ex:.3e}  y {ey:.3e}")
    assert xg.grad.shape == x.shape and ex <= GRAD_TOL and ey <= GRAD_TOL
    x64.grad, y64.grad = None, None
    R.ms_ssim(x64, y64, size_average=True).backward()
    xg.grad, yg.grad = None, None
    M.MS_SSIM(data_range=1.0, size_average=True)(xg, yg).backward()
    assert _rel(xg.grad, x64.grad) <= GRAD_TOL and _rel(yg.grad, y64.grad) <= GRAD_TOL


def test_identity_is_one():
    from vcm_ts_amd import metrics as M

    for H, W in SIZES:
        x = _on_device(_pair(H, W, 0.03)[0], H)
        ms = M.ms_ssim(x, x, size_average=False)
        assert float((ms - 1.0).abs().max()) <= 1e-6, (H, W, ms)


@pytest.mark.parametrize("size", ((1080, 1920), (270, 486), (161, 176)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_cropped_view_and_its_copy_are_bit_identical(size):
    """A crop t[..., :h, :w] of a larger contiguous tensor is read in place through its strides: same bits as its
    .contiguous() copy, forward and gradient; the odd sizes go through the padded pooling."""
    from vcm_ts_amd import metrics as M

    H, W = size
    x, y = _pair(H, W, 0.03)
    big_x = torch.rand(2, 3, H + 8, W + 24, device=DEV)
    big_y = torch.rand(2, 3, H + 8, W + 24, device=DEV)
    big_x[..., :H, :W], big_y[..., :H, :W] = x.to(DEV), y.to(DEV)
    vx, vy = big_x[..., :H, :W], big_y[..., :H, :W]
    assert not vx.is_contiguous()
    g = torch.tensor([0.7, 1.3], device=DEV)
    res = []
    for a, b in ((vx, vy), (vx.contiguous(), vy.contiguous()), (vx, vy.contiguous())):
        a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
        ms, levels, sse = M.measure(a, b, want_levels=True)
        (M.ms_ssim(a, b, size_average=False) * g).sum().backward()
        res.append((ms, levels, sse, a.grad.contiguous(), b.grad.contiguous()))
    for other in res[1:]:
        for p, q in zip(res[0], other):
            assert torch.equal(p, q)
    assert R.level_sizes(H)[-1] == {1080: 68, 270: 17, 161: 11}[H]


def test_clipped_levels_give_zero_like_the_restatement():
    """y = 1 - x on a textured picture: cs is negative at every level, the relu cuts it, the product is 0 (forward only:
    the derivative of v^w at v = 0 is not a number to pin)."""
    from vcm_ts_amd import metrics as M

    x = torch.rand(2, 3, 200, 200, generator=torch.Generator().manual_seed(3))
    ref = R.ms_ssim(x.double(), 1.0 - x.double())
    assert float(ref.abs().max()) == 0.0
    ms, levels, _ = M.measure(x.to(DEV), (1.0 - x).to(DEV), want_levels=True)
    assert float(ms.abs().max()) == 0.0
    assert float(levels[:4].abs().max()) == 0.0


def test_forward_and_gradient_are_run_to_run_identical_also_beside_other_work():
    from vcm_ts_amd import metrics as M

    x, y = _pair(270, 486, 0.03)
    x, y = x.to(DEV), y.to(DEV)
    g = torch.tensor([1.0, 0.5], device=DEV)

    def once():
        ms, levels, sse = M.measure(x, y, want_levels=True)
        return ms, levels, sse, M._grad(x, y, g, 1.0)

    first = once()
    for a, b in zip(first, once()):
        assert torch.equal(a, b)
    # the same while another stream runs the codec's own convolutions (split-fp16 MFMA kernels: the neighbours next to
    # which DESIGN.md 4b found packed-FP32 code to differ from run to run)
    from vcm_ts_amd.dmc import DMC

    m = DMC().to(DEV).eval()
    clip = _pictures().to(DEV)
    dpb = {"ref_frame": clip[:, 0], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0)  # (packs the filters, allocates the workspace)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        for _ in range(4):
            m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0)
    busy = [once() for _ in range(3)]
    torch.cuda.synchronize(DEV)
    for run in busy:
        for a, b in zip(first, run):
            assert torch.equal(a, b)


def test_python_refusals():
    from vcm_ts_amd import metrics as M

    ok = torch.rand(1, 3, 176, 176, device=DEV)
    for bad in (torch.rand(1, 3, 160, 400, device=DEV), torch.rand(1, 3, 400, 160, device=DEV)):
        with pytest.raises(ValueError):
            M.ms_ssim(bad, bad)
    with pytest.raises(ValueError):
        M.ms_ssim(ok.half(), ok.half())
    with pytest.raises(ValueError):
        M.ms_ssim(ok.cpu(), ok.cpu())
    with pytest.raises(ValueError):
        M.ms_ssim(ok, ok[..., :170, :])
    with pytest.raises(ValueError):
        M.psnr(ok.cpu(), ok.cpu())
    with pytest.raises(ValueError):  # the clamp is not differentiable in the argument it clamps
        M.ms_ssim(ok.clone().requires_grad_(), ok, clamp01=True)
    assert float(M.ms_ssim(ok, ok)) == pytest.approx(1.0, abs=1e-6)


def test_c_abi_refuses_on_the_device_too():
    """Real device buffers, bad shapes / flags: DCVC_E_ARG, nothing launched (the host-only half is in
    tests/test_metrics_host.py)."""
    from vcm_ts_amd import lib

    L = lib.hip()
    x = torch.rand(1, 3, 176, 176, device=DEV)
    ws = torch.empty(L.dcvc_ms_ssim_workspace_bytes(1, 3, 176, 176, 1) // 4, device=DEV)
    out = torch.full((1,), -7.0, device=DEV)
    p = x.data_ptr()
    args = dict(H=176, W=176, rs=176, ps=176 * 176, L=1.0, clamp=0)

    def fwd(**kw):
        a = {**args, **kw}
        return L.dcvc_ms_ssim(p, p, 1, 3, a["H"], a["W"], a["rs"], a["ps"], a["rs"], a["ps"], a["L"], a["clamp"],
                              ws.data_ptr(), out.data_ptr(), None, None, None)

    assert fwd(H=160, ps=160 * 176) == -1 and fwd(W=160) == -1 and fwd(rs=175) == -1 and fwd(ps=100) == -1 and fwd(L=0.0) == -1
    assert L.dcvc_ms_ssim_grad(p, p, 1, 3, 176, 176, 176, 176 * 176, 176, 176 * 176, 1.0, 1, ws.data_ptr(), out.data_ptr(),
                               ws.data_ptr(), None) == -1  # clamp01_x with a gradient
    torch.cuda.synchronize(DEV)
    assert float(out) == -7.0
    assert fwd() == 0
    torch.cuda.synchronize(DEV)
    assert float(out) == pytest.approx(1.0, abs=1e-6)


def test_psnr_at_1080p():
    from vcm_ts_amd import metrics as M

    x, y = _pair(1080, 1920, 0.03)
    y = y + 0.2 * (torch.rand(y.shape, generator=torch.Generator().manual_seed(1)) - 0.5)  # some values leave [0, 1]
    got = M.psnr(_on_device(y, 1080), _on_device(x, 1080))
    want = R.psnr(y, x)
    print(f"psnr gpu {float(got):.6f} dB  float64 {want:.6f} dB")
    assert abs(float(got) - want) <= PSNR_TOL_DB
    unclamped = float(10 * torch.log10(1.0 / ((y.double() - x.double()) ** 2).mean()))
    assert abs(float(M.psnr(y.to(DEV), x.to(DEV), clamp01=False)) - unclamped) <= PSNR_TOL_DB


# ----------------------------------------------------------------------------------------------- codec API
EVAL_KEYS = {"bpp_mv_y", "bpp_mv_z", "bpp_y", "bpp_z", "bpp", "me_mse", "mse", "dpb", "bit", "bit_y", "bit_z", "bit_mv_y",
             "bit_mv_z", "_views"}


def _pictures(n=2, t=2, h=256, w=256):
    from vcm_ts_amd.synthetic import frames

    return torch.from_numpy(np.stack([frames(40 + i, t, h, w) for i in range(n)]))  # (N, T, 3, H, W)


def _dmc_noise(seed, N=2, h=256, w=256, device=None):
    g = torch.Generator().manual_seed(seed)
    shapes = (("y", (N, 96, h // 16, w // 16)), ("mv_y", (N, 64, h // 16, w // 16)), ("z", (N, 64, h // 64, w // 64)),
              ("mv_z", (N, 64, h // 64, w // 64)))
    return {k: (torch.rand(s, generator=g) - 0.5).to(device or "cpu") for k, s in shapes}


def _tame_output(dmc):
    """The name-seeded weights are not a trained codec: their reconstruction is unrelated to the picture, some level's
    mean cs is negative, the relu cuts it and MS-SSIM is exactly 0 with a zero gradient -- nothing to compare.  With the
    last convolution scaled down around a mid-grey bias the reconstruction is nearly flat, every cs_map is about
    C2 / (s1 + C2) > 0 (|2 s12| stays below C2), and value and gradient are non-trivial numbers through the whole net."""
    p = dict(dmc.named_parameters())
    with torch.no_grad():
        p["recon_generation_net.recon_conv.weight"].mul_(0.01)
        p["recon_generation_net.recon_conv.bias"].fill_(0.5)
    return dmc


def _ref_dist_gradient(x, recon):
    """d/d recon of sum(1 - ms_ssim(x, recon)) by the float64 restatement's autograd."""
    r = recon.detach().cpu().double().contiguous().requires_grad_()
    (1.0 - R.ms_ssim(x.cpu().double(), r)).sum().backward()
    return r.grad


def _flat_grads(model):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).double().cpu()
                      for _, p in sorted(model.named_parameters())])


def test_dmc_keys_and_eval_value():
    from vcm_ts_amd.dmc import DMC

    clip = _pictures().to(DEV)
    m = _tame_output(DMC().to(DEV)).eval()
    dpb = {"ref_frame": clip[:, 0], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    assert m.report_ssim is False
    assert set(m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0).keys()) == EVAL_KEYS
    m.train()
    assert set(m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0).keys()) == EVAL_KEYS - {"_views"}
    m.eval()
    m.report_ssim = True
    out = m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0)
    assert set(out.keys()) == EVAL_KEYS | {"ssim", "ssim_dist"}
    want = R.ms_ssim(clip[:, 1].cpu().double(), out["dpb"]["ref_frame"].cpu().double().contiguous())
    print("ssim", out["ssim"].tolist(), "ref64", want.tolist())
    assert out["ssim"].shape == (2,) and float(want.min()) > 0.01
    assert float((out["ssim"].cpu().double() - want).abs().max()) <= VALUE_TOL
    assert torch.equal(out["ssim_dist"], 1.0 - out["ssim"])


@pytest.mark.parametrize("graphed", (False, True), ids=("eager", "graph_training"))
def test_dmc_ssim_dist_gradient_enters_through_the_reconstruction(graphed):
    """loss = ssim_dist.sum() in .train() mode must leave the parameter gradients that back-propagating the float64
    restatement's gradient through out["dpb"]["ref_frame"] of an identical forward leaves: only the new link is
    compared, not the codec's own gradient kernels."""
    from vcm_ts_amd.dmc import DMC

    clip = _pictures().to(DEV)
    m = _tame_output(DMC().to(DEV)).train()
    m.report_ssim, m.graph_training = True, graphed
    m._noise_override = _dmc_noise(11, device=DEV)
    for p in m.parameters():
        p.requires_grad_(True)
    dpb = {"ref_frame": clip[:, 0], "ref_feature": None, "ref_y": None, "ref_mv_y": None}
    out = m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0)
    assert out["ssim"].requires_grad and out["ssim_dist"].shape == (2,)
    out["ssim_dist"].sum().backward()
    got = _flat_grads(m)
    for p in m.parameters():
        p.grad = None
    again = m.forward_one_frame(clip[:, 1], dpb, 1.0, 1.0)
    recon = again["dpb"]["ref_frame"]
    assert torch.equal(again["ssim"], out["ssim"])
    recon.backward(_ref_dist_gradient(clip[:, 1], recon).float().to(DEV))
    want = _flat_grads(m)
    if graphed:
        assert len(m._frame_graphs) == 1 and not any(f.busy for f in m._frame_graphs.values())
    err = float((got - want).norm() / want.norm())
    print("parameter gradient relative error", err, "norm", float(want.norm()))
    assert float(want.norm()) > 0 and err <= GRAD_TOL
    m._noise_override = None


def test_intra_ssim_dist_gradient_enters_through_x_hat():
    from vcm_ts_amd.intra import IntraNoAR

    x = _pictures()[:, 0].to(DEV)
    m = IntraNoAR().to(DEV).eval()
    assert "ssim" not in m(x, 1.0)
    m.report_ssim = True
    ev = m(x, 1.0)
    want = R.ms_ssim(x.cpu().double(), ev["x_hat"].cpu().double().contiguous())
    assert float((ev["ssim"].cpu().double() - want).abs().max()) <= VALUE_TOL
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    torch.manual_seed(21)
    out = m(x, 1.0)
    out["ssim_dist"].sum().backward()
    got = _flat_grads(m)
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(21)
    again = m(x, 1.0)
    assert torch.equal(again["ssim"], out["ssim"])
    again["x_hat"].backward(_ref_dist_gradient(x, again["x_hat"]).float().to(DEV))
    want = _flat_grads(m)
    err = float((got - want).norm() / want.norm())
    print("parameter gradient relative error", err)
    assert float(want.norm()) > 0 and err <= GRAD_TOL


def test_wrapper_trains_on_ssim_dist():
    from vcm_ts_amd.dcvc_hem import build_model, make_cfg

    clip = _pictures(t=3).to(DEV)
    model = build_model(make_cfg(lambdas=(85.0, 380.0)), precision="fp32").to(DEV).train()
    model.activate_modules_all()
    _tame_output(model.dmc)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    with pytest.raises((KeyError, AssertionError)):
        model("single", clip, clip, "ssim_dist", ["bpp"], p_frames=1, perceptual_loss=False, optimizer=opt, is_train=True)
    model.dmc.report_ssim = True
    before = {k: v.detach().clone() for k, v in model.dmc.named_parameters()}
    r = model("single", clip, clip, "ssim_dist", ["bpp"], p_frames=1, perceptual_loss=False, optimizer=opt, is_train=True)
    assert r["single_forwards"] == 2
    for k in ("rate", "dist", "loss"):
        assert bool(torch.isfinite(r[k]).all()), k
    assert float(r["dist"].min()) > 0 and float(r["dist"].max()) < 1
    assert any(not torch.equal(v, before[k]) for k, v in model.dmc.named_parameters())


# ----------------------------------------------------------------------------------------------- run_codec --report
REPORT_KEYS = {"frame_pixel_num", "i_frame_num", "p_frame_num", "ave_i_frame_bpp", "ave_i_frame_psnr", "ave_i_frame_msssim",
               "ave_p_frame_bpp", "ave_p_frame_psnr", "ave_p_frame_msssim", "ave_all_frame_bpp", "ave_all_frame_psnr",
               "ave_all_frame_msssim", "frame_bpp", "frame_psnr", "frame_msssim", "frame_type"}


def test_encode_folder_report(tmp_path):
    from PIL import Image

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S
    from vcm_ts_amd.synthetic import frames

    n, gop, h, w = 12, 4, 256, 256
    src = tmp_path / "frames"
    src.mkdir()
    for t, f in enumerate(frames(77, n, h, w)):
        Image.fromarray(np.clip(np.rint(f.transpose(1, 2, 0) * 255), 0, 255).astype(np.uint8)).save(src / f"im{t + 1:05d}.png")
    plain_bits, size = RC.encode_folder(str(src), str(tmp_path / "plain"), gop=gop, q=(1.0, 1.0, 1.0))
    assert size == (h, w)
    # what a decoder reconstructs from those files, as floats
    i_net, p_net = RC._nets(DEV, None)
    i_net.update()
    p_net.update()
    want_psnr, want_ms = [], []
    with torch.no_grad():
        for t in range(n):
            path = str(tmp_path / "plain" / f"im{t + 1:05d}.bin")
            if t % gop == 0:
                hh, ww, qi, payload = S.decode_i(path)
                dpb = {"ref_frame": i_net.decompress(payload, hh, ww, qi / 100)["x_hat"], "ref_feature": None, "ref_y": None,
                       "ref_mv_y": None}
            else:
                qmv, qy, payload = S.decode_p(path)
                dpb = p_net.decompress(dpb, payload, h, w, qmv / 100, qy / 100)["dpb"]
            rec = dpb["ref_frame"][..., :h, :w].cpu().double().clamp(0, 1).contiguous()
            x = torch.from_numpy(RC.PNGReader.load(str(src / f"im{t + 1:05d}.png")))[None].double()
            want_psnr.append(R.psnr(rec, x))
            want_ms.append(float(R.ms_ssim(rec, x)))
    for streams in (1, 2):
        out = tmp_path / f"report{streams}"
        bits, size, rd = RC.encode_folder(str(src), str(out), gop=gop, q=(1.0, 1.0, 1.0), gop_streams=streams,
                                          report=str(tmp_path / f"rd{streams}.json"))
        assert bits == plain_bits
        for t in range(n):
            name = f"im{t + 1:05d}.bin"
            assert (out / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
        on_disk = json.loads((tmp_path / f"rd{streams}.json").read_text())
        assert set(on_disk) == REPORT_KEYS and on_disk == json.loads(json.dumps(rd))
        assert rd["frame_pixel_num"] == h * w and rd["i_frame_num"] == 3 and rd["p_frame_num"] == 9
        assert rd["frame_type"] == [0 if t % gop == 0 else 1 for t in range(n)]
        np.testing.assert_allclose(rd["frame_bpp"], np.array(bits) / (h * w), rtol=1e-12)
        print("streams", streams, "psnr", rd["frame_psnr"], "ms-ssim", rd["frame_msssim"])
        assert np.abs(np.array(rd["frame_psnr"]) - np.array(want_psnr)).max() <= PSNR_TOL_DB
        assert np.abs(np.array(rd["frame_msssim"]) - np.array(want_ms)).max() <= VALUE_TOL
        i_idx = [t for t in range(n) if t % gop == 0]
        p_idx = [t for t in range(n) if t % gop]
        for kind, idx in (("i", i_idx), ("p", p_idx), ("all", list(range(n)))):
            for key, vals in (("bpp", rd["frame_bpp"]), ("psnr", rd["frame_psnr"]), ("msssim", rd["frame_msssim"])):
                assert rd[f"ave_{kind}_frame_{key}"] == pytest.approx(np.mean([vals[t] for t in idx]), rel=1e-9)
