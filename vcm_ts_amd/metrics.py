"""Quality metrics on the device (include/dcvc_hip_metrics.h, csrc/metrics.hip): MS-SSIM with its gradient, and PSNR
from the squared error the same kernel accumulates.

``ms_ssim`` / ``MS_SSIM`` follow pytorch_msssim 1.0 as the reference uses it
(DCVC_HEM/src/models/common_model.py:7,29: ``MS_SSIM(data_range=1.0, size_average=False)``; src/utils/common.py:63-112
for the test harness's PSNR and MS-SSIM per picture).  Inputs are fp32 (N, C, H, W) tensors on the GPU; a crop
``t[..., :h, :w]`` of a contiguous tensor is read in place through its strides.  There is no fallback: anything the
kernels do not take is a ValueError, never a quiet torch implementation.
"""
from __future__ import annotations

import torch
from torch import nn

from . import devargs, lib
from .devargs import MAX_SIDE, planar

MIN_SIDE = 161  # pytorch_msssim asserts min(H, W) > (11 - 1) * 2**4


def _check(x, y):
    for t in (x, y):
        devargs.on_gpu(t, "ms_ssim", noun="operand")
        if t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"ms_ssim: expected (N, C, H, W) float32 operands, got {tuple(t.shape)} {t.dtype}")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"operands differ: {tuple(x.shape)} on {x.device} and {tuple(y.shape)} on {y.device}")
    if min(x.shape[-2:]) < MIN_SIDE:
        raise ValueError(f"image sides must exceed 160 for the five levels of MS-SSIM, got {tuple(x.shape[-2:])}")
    if x.shape[0] < 1 or x.shape[1] < 1 or x.shape[0] * x.shape[1] > 65535 or max(x.shape[-2:]) > MAX_SIDE:
        raise ValueError(f"unsupported shape {tuple(x.shape)}")


def _workspace(N, C_, H, W, want_grad, device):
    n = lib.hip().dcvc_ms_ssim_workspace_bytes(N, C_, H, W, int(want_grad))
    if n <= 0:
        raise ValueError(f"unsupported shape {(N, C_, H, W)}")
    return torch.empty(n // 4, dtype=torch.float32, device=device)


def measure(x, y, data_range=1.0, clamp01=False, want_levels=False, want_sse=True):
    """One forward launch sequence, nothing read back: (ms (N,), kept level values (5, N, C) or None, per-sample sum of
    squared differences (N,) or None).  clamp01 clamps `x` to [0, 1] as it is loaded."""
    _check(x, y)
    x, y = x.detach(), y.detach()
    N, C_, H, W = x.shape
    xs, xr, xp = planar(x)
    ys, yr, yp = planar(y)
    ws = _workspace(N, C_, H, W, False, x.device)
    ms = torch.empty(N, dtype=torch.float32, device=x.device)
    levels = torch.empty((5, N, C_), dtype=torch.float32, device=x.device) if want_levels else None
    sse = torch.empty(N, dtype=torch.float32, device=x.device) if want_sse else None
    devargs.launch("dcvc_ms_ssim", x.device, xs.data_ptr(), ys.data_ptr(), N, C_, H, W, xr, xp, yr, yp, float(data_range),
                   int(bool(clamp01)), ws.data_ptr(), ms.data_ptr(), None if levels is None else levels.data_ptr(),
                   None if sse is None else sse.data_ptr())
    return ms, levels, sse


def _grad(x, y, g_ms, data_range):
    """d/dx of sum_n g_ms[n] * ms_ssim(x, y)[n]"""
    N, C_, H, W = x.shape
    xs, xr, xp = planar(x)
    ys, yr, yp = planar(y)
    ws = _workspace(N, C_, H, W, True, x.device)
    gx = torch.empty((N, C_, H, W), dtype=torch.float32, device=x.device)
    g_ms = g_ms.detach().to(torch.float32).contiguous()
    devargs.launch("dcvc_ms_ssim_grad", x.device, xs.data_ptr(), ys.data_ptr(), N, C_, H, W, xr, xp, yr, yp, float(data_range),
                   0, ws.data_ptr(), g_ms.data_ptr(), gx.data_ptr())
    return gx


class _MsSsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range, clamp01):
        if clamp01 and x.requires_grad:
            raise ValueError("ms_ssim(clamp01=True) is not differentiable in its first argument")
        ms, _, _ = measure(x, y, data_range, clamp01, want_sse=False)
        ctx.save_for_backward(x, y)
        ctx.data_range, ctx.clamp01 = data_range, clamp01
        return ms

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        x, y = x.detach(), y.detach()
        if ctx.clamp01:  # (only y can want a gradient here: its partner is the clamped picture)
            x = x.clamp(0.0, 1.0)
        gx = _grad(x, y, g, ctx.data_range) if ctx.needs_input_grad[0] else None
        gy = _grad(y, x, g, ctx.data_range) if ctx.needs_input_grad[1] else None  # the function is symmetric
        return gx, gy, None, None


def ms_ssim(x, y, data_range=1.0, size_average=True, clamp01=False):
    """pytorch_msssim.ms_ssim(x, y, data_range, size_average) for fp32 GPU tensors, differentiable in either argument.
    (N,) values with size_average=False, their mean otherwise.  clamp01: clamp `x` to [0, 1] on load."""
    _check(x, y)
    ms = _MsSsimFn.apply(x, y, float(data_range), bool(clamp01))
    return ms.mean() if size_average else ms


class MS_SSIM(nn.Module):
    """The module the reference's codec base class owns: MS_SSIM(data_range=1.0, size_average=False)."""

    def __init__(self, data_range=1.0, size_average=True):
        super().__init__()
        self.data_range, self.size_average = data_range, size_average

    def forward(self, x, y):
        return ms_ssim(x, y, data_range=self.data_range, size_average=self.size_average)


def psnr_from_sse(sse, elements_per_sample):
    """10 log10(1 / mse), mse over ALL elements of the batch (DCVC_HEM/test_video.py:74-77)."""
    mse = sse.double().sum() / (elements_per_sample * sse.numel())
    return 10.0 * torch.log10(1.0 / mse)


def psnr(x_hat, x, clamp01=True):
    """PSNR in dB of `x_hat` (clamped to [0, 1] by default, as the test harness does) against `x`, as a 0-d float64
    tensor on the device; the squared error comes from the MS-SSIM kernel's loads (same size limits)."""
    _, _, sse = measure(x_hat, x, 1.0, clamp01, want_sse=True)
    return psnr_from_sse(sse, x.shape[1] * x.shape[2] * x.shape[3])
