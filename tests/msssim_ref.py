"""The yardstick of tests/test_gpu_metrics.py: pytorch_msssim.ms_ssim (1.0) restated with stock torch on the CPU, float64 by
default, its gradient from autograd.  The package itself is not installed where this suite runs, so this restatement is
"parity unpinned against the package"  -- it follows the definition in include/dcvc_hip_metrics.h, which is
the package's code path for 4-d inputs: depth-wise separable 11-tap Gaussian without padding, five levels,
avg_pool2d(2, padding=size % 2) between them, relu on the kept values, weighted product, mean over the channels.
"""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(dtype=torch.float64, size=11, sigma=1.5):
    coords = torch.arange(size, dtype=dtype) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def gaussian_filter(x, win):
    C = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return F.conv2d(x, win.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)


def ssim_level(x, y, win, data_range=1.0):
    """(ssim, cs), each (N, C): the means of the two maps over the valid pixels."""
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = gaussian_filter(x, win), gaussian_filter(y, win)
    s1 = gaussian_filter(x * x, win) - mu1 * mu1
    s2 = gaussian_filter(y * y, win) - mu2 * mu2
    s12 = gaussian_filter(x * y, win) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def level_sizes(n, levels=5):
    out = [n]
    for _ in range(levels - 1):
        n = (n + 2 * (n % 2) - 2) // 2 + 1
        out.append(n)
    return out


def ms_ssim_levels(x, y, data_range=1.0):
    """(5, N, C): relu(cs) of levels 0..3, relu(ssim) of level 4."""
    if min(x.shape[-2:]) <= (11 - 1) * 2 ** 4:
        raise ValueError("image sides must exceed 160 for five levels")
    win = window(x.dtype)
    kept = []
    for level in range(5):
        ssim, cs = ssim_level(x, y, win, data_range)
        if level < 4:
            kept.append(torch.relu(cs))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, kernel_size=2, padding=pad), F.avg_pool2d(y, kernel_size=2, padding=pad)
    kept.append(torch.relu(ssim))
    return torch.stack(kept, 0)


def ms_ssim(x, y, data_range=1.0, size_average=False):
    """x, y: (N, C, H, W) CPU tensors of one floating dtype.  (N,) per-sample values, or their mean."""
    kept = ms_ssim_levels(x, y, data_range)
    w = torch.tensor(WEIGHTS, dtype=x.dtype).view(-1, 1, 1)
    val = torch.prod(kept ** w, dim=0).mean(1)
    return val.mean() if size_average else val


def psnr(x_hat, x):
    """10 log10(1 / mse) over all elements, the first operand clamped to [0, 1] (float64 throughout)."""
    mse = ((x_hat.double().clamp(0, 1) - x.double()) ** 2).mean()
    return float(10 * torch.log10(1.0 / mse))


def smooth_pair(seed, N, C, H, W, sigma):
    """The issue's test images: smooth random pictures in [0, 1] (float32), the second one with Gaussian error of
    standard deviation `sigma` on two thirds of the picture and exactly equal to the first on the rest."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(N, C, (H + 7) // 8 + 2, (W + 7) // 8 + 2, generator=g, dtype=torch.float64)
    x = F.interpolate(low, scale_factor=8, mode="bicubic", align_corners=False)[..., 4 : 4 + H, 4 : 4 + W]
    x = (0.8 * x + 0.1 + 0.02 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    noise = sigma * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    noise[..., :, (2 * W) // 3 :] = 0
    y = x + noise
    return x.float().contiguous(), y.float().contiguous()
