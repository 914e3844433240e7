"""References of the hand-written backward kernels (csrc/backward.hip) for tests/test_backward_ref_host.py and
tests/test_gpu_backward_exact.py: torch CPU autograd in float64, and generators of EXACT data.

Why exact data.  The fp32 weight gradient is a chain of fmaf's, its bf16 split is exact whenever the operands fit in
bf16, the warp scatter is integer fixed point with a power-of-two scale and up2's weights are dyadic.  With small
integers (|v| <= 4) and dyadic slopes / gates / flows every product and every partial sum is a multiple of one
quantum q, and as long as every partial sum stays below 2^24 q it is exactly representable in fp32: the fp32 result
then does not depend on the summation order, the tiling or the split count, and equals the float64 result cast to
fp32 BIT FOR BIT.  Every generator asserts that 2^24 q condition on an upper bound of its partial sums (`headroom`),
and the host tests show the order-independence on the references alone (fp64 == fp32 == fp32 on the flipped problem).

What exact data cannot see: integers have a zero bf16 `lo` part, so the hi.lo and lo.hi MFMAs of the fast weight
gradient contribute nothing.  `wgrad_float` + `wgrad_magnitude` serve the float-valued per-element bounds for those.

Nothing here touches a GPU."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dcvc_ref as R

F32 = np.float32
TWO24 = float(2 ** 24)
VMAX = 4  # |integer| of every exact operand


def ints(g, shape, vmax=VMAX):
    return torch.randint(-vmax, vmax + 1, tuple(shape), generator=g).float()


def quantum(slope):
    """the grid a LeakyReLU with this slope keeps integers on"""
    if slope is None or slope == 0 or slope >= 1:
        return 1.0
    assert slope in (0.25, 0.5), slope
    return float(slope)


def assert_bits(got, want, what="", axes=None):
    """Bit-for-bit equality of two fp32 arrays; on failure names the tensor, the index (labelled by `axes`, e.g.
    "co,ci,ky,kx") and the got / want values with their bit patterns."""
    got = np.ascontiguousarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=F32)
    want = np.ascontiguousarray(want.detach().cpu().numpy() if torch.is_tensor(want) else want, dtype=F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gb, wb = got.view(np.uint32).ravel(), want.view(np.uint32).ravel()
    # +0 and -0 are different bit patterns of the same gradient: a sum of exact terms that cancels gives +0 in every
    # order, a product with a zero factor keeps the sign of the other -- both conventions are "exact"
    bad = np.flatnonzero((gb != wb) & ~((got.ravel() == 0) & (want.ravel() == 0)))
    if bad.size:
        i = np.unravel_index(bad[0], got.shape)
        where = f"({axes})={tuple(int(v) for v in i)}" if axes else f"{tuple(int(v) for v in i)}"
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at {where}: got "
                             f"{got.ravel()[bad[0]]!r} (0x{gb[bad[0]]:08x}) want {want.ravel()[bad[0]]!r} (0x{wb[bad[0]]:08x})")


def _headroom(bounds):
    """bounds: {name: (largest |partial sum| bound, quantum)} -> the smallest 2^24 q / bound, asserted > 1"""
    worst = min(TWO24 * q / max(m, q) for m, q in bounds.values())
    for k, (m, q) in bounds.items():
        assert m < TWO24 * q, f"{k}: partial sums up to {m} are not exact on the grid {q}"
    return worst


# =====================================================================================================================
# convolution: whole layer (the signature of tests/diag/grad_check.py::conv_case)
def conv_geometry(ks, stride, H, W):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def conv_exact(seg_C, Cout, ks, stride, H, W, N=2, in_slope=None, out_slope=None, ps=False, res=False, res2=False,
               gate=False, cin_slice=None, seed=0):
    """Exact data of one layer.  x, w, b, dY, res, res2: integers |v| <= 4 (slopes must come from {0, 0.25, 0.5}); gates
    from {0.5, 1, 2}.  The top-left corner of x is zero and every second bias is zero, so the pre-activations of those
    channels there are exactly 0 (the activation's derivative at 0 is `slope`, for torch and for the kernels), and the
    zeros of x sit on the activation-on-load's kink."""
    g = torch.Generator().manual_seed(7000 + seed)
    Cin = sum(seg_C)
    CinT = Cin if cin_slice is None else cin_slice[2]
    Ho, Wo = conv_geometry(ks, stride, H, W)
    m = 2 if ps else 1
    Cf = Cout // 4 if ps else Cout
    c = dict(seg_C=tuple(seg_C), Cout=Cout, ks=ks, stride=stride, H=H, W=W, N=N, in_slope=in_slope, out_slope=out_slope,
             ps=ps, cin_slice=cin_slice, Ho=Ho, Wo=Wo)
    c["w"] = ints(g, (Cout, CinT, ks, ks))
    c["b"] = ints(g, (Cout,))
    c["b"][::2] = 0
    c["xs"] = [ints(g, (N, ci, H, W)) for ci in seg_C]
    for x in c["xs"]:
        x[0, :, : ks + stride, : ks + stride] = 0
    c["res"] = ints(g, (N, Cf, Ho * m, Wo * m)) if res else None
    c["res2"] = ints(g, (N, Cf, Ho * m, Wo * m)) if res2 else None
    c["gate"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, Cf), generator=g)] if gate else None
    c["dout"] = ints(g, (N, Cf, Ho * m, Wo * m))
    qx, qd = quantum(in_slope), quantum(out_slope)
    V = float(VMAX)
    c["headroom"] = _headroom({
        "forward": (Cin * ks * ks * V * V + V, qx),
        "dw": (N * Ho * Wo * V * V, qx * qd),
        "db": (N * Ho * Wo * V, qd),
        "dx": (Cout * ks * ks * V * V, qd * qx),
        "dgate": (Ho * m * Wo * m * V * V, 1.0),
        "dres": (2 * V, 0.5),
    })
    return c


def conv_backward(c, dtype=torch.float64):
    """torch CPU autograd of the layer in `dtype`; every result cast to fp32."""
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_()
    xr = [leaf(x) for x in c["xs"]]
    wr, br, rr, rr2, gr = leaf(c["w"]), leaf(c["b"]), leaf(c["res"]), leaf(c["res2"]), leaf(c["gate"])
    xin = torch.cat(xr, 1)
    if c["in_slope"] is not None:
        xin = F.leaky_relu(xin, c["in_slope"])
    ws = wr if c["cin_slice"] is None else wr[:, c["cin_slice"][0]:c["cin_slice"][1]]
    y = F.conv2d(xin, ws, br, stride=c["stride"], padding=c["ks"] // 2)
    if c["out_slope"] is not None:
        y = F.leaky_relu(y, c["out_slope"])
    if c["ps"]:
        y = F.pixel_shuffle(y, 2)
    if rr is not None:
        y = y + (rr * gr[:, :, None, None] if gr is not None else rr)
    if rr2 is not None:
        y = rr2 + y
    y.backward(c["dout"].to(dtype))
    out = {"out": y.detach().float(), "dw": wr.grad.float(), "db": br.grad.float()}
    for i, x in enumerate(xr):
        out[f"dx{i}"] = x.grad.float()
    if rr is not None:
        out["dres"] = rr.grad.float()
    if rr2 is not None:
        out["dres2"] = rr2.grad.float()
    if gr is not None:
        out["dgate"] = gr.grad.float()
    return out


CONV_AXES = {"out": "n,c,y,x", "dw": "co,ci,ky,kx", "db": "co", "dres": "n,c,y,x", "dres2": "n,c,y,x", "dgate": "n,c"}


def conv_axes(k):
    return CONV_AXES.get(k, "n,c,y,x")


def conv_flipped(c):
    """The same layer with the batch reversed and, where the geometry is symmetric (stride-1 without PixelShuffle, or a
    stride-2 axis whose last window ends on the last pixel), each spatial axis reversed: a different order of every
    sum.  -> (flipped case, function mapping the flipped problem's results back)."""
    dims = [0]
    pad = c["ks"] // 2
    if not c["ps"]:
        for d, L in ((2, c["H"]), (3, c["W"])):
            if (L + 2 * pad - c["ks"]) % c["stride"] == 0:
                dims.append(d)
    sp = [d for d in dims if d >= 2]
    f = dict(c)
    f["xs"] = [x.flip(dims) for x in c["xs"]]
    f["w"] = c["w"].flip(sp) if sp else c["w"]
    for k in ("res", "res2", "dout"):
        f[k] = c[k].flip(dims) if c[k] is not None else None
    f["gate"] = c["gate"].flip([0]) if c["gate"] is not None else None

    def back(r):
        o = {}
        for k, v in r.items():
            if k == "dw":
                o[k] = v.flip(sp) if sp else v
            elif k == "db":
                o[k] = v
            elif k == "dgate":
                o[k] = v.flip([0])
            else:
                o[k] = v.flip(dims)
        return o

    return f, back


# =====================================================================================================================
# weight gradient alone (the C ABI of dcvc_conv_wgrad)
def wgrad(x, dpre, ks, stride, in_slope=None, dtype=torch.float64):
    """x (N, C, H, W), dpre (N, Cout, Ho, Wo) -> dw (Cout, C, ks, ks), db (Cout) in `dtype`, by autograd of F.conv2d"""
    xin = x.to(dtype)
    if in_slope is not None:
        xin = F.leaky_relu(xin, in_slope)
    w = torch.zeros(dpre.shape[1], x.shape[1], ks, ks, dtype=dtype, requires_grad=True)
    y = F.conv2d(xin, w, stride=stride, padding=ks // 2)
    assert y.shape == dpre.shape, (y.shape, dpre.shape)
    y.backward(dpre.to(dtype))
    return w.grad, dpre.to(dtype).sum((0, 2, 3))


def wgrad_exact(C, Cout, ks, stride, H, W, N=1, in_slope=None, seed=0):
    """-> x (N, C, H, W), dpre (N, Cout, Ho, Wo): integers |v| <= 4, with zeros of x planted for the activation on load"""
    g = torch.Generator().manual_seed(9000 + seed)
    Ho, Wo = conv_geometry(ks, stride, H, W)
    x, dpre = ints(g, (N, C, H, W)), ints(g, (N, Cout, Ho, Wo))
    x[0, :, :2, :3] = 0
    q = quantum(in_slope)
    _headroom({"dw": (N * Ho * Wo * float(VMAX * VMAX), q), "db": (N * Ho * Wo * float(VMAX), 1.0)})
    return x, dpre


def wgrad_float(C, Cout, ks, H, W, N, dy_mag, seed=0):
    """Float-valued data of the per-element bounds: x = randn * a per-channel magnitude from {1e-4, 1, 30},
    dY = randn * dy_mag (the issue's per-call magnitudes are 1e-9, 1, 3e4)."""
    g = torch.Generator().manual_seed(11000 + seed)
    mags = torch.tensor([1e-4, 1.0, 30.0])[torch.arange(C) % 3][torch.randperm(C, generator=g)]
    x = torch.randn(N, C, H, W, generator=g) * mags.view(1, C, 1, 1)
    Ho, Wo = conv_geometry(ks, 1, H, W)
    dy = torch.randn(N, Cout, Ho, Wo, generator=g) * dy_mag
    return x, dy


def wgrad_magnitude(x, dpre, ks, stride):
    """M_e = sum |dY| |X| per weight element, float64"""
    return wgrad(x.abs(), dpre.abs(), ks, stride)[0]


def wgrad_magnitude_brute(x, dpre, ks, stride):
    x, d = x.double().numpy(), dpre.double().numpy()
    N, C, H, W = x.shape
    _, Cout, Ho, Wo = d.shape
    pad = ks // 2
    M = np.zeros((Cout, C, ks, ks))
    for co in range(Cout):
        for ci in range(C):
            for ky in range(ks):
                for kx in range(ks):
                    s = 0.0
                    for n in range(N):
                        for oy in range(Ho):
                            for ox in range(Wo):
                                iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                                if 0 <= iy < H and 0 <= ix < W:
                                    s += abs(d[n, co, oy, ox]) * abs(x[n, ci, iy, ix])
                    M[co, ci, ky, kx] = s
    return M


def largest_product(x, dpre, ks, stride, idx):
    """the largest-magnitude single product dY * X of weight element idx = (co, ci, ky, kx), float64"""
    co, ci, ky, kx = idx
    pad = ks // 2
    xp = F.pad(x.double(), (pad, pad, pad, pad))
    Ho, Wo = dpre.shape[2:]
    win = xp[:, ci, ky: ky + (Ho - 1) * stride + 1: stride, kx: kx + (Wo - 1) * stride + 1: stride]
    p = (dpre.double()[:, co] * win).reshape(-1)
    return float(p[p.abs().argmax()])


def bf16_round(t):
    return t.to(torch.bfloat16).double()


def fp32_constant(ref32, ref64, M):
    """c of the fp32 bound c * 2^-24 * M_e: 4 x the reference's own worst error in units of 2^-24 M_e (the factor 4 is
    the tier-B margin of tests/diag/grad_check.py::tier_check: another summation order of the same arithmetic)"""
    ok = M > 0
    return 4.0 * float(((ref32.double() - ref64).abs()[ok] / (2.0 ** -24 * M[ok])).max())


FLOAT_CASES = [(1, 40, 33), (3, 64, 64), (7, 8, 32)]  # ks, C, Cout of the float-valued bounds: 17 x 45, 2 x 5 tiles
FLOAT_HW, FLOAT_N = (17, 45), 1
DY_MAGS = (1e-9, 1.0, 3e4)


@functools.lru_cache(maxsize=None)
def float_case(ks, C, Cout, mag):
    """-> x, dY, ref64, ref32 (torch's fp32 CPU autograd of the same case), M: computed once, shared, never modified"""
    x, dy = wgrad_float(C, Cout, ks, *FLOAT_HW, FLOAT_N, mag, seed=ks)
    ref64 = wgrad(x, dy, ks, 1)[0]
    ref32 = wgrad(x, dy, ks, 1, dtype=torch.float32)[0]
    return x, dy, ref64, ref32, wgrad_magnitude(x, dy, ks, 1)


# =====================================================================================================================
# warp
WARP_SIZES = (3, 5, 9, 17, 33)  # (size - 1) / 2 is a power of two: ix = x + fx exactly, for torch's grid and the kernel's


def warp_exact(C, N, H, W, seed=0, dout_scale=1.0):
    """src, dout: integers |v| <= 4 (dout times a power of two: the scatter's fixed-point scale adapts per call);
    flow: multiples of 1/8 such that the sample positions are, by pixel category,
      0 sub-pixel, inside              1 exactly on integer lines, inside
      2 exactly on a border line (x = 0 or W-1, or y = 0 or H-1; the other coordinate sub-pixel)
      3 beyond a border (every side occurs)   4 all at one sub-pixel position (1.5, 1.25): one 2x2 source block
      5 all exactly at source pixel (1, 1).
    Every category occurs in every sample.  prefill_*: what dsrc / dflow hold before the call (+= semantics)."""
    assert H in WARP_SIZES and W in WARP_SIZES
    g = torch.Generator().manual_seed(13000 + seed)
    src = ints(g, (N, C, H, W))
    dout = ints(g, (N, C, H, W)) * dout_scale
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    cat = torch.randint(0, 6, (N, H, W), generator=g)
    side = torch.randint(0, 4, (N, H, W), generator=g)      # 0 left, 1 right, 2 top, 3 bottom
    k = torch.arange(min(24, H * W))                        # the first pixels: every category, with every side in turn
    cat.view(N, -1)[:, : len(k)] = k % 6
    side.view(N, -1)[:, : len(k)] = (k // 6 + 2 * torch.arange(N).view(N, 1)) % 4
    eighth = lambda lo, hi: torch.randint(int(lo * 8), int(hi * 8) + 1, (N, H, W), generator=g).float() / 8
    tx, ty = eighth(0.125, W - 1.125), eighth(0.125, H - 1.125)              # 0: strictly inside, any eighth
    ix_int = torch.randint(1, max(W - 1, 2), (N, H, W), generator=g).float()
    iy_int = torch.randint(1, max(H - 1, 2), (N, H, W), generator=g).float()
    tx, ty = torch.where(cat == 1, ix_int, tx), torch.where(cat == 1, iy_int, ty)
    bx = torch.where(side == 0, torch.zeros(()), torch.full((), W - 1.0))
    by = torch.where(side == 2, torch.zeros(()), torch.full((), H - 1.0))
    tx = torch.where((cat == 2) & (side < 2), bx, tx)
    ty = torch.where((cat == 2) & (side >= 2), by, ty)
    far = eighth(0.125, 3.0)
    tx = torch.where((cat == 3) & (side == 0), -far, torch.where((cat == 3) & (side == 1), W - 1 + far, tx))
    ty = torch.where((cat == 3) & (side == 2), -far, torch.where((cat == 3) & (side == 3), H - 1 + far, ty))
    tx, ty = torch.where(cat == 4, torch.full((), 1.5), tx), torch.where(cat == 4, torch.full((), 1.25), ty)
    tx, ty = torch.where(cat == 5, torch.ones(()), tx), torch.where(cat == 5, torch.ones(()), ty)
    flow = torch.stack([tx - xx, ty - yy], 1)
    assert torch.equal(flow * 8, (flow * 8).round())
    for k in range(6):
        assert bool((cat == k).flatten(1).any(1).all()), k
    d = dict(src=src, flow=flow, dout=dout, cat=cat, dout_scale=dout_scale,
             prefill_src=ints(g, (N, C, H, W)) * dout_scale, prefill_flow=ints(g, (N, 2, H, W)) * dout_scale)
    V = float(VMAX)
    # dsrc: every pixel's tap may land on one source element (weights are multiples of 1/64, <= 1); dflow: C channels of
    # |g| * (|s| |dv| + |n| |dv|) <= V * 2V on the grid 1/8; both relative to the power-of-two dout scale
    d["headroom"] = _headroom({"dsrc": (H * W * V + V, 1.0 / 64), "dflow": (C * V * 2 * V + V, 1.0 / 8)})
    return d


def warp_positions(flow):
    """sample positions in pixels (float64, exact for warp_exact's sizes): ix = x + fx, iy = y + fy"""
    N, _, H, W = flow.shape
    ix = torch.arange(W, dtype=torch.float64).view(1, 1, W) + flow[:, 0].double()
    iy = torch.arange(H, dtype=torch.float64).view(1, H, 1) + flow[:, 1].double()
    return ix, iy


def warp_masks(flow):
    """(N, 2, H, W) bool: False where the documented convention zeroes dflow (position at or beyond the border)"""
    N, _, H, W = flow.shape
    ix, iy = warp_positions(flow)
    return torch.stack([(ix > 0) & (ix < W - 1), (iy > 0) & (iy < H - 1)], 1)


def warp_backward(src, flow, dout, dtype=torch.float64):
    """autograd of oracle.dcvc_ref.warp (F.grid_sample bilinear / border / align_corners) -> dsrc, dflow in `dtype`"""
    s, f = src.detach().to(dtype).clone().requires_grad_(), flow.detach().to(dtype).clone().requires_grad_()
    R.warp(s, f).backward(dout.to(dtype))
    return s.grad, f.grad


def warp_backward_plain(src, flow, dout):
    """The convention include/dcvc_hip_grad.h documents, written out in float64 numpy without torch: floor taps, taps
    beyond the last row / column dropped, dflow zero where the position is <= 0 or >= size - 1.  The host test holds
    torch's grid_sample backward against this at the planted positions."""
    N, C, H, W = src.shape
    ix, iy = (t.numpy() for t in warp_positions(flow))
    mx = ~((ix <= 0) | (ix >= W - 1))
    my = ~((iy <= 0) | (iy >= H - 1))
    ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    w, nn = ix - x0, iy - y0
    e, s = 1 - w, 1 - nn
    x1in, y1in = x0 + 1 <= W - 1, y0 + 1 <= H - 1
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    S = src.double().numpy().transpose(0, 2, 3, 1)   # NHWC
    G = dout.double().numpy().transpose(0, 2, 3, 1)
    n = np.broadcast_to(np.arange(N).reshape(N, 1, 1), (N, H, W))
    tap = lambda yi, xi, ok: S[n, yi, xi] * ok[..., None]
    vnw, vne = tap(y0, x0, np.ones_like(x1in)), tap(y0, x1, x1in)
    vsw, vse = tap(y1, x0, y1in), tap(y1, x1, x1in & y1in)
    s_, nn_, e_, w_ = (t[..., None] for t in (s, nn, e, w))
    gx = (G * (s_ * (vne - vnw) + nn_ * (vse - vsw))).sum(-1) * mx
    gy = (G * (e_ * (vsw - vnw) + w_ * (vse - vne))).sum(-1) * my
    ds = np.zeros_like(S)
    for yi, xi, wt, ok in ((y0, x0, s * e, np.ones_like(x1in)), (y0, x1, s * w, x1in), (y1, x0, nn * e, y1in),
                           (y1, x1, nn * w, x1in & y1in)):
        np.add.at(ds, (n, yi, xi), G * (wt * ok)[..., None])
    return ds.transpose(0, 3, 1, 2), np.stack([gx, gy], 1)


def warp_flipped(d):
    """batch and x axis reversed (positions mirror: flow_x changes sign) -> (src, flow, dout), back(dsrc, dflow)"""
    dims = [0, 3]
    flow = d["flow"].flip(dims) * torch.tensor([-1.0, 1.0]).view(1, 2, 1, 1)

    def back(ds, df):
        return ds.flip(dims), df.flip(dims) * torch.tensor([-1.0, 1.0], dtype=df.dtype).view(1, 2, 1, 1)

    return (d["src"].flip(dims), flow, d["dout"].flip(dims)), back


# =====================================================================================================================
# up2 / down2
def resample_exact(N, C, H, W, factor, seed=0):
    """integer dout of the (N, C, H * factor, W * factor) output (factor 2: up2; 0.5: down2) and integer prefill of dsrc"""
    g = torch.Generator().manual_seed(15000 + seed)
    dout = ints(g, (N, C, int(H * factor), int(W * factor)))
    prefill = ints(g, (N, C, H, W))
    # <= 36 output pixels reach one source element with weights on the grid 1/16 (up2), one with weight 1/4 (down2);
    # scales 0.5 .. 2
    _headroom({"dsrc": (36 * float(VMAX) * 2 + VMAX, 1.0 / 32)})
    return dout, prefill


def up2_backward(dout, scale, prefill=None, dtype=torch.float64):
    N, C, H2, W2 = dout.shape
    x = torch.zeros(N, C, H2 // 2, W2 // 2, dtype=dtype, requires_grad=True)
    (R.up2(x) * scale).backward(dout.to(dtype))
    return x.grad if prefill is None else x.grad + prefill.to(dtype)


def down2_backward(dout, scale, prefill=None, dtype=torch.float64):
    N, C, Hh, Wh = dout.shape
    x = torch.zeros(N, C, Hh * 2, Wh * 2, dtype=dtype, requires_grad=True)
    (R.down2(x) * scale).backward(dout.to(dtype))
    return x.grad if prefill is None else x.grad + prefill.to(dtype)
