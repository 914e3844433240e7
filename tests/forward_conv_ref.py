"""References of the forward convolution kernels (csrc/conv_mfma.hip, conv_small.hip, conv_k32.hip) for
tests/test_forward_conv_ref_host.py and tests/test_gpu_conv_exact.py: torch's CPU convolution in float64 with the
kernels' epilogue, generators of EXACT data, `split64`, the documented split-fp16 arithmetic restated in float64, and
`fmaf_chain`, fp32 mode restated as the chain of fused multiply-adds in the order conv_mfma.hip documents.

Three exact families.  In each every product and every partial sum is a multiple of one quantum q and stays below
2^24 q, so the fp32 accumulation of the kernels is exact whatever its order, tiling or instruction shape, and the result
is the float64 result cast to fp32 BIT FOR BIT (tests/backward_ref.py explains the principle; every generator asserts
the 2^24 q condition as `headroom`, the host test shows the order-independence on the references alone).

  "int"    x, w, b, residuals: integers |v| <= 4; slopes from {0, 1/4, 1/2}; gates from {1/2, 1, 2}.  The lo parts of
           the split-fp16 operands are zero: this family sees indexing, tiling, epilogues -- not the lo planes.
  "gridx"  x = k 2^-10, |x| <= 4, against integer w;   "gridw": integer x against w = k 2^-10, |w| <= 4.
           8 x = k 2^-7 (64 w = k 2^-4) with |k| <= 4096 needs 13 bits: fp16 holds 11, the rest is lo = sv - hi, exact,
           and NON-ZERO exactly for odd k beyond 2048.  The generator draws at least half of the gridded operands from
           there (a uniform draw gives 25 %) and asserts the share.  The other operand is an integer, whose lo is zero:
           the dropped xl.wl is exactly zero, so xh.wh + xh.wl + xl.wh is the exact product and the lo planes carry data
           that a wrong lane group, a swapped plane or a flushed lo would lose.  (The integer operand's magnitude is
           lowered where Cin ks^2 would exhaust the headroom: the 7x7 cases.)
  "sub"    x = k 2^-27, |k| <= 2^10: 8 x = k 2^-24 lies on fp16's SUBNORMAL grid (hi is a subnormal, lo zero); integer w,
           no activation, zero bias, no residual.  Pins "gfx950's MFMA honours fp16 subnormals" and the denormal mode of
           the fp32 -> fp16 conversion, per kernel.

Nothing here touches a GPU."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import backward_ref as BR

F16_MAX = 65504.0
ACT_SCALE, WGT_SCALE = 8.0, 64.0
ACT_LIMIT = F16_MAX / ACT_SCALE  # 8188
GRID = 2.0 ** -10
SUB = 2.0 ** -27
FAMILIES = ("int", "gridx", "gridw", "sub")


def _grid_ints(g, shape, share=0.6):
    """k with |k| <= 4096; about `share` of them odd and beyond 2048 (the values whose fp16 lo part is non-zero)"""
    k = torch.randint(-4096, 4097, tuple(shape), generator=g)
    odd = 2049 + 2 * torch.randint(0, 1024, tuple(shape), generator=g)  # 2049 .. 4095, odd
    sign = 1 - 2 * torch.randint(0, 2, tuple(shape), generator=g)
    pick = torch.rand(tuple(shape), generator=g) < share
    return torch.where(pick, odd * sign, k).float()


def lo_share(v, scale):
    """fraction of the elements of v whose split-fp16 lo part (at pre-scale `scale`) is non-zero"""
    hi, lo = split_f16(v, scale)
    return float((lo != 0).mean())


def exact_case(family, seg_C, Cout, ks, stride, H, W, N=2, in_slope=None, out_act=0, out_slope=None, ps=False, res=False,
               gate=False, res2=False, seed=0):
    """Exact data of one layer -> dict.  out_act as dcvc_conv_args: 0 none, 1 LeakyReLU(out_slope), 2 clamp to [0, 1],
    3 the mask epilogue (res2 is the mask source: out = conv * (res2 > 0 ? 1 : out_slope) [+ res]).  The top-left corner
    of image 0 is zero, so zeros sit on the kink of the activation on load."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(21000 + seed)
    Cin = sum(seg_C)
    Ho, Wo = BR.conv_geometry(ks, stride, H, W)
    m = 2 if ps else 1
    Cf = Cout // 4 if ps else Cout
    if out_act in (1, 3):
        assert out_slope in (0, 0.0, 0.25, 0.5), out_slope
    assert out_act != 3 or res2
    if family == "sub":
        assert in_slope is None and out_act == 0 and not (res or res2 or gate)
    V = float(BR.VMAX)
    qx = BR.quantum(in_slope)
    # largest integer magnitude of the NON-gridded operand that keeps every partial sum below 2^24 quanta; the epilogue's
    # terms (bias V, gated residual 2 V, second residual V) are counted four times, which covers a pre-activation shrunk
    # by an output slope of 1/4 before they are added
    extras = 4 * 4 * V
    if family == "int":
        imax, q, big = BR.VMAX, qx, V
    elif family in ("gridx", "gridw"):
        q, big = GRID * qx, V
        imax = max((i for i in range(1, BR.VMAX + 1) if Cin * ks * ks * V * i + extras < BR.TWO24 * q), default=0)
        assert imax >= 1, f"{family} {seg_C} k{ks}: no integer magnitude leaves headroom"
    else:
        imax, q, big = BR.VMAX, SUB, 1024 * SUB
    c = dict(family=family, seg_C=tuple(seg_C), Cout=Cout, ks=ks, stride=stride, H=H, W=W, N=N, in_slope=in_slope,
             out_act=out_act, out_slope=out_slope, ps=ps, Ho=Ho, Wo=Wo, Cf=Cf, m=m, imax=imax, cin_slice=None, dout=None)
    if family == "gridw":
        c["w"] = _grid_ints(g, (Cout, Cin, ks, ks)) * GRID
        assert lo_share(c["w"], WGT_SCALE) >= 0.5
    else:
        c["w"] = BR.ints(g, (Cout, Cin, ks, ks), imax if family == "gridx" else BR.VMAX)
    c["b"] = BR.ints(g, (Cout,))
    c["b"][::2] = 0
    if family == "sub":
        c["b"].zero_()
    xs = []
    for ci in seg_C:
        if family == "gridx":
            x = _grid_ints(g, (N, ci, H, W)) * GRID
        elif family == "sub":
            x = torch.randint(-1024, 1025, (N, ci, H, W), generator=g).float() * SUB
        else:
            x = BR.ints(g, (N, ci, H, W), imax if family == "gridw" else BR.VMAX)
        x[0, :, :2, :3] = 0
        xs.append(x)
    c["xs"] = xs
    if family == "gridx":
        assert lo_share(torch.cat(xs, 1), ACT_SCALE) >= 0.5
    if family == "sub":  # every 8 x is an fp16 subnormal (or zero) and has no lo part
        hi, lo = split_f16(torch.cat(xs, 1), ACT_SCALE)
        assert float(np.abs(hi).max()) <= 2.0 ** -14 and not lo.any() and float((hi != 0).mean()) > 0.9
    c["res"] = BR.ints(g, (N, Cf, Ho * m, Wo * m)) if res else None
    c["res2"] = BR.ints(g, (N, Cf, Ho * m, Wo * m)) if res2 else None
    c["gate"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, Cf), generator=g)] if gate else None
    xmax, wmax = max(float(x.abs().max()) for x in xs), float(c["w"].abs().max())
    assert xmax <= big and wmax <= V
    c["headroom"] = BR._headroom({"forward": (Cin * ks * ks * xmax * wmax + (0.0 if family == "sub" else extras), q)})
    return c


def epilogue(y, c, dtype):
    """bias is already in y.  The order of dcvc_conv2d's epilogue: activation, pixel shuffle, (gated) residual, res2"""
    t = lambda v: None if v is None else v.to(dtype)
    res, res2, gate = t(c["res"]), t(c["res2"]), t(c["gate"])
    if c["out_act"] == 1:
        y = F.leaky_relu(y, c["out_slope"])
    elif c["out_act"] == 2:
        y = y.clamp(0.0, 1.0)
    if c["ps"]:
        y = F.pixel_shuffle(y, 2)
    if c["out_act"] == 3:
        y = y * torch.where(res2 > 0, torch.ones((), dtype=dtype), torch.full((), float(c["out_slope"]), dtype=dtype))
        return y + res if res is not None else y
    if res is not None:
        y = y + (res * gate[:, :, None, None] if gate is not None else res)
    if res2 is not None:
        y = res2 + y
    return y


def forward(c, dtype=torch.float64, xs=None):
    """torch's CPU convolution of the layer in `dtype` with the kernels' epilogue -> (N, Cf, Ho m, Wo m) in `dtype`"""
    xin = torch.cat([x.to(dtype) for x in (xs or c["xs"])], 1)
    if c["in_slope"] is not None:
        xin = F.leaky_relu(xin, c["in_slope"])
    y = F.conv2d(xin, c["w"].to(dtype), c["b"].to(dtype), stride=c["stride"], padding=c["ks"] // 2)
    return epilogue(y, c, dtype)


def flipped(c):
    """BR.conv_flipped of a forward case: batch and (where symmetric) spatial axes reversed -> (case, back(out))"""
    f, back = BR.conv_flipped(c)
    return f, lambda out: back({"out": out})["out"]


# =====================================================================================================================
# the split-fp16 arithmetic of kernel_common.h, restated in float64
def split_f16(v, scale):
    """-> hi, lo as float64 numpy arrays: sv = clamp(v * scale, +-65504) in fp32, hi = fp16(sv), lo = fp16(sv - hi) with
    numpy's round-to-nearest-even conversion, subnormals kept"""
    a = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float32)
    sv = np.clip(a * np.float32(scale), np.float32(-F16_MAX), np.float32(F16_MAX))
    hi = sv.astype(np.float16)
    lo = (sv - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _conv64(x, w, stride, ks):
    return F.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, stride=stride, padding=ks // 2)


def split64(x, w, b, ks, stride, in_slope=None, x_lo=True, flush_subnormal_lo=False):
    """(xh.wh + xh.wl + xl.wh) / 512 convolved in float64, + bias: what the split-fp16 kernels compute apart from their
    fp32 accumulation.  The two switches build the WRONG kernels of the teeth test: x reduced to its hi part, and a lo
    part flushed to zero where it is an fp16 subnormal."""
    if in_slope is not None:
        x = F.leaky_relu(x.float(), in_slope)
    xh, xl = split_f16(x, ACT_SCALE)
    wh, wl = split_f16(w, WGT_SCALE)
    if flush_subnormal_lo:
        xl = np.where(np.abs(xl) < 2.0 ** -14, 0.0, xl)
        wl = np.where(np.abs(wl) < 2.0 ** -14, 0.0, wl)
    y = _conv64(xh, wh, stride, ks) + _conv64(xh, wl, stride, ks)
    if x_lo:
        y = y + _conv64(xl, wh, stride, ks)
    y = y / (ACT_SCALE * WGT_SCALE)
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def split_bound(x, w, ks, stride):
    """sum over the products of  3 2^-22 |x w| + 2^-28 |w| + 2^-31 |x|  (the figures of kernel_common.h and dcvc_hip.h; the
    derivation is in tests/test_forward_conv_ref_host.py), times 1 + 2^-10 for the second-order terms; float64"""
    ax, aw = x.double().abs(), w.double().abs()
    conv = lambda a, b_: F.conv2d(a, b_, None, stride=stride, padding=ks // 2)
    t = 3 * 2.0 ** -22 * conv(ax, aw) + 2.0 ** -28 * conv(torch.ones_like(ax), aw) + 2.0 ** -31 * conv(ax, torch.ones_like(aw))
    return t * (1 + 2.0 ** -10)


def magnitude(x, w, b, ks, stride):
    """M_e = sum |x||w| + |b| per output, float64"""
    M = F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=ks // 2)
    return M if b is None else M + b.double().abs().view(1, -1, 1, 1)


# =====================================================================================================================
# float-valued data of the per-element bounds
X_MAGS = (2.0 ** -17, 1e-4, 1.0, 30.0, 4000.0)  # per IMAGE: 8 x 2^-17: lo and part of hi are fp16 subnormals
W_MAGS = (1e-3, 1.0, 8.0, 500.0)                # per OUTPUT CHANNEL
# (ks, Cin, Cout): BR.FLOAT_CASES, and one more per form that none of those reaches (conv_small: Cout <= 16; conv_k32's 1x1)
FLOAT_CASES = list(BR.FLOAT_CASES) + [(3, 24, 12), (7, 16, 2), (1, 64, 32)]
FLOAT_HW, FLOAT_N = BR.FLOAT_HW, 3


@functools.lru_cache(maxsize=None)
def float_case(ks, Cin, Cout):
    """-> dict(x, w, b, ref64, ref32, M, split): computed once, shared, never modified.  Magnitudes are drawn per image and
    per output channel, so that no output's sum is dominated by a louder neighbour; values are randn clipped to +-2, which
    keeps |x| <= 8000 < 8188 and |w| <= 1000 < 1023: nothing is clamped."""
    i = FLOAT_CASES.index((ks, Cin, Cout))
    g = torch.Generator().manual_seed(23000 + i)
    xm = torch.tensor(X_MAGS)[(torch.arange(FLOAT_N) * 2 + i) % len(X_MAGS)]
    wm = torch.tensor(W_MAGS)[(torch.arange(Cout) + i) % len(W_MAGS)][torch.randperm(Cout, generator=g)]
    x = torch.randn(FLOAT_N, Cin, *FLOAT_HW, generator=g).clamp(-2, 2) * xm.view(-1, 1, 1, 1)
    w = torch.randn(Cout, Cin, ks, ks, generator=g).clamp(-2, 2) * wm.view(-1, 1, 1, 1)
    b = torch.randn(Cout, generator=g) * wm
    ref64 = F.conv2d(x.double(), w.double(), b.double(), padding=ks // 2)
    ref32 = F.conv2d(x, w, b, padding=ks // 2)
    return dict(x=x, w=w, b=b, xm=xm, wm=wm, ref64=ref64, ref32=ref32, M=magnitude(x, w, b, ks, 1),
                split=split64(x, w, b, ks, 1))


# =====================================================================================================================
# fp32 mode as an fmaf chain in the kernel's K order
def fma32(a, b, c):
    """Correctly rounded fp32 fused multiply-add of fp32 arrays, vectorised: the product of two fp32 numbers is exact in
    float64 (48 bits); TwoSum gives p + c = s + e exactly; s rounds to fp32 like the true sum unless s sits exactly on the
    tie between two fp32 numbers while e != 0 -- then the true sum is off the tie, on the side of e's sign.
    (Finite values away from fp32's overflow and subnormal range; tests/test_forward_conv_ref_host.py proves it against
    `fractions`.)"""
    a64, b64, c64 = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a64 * b64
    s = p + c64
    t = s - p
    e = (p - (s - t)) + (c64 - t)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    go_up = (s == (r64 + up) / 2) & (s != r64) & (e > 0)
    go_dn = (s == (r64 + dn) / 2) & (s != r64) & (e < 0)
    return np.where(go_up, up, np.where(go_dn, dn, r64)).astype(np.float32)


# channel order inside a 16-channel chunk: k2 -> j -> lane half h, channel 8 k2 + 4 h + j (conv_mfma.hip: "lane-half h of the
# MFMA takes channels 8*k2+4*h+j"; v_mfma_f32_32x32x2_f32 adds its k = 0 product, lane half 0, before k = 1)
CHUNK_ORDER = tuple(8 * k2 + 4 * h + j for k2 in range(2) for j in range(4) for h in range(2))


def fmaf_chain(xs, w, b, ks, stride):
    """dcvc_conv2d in DCVC_PREC_FP32 as the chain of fmaf's that conv_mfma.hip spells out: segments in order -> 16-channel
    chunks (a chunk never straddles a segment) -> taps row-major (ky, kx), whether the filter is staged whole or by rows
    -> k2 -> j -> lane half; acc starts at 0 and the bias is added last with one fp32 addition.  Channels that pad a chunk
    are zero on both sides (fma(0, 0, acc) == acc) and are skipped; out-of-picture pixels are zeros and are NOT skipped
    (fma(0, w, acc) == acc as well, the padding below does it)."""
    N, (Cout, pad) = xs[0].shape[0], (w.shape[0], ks // 2)
    Ho, Wo = BR.conv_geometry(ks, stride, *xs[0].shape[2:])
    wn = w.numpy().astype(np.float32)
    acc = np.zeros((N, Cout, Ho, Wo), np.float32)
    cin0 = 0
    for x in xs:
        xp = np.pad(x.numpy().astype(np.float32), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        Cs = x.shape[1]
        for c0 in range(0, Cs, 16):
            for ky in range(ks):
                for kx in range(ks):
                    for cc in CHUNK_ORDER:
                        if c0 + cc >= Cs:
                            continue
                        win = xp[:, c0 + cc, ky: ky + (Ho - 1) * stride + 1: stride, kx: kx + (Wo - 1) * stride + 1: stride]
                        acc = fma32(win[:, None], wn[None, :, cin0 + c0 + cc, ky, kx, None, None], acc)
        cin0 += Cs
    return torch.from_numpy(acc + b.numpy().astype(np.float32)[None, :, None, None])


CHAIN_CASES = [  # (ks, stride, seg_C, Cout): one per (ks, stride); a chunk tail (24 = 16 + 8), two segments, both NT
    (1, 1, (24, 16), 24), (1, 2, (40,), 40), (3, 1, (24, 16), 40), (3, 2, (24,), 24), (7, 1, (8,), 32)]


@functools.lru_cache(maxsize=None)
def chain_case(i):
    """float data of CHAIN_CASES[i] (per-channel magnitudes {1e-4, 1, 30}), its fmaf chain and float64 reference: computed
    once, shared, never modified"""
    ks, stride, seg_C, Cout = CHAIN_CASES[i]
    g = torch.Generator().manual_seed(25000 + i)
    H, W = (13, 37) if stride == 1 else (26, 75)
    Cin = sum(seg_C)
    mags = torch.tensor([1e-4, 1.0, 30.0])[torch.arange(Cin) % 3][torch.randperm(Cin, generator=g)]
    x = torch.randn(1, Cin, H, W, generator=g) * mags.view(1, -1, 1, 1)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / float(np.sqrt(Cin * ks * ks))
    b = torch.randn(Cout, generator=g) * 0.1
    xs = list(x.split(list(seg_C), 1))
    Ho, Wo = BR.conv_geometry(ks, stride, H, W)
    layer = dict(family="float", seg_C=tuple(seg_C), Cout=Cout, ks=ks, stride=stride, H=H, W=W, N=1, Ho=Ho, Wo=Wo, m=1, Cf=Cout,
                 ps=False, in_slope=None, out_act=0, out_slope=None, xs=xs, w=w, b=b, res=None, res2=None, gate=None)
    ref64 = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=ks // 2)
    return layer, fmaf_chain(xs, w, b, ks, stride), ref64, magnitude(x, w, b, ks, stride)
