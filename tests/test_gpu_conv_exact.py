"""The forward convolution kernels (csrc/conv_mfma.hip, conv_small.hip, conv_k32.hip) element by element through the C ABI,
on a real MI355X: each entry point and each template instantiation is selected HERE, not by Engine routing.

A. exact data (tests/forward_conv_ref.py: integers; the hi/lo grid, whose lo planes carry data; the fp16-subnormal range)
   bit for bit against the float64 reference cast to fp32, twice.   B. banded launches.   C. float data per element
   against bounds taken from the references alone.   D. the range guard (DCVC_STATUS_ACT_SATURATED), the clamp on load,
   NaN outputs.   E. refusals (DCVC_E_ARG with nothing written).   F. fp32 mode on float data, bit for bit the fmaf chain
   that conv_mfma.hip documents.

Every operand is a channel slice of a wider NaN-filled buffer between sentinel guard words: a read outside a view
poisons the result, and after every call everything outside the output view must be untouched (inputs and residuals
bit for bit what they were).  Every call gets a status word of the test's own.

Which case reaches which instantiation (the launcher's rules, restated by `run_conv` and asserted there):
  conv_mfma<KS, S, RPW, NT, SPLIT>: SPLIT = precision fp16x3; NT = 2 iff Cout_pad % 64 == 0 (Cout 40, 64; not 24, 96, 3,
    33); RPW = 1 ("rows 4") for stride 1 with fewer than 384 8-row workgroups and no tile_rows -- every stride-1 case
    here, asserted -- and for every stride-2 launch; RPW = 2 ("rows 8") through tile_row0 = 0, tile_rows = nty, and for
    chan_partial.  MFMA_CASES x {fp32, fp16x3} x {rows 4, rows 8} therefore covers <1,1,*>, <3,1,*>, <7,1,*> with RPW 1 and
    2, NT 1 and 2, and <1,2,1,*>, <3,2,1,*>.  Epilogues: vector (out / res 16-byte addressable, Cfinal % 4 == 0) and scalar
    (Cout 3, 33, pixel shuffle to 10 channels, or an output view at channel offset 1).
  conv_mfma<7,1,2,NT,true,PAIR>: PAIRED_CASES, NT = 1 (Cout 32) and 2 (Cout 64).
  conv_small<3>, <7>: SMALL_CASES.
  conv_k32<KS, NTW, NWAVE>: <3,4,8> ks 3, Cout_pad % 64 == 0, 8 waves; <3,4,4> the same after dcvc_conv_k32_set_waves(4);
    <3,2,4> ks 3, Cout 32 or 96; <1,4,4> ks 1, Cout 64 or 128; <1,2,4> ks 1, Cout 32 or 96.  Each with the plain store branch
    and with the res2 / chan_partial branch of the epilogue."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import backward_ref as BR
from tests import forward_conv_ref as FR

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 12345.0
GUARD = 1024
FP32, FAST = 0, 1
E_ARG = -1
AX = "n,c,y,x"
DEV = "cuda:0"
FORMS = {"mfma32": ("mfma", FP32), "mfma16": ("mfma", FAST), "paired": ("paired", FAST), "small": ("small", FAST),
         "k32": ("k32", FAST)}


@pytest.fixture(scope="module")
def eng():
    from vcm_ts_amd.engine import Engine

    return Engine(DEV, "fp32")


def r4(c):
    return (c + 3) // 4 * 4


def bits(t):
    return t.contiguous().view(torch.int32)


class Frame:
    """C channels at channel offset `off` of an (N, H, W, cs) region filled with `fill`, between two guards of SENT"""

    def __init__(self, shape, off, cs, data=None, fill=NAN):
        N, Cc, H, W = shape
        assert off + Cc <= cs and cs % 4 == 0
        self.N, self.C, self.H, self.W, self.off, self.cs = N, Cc, H, W, off, cs
        n = N * H * W * cs
        self.big = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.region = self.big[GUARD:GUARD + n].view(N, H, W, cs)
        self.region.fill_(fill)
        if data is not None:
            self.region[..., off:off + Cc] = data.permute(0, 2, 3, 1).to(DEV)
        self.ptr = self.big.data_ptr() + 4 * (GUARD + off)
        self.before = self.big.clone()

    def unchanged(self):
        return torch.equal(bits(self.big), bits(self.before))

    def outside_untouched(self):
        """guards and the channels outside the view hold what they held"""
        keep = torch.ones(self.cs, dtype=torch.bool, device=DEV)
        keep[self.off:self.off + self.C] = False
        n = self.region.numel()
        b0 = self.before[GUARD:GUARD + n].view(self.region.shape)
        return (torch.equal(self.big[:GUARD], self.before[:GUARD]) and torch.equal(self.big[GUARD + n:], self.before[GUARD + n:])
                and torch.equal(bits(self.region[..., keep]), bits(b0[..., keep])))

    def nchw(self):
        return self.region[..., self.off:self.off + self.C].permute(0, 3, 1, 2).contiguous().cpu()


def _segs(seg_C):
    return (C.c_int32 * len(seg_C))(*seg_C)


def pack(L, kind, prec, c):
    """the host packer of the form, through ctypes -> (wpack, bpack) on the device, Cout_pad"""
    w = np.ascontiguousarray(c["w"].numpy(), dtype=np.float32)
    b = np.ascontiguousarray(c["b"].numpy(), dtype=np.float32)
    Cout, Cin, ks, _ = w.shape
    seg_C, ps = c["seg_C"], int(c["ps"])
    cp = C.c_int32(0)
    if kind == "mfma":
        n = L.dcvc_conv_pack_size(Cout, ks, len(seg_C), _segs(seg_C), C.byref(cp)) * 4
    elif kind == "paired":
        n = L.dcvc_conv_pack_size_paired(Cout, Cin, C.byref(cp)) * 4
    elif kind == "small":
        n, cp = L.dcvc_conv_small_pack_bytes(Cout, ks, len(seg_C), _segs(seg_C)), C.c_int32(16)
    else:
        n = L.dcvc_conv_k32_pack_bytes(Cout, ks, len(seg_C), _segs(seg_C), C.byref(cp))
    assert n > 0, (kind, n)
    wp, bp = np.zeros(n // 4, np.float32), np.zeros(cp.value, np.float32)
    if kind == "mfma":
        rc = L.dcvc_conv_pack_weights(w.ctypes.data, b.ctypes.data, Cout, ks, len(seg_C), _segs(seg_C), ps, prec, wp.ctypes.data, bp.ctypes.data)
    elif kind == "paired":
        rc = L.dcvc_conv_pack_weights_paired(w.ctypes.data, b.ctypes.data, Cout, Cin, wp.ctypes.data, bp.ctypes.data)
    elif kind == "small":
        rc = L.dcvc_conv_small_pack_weights(w.ctypes.data, b.ctypes.data, Cout, ks, len(seg_C), _segs(seg_C), wp.ctypes.data, bp.ctypes.data)
    else:
        rc = L.dcvc_conv_k32_pack_weights(w.ctypes.data, b.ctypes.data, Cout, ks, len(seg_C), _segs(seg_C), ps, wp.ctypes.data, bp.ctypes.data)
    assert rc == 0, (kind, rc)
    return torch.from_numpy(wp).to(DEV), torch.from_numpy(bp).to(DEV), cp.value


def wgs8(c, Cout_pad):
    """8-row workgroups of a stride-1 dcvc_conv2d launch: below 384 it runs on the 4-row instantiations (conv_mfma.hip)"""
    return ((c["Wo"] + 31) // 32) * ((c["Ho"] + 7) // 8) * (Cout_pad // (64 if Cout_pad % 64 == 0 else 32)) * c["N"]


def run_conv(e, form, c, rows=None, waves=8, band=None, oview=None, xview=None, chan_partial=False, status=0, mutate=None,
             expect=0, xs=None):
    """One launch of the form's entry point on the engine's stream.  rows: 4 / 8 selects dcvc_conv2d's tile height (None:
    whatever the launcher takes); band = (tile_row0, tile_rows); oview / xview = (channel offset, channel stride) of the
    output (and residual) / input views; status: initial value of the call's own status word, None passes NULL.
    -> dict(out = the output view as a CPU NCHW tensor, status = the word afterwards, mean = channel means or None)"""
    from vcm_ts_amd import lib

    L = e.L
    kind, prec = FORMS[form]
    N, H, W, Ho, Wo, m, Cf, Cout, ks, stride = (c[k] for k in ("N", "H", "W", "Ho", "Wo", "m", "Cf", "Cout", "ks", "stride"))
    wp, bp, cpad = pack(L, kind, prec, c)
    what = f"{form} {c['seg_C']}->{Cout} k{ks} s{stride} {H}x{W} N{N} rows={rows} waves={waves} band={band} oview={oview}"
    X = [Frame(x.shape, *(xview or (4, r4(4 + x.shape[1]) + 4)), data=x) for x in (xs or c["xs"])]
    ooff, ocs = oview or (4, r4(4 + Cf) + 4)
    O = Frame((N, Cf, Ho * m, Wo * m), ooff, ocs)
    R1 = Frame(c["res"].shape, ooff, ocs + 4, data=c["res"]) if c["res"] is not None else None
    R2 = Frame(c["res2"].shape, ooff, ocs + 8, data=c["res2"]) if c["res2"] is not None else None
    G = None
    if c["gate"] is not None:
        G = torch.full((N * Cf + 8,), NAN, dtype=torch.float32, device=DEV)
        G[:N * Cf] = c["gate"].reshape(-1).to(DEV)
    ST = torch.tensor([-1, status or 0, -1], dtype=torch.int32, device=DEV)
    a = lib.ConvArgs()
    for i, (f, cc) in enumerate(zip(X, c["seg_C"])):
        a.seg[i].ptr, a.seg[i].C, a.seg[i].cs = f.ptr, cc, f.cs
    a.nseg, a.N, a.Hin, a.Win = len(X), N, H, W
    a.in_act, a.in_slope = (0, 0.0) if c["in_slope"] is None else (1, float(c["in_slope"]))
    a.wpack, a.bpack = wp.data_ptr(), bp.data_ptr()
    a.ks, a.stride, a.Cout, a.Cout_pad = ks, stride, Cout, cpad
    a.out, a.out_cs = O.ptr, O.cs
    a.out_act, a.out_slope = c["out_act"], float(c["out_slope"] or 0.0)
    a.pixel_shuffle = int(c["ps"])
    if R1 is not None:
        a.res, a.res_cs = R1.ptr, R1.cs
    if R2 is not None:
        a.res2, a.res2_cs = R2.ptr, R2.cs
    if G is not None:
        a.res_gate = G.data_ptr()
    a.precision = prec
    a.status = None if status is None else ST.data_ptr() + 4
    a.pair_taps = int(kind == "paired")
    nty = -(-Ho // int(L.dcvc_conv_tile_rows(ks, stride)))
    CP = parts = None
    if chan_partial:
        parts = int(L.dcvc_conv_chan_partial_parts(ks, stride, Ho, Wo))
        assert parts == nty * ((Wo + 31) // 32)
        CP = torch.full((GUARD + N * parts * cpad + GUARD,), NAN, dtype=torch.float32, device=DEV)
        CP[:GUARD], CP[GUARD + N * parts * cpad:] = SENT, SENT
        a.chan_partial = CP.data_ptr() + 4 * GUARD
    if kind == "mfma" and rows is not None:
        assert band is None
        if rows == 8:
            a.tile_row0, a.tile_rows = 0, nty
        else:  # the documented rule must send this launch to the 4-row tiles, or the case is empty
            assert rows == 4 and stride == 1 and not chan_partial and wgs8(c, cpad) < 384, what
    if band is not None:
        a.tile_row0, a.tile_rows = band
    if mutate is not None:
        mutate(a)
    fn = {"mfma": L.dcvc_conv2d, "paired": L.dcvc_conv2d, "small": L.dcvc_conv2d_small, "k32": L.dcvc_conv2d_k32}[kind]
    if waves != 8:
        assert kind == "k32" and L.dcvc_conv_k32_set_waves(waves) == 0
    try:
        rc = fn(C.byref(a), e.stream())
    finally:
        if waves != 8:
            assert L.dcvc_conv_k32_set_waves(8) == 0
    torch.cuda.synchronize()
    st = ST.cpu()
    assert int(st[0]) == -1 and int(st[2]) == -1, f"{what}: wrote beside the status word"
    for f in X + [r for r in (R1, R2) if r is not None]:
        assert f.unchanged(), f"{what}: an input or residual buffer was written"
    if G is not None:
        assert bool(torch.isnan(G[N * Cf:]).all())
    if expect:
        assert rc == expect, f"{what}: returned {rc}, expected {expect}"
        assert O.unchanged(), f"{what}: a refused call wrote to the output"
        assert int(st[1]) == (status or 0), f"{what}: a refused call changed the status word"
        assert CP is None or bool(torch.isnan(CP[GUARD:-GUARD]).all()), f"{what}: a refused call wrote chan_partial"
        return None
    lib.check(rc, what)
    assert O.outside_untouched(), f"{what}: wrote outside the output view (guards or channels outside [{ooff}, {ooff + Cf}))"
    if status is None:
        assert int(st[1]) == 0, f"{what}: status word written although NULL was passed"
    mean = None
    if chan_partial:
        assert bool((CP[:GUARD] == SENT).all()) and bool((CP[-GUARD:] == SENT).all()), f"{what}: wrote beside chan_partial"
        MEAN = torch.full((N * Cout + 8,), NAN, dtype=torch.float32, device=DEV)
        lib.check(L.dcvc_channel_mean_finish(a.chan_partial, parts, cpad, MEAN.data_ptr(), N, Cout, Ho * Wo, e.stream()), "mean_finish")
        torch.cuda.synchronize()
        assert bool(torch.isnan(MEAN[N * Cout:]).all())
        mean = MEAN[:N * Cout].view(N, Cout).cpu()
    return dict(out=O.nchw(), status=int(st[1]), mean=mean)


def exact_mean(want64, HW):
    """the channel mean as the finishing kernel forms it on exact data: the exact sum, ONE correctly rounded fp32 division"""
    s = want64.sum((2, 3)).numpy()
    q = 2.0 ** -4  # every partial sum, in any order, is a multiple of q below 2^24 q: the integer family's grid
    assert bool((want64 / q == (want64 / q).round()).all()) and float(want64.abs().sum((2, 3)).max()) < BR.TWO24 * q
    return torch.from_numpy(s.astype(np.float32) / np.float32(HW))


def check_exact(e, form, c, want64, **kw):
    """bit for bit against the float64 reference cast to fp32, twice, the same bits both times -> the result"""
    assert c["headroom"] > 1
    first = None
    for run in range(2):
        r = run_conv(e, form, c, **kw)
        what = f"{form} {c['family']} {c['seg_C']}->{c['Cout']} k{c['ks']} s{c['stride']} {kw} run {run}"
        BR.assert_bits(r["out"], want64.float(), what, AX)
        if r["mean"] is not None:
            BR.assert_bits(r["mean"], exact_mean(want64, c["Ho"] * c["Wo"]), "channel mean " + what, "n,c")
        if first is not None:
            assert torch.equal(bits(r["out"]), bits(first["out"])), f"{what}: two runs differ"
        first = r
    return first


GEOM = ("seg_C", "Cout", "ks", "stride", "H", "W", "ps", "N")


@functools.lru_cache(maxsize=None)
def case(table, i, family):
    """exact data of a table row and its float64 reference: computed once, shared by every precision / rows / waves variant.
    The subnormal family has no epilogue (1 + k 2^-27 is no fp32 number); the grid families take the activation on load only
    in the integer family's place (a slope on the 2^-10 grid costs two more bits of headroom)."""
    kw = {k: v for k, v in globals()[table][i].items() if k not in ("name", "oview", "xview", "chan", "waves", "fams")}
    if family == "sub":
        kw = {k: v for k, v in kw.items() if k in GEOM}
    elif family != "int":
        kw.pop("in_slope", None)
    c = FR.exact_case(family, seed=i + 100 * len(table), **kw)
    return c, FR.forward(c)


S1, S2 = dict(H=13, W=37), dict(H=26, W=75)  # output 13 x 37: 2 x 2 tiles of 8 x 32 (4 x 2 of 4 x 32), partial both ways
ALLF = ("int", "gridx", "gridw", "sub")
MFMA_CASES = [
    dict(name="k1_24to24", seg_C=(24,), Cout=24, ks=1, stride=1, **S1, fams=ALLF),
    dict(name="k1s2_40to40_act", seg_C=(40,), Cout=40, ks=1, stride=2, **S2, out_act=1, out_slope=0.25, fams=ALLF),
    dict(name="k3_2seg_to96_gate", seg_C=(24, 16), Cout=96, ks=3, stride=1, **S1, res=True, gate=True, fams=ALLF),
    dict(name="k3_40to64_inact_res_res2", seg_C=(40,), Cout=64, ks=3, stride=1, **S1, in_slope=0.25, out_act=1, out_slope=0.5,
         res=True, res2=True, fams=ALLF),
    dict(name="k3s2_3seg_to40_clamp", seg_C=(16, 24, 40), Cout=40, ks=3, stride=2, **S2, out_act=2, fams=ALLF),
    dict(name="k7_24to24_relu", seg_C=(24,), Cout=24, ks=7, stride=1, **S1, out_act=1, out_slope=0.0, fams=ALLF),
    dict(name="k7_8to64_res", seg_C=(8,), Cout=64, ks=7, stride=1, **S1, res=True, fams=ALLF),
    dict(name="k3s2_24to24_inact", seg_C=(24,), Cout=24, ks=3, stride=2, **S2, in_slope=0.5, fams=("int",)),
    # scalar epilogue
    dict(name="k3_24to3_scalar", seg_C=(24,), Cout=3, ks=3, stride=1, **S1, res=True, out_act=2, fams=("int", "gridx")),
    dict(name="k1_40to33_scalar_gate", seg_C=(40,), Cout=33, ks=1, stride=1, **S1, res=True, gate=True, res2=True, fams=("int", "gridw")),
    dict(name="k3_16to24_offset1", seg_C=(16,), Cout=24, ks=3, stride=1, **S1, res=True, oview=(1, 28), fams=("int", "sub")),
    dict(name="k3s2_40to3_scalar", seg_C=(40,), Cout=3, ks=3, stride=2, **S2, out_act=1, out_slope=0.25, fams=("int",)),
    # pixel shuffle: vector (24 final channels) and scalar (10)
    dict(name="k3_ps_24to96_act_res", seg_C=(24,), Cout=96, ks=3, stride=1, **S1, ps=True, out_act=1, out_slope=0.25, res=True,
         fams=("int", "gridx")),
    dict(name="k1_ps_40to40_scalar", seg_C=(40,), Cout=40, ks=1, stride=1, **S1, ps=True, fams=("int",)),
    # the mask epilogue (out_act 3), without and with a residual
    dict(name="k3_mask", seg_C=(24,), Cout=40, ks=3, stride=1, **S1, out_act=3, out_slope=0.25, res2=True, fams=("int",)),
    dict(name="k3s2_mask_res", seg_C=(24,), Cout=24, ks=3, stride=2, **S2, out_act=3, out_slope=0.5, res=True, res2=True, fams=("int",)),
    dict(name="k1_mask_res_scalar", seg_C=(40,), Cout=33, ks=1, stride=1, **S1, out_act=3, out_slope=0.0, res=True, res2=True, fams=("int",)),
    # fused channel sums (always the 8-row tiles; stride 2: 4-row)
    dict(name="k3_chan_sums", seg_C=(40,), Cout=64, ks=3, stride=1, **S1, out_act=1, out_slope=0.25, chan=True, fams=("int",)),
    dict(name="k3s2_chan_sums_gate", seg_C=(24,), Cout=24, ks=3, stride=2, **S2, res=True, gate=True, chan=True, fams=("int",)),
]
PAIRED_CASES = [
    dict(name="3to32", seg_C=(3,), Cout=32, ks=7, stride=1, **S1, fams=ALLF),
    dict(name="6to64_res", seg_C=(6,), Cout=64, ks=7, stride=1, **S1, res=True, out_act=1, out_slope=0.0, fams=ALLF),
    dict(name="8to32_inact", seg_C=(8,), Cout=32, ks=7, stride=1, **S1, in_slope=0.25, res=True, res2=True, fams=("int", "gridw")),
    dict(name="8to64_scalar", seg_C=(8,), Cout=64, ks=7, stride=1, **S1, oview=(1, 72), fams=("int", "gridx")),
]
SMALL_CASES = [
    dict(name="k3_3to2", seg_C=(3,), Cout=2, ks=3, stride=1, **S1, fams=ALLF),
    dict(name="k3_2seg_to3_res_clamp", seg_C=(16, 32), Cout=3, ks=3, stride=1, **S1, res=True, out_act=2, fams=ALLF),
    dict(name="k3_24to12_act", seg_C=(24,), Cout=12, ks=3, stride=1, **S1, out_act=1, out_slope=0.25, oview=(1, 16), fams=ALLF),
    dict(name="k3_16to16", seg_C=(16,), Cout=16, ks=3, stride=1, **S1, in_slope=0.5, fams=("int",)),
    dict(name="k7_16to2_res", seg_C=(16,), Cout=2, ks=7, stride=1, **S1, res=True, fams=ALLF),
    dict(name="k7_24to16_inact", seg_C=(24,), Cout=16, ks=7, stride=1, **S1, in_slope=0.25, fams=ALLF),
    dict(name="k7_3to12", seg_C=(3,), Cout=12, ks=7, stride=1, **S1, out_act=1, out_slope=0.0, fams=("int", "gridw")),
]
K32_CASES = [  # waves: the wave counts to run (4 only changes <3,4,*>)
    dict(name="k3_32to64", seg_C=(32,), Cout=64, ks=3, stride=1, **S1, waves=(8, 4), fams=ALLF),
    dict(name="k3_64to128_gate_act", seg_C=(64,), Cout=128, ks=3, stride=1, **S1, res=True, gate=True, out_act=1, out_slope=0.25,
         waves=(8, 4), xview=(32, 128), fams=("int", "gridx")),
    dict(name="k3_2seg_to96_res2", seg_C=(32, 64), Cout=96, ks=3, stride=1, **S1, res2=True, waves=(8,), xview=(64, 128), fams=ALLF),
    dict(name="k3_3seg_to32_inact", seg_C=(64, 32, 32), Cout=32, ks=3, stride=1, **S1, in_slope=0.25, out_act=1, out_slope=0.5,
         waves=(8,), fams=("int", "gridw")),
    dict(name="k1_64to64_ps_res", seg_C=(64,), Cout=64, ks=1, stride=1, **S1, ps=True, res=True, waves=(8,), fams=ALLF),
    dict(name="k1_32to96_chan_sums", seg_C=(32,), Cout=96, ks=1, stride=1, **S1, chan=True, waves=(8,), fams=("int",)),
    dict(name="k3_64to64_chan_sums_gate", seg_C=(64,), Cout=64, ks=3, stride=1, **S1, res=True, gate=True, chan=True, waves=(8, 4),
         fams=("int",)),
    dict(name="k3_32to128_ps_act", seg_C=(32,), Cout=128, ks=3, stride=1, **S1, ps=True, out_act=1, out_slope=0.25, waves=(8, 4),
         fams=("int",)),
    dict(name="k1_2seg_to128_res_res2_clamp", seg_C=(32, 64), Cout=128, ks=1, stride=1, **S1, res=True, res2=True, out_act=2,
         waves=(8,), fams=("int", "gridw")),
    dict(name="k3_32to96_chan_sums_res2", seg_C=(32,), Cout=96, ks=3, stride=1, **S1, res2=True, chan=True, in_slope=0.0, waves=(8,),
         fams=("int",)),
]


def params(table):
    rows = globals()[table]
    return [pytest.param(i, f, id=f"{r['name']}-{f}") for i, r in enumerate(rows) for f in r["fams"]]


# =====================================================================================================================
# A. exact data, bit for bit, every instantiation
@pytest.mark.parametrize("form", ["mfma32", "mfma16"])
@pytest.mark.parametrize("i,family", params("MFMA_CASES"))
def test_conv2d_exact_data_bit_for_bit(eng, i, family, form):
    """dcvc_conv2d in both precisions, on the 4-row and on the 8-row instantiation where the stride is 1"""
    row = MFMA_CASES[i]
    c, want = case("MFMA_CASES", i, family)
    chan = row.get("chan", False)
    variants = (None,) if row["stride"] == 2 else ((8,) if chan else (4, 8))
    seen = [check_exact(eng, form, c, want, rows=r, oview=row.get("oview"), chan_partial=chan) for r in variants]
    assert all(torch.equal(bits(s["out"]), bits(seen[0]["out"])) for s in seen)
    assert all(s["status"] == 0 for s in seen)


@pytest.mark.parametrize("i,family", params("PAIRED_CASES"))
def test_tap_paired_conv_exact_data_bit_for_bit(eng, i, family):
    c, want = case("PAIRED_CASES", i, family)
    assert check_exact(eng, "paired", c, want, oview=PAIRED_CASES[i].get("oview"))["status"] == 0


@pytest.mark.parametrize("i,family", params("SMALL_CASES"))
def test_conv2d_small_exact_data_bit_for_bit(eng, i, family):
    c, want = case("SMALL_CASES", i, family)
    assert check_exact(eng, "small", c, want, oview=SMALL_CASES[i].get("oview"))["status"] == 0


@pytest.mark.parametrize("i,family", params("K32_CASES"))
def test_conv2d_k32_exact_data_bit_for_bit(eng, i, family):
    row = K32_CASES[i]
    c, want = case("K32_CASES", i, family)
    for waves in row["waves"]:
        r = check_exact(eng, "k32", c, want, waves=waves, xview=row.get("xview"), chan_partial=row.get("chan", False))
        assert r["status"] == 0


# =====================================================================================================================
# B. banded launches
B1, B2 = dict(H=29, W=37), dict(H=57, W=73)  # output 29 x 37: 4 tile rows of 8, stride 2: 8 tile rows of 4
BAND_CASES = [
    ("mfma32", dict(seg_C=(24,), Cout=40, ks=3, stride=1, **B1, res=True, out_act=1, out_slope=0.25)),
    ("mfma16", dict(seg_C=(24,), Cout=24, ks=1, stride=1, **B1)),
    ("mfma16", dict(seg_C=(24,), Cout=24, ks=3, stride=2, **B2, res=True)),
    ("mfma32", dict(seg_C=(40,), Cout=3, ks=1, stride=2, **B2)),
    ("mfma16", dict(seg_C=(8,), Cout=32, ks=7, stride=1, **B1)),
    ("paired", dict(seg_C=(8,), Cout=32, ks=7, stride=1, **B1)),
    ("k32", dict(seg_C=(32,), Cout=64, ks=3, stride=1, **B1, res=True, res2=True)),
    ("k32", dict(seg_C=(64,), Cout=32, ks=1, stride=1, **B1, out_act=1, out_slope=0.5)),
]


@pytest.mark.parametrize("j", range(len(BAND_CASES)), ids=[f"{f}-k{k['ks']}s{k['stride']}" for f, k in BAND_CASES])
def test_banded_launches_write_exactly_their_rows_and_add_up_to_the_picture(eng, j):
    """tile_row0 / tile_rows: the picture as bands (0,1), (1,2), (3,1) (stride 2, 8 tile rows: and (4,4)), and one band that
    reaches beyond the last tile row and is clamped, each into a NaN-filled output: exactly the band's rows are written and
    the union is the unbanded result, bit for bit.  A band that starts outside the picture is refused."""
    form, kw = BAND_CASES[j]
    c = FR.exact_case("int", seed=300 + j, **kw)
    want = FR.forward(c).float()
    tr = int(eng.L.dcvc_conv_tile_rows(c["ks"], c["stride"]))
    nty = -(-c["Ho"] // tr)
    assert nty == (4 if c["stride"] == 1 else 8)
    whole = run_conv(eng, form, c)["out"]
    BR.assert_bits(whole, want, f"unbanded {form}", AX)
    bands = [(0, 1), (1, 2), (3, 1)] + ([(4, nty - 4)] if nty > 4 else [])
    union = torch.full_like(want, NAN)
    for r0, nr in bands + [(nty - 2, 5)]:
        got = run_conv(eng, form, c, band=(r0, nr))["out"]
        y0, y1 = r0 * tr, min((r0 + nr) * tr, c["Ho"])
        inside = torch.zeros(c["Ho"], dtype=torch.bool)
        inside[y0:y1] = True
        assert bool(torch.isnan(got[:, :, ~inside]).all()), f"band ({r0}, {nr}) wrote outside rows [{y0}, {y1})"
        BR.assert_bits(got[:, :, inside], want[:, :, inside], f"band ({r0}, {nr}) of {form}", AX)
        if (r0, nr) in bands:
            assert bool(torch.isnan(union[:, :, inside]).all())
            union[:, :, inside] = got[:, :, inside]
    assert torch.equal(bits(union), bits(whole))
    for r0 in (nty, nty + 3, -1):
        run_conv(eng, form, c, band=(r0, 1), expect=E_ARG)


def test_conv2d_small_refuses_bands(eng):
    c = FR.exact_case("int", (16,), 2, 7, 1, 29, 37)
    run_conv(eng, "small", c, band=(0, 1), expect=E_ARG)
    run_conv(eng, "small", c, band=(1, 2), expect=E_ARG)


# =====================================================================================================================
# C. float data, per element
def float_forms(ks, Cin, Cout):
    f = [("mfma32", dict(rows=4)), ("mfma32", dict(rows=8)), ("mfma16", dict(rows=4)), ("mfma16", dict(rows=8))]
    if ks == 7 and Cin <= 8:
        f.append(("paired", {}))
    if ks in (3, 7) and Cout <= 16:
        f.append(("small", {}))
    if ks in (1, 3) and Cin % 32 == 0 and Cout % 4 == 0:
        f += [("k32", dict(waves=8))] + ([("k32", dict(waves=4))] if ks == 3 and Cout % 64 == 0 else [])
    return f


def float_layer(d, ks):
    x, w = d["x"], d["w"]
    return dict(family="float", seg_C=(x.shape[1],), Cout=w.shape[0], ks=ks, stride=1, H=x.shape[2], W=x.shape[3], N=x.shape[0],
                Ho=x.shape[2], Wo=x.shape[3], m=1, Cf=w.shape[0], ps=False, in_slope=None, out_act=0, out_slope=None, xs=[x], w=w,
                b=d["b"], res=None, res2=None, gate=None)


@pytest.mark.parametrize("ks,Cin,Cout", FR.FLOAT_CASES, ids=lambda v: str(v))
def test_float_data_within_per_element_bounds(eng, ks, Cin, Cout):
    """Activation magnitudes per image from {2^-17, 1e-4, 1, 30, 4000}, weight magnitudes per output channel from {1e-3, 1, 8,
    500}, 17 x 45, N = 3: no output's sum is dominated by a louder neighbour.  Per element, none excluded, with
    M_e = sum |x||w| + |b| in float64:
        fp32 mode:    |got - ref64|   <= c 2^-24 M_e
        fp16x3 forms: |got - split64| <= c 2^-24 M_e     split64: the documented hi/lo arithmetic in float64
                      (forward_conv_ref.split64; tests/test_forward_conv_ref_host.py holds |split64 - ref64| to the documented
                      3 2^-22 |x w| + 2^-28 |w| + 2^-31 |x| per product, and shows that this bound rejects a kernel that drops
                      the lo part of x, flushes subnormal lo parts or drops one product)
    c = BR.fp32_constant of torch's fp32 CPU convolution against float64: the reference's own error, never the kernel's,
    recomputed where the test runs and printed.  Measured on the MI355X host, c and the kernels' worst error in units of
    2^-24 M_e (4- and 8-row tiles, 4 and 8 waves agree to every digit):
        1x1 40->33: c 58.5   fp32 3.54   fp16x3 conv_mfma 2.95
        3x3 64->64: c 13.9   fp32 4.32   fp16x3 conv_mfma 2.69   conv_k32 2.97
        7x7  8->32: c 20.1   fp32 4.15   fp16x3 conv_mfma 2.27   paired 2.27
        3x3 24->12: c 11.4   fp32 4.24   fp16x3 conv_mfma 2.23   conv_small 2.23
        7x7 16->2:  c 14.2   fp32 3.81   fp16x3 conv_mfma 2.27   conv_small 2.27
        1x1 64->32: c 61.2   fp32 3.61   fp16x3 conv_mfma 2.82   conv_k32 3.02
    i.e. at most 0.37 of the bound.  (c is large for 1x1 because torch adds the products onto the bias channel by channel.)"""
    d = FR.float_case(ks, Cin, Cout)
    cst = BR.fp32_constant(d["ref32"], d["ref64"], d["M"])
    bound = cst * 2.0 ** -24 * d["M"]
    layer = float_layer(d, ks)
    failures = []
    for form, kw in float_forms(ks, Cin, Cout):
        got = run_conv(eng, form, layer, **kw)["out"].double()
        ref = d["ref64"] if form == "mfma32" else d["split"]
        err = (got - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        ratio = err / bound
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"k{ks} {Cin}->{Cout} {form} {kw}: c = {cst:.3f}, worst error / bound = {float(ratio[i]):.3f} at ({AX})="
              f"{tuple(int(v) for v in i)}, worst error / (2^-24 M) = {float(ratio[i]) * cst:.3f}")
        if not bool((err <= bound).all()):
            gi = got[i].float()
            failures.append(f"{form} {kw}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst at ({AX})="
                            f"{tuple(int(v) for v in i)}: got {float(gi)!r} (0x{int(gi.view(torch.int32)) & 0xffffffff:08x}) want "
                            f"{float(ref[i])!r} error {float(err[i]):.3e} > {float(bound[i]):.3e}")
    assert not failures, "\n".join(failures)


# =====================================================================================================================
# D. range edges and the status word
LIMIT = 8188.0
NEXT = float(np.nextafter(np.float32(LIMIT), np.float32(np.inf)))
RANGE_PATHS = [  # (name, form, layer, run_conv arguments)
    ("mfma16_vector_rows4", "mfma16", dict(seg_C=(24,), Cout=24, ks=3), dict(rows=4)),
    ("mfma16_vector_rows8", "mfma16", dict(seg_C=(24,), Cout=64, ks=1), dict(rows=8)),
    ("mfma16_scalar", "mfma16", dict(seg_C=(24,), Cout=3, ks=3), dict(rows=8)),
    ("mfma32_vector", "mfma32", dict(seg_C=(24,), Cout=24, ks=7), dict(rows=4)),
    ("mfma16_s2_scalar", "mfma16", dict(seg_C=(24,), Cout=33, ks=1, stride=2), {}),
    ("paired", "paired", dict(seg_C=(8,), Cout=32, ks=7), {}),
    ("small_k3", "small", dict(seg_C=(16,), Cout=3, ks=3), {}),
    ("small_k7", "small", dict(seg_C=(16,), Cout=16, ks=7), {}),
    ("k32_plain_8waves", "k32", dict(seg_C=(32,), Cout=64, ks=3), dict(waves=8)),
    ("k32_plain_narrow", "k32", dict(seg_C=(32,), Cout=32, ks=1), {}),
    ("k32_res2_branch", "k32", dict(seg_C=(32,), Cout=64, ks=3, res2=True), dict(waves=4)),
    ("k32_chan_partial_branch", "k32", dict(seg_C=(32,), Cout=96, ks=1), dict(chan_partial=True)),
]


def range_layer(kw, bias):
    """Every output channel copies input channel 0 (centre-tap weight 1) and adds its bias.  Channel 0 holds 4000 and, at the
    LAST pixel of the last image -- inside the partial tiles --, exactly 8188 = 65504 / 8; res2 (where present) is zero."""
    kw = dict(kw)
    stride = kw.pop("stride", 1)
    H, W = (13, 37) if stride == 1 else (25, 73)
    c = FR.exact_case("int", stride=stride, H=H, W=W, **kw)
    c["w"].zero_()
    c["w"][:, 0, c["ks"] // 2, c["ks"] // 2] = 1.0
    c["xs"][0][:, 0] = 4000.0
    c["xs"][0][-1, 0, -1, -1] = LIMIT
    if c["res2"] is not None:
        c["res2"].zero_()
    c["b"] = bias.clone()
    return c, FR.forward(c).float()


@pytest.mark.parametrize("name,form,kw,run", RANGE_PATHS, ids=[p[0] for p in RANGE_PATHS])
def test_range_guard_boundary_infinities_and_nan(eng, name, form, kw, run):
    """DCVC_STATUS_ACT_SATURATED per kernel and epilogue path, all exact: an output of exactly 8188 (and partial tiles, padded
    channels) leaves the word alone; nextafter(8188), reached through the bias in ONE element, sets it; the word is OR-ed
    (another bit survives) and never cleared by a clean launch; +-Inf set it; NULL works and changes no output bit.  A NaN
    output is flagged by dcvc_conv2d_small only -- the sentence in include/dcvc_hip.h at DCVC_STATUS_ACT_SATURATED."""
    Cout = kw["Cout"]
    zero = torch.zeros(Cout)
    c, want = range_layer(kw, zero)
    assert float(want.max()) == LIMIT and int((want == LIMIT).sum()) == Cout
    r = run_conv(eng, form, c, status=2, **run)
    BR.assert_bits(r["out"], want, f"{name} at the limit", AX)
    assert r["status"] == 2, f"{name}: an output of exactly 8188 set the flag"
    eps = zero.clone()
    eps[-1] = NEXT - LIMIT
    c, want = range_layer(kw, eps)
    assert int((want > LIMIT).sum()) == 1 and float(want[-1, -1, -1, -1]) == NEXT
    r = run_conv(eng, form, c, status=2, **run)
    BR.assert_bits(r["out"], want, f"{name} one ulp beyond", AX)
    assert r["status"] == 3, f"{name}: nextafter(8188) in the last element did not set the flag (word {r['status']})"
    assert run_conv(eng, form, range_layer(kw, zero)[0], status=3, **run)["status"] == 3  # a clean launch clears nothing
    null = run_conv(eng, form, c, status=None, **run)
    assert torch.equal(bits(null["out"]), bits(r["out"]))
    for v in (float("inf"), -float("inf")):
        b = zero.clone()
        b[0] = v
        c, want = range_layer(kw, b)
        r = run_conv(eng, form, c, **run)
        BR.assert_bits(r["out"], want, f"{name} bias {v}", AX)
        assert r["status"] == 1, f"{name}: an output of {v} did not set the flag"
    b = zero.clone()
    b[Cout // 2] = NAN
    c, want = range_layer(kw, b)
    r = run_conv(eng, form, c, **run)
    finite = torch.ones(Cout, dtype=torch.bool)
    finite[Cout // 2] = False
    assert bool(torch.isnan(r["out"][:, ~finite]).all())
    BR.assert_bits(r["out"][:, finite], want[:, finite], f"{name} beside a NaN channel", AX)
    assert r["status"] == (1 if form == "small" else 0), f"{name}: word {r['status']} after a NaN output"


CLAMP_PATHS = [
    ("mfma16", dict(seg_C=(24,), Cout=24, ks=3, stride=1, **S1), dict(rows=4)),
    ("mfma16", dict(seg_C=(24,), Cout=64, ks=3, stride=1, **S1, in_slope=0.25), dict(rows=8)),
    ("mfma16", dict(seg_C=(24,), Cout=24, ks=3, stride=2, **S2), {}),
    ("paired", dict(seg_C=(8,), Cout=32, ks=7, stride=1, **S1), {}),
    ("small", dict(seg_C=(24,), Cout=3, ks=7, stride=1, **S1), {}),
    ("k32", dict(seg_C=(32,), Cout=64, ks=3, stride=1, **S1), dict(waves=8)),
    ("k32", dict(seg_C=(64,), Cout=32, ks=1, stride=1, **S1, in_slope=0.25), {}),
]


@pytest.mark.parametrize("form,kw,run", CLAMP_PATHS, ids=[f"{p[0]}-k{p[1]['ks']}s{p[1]['stride']}" for p in CLAMP_PATHS])
def test_split_fp16_inputs_are_clamped_at_8188_on_load(eng, form, kw, run):
    """Inputs of 8188.5, 1e6 and -1e6 give bit for bit the result of +-8188 (after the activation on load, where there is
    one: -1e6 * 1/4 is still beyond the range); 8188 * 8 = 65504 is an fp16 number, so integer weights keep every sum exact."""
    c = FR.exact_case("int", seed=500, **kw)
    x = c["xs"][0]
    spots = [((0, 0, 5, 5), 8188.5, LIMIT), ((1, 1, 6, 20), 1e6, LIMIT), ((1, 0, -1, -1), -1e6, -LIMIT), ((0, 2, 0, 0), LIMIT, LIMIT)]
    clamped = x.clone()
    for idx, v, cl in spots:
        x[idx] = v
        clamped[idx] = cl
    BR._headroom({"forward": (sum(c["seg_C"]) * c["ks"] ** 2 * 16.0 + 2 * LIMIT * 4, BR.quantum(c["in_slope"]))})
    ref = dict(c)
    if c["in_slope"] is not None:  # clamp AFTER the activation: leaky(-1e6) = -250000 -> -8188
        ref["in_slope"] = None
        clamped = torch.nn.functional.leaky_relu(x.double(), c["in_slope"]).clamp(-LIMIT, LIMIT).float()
    want = FR.forward(ref, xs=[clamped]).float()
    r = run_conv(eng, form, c, **run)
    BR.assert_bits(r["out"], want, f"{form} clamp on load", AX)
    assert r["status"] == 1  # outputs of 4 x 8188 are beyond the range


# =====================================================================================================================
# E. refusals: DCVC_E_ARG before anything is launched, nothing written
def setter(**kw):
    def f(a):
        for k, v in kw.items():
            if k.startswith("seg0_"):
                setattr(a.seg[0], k[5:], v(a) if callable(v) else v)
            else:
                setattr(a, k, v(a) if callable(v) else v)
    return f


COMMON_REFUSALS = [  # conv_args_ok (kernel_common.h): all three entry points
    dict(nseg=0), dict(nseg=4), dict(out=None), dict(wpack=None), dict(bpack=None), dict(seg0_ptr=None),
    dict(seg0_cs=lambda a: a.seg[0].cs + 1), dict(seg0_cs=lambda a: a.seg[0].C - 4), dict(seg0_ptr=lambda a: a.seg[0].ptr + 4),
    dict(N=0), dict(N=-1), dict(Hin=0), dict(Win=0), dict(Hin=-13), dict(Cout=0),
]
CONV2D_REFUSALS = COMMON_REFUSALS + [
    dict(stride=3), dict(stride=0), dict(precision=2), dict(precision=-1), dict(Cout_pad=lambda a: a.Cout_pad + 1),
    dict(Cout=lambda a: a.Cout_pad + 1), dict(pixel_shuffle=1, Cout=23), dict(out_act=-1), dict(out_act=4), dict(ks=5), dict(ks=2),
    dict(ks=7, stride=2),
    dict(out_act=3),                                            # the mask epilogue needs res2 ...
    dict(out_act=3, res2=lambda a: a.out, res2_cs=lambda a: a.out_cs, res_gate=lambda a: a.bpack),  # ... and has no gate,
    dict(out_act=3, res2=lambda a: a.out, res2_cs=lambda a: a.out_cs, chan_partial=lambda a: a.out),  # no channel sums,
    dict(out_act=3, res2=lambda a: a.out, res2_cs=lambda a: a.out_cs, pixel_shuffle=1),               # no pixel shuffle
    dict(chan_partial=lambda a: a.out, out=lambda a: a.out + 4),  # channel sums need the 16-byte epilogue ...
    dict(chan_partial=lambda a: a.out, pixel_shuffle=1),          # ... and no pixel shuffle
    dict(tile_rows=1, tile_row0=2), dict(tile_rows=1, tile_row0=-1), dict(tile_rows=7, tile_row0=100),
]
PAIR_REFUSALS = [dict(nseg=2), dict(seg0_C=12, seg0_cs=16), dict(precision=FP32), dict(pixel_shuffle=1)]
K32_REFUSALS = COMMON_REFUSALS + [
    dict(stride=2), dict(ks=7), dict(ks=5), dict(precision=FP32), dict(Cout_pad=lambda a: a.Cout_pad + 1),
    dict(Cout=lambda a: a.Cout_pad + 1), dict(pixel_shuffle=1, Cout=62), dict(out_act=3), dict(out_act=-1), dict(seg0_C=16),
    dict(seg0_C=48, seg0_cs=48), dict(seg0_C=0),
    dict(Hin=4096, Win=4096),                                   # 2^24 output pixels: the 24-bit pixel index
    dict(Hin=2048, Win=2048, pixel_shuffle=1),                  # ... counted after the pixel shuffle
    dict(out_cs=1 << 22), dict(seg0_cs=1 << 22),                # the 24-bit channel stride (in bytes)
    dict(res=lambda a: a.out, res_cs=1 << 22), dict(res2=lambda a: a.out, res2_cs=1 << 22),
    dict(Hin=4000, Win=4000, out_cs=128),                       # an output image of 4 GiB or more
    dict(Hin=4000, Win=4000, seg0_cs=128),                      # an input image of 4 GiB or more
    dict(Hin=4000, Win=4000, res=lambda a: a.out, res_cs=128), dict(Hin=4000, Win=4000, res2=lambda a: a.out, res2_cs=128),
    dict(in_act=1, in_slope=-0.125), dict(in_act=1, in_slope=1.5), dict(in_act=1, in_slope=NAN),
    dict(out=lambda a: a.out + 4), dict(out_cs=lambda a: a.out_cs + 1), dict(Cout=62),  # no scalar epilogue
    dict(chan_partial=lambda a: a.out, pixel_shuffle=1),
    dict(tile_rows=1, tile_row0=2), dict(tile_rows=1, tile_row0=-1),
]
SMALL_REFUSALS = COMMON_REFUSALS + [
    dict(out_act=3), dict(out_act=-1), dict(tile_rows=1), dict(Cout=17), dict(ks=1), dict(ks=5), dict(stride=2),
    dict(pixel_shuffle=1), dict(res_gate=lambda a: a.bpack), dict(res2=lambda a: a.out, res2_cs=lambda a: a.out_cs),
    dict(chan_partial=lambda a: a.out), dict(precision=FP32),
]
REFUSALS = ([("mfma16", r) for r in CONV2D_REFUSALS] + [("mfma32", r) for r in CONV2D_REFUSALS[15:]] +
            [("paired", r) for r in PAIR_REFUSALS] + [("k32", r) for r in K32_REFUSALS] + [("small", r) for r in SMALL_REFUSALS])


def test_refused_arguments_return_e_arg_and_write_nothing(eng):
    """Every row is refused on the host before any launch (checked in the source: conv_args_ok, the entry points and, for the
    band rows, launch() before hipLaunchKernelGGL) -- the buffers are the small ones of a 13 x 37 layer, only the ARGUMENTS
    claim the sizes beyond dcvc_conv2d_k32's limits.  Output, status word and chan_partial must be untouched."""
    layers = {"mfma16": FR.exact_case("int", (24,), 24, 3, 1, **S1), "mfma32": FR.exact_case("int", (24,), 24, 3, 1, **S1),
              "paired": FR.exact_case("int", (8,), 32, 7, 1, **S1), "k32": FR.exact_case("int", (32,), 64, 3, 1, **S1),
              "small": FR.exact_case("int", (16,), 3, 3, 1, **S1)}
    for form, row in REFUSALS:
        try:
            run_conv(eng, form, layers[form], mutate=setter(**row), expect=E_ARG)
        except AssertionError as ex:
            raise AssertionError(f"{form} {({k: (v if not callable(v) else '<derived>') for k, v in row.items()})}: {ex}") from None
    for form, c in layers.items():  # and the unmutated layers run
        BR.assert_bits(run_conv(eng, form, c)["out"], FR.forward(c).float(), f"{form} unmutated", AX)


# =====================================================================================================================
# F. fp32 mode is the documented fmaf chain
@pytest.mark.parametrize("i", range(len(FR.CHAIN_CASES)), ids=lambda i: "k%ds%d" % FR.CHAIN_CASES[i][:2])
def test_fp32_mode_is_the_documented_fmaf_chain_bit_for_bit(eng, i):
    """DCVC_PREC_FP32 on FLOAT data (per-channel magnitudes {1e-4, 1, 30}), every element bit for bit: v_mfma_f32_32x32x2_f32
    is a k-ordered chain of fmaf's, and conv_mfma.hip spells out the order -- segment, 16-channel chunk, tap (row-major,
    staged whole or by filter rows), k2, j, lane half -- which forward_conv_ref.fmaf_chain restates with an exact vectorised
    fma (the order is read from the source, not fitted to a result).  The 4-row and the 8-row tiles must give these same
    bits: a tile's shape changes nothing in an output's chain."""
    layer, chain, ref64, M = FR.chain_case(i)
    for rows in ((None,) if layer["stride"] == 2 else (4, 8)):
        got = run_conv(eng, "mfma32", layer, rows=rows)["out"]
        err = (got.double() - ref64).abs() / (2.0 ** -24 * M)
        print(f"k{layer['ks']} s{layer['stride']} rows={rows}: {int((bits(got) != bits(chain)).sum())} of {got.numel()} elements differ "
              f"from the chain; worst |got - ref64| = {float(err.max()):.3f} x 2^-24 M_e")
        BR.assert_bits(got, chain, f"fp32 k{layer['ks']} s{layer['stride']} rows={rows} against the fmaf chain", AX)
