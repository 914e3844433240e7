"""The hand-written convolution and resampling backward kernels (csrc/backward.hip) element by element, on a real MI355X.

On the exact data of tests/backward_ref.py (small integers, dyadic slopes / gates / flows) every partial sum is exactly
representable, so the fp32 result does not depend on summation order, tiling, split count or load path, and EVERY element
is demanded bit for bit against the float64 autograd reference cast to fp32 (tests/test_backward_ref_host.py proves that
property on the references alone).  A dropped pixel, a doubled tap, a wrong border row or a stale tile of the software
pipeline cannot hide behind a tolerance.  (A zero gradient has no sign: +0 and -0 compare equal, see assert_bits.)

Every output lives in a wider buffer filled with NaN: dw outside [cin_offset, cin_offset + C), db beyond Cout, channels
outside a view, and the words behind the scratch must be untouched afterwards; inputs are NaN outside their views too,
so a read outside a view poisons the result.

Exact data cannot see the hi.lo / lo.hi terms of the split-bf16 weight gradient (integers have a zero lo part): part D
holds float-valued data to per-element bounds derived from the references, never from what the kernels return.

How many tiles a weight-gradient workgroup walks (the launcher's rule, dcvc_conv_wgrad in backward.hip):
    splits = min(256, ntiles, max(ceil(512 / (nct * groups)), ntiles / 8), scratch_floats / scratch_min)
with ntiles = N * ceil(Ho / 4) * ceil(Wo / TW) (TW 32, stride 2: 16), nct = ceil(Cout / 32) * ceil(C / 32), groups = 7
for 7x7 else 1.  Whenever nct * groups * ntiles <= 512 every workgroup handles ONE tile -- all of
tests/test_gpu_backward.py::CONV_CASES.  Here the pipelined loop runs (a) pinned through scratch_floats = k * scratch_min:
64->64 3x3 at 17x45 has 2 x 5 tiles, k = 1 walks 10, k = 3 walks 4 + 3 + 3; (b) naturally through the Tape: 8->32 7x7,
N = 3, 40x72 (90 tiles, 74 splits) and 128->128 3x3, N = 2, 24x72 (36 tiles, 32 splits); `wgrad_splits` restates the
rule and the tests assert splits < ntiles, so a later change of the rule cannot silently empty these cases."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import backward_ref as BR

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 12345.0
FP32, FAST = 0, 1
E_ARG = -1
WGRAD_AX = "co,ci,ky,kx"


@pytest.fixture(scope="module")
def eng():
    from vcm_ts_amd.engine import Engine

    return Engine("cuda:0", "fp32")


@pytest.fixture(scope="module")
def eng_fast():
    from vcm_ts_amd.engine import Engine

    return Engine("cuda:0", "fp16x3")


def r4(c):
    return (c + 3) // 4 * 4


def wide(x, off, cs, fill=NAN):
    """View of x's channels (NCHW, CPU) at channel offset `off` of a `fill`-ed (N, H, W, cs) device buffer"""
    from vcm_ts_amd.engine import View

    N, Cc, H, W = x.shape
    base = torch.full((N, H, W, cs), fill, dtype=torch.float32, device="cuda:0")
    v = View(base, Cc, off)
    v.nchw().copy_(x.to(base.device))
    return v


def read(v, what):
    """the view's channels as a CPU NCHW tensor, after checking that every other channel of its buffer is still NaN"""
    torch.cuda.synchronize()
    b = v.base.cpu()
    keep = torch.ones(v.cs, dtype=torch.bool)
    keep[v.coff:v.coff + v.C] = False
    assert bool(torch.isnan(b[..., keep]).all()), f"{what}: wrote outside channels [{v.coff}, {v.coff + v.C}) of {v}"
    return b[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).contiguous()


def wgrad_splits(N, Ho, Wo, Cc, Cout, ks, stride, scratch_floats, per_split):
    """the launcher's documented split rule -> (splits, ntiles)"""
    nct = ((Cout + 31) // 32) * ((Cc + 31) // 32)
    groups = 7 if ks == 7 else 1
    TW = 32 if stride == 1 else 16
    ntiles = N * ((Ho + 3) // 4) * ((Wo + TW - 1) // TW)
    splits = max(-(-512 // (nct * groups)), ntiles // 8)
    splits = max(1, min(splits, 256, ntiles, scratch_floats // per_split))
    return splits, ntiles


# =====================================================================================================================
# B. dcvc_conv_wgrad through the C ABI
def run_wgrad(e, x, dpre, ks, stride, prec, k=None, xv=(0, None), dv=(0, None), in_slope=None, cin_pad=(2, 3), prefill=None,
              with_db=True, mutate=None, expect=0):
    """One dcvc_conv_wgrad call on the engine's stream with NaN canaries everywhere.  k: scratch_floats = k * scratch_min
    (None: 64 x, more than any case here has tiles).  xv / dv: (channel offset, channel stride) of the x / dpre views.
    prefill: integer content of the dw slice, accumulated onto (overwrite = 0).  -> dw slice, db (CPU) or None."""
    from vcm_ts_amd import lib

    L, dev = e.L, torch.device("cuda:0")
    N, Cc, H, W = x.shape
    Cout, Ho, Wo = dpre.shape[1:]
    X = wide(x, xv[0], xv[1] or r4(xv[0] + Cc))
    zs = stride
    Hd, Wd = (H, W) if zs == 2 else (Ho, Wo)
    dcs = dv[1] or r4(dv[0] + Cout)
    D = torch.full((N, Hd, Wd, dcs), NAN, dtype=torch.float32, device=dev)  # between the samples of a zero-inserted
    D[:, ::zs, ::zs, dv[0]:dv[0] + Cout][:, :Ho, :Wo] = dpre.permute(0, 2, 3, 1).to(dev)  # dpre: NaN, never to be read
    before, after = cin_pad
    DW = torch.full((Cout, before + Cc + after, ks, ks), NAN, dtype=torch.float32, device=dev)
    if prefill is not None:
        DW[:, before:before + Cc] = prefill.to(dev)
    DB = torch.full((Cout + 7,), NAN, dtype=torch.float32, device=dev)
    per = int(L.dcvc_conv_wgrad_scratch_min(Cout, Cc, ks))
    assert per > 0
    floats = per * (k or 64)
    SC = torch.full((floats + 256,), NAN, dtype=torch.float32, device=dev)
    SC[floats:] = SENT
    a = lib.WgradArgs()
    a.x, a.x_cs, a.C = X.ptr, X.cs, Cc
    a.in_act, a.in_slope = (0, 0.0) if in_slope is None else (1, float(in_slope))
    a.dpre, a.dpre_cs, a.zs, a.Hd, a.Wd = D.data_ptr() + 4 * dv[0], dcs, zs, Hd, Wd
    a.N, a.Hin, a.Win, a.Ho, a.Wo, a.Cout, a.ks, a.stride = N, H, W, Ho, Wo, Cout, ks, stride
    a.dw, a.Cin_total, a.cin_offset = DW.data_ptr(), before + Cc + after, before
    a.scratch, a.scratch_floats = SC.data_ptr(), floats
    a.overwrite = int(prefill is None)
    a.db = DB.data_ptr() if with_db else None
    a.precision = prec
    if mutate is not None:
        mutate(a)
    rc = L.dcvc_conv_wgrad(C.byref(a), e.stream())
    torch.cuda.synchronize()
    what = f"wgrad {Cc}->{Cout} k{ks} s{stride} {H}x{W} N{N} prec{prec} k={k} xv={xv} dv={dv}"
    if expect:
        assert rc == expect, f"{what}: returned {rc}, expected {expect}"
        assert bool(torch.isnan(DW).all()) and bool(torch.isnan(DB).all()) and bool(torch.isnan(SC[:floats]).all()), \
            f"{what}: a refused call wrote something"
        return None, None
    lib.check(rc, what)
    dw = DW.cpu()
    out_of_slice = torch.cat([dw[:, :before], dw[:, before + Cc:]], 1)
    assert bool(torch.isnan(out_of_slice).all()), f"{what}: dw written outside input channels [{before}, {before + Cc})"
    assert bool((SC[floats:] == SENT).all()), f"{what}: wrote behind scratch_floats"
    db = DB.cpu()
    assert bool(torch.isnan(db[Cout:]).all()), f"{what}: db written beyond Cout"
    assert bool(torch.isnan(db).all()) or with_db, f"{what}: db written although NULL was passed"
    return dw[:, before:before + Cc].contiguous(), (db[:Cout] if with_db else None)


@functools.lru_cache(maxsize=None)
def wg_case(Cc, Cout, ks, stride, H, W, N, in_slope=None):
    """exact data and its float64 reference cast to fp32: computed once, shared by both precisions and every variant"""
    x, d = BR.wgrad_exact(Cc, Cout, ks, stride, H, W, N, in_slope, seed=Cc * 5 + Cout + ks + H + N)
    dw, db = BR.wgrad(x, d, ks, stride, in_slope)
    return x, d, dw.float(), db.float()


def check_wgrad(e, prec, Cc, Cout, ks, stride, H, W, N, in_slope=None, **kw):
    x, d, dw, db = wg_case(Cc, Cout, ks, stride, H, W, N, in_slope)
    got_w, got_b = run_wgrad(e, x, d, ks, stride, prec, in_slope=in_slope, **kw)
    what = f"{Cc}->{Cout} k{ks} s{stride} {H}x{W} N{N} prec{prec} {kw}"
    BR.assert_bits(got_w, dw, "dw " + what, WGRAD_AX)
    if got_b is not None:
        BR.assert_bits(got_b, db, "db " + what, "co")
    return got_w


CHANNELS = [(64, 64), (3, 64), (64, 3), (16, 2), (40, 33)]
HW_S1 = [(17, 45), (4, 32), (5, 33), (1, 1)]
HW_S2 = [(21, 37), (20, 37)]
PRECS = pytest.mark.parametrize("prec", [FP32, FAST], ids=["fp32", "fp16x3"])


@PRECS
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_wgrad_stride1_grid_bit_for_bit(eng, ch, ks, prec):
    """1x1 and 3x3 on the fp32 MFMA kernel and on the bf16 hi/lo kernel: channel counts with tails in both tile
    dimensions (3, 2, 33, 40), sizes that are no multiple of the 4 x 32 tile, a single pixel, one and two samples; db
    (Cout = 33: the tail tile of the bias partials) from the same pass."""
    for H, W in HW_S1:
        for N in (1, 2):
            check_wgrad(eng, prec, ch[0], ch[1], ks, 1, H, W, N)


@PRECS
def test_wgrad_7x7_grid_bit_for_bit(eng, prec):
    for H, W in HW_S1:
        for N in (1, 2):
            check_wgrad(eng, prec, 8, 32, 7, 1, H, W, N)


@PRECS
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_wgrad_stride2_with_zero_inserted_dpre_bit_for_bit(eng, ch, ks, prec):
    """stride 2 reads dpre at (2 oy, 2 ox) of an Hd x Wd = input-sized buffer (the positions between the samples hold NaN
    here: the weight gradient must never read them); odd sizes make the last output row / column end on the last input
    pixel (21, 37) or one before it (20).  Fast mode keeps stride-2 layers on the fp32 kernel."""
    for H, W in HW_S2:
        for N in (1, 2):
            check_wgrad(eng, prec, ch[0], ch[1], ks, 2, H, W, N)


@PRECS
def test_wgrad_split_counts_pinned_by_scratch_give_the_same_bits(eng, prec):
    """64->64 3x3 at 17x45, N = 1: 2 x 5 tiles.  scratch_floats = k * scratch_min pins the split count: k = 1 makes one
    workgroup per channel tile walk all 10 tiles through the register pipeline, k = 3 walks 4 + 3 + 3 (uneven trip
    counts), a large scratch gives one tile per workgroup.  The same for 8->32 7x7 with two samples (20 tiles)."""
    for Cc, Cout, ks, N in ((64, 64, 3, 1), (8, 32, 7, 2), (40, 33, 1, 2)):
        per = int(eng.L.dcvc_conv_wgrad_scratch_min(Cout, Cc, ks))
        seen = []
        for k in (1, 3, None):
            splits, ntiles = wgrad_splits(N, 17, 45, Cc, Cout, ks, 1, per * (k or 64), per)
            assert ntiles == 10 * N and splits == (k or ntiles), (splits, ntiles)
            seen.append(check_wgrad(eng, prec, Cc, Cout, ks, 1, 17, 45, N, k=k))
        assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])


VIEWS = [(1, 8), (4, 8), (0, 1)]  # (channel offset, extra stride): unaligned pointer, aligned slice, stride = C + 1


@PRECS
@pytest.mark.parametrize("Cc,Cout,ks,stride", [(64, 64, 3, 1), (40, 36, 1, 1), (8, 32, 7, 1), (40, 33, 3, 2)],
                         ids=["64to64k3", "40to36k1", "8to32k7", "40to33k3s2"])
def test_wgrad_views_scalar_and_vector_load_paths(eng, Cc, Cout, ks, stride, prec):
    """x and dpre as channel slices: offset 1 (pointer not 16-byte aligned: scalar loads), offset 4 of a buffer of stride
    C + 8 (vector loads for C = 64 / 40 / 8, scalar for Cout = 33: stride 41), offset 0 of a buffer of stride C + 1
    (scalar).  Each must give the bits of the dense, aligned call; with k = 1 the scalar path also runs the tile loop."""
    H, W = ((21, 37) if stride == 2 else (17, 45))
    dense = check_wgrad(eng, prec, Cc, Cout, ks, stride, H, W, 1)
    for off, extra in VIEWS:
        for kw in (dict(xv=(off, Cc + extra)), dict(dv=(off, Cout + extra)),
                   dict(xv=(off, Cc + extra), dv=(off, Cout + extra), k=1)):
            assert torch.equal(check_wgrad(eng, prec, Cc, Cout, ks, stride, H, W, 1, **kw), dense), kw


@PRECS
def test_wgrad_accumulates_onto_integer_prefill_exactly(eng, prec):
    for Cc, Cout, ks, stride, H, W in ((40, 33, 3, 1, 17, 45), (64, 64, 1, 2, 21, 37), (8, 32, 7, 1, 5, 33)):
        x, d, dw, db = wg_case(Cc, Cout, ks, stride, H, W, 2)
        pre = BR.ints(torch.Generator().manual_seed(ks), dw.shape, 50)
        for k in (1, None):
            got_w, got_b = run_wgrad(eng, x, d, ks, stride, prec, k=k, prefill=pre)
            BR.assert_bits(got_w, (pre.double() + dw.double()).float(), f"dw += k{ks} s{stride} k={k}", WGRAD_AX)
            BR.assert_bits(got_b, db, "db is written (=), not accumulated", "co")


@PRECS
@pytest.mark.parametrize("slope", [0.25, 0.0])
def test_wgrad_activation_on_load(eng, slope, prec):
    """in_act = 1: x is LeakyReLU'd when the tile is written to LDS (zeros of x are planted on the kink)"""
    for Cc, Cout, ks, stride, H, W in ((64, 64, 3, 1, 17, 45), (3, 64, 1, 1, 5, 33), (8, 32, 7, 1, 5, 33), (40, 33, 3, 2, 21, 37)):
        for k in (1, None):
            check_wgrad(eng, prec, Cc, Cout, ks, stride, H, W, 2, in_slope=slope, k=k)


@PRECS
def test_wgrad_without_db_writes_the_same_dw_and_no_bias(eng, prec):
    for Cc, Cout, ks in ((40, 33, 3), (64, 3, 1), (8, 32, 7)):
        a = check_wgrad(eng, prec, Cc, Cout, ks, 1, 17, 45, 2, with_db=False)
        assert torch.equal(a, check_wgrad(eng, prec, Cc, Cout, ks, 1, 17, 45, 2))


def test_wgrad_argument_checks_return_e_arg_without_a_launch(eng):
    x, d, _, _ = wg_case(16, 2, 3, 1, 5, 33, 1)
    x7, d7, _, _ = wg_case(8, 32, 7, 1, 5, 33, 1)
    x2, d2, _, _ = wg_case(3, 64, 3, 2, 21, 37, 1)

    def setter(**kw):
        def f(a):
            for k_, v in kw.items():
                setattr(a, k_, v(a) if callable(v) else v)
        return f

    for xx, dd, ks, stride, mut in (
            (x, d, 3, 1, setter(ks=5)),
            (x7, d7, 7, 1, setter(stride=2)),
            (x, d, 3, 1, setter(Ho=lambda a: a.Ho - 1)),
            (x, d, 3, 1, setter(Wo=lambda a: a.Wo - 1)),
            (x, d, 3, 1, setter(cin_offset=lambda a: a.Cin_total - a.C + 1)),
            (x, d, 3, 1, setter(scratch_floats=lambda a: a.scratch_floats // 64 - 1)),
            (x2, d2, 3, 2, setter(Hd=lambda a: (a.Ho - 1) * 2)),
            (x2, d2, 3, 2, setter(Wd=lambda a: (a.Wo - 1) * 2)),
            (x, d, 3, 1, setter(precision=2))):
        for prec in (FP32, FAST):
            run_wgrad(eng, xx, dd, ks, stride, prec, mutate=mut, expect=E_ARG)


# =====================================================================================================================
# C. whole conv backward through the Tape on exact data
TAPE_CASES = [  # the epilogues of tests/test_gpu_backward.py::CONV_CASES with dyadic slopes
    dict(name="k3s1_act_res", seg_C=(64,), Cout=64, ks=3, stride=1, H=20, W=36, out_slope=0.25, res=True),
    dict(name="k3s1_plain", seg_C=(64,), Cout=64, ks=3, stride=1, H=20, W=36),
    dict(name="k3s2_act", seg_C=(64,), Cout=64, ks=3, stride=2, H=20, W=36, out_slope=0.25),
    dict(name="k1s2", seg_C=(64,), Cout=64, ks=1, stride=2, H=20, W=36),
    dict(name="k1s1_gate", seg_C=(32, 32), Cout=64, ks=1, stride=1, H=20, W=36, res=True, gate=True),
    dict(name="k7_relu", seg_C=(8,), Cout=32, ks=7, stride=1, H=24, W=40, out_slope=0.0),
    dict(name="k7_to2_res", seg_C=(16,), Cout=2, ks=7, stride=1, H=24, W=40, res=True),
    dict(name="k3_ps_act", seg_C=(64,), Cout=256, ks=3, stride=1, H=12, W=20, out_slope=0.25, ps=True),
    dict(name="k1_ps", seg_C=(128,), Cout=256, ks=1, stride=1, H=12, W=20, ps=True),
    dict(name="k3_inact_res2", seg_C=(128,), Cout=64, ks=3, stride=1, H=12, W=20, in_slope=0.25, out_slope=0.5, res=True,
         res2=True),
    dict(name="k3_seg3", seg_C=(64, 64, 96), Cout=96, ks=3, stride=1, H=8, W=12, out_slope=0.5),
    dict(name="k3_cinslice", seg_C=(128,), Cout=192, ks=3, stride=1, H=8, W=12, out_slope=0.5, cin_slice=(0, 128, 192)),
    dict(name="k3_3to64", seg_C=(3,), Cout=64, ks=3, stride=1, H=20, W=36),
    dict(name="k3_67s2", seg_C=(3, 64), Cout=64, ks=3, stride=2, H=20, W=36),
    dict(name="k3_64to3", seg_C=(64,), Cout=3, ks=3, stride=1, H=20, W=36),
    dict(name="k3_odd_size", seg_C=(64,), Cout=64, ks=3, stride=1, H=17, W=45, N=1, out_slope=0.25),
    # stride 2 at odd sizes: Hd x Wd of the zero-inserted dpre equals the input size, last row / column on the last pixel
    dict(name="k3s2_21x37", seg_C=(64,), Cout=64, ks=3, stride=2, H=21, W=37, out_slope=0.25),
    dict(name="k3s2_20x37", seg_C=(64,), Cout=64, ks=3, stride=2, H=20, W=37, out_slope=0.0, res=True),
    dict(name="k1s2_21x37", seg_C=(40,), Cout=33, ks=1, stride=2, H=21, W=37),
    dict(name="k3_67s2_21x37", seg_C=(3, 64), Cout=64, ks=3, stride=2, H=21, W=37, in_slope=0.5),
    # several tiles per workgroup by the launcher's own rule (nct * groups * ntiles > 512)
    dict(name="k7_many_tiles", seg_C=(8,), Cout=32, ks=7, stride=1, H=40, W=72, N=3, out_slope=0.0, many=True),
    dict(name="k3_many_tiles", seg_C=(128,), Cout=128, ks=3, stride=1, H=24, W=72, N=2, out_slope=0.25, many=True),
]


@functools.lru_cache(maxsize=None)
def tape_case(i):
    """exact data of TAPE_CASES[i] and its float64 reference: computed once, shared by both precisions"""
    kw = {k: v for k, v in TAPE_CASES[i].items() if k not in ("name", "many")}
    c = BR.conv_exact(seed=i, **kw)
    return c, BR.conv_backward(c)


def tape_conv(e, name, c):
    """conv_case of tests/diag/grad_check.py on given data -> every result as a CPU tensor"""
    from vcm_ts_amd.grad import Tape

    dev = e.device
    N, H, W, Ho, Wo, ps = c["N"], c["H"], c["W"], c["Ho"], c["Wo"], c["ps"]
    m, Cf = (2, c["Cout"] // 4) if ps else (1, c["Cout"])
    w = c["w"].to(dev).requires_grad_()
    b = c["b"].to(dev).requires_grad_()
    tape = Tape(e)
    e.tape = tape
    try:
        vs = [e.from_nchw(x.to(dev), e.buf(f"{name}.x{i}", N, H, W, x.shape[1])) for i, x in enumerate(c["xs"])]
        rv = e.from_nchw(c["res"].to(dev), e.buf(f"{name}.res", N, Ho * m, Wo * m, Cf)) if c["res"] is not None else None
        rv2 = e.from_nchw(c["res2"].to(dev), e.buf(f"{name}.res2", N, Ho * m, Wo * m, Cf)) if c["res2"] is not None else None
        gv = c["gate"].to(dev).contiguous().view(-1) if c["gate"] is not None else None
        pk = e.pack((name,), w, b, c["seg_C"], ps, None if c["cin_slice"] is None else c["cin_slice"][:2])
        out = e.buf(f"{name}.out", N, Ho * m, Wo * m, Cf)
        e.conv(pk, vs, out, stride=c["stride"], in_slope=c["in_slope"], out_slope=c["out_slope"], res=rv, gate=gv, res2=rv2)
    finally:
        e.tape = None
    got = {"out": e.to_nchw(out).cpu()}
    e.from_nchw(c["dout"].to(dev), tape.grad(out))
    tape.backward()
    torch.cuda.synchronize()
    got["dw"], got["db"] = tape.pgrads[id(w)].cpu(), tape.pgrads[id(b)].cpu()
    for i, v in enumerate(vs):
        got[f"dx{i}"] = e.to_nchw(tape.grad(v)).cpu()
    if rv is not None:
        got["dres"] = e.to_nchw(tape.grad(rv)).cpu()
    if rv2 is not None:
        got["dres2"] = e.to_nchw(tape.grad(rv2)).cpu()
    if gv is not None:
        got["dgate"] = tape.vec[gv.data_ptr()].view(N, Cf).cpu()
    return got


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("case", TAPE_CASES, ids=[c["name"] for c in TAPE_CASES])
def test_conv_backward_through_the_tape_bit_for_bit(eng, eng_fast, case, precision):
    """Forward output, dw, db, every dx, dres, dres2 and dgate of a recorded layer, bit for bit, twice.

    fp16x3: the forward and the data gradient run on the split-fp16 kernels, stride-1 weight gradients on the split-bf16
    kernel.  All of it is exact on these data by construction: every activation, weight and gradient operand is a
    multiple of 1/4 of magnitude <= 4 (integers, times slopes from {0, 1/4, 1/2}), which fp16 and bf16 hold exactly (lo
    parts are zero, the pre-scales of the lo terms are powers of two), and the accumulation is fp32 in both modes.  No
    quantity of the fast path needs a bound here."""
    from vcm_ts_amd.grad import WGRAD_SCRATCH_FLOATS

    e = eng if precision == "fp32" else eng_fast
    name, many = case["name"], case.get("many", False)
    c, want = tape_case(TAPE_CASES.index(case))
    assert c["headroom"] > 1
    if many:
        for Cc in c["seg_C"]:
            per = int(e.L.dcvc_conv_wgrad_scratch_min(c["Cout"], Cc, c["ks"]))
            splits, ntiles = wgrad_splits(c["N"], c["Ho"], c["Wo"], Cc, c["Cout"], c["ks"], c["stride"], WGRAD_SCRATCH_FLOATS, per)
            nct = ((c["Cout"] + 31) // 32) * ((Cc + 31) // 32)
            assert nct * (7 if c["ks"] == 7 else 1) * ntiles > 512 and splits < ntiles, (splits, ntiles)
    first = None
    for run in range(2):
        got = tape_conv(e, f"x_{precision}_{name}", c)
        assert set(got) == set(want)
        for k in want:
            BR.assert_bits(got[k], want[k], f"{name} {precision} run {run}: {k}", BR.conv_axes(k))
        if first is not None:
            for k in got:
                assert torch.equal(got[k].view(torch.int32), first[k].view(torch.int32)), f"{name}: {k} differs between two runs"
        first = got


# =====================================================================================================================
# D. float-valued weight gradients against per-element bounds (the lo terms of the bf16 split)
@PRECS
@pytest.mark.parametrize("mag", BR.DY_MAGS)
@pytest.mark.parametrize("ks,Cc,Cout", BR.FLOAT_CASES, ids=["k1_40to33", "k3_64to64", "k7_8to32"])
def test_wgrad_float_data_within_per_element_bounds(eng, ks, Cc, Cout, mag, prec):
    """x = randn x per-channel {1e-4, 1, 30}, dY = randn x {1e-9, 1, 3e4}, 17x45 (2 x 5 tiles), with every tile in one
    workgroup (k = 1) and one tile per workgroup.  Per element, no element excluded: |got - ref64| <= bound,
        fp32:   c * 2^-24 * M_e      M_e = sum |dY||X| (float64),
                c = 4 * max_e |ref32 - ref64| / (2^-24 M_e), ref32 = torch's fp32 CPU autograd of the same case -- measured
                against the REFERENCE, never the kernel; 4 is the tier-B margin of grad_check.tier_check (another
                summation order of the same arithmetic)
        fp16x3: 2^-16 * M_e + the fp32 bound: include/dcvc_hip_grad.h's figure (dropped lo.lo, two bf16 truncations of lo,
                each <= 2^-18 |a||b|).
    c comes from the CPU reference alone (tests/test_backward_ref_host.py::test_float_bounds_have_teeth prints it and shows
    that the LOOSER bound rejects X or dY rounded to bf16 and a single dropped product); it depends on how the host's
    convolution blocks its sums, so the test recomputes it where it runs.  Measured for |dY| ~ 1e-9 / 1 / 3e4:
        on the MI355X host:  1x1 40->33: 4.38 / 3.53 / 5.79   3x3 64->64: 15.16 / 13.65 / 13.80   7x7 8->32: 14.63 / 13.91 / 13.37
        on a build host:     1x1 40->33: 6.31 / 5.06 / 3.76   3x3 and 7x7 as above
    The kernels' worst error / bound there: fp32 0.27 (all tiles in one workgroup) and 0.11 (one tile each), i.e. at most
    1.6 x 2^-24 M_e; fp16x3 0.08, i.e. at most 21.4 x 2^-24 M_e = 0.084 x 2^-16 M_e."""
    x, dy, ref64, ref32, M = BR.float_case(ks, Cc, Cout, mag)
    c = BR.fp32_constant(ref32, ref64, M)
    bound = c * 2.0 ** -24 * M + (2.0 ** -16 * M if prec == FAST else 0.0)
    for k in (1, None):
        got, _ = run_wgrad(eng, x, dy, ks, 1, prec, k=k)
        err = (got.double() - ref64).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        ratio = err / bound
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"ks {ks} {Cc}->{Cout} |dY|~{mag:g} prec {prec} k={k}: c = {c:.3f}, worst error / bound = {float(ratio[i]):.3f} "
              f"at ({WGRAD_AX})={tuple(int(v) for v in i)}, worst error / (2^-24 M) = {float((err / (2.0 ** -24 * M)).max()):.3f}")
        assert bool((err <= bound).all()), \
            f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst at ({WGRAD_AX})={tuple(int(v) for v in i)}: " \
            f"got {float(got[i])!r} want {float(ref64[i])!r} error {float(err[i]):.3e} > {float(bound[i]):.3e}"


# =====================================================================================================================
# E. warp / up2 / down2 backward
WARP_HW = [(3, 3), (5, 9), (17, 5), (9, 33), (33, 17)]


@functools.lru_cache(maxsize=None)
def warp_case(Cc, N, H, W, scale):
    d = BR.warp_exact(Cc, N, H, W, seed=Cc + H + N, dout_scale=scale)
    s64, f64 = BR.warp_backward(d["src"], d["flow"], d["dout"])
    return d, s64, f64


def run_warp(e, d, dsrc_view, dflow_view, fix, zero_prefill=False):
    """dsrc_view / dflow_view: (offset, stride) or None for a NULL pointer -> (dsrc, dflow) CPU NCHW (or None)"""
    from vcm_ts_amd import lib

    N, Cc, H, W = d["src"].shape
    S = wide(d["src"], 3, Cc + 5)
    Fl = wide(d["flow"], 1, 7)
    G = wide(d["dout"], 4, r4(Cc) + 8)
    ps, pf = d["prefill_src"], d["prefill_flow"]
    if zero_prefill:
        ps, pf = torch.zeros_like(ps), torch.zeros_like(pf)
    DS = wide(ps, *dsrc_view) if dsrc_view else None
    DF = wide(pf, *dflow_view) if dflow_view else None
    lib.check(e.L.dcvc_warp_bwd(S.ptr, S.cs, Fl.ptr, Fl.cs, G.ptr, G.cs, DS.ptr if DS else None, DS.cs if DS else 0,
                                DF.ptr if DF else None, DF.cs if DF else 0, N, H, W, Cc,
                                fix.data_ptr() if DS else None, e.stream()), "warp_bwd")
    what = f"warp_bwd C{Cc} N{N} {H}x{W} x{d['dout_scale']:g}"
    return (read(DS, what + " dsrc") if DS else None), (read(DF, what + " dflow") if DF else None)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -30, 2.0 ** 14], ids=["x1", "x2^-30", "x2^14"])
@pytest.mark.parametrize("Cc", [1, 3, 8, 24, 64, 130])
def test_warp_bwd_bit_for_bit(eng, Cc, scale):
    """dcvc_warp_bwd on sub-pixel, integer-line, border, out-of-picture and many-to-one positions (backward_ref.warp_exact):
    dsrc (64-bit fixed-point scatter, scale chosen per call from max |dout|: three magnitudes) and dflow bit for bit onto
    non-zero prefill; dflow exactly 0 where the position is at or beyond a border; either output alone gives the other's
    bits; fix_scratch, control word included, is all zero afterwards and a second call on it gives the same bits.  C = 130:
    64 lanes per pixel, each looping over channels; C = 1 and 3: no power of two."""
    for H, W in WARP_HW:
        for N in (1, 2):
            d, s64, f64 = warp_case(Cc, N, H, W, scale)
            what = f"C{Cc} N{N} {H}x{W} x{scale:g}"
            n = N * H * W * Cc + 1
            fix = torch.zeros(n + 8, dtype=torch.int64, device="cuda:0")
            fix[n:] = 0x5A5A5A5A
            want_s = (d["prefill_src"].double() + s64).float()
            want_f = (d["prefill_flow"].double() + f64).float()
            odd, even = (Cc + 5) | 1, (Cc + 8) & ~1
            for rep, (sv, fv) in enumerate((((1, odd), (4, 8)), ((4, even), (1, 5)))):
                ds, df = run_warp(eng, d, sv, fv, fix)
                BR.assert_bits(ds, want_s, f"dsrc {what} view {sv} call {rep}", "n,c,y,x")
                BR.assert_bits(df, want_f, f"dflow {what} view {fv} call {rep}", "n,xy,y,x")
                assert bool((fix[:n] == 0).all()), f"{what}: fix_scratch is not all zero after call {rep}"
                assert bool((fix[n:] == 0x5A5A5A5A).all()), f"{what}: wrote behind fix_scratch"
            ds, none = run_warp(eng, d, (4, even), None, fix)
            assert none is None
            BR.assert_bits(ds, want_s, f"dsrc alone {what}", "n,c,y,x")
            assert bool((fix[:n] == 0).all())
            none, df = run_warp(eng, d, None, (4, 8), fix, zero_prefill=True)
            assert none is None
            BR.assert_bits(df, f64.float(), f"dflow alone {what}", "n,xy,y,x")
            mask = BR.warp_masks(d["flow"])
            assert bool((df[~mask] == 0).all()), f"{what}: dflow is not exactly 0 at or beyond a border"
            assert bool((fix[:n] == 0).all())


@pytest.mark.parametrize("Cc", [2, 67])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (2, 2), (5, 7), (6, 5)])
def test_up2_bwd_bit_for_bit(eng, H, W, Cc):
    """dcvc_up2_bwd (a gather with dyadic weights) onto integer prefill: one-pixel pictures and rows (i1 clamps onto i0,
    both weights land on one source), odd and even strides, offsets 1 and 4, scales 2 and 1."""
    from vcm_ts_amd import lib

    N = 2
    dout, pre = BR.resample_exact(N, Cc, H, W, 2, seed=H * W + Cc)
    for scale in (2.0, 1.0):
        want = BR.up2_backward(dout, scale, pre).float()
        for (go, gcs), (so, scs) in (((4, r4(Cc) + 8), (1, (Cc + 3) | 1)), ((1, Cc + 2), (4, (Cc + 8) & ~1))):
            G, DS = wide(dout, go, gcs), wide(pre, so, scs)
            lib.check(eng.L.dcvc_up2_bwd(G.ptr, G.cs, DS.ptr, DS.cs, N, H, W, Cc, scale, eng.stream()), "up2_bwd")
            BR.assert_bits(read(DS, "up2_bwd"), want, f"up2_bwd {H}x{W} C{Cc} x{scale} dsrc at {so}/{scs}", "n,c,y,x")


@pytest.mark.parametrize("Cc", [3, 64])
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (4, 6)])
def test_down2_bwd_bit_for_bit(eng, H, W, Cc):
    """dcvc_down2_bwd is one multiply (by scale / 4 = 1/8) and one add deep: bit-identical on integers with integer
    prefill and on arbitrary floats (product exact, the add onto the prefill is one IEEE operation)."""
    from vcm_ts_amd import lib

    N = 2
    dout, pre = BR.resample_exact(N, Cc, H, W, 0.5, seed=H * W + Cc)
    g = torch.Generator().manual_seed(H + W + Cc)
    fl, fpre = torch.randn(dout.shape, generator=g) * 1e-3, torch.randn(pre.shape, generator=g)
    want_f = fpre + BR.down2_backward(fl, 0.5).float()  # fp32: exact product, one rounded add
    for dd, pp, want in ((dout, pre, BR.down2_backward(dout, 0.5, pre).float()), (fl, torch.zeros_like(pre), BR.down2_backward(fl, 0.5).float()),
                         (fl, fpre, want_f)):
        for (go, gcs), (so, scs) in (((4, r4(Cc) + 8), (1, (Cc + 3) | 1)), ((1, Cc + 2), (4, (Cc + 8) & ~1))):
            G, DS = wide(dd, go, gcs), wide(pp, so, scs)
            lib.check(eng.L.dcvc_down2_bwd(G.ptr, G.cs, DS.ptr, DS.cs, N, H, W, Cc, 0.5, eng.stream()), "down2_bwd")
            BR.assert_bits(read(DS, "down2_bwd"), want, f"down2_bwd {H}x{W} C{Cc} dsrc at {so}/{scs}", "n,c,y,x")


@pytest.mark.parametrize("H,W", [(5, 6), (6, 5), (3, 3), (1, 2)])
def test_down2_bwd_refuses_odd_sizes_without_writing(eng, H, W):
    G = wide(torch.ones(1, 3, max(H // 2, 1), max(W // 2, 1)), 0, 4)
    DS = wide(torch.zeros(1, 3, H, W), 1, 7, fill=SENT)
    DS.base.fill_(SENT)
    assert eng.L.dcvc_down2_bwd(G.ptr, G.cs, DS.ptr, DS.cs, 1, H, W, 3, 0.5, eng.stream()) == E_ARG
    torch.cuda.synchronize()
    assert bool((DS.base == SENT).all())


def test_resampling_backward_through_the_tape_bit_for_bit(eng):
    """warp, up2 and down2 once each as the Tape drives them (zero-initialised gradient buffers of the forward layout),
    and the odd-size down2 must raise instead of writing."""
    from vcm_ts_amd import lib
    from vcm_ts_amd.grad import Tape

    e, dev = eng, eng.device
    d, s64, f64 = warp_case(24, 2, 5, 9, 1.0)
    tape = Tape(e)
    e.tape = tape
    try:
        sv = e.from_nchw(d["src"].to(dev), e.buf("xw.src", 2, 5, 9, 24))
        fv = e.from_nchw(d["flow"].to(dev), e.buf("xw.flow", 2, 5, 9, 2))
        ov = e.warp(sv, fv, e.buf("xw.out", 2, 5, 9, 24))
        dout_u, _ = BR.resample_exact(2, 3, 5, 7, 2, seed=1)
        dout_d, _ = BR.resample_exact(2, 3, 6, 10, 0.5, seed=2)
        xu = e.from_nchw(torch.zeros(2, 3, 5, 7).to(dev), e.buf("xu.x", 2, 5, 7, 3))
        ou = e.up2(xu, e.buf("xu.o", 2, 10, 14, 3), scale=2.0)
        xd = e.from_nchw(torch.zeros(2, 3, 6, 10).to(dev), e.buf("xd.x", 2, 6, 10, 3))
        od = e.down2(xd, e.buf("xd.o", 2, 3, 5, 3), scale=0.5)
    finally:
        e.tape = None
    e.from_nchw(d["dout"].to(dev), tape.grad(ov))
    e.from_nchw(dout_u.to(dev), tape.grad(ou))
    e.from_nchw(dout_d.to(dev), tape.grad(od))
    tape.backward()
    BR.assert_bits(e.to_nchw(tape.grad(sv)), s64.float(), "tape warp dsrc", "n,c,y,x")
    BR.assert_bits(e.to_nchw(tape.grad(fv)), f64.float(), "tape warp dflow", "n,xy,y,x")
    BR.assert_bits(e.to_nchw(tape.grad(xu)), BR.up2_backward(dout_u, 2.0).float(), "tape up2", "n,c,y,x")
    BR.assert_bits(e.to_nchw(tape.grad(xd)), BR.down2_backward(dout_d, 0.5).float(), "tape down2", "n,c,y,x")
    assert bool((e._fix_scratch == 0).all())
    # odd size: the Tape's down2 backward raises and the source gradient stays untouched
    t2 = Tape(e)
    e.tape = t2
    try:
        xo, oo = e.buf("xo.x", 1, 5, 7, 3), e.buf("xo.o", 1, 2, 3, 3)
    finally:
        e.tape = None
    e.from_nchw(torch.ones(1, 3, 2, 3).to(dev), t2.grad(oo))
    with pytest.raises(lib.KernelError):
        t2._b_down2(xo, oo, 0.5)
    torch.cuda.synchronize()
    assert bool((e.to_nchw(t2.grad(xo)) == 0).all())
