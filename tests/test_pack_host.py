"""The four host weight packers of include/dcvc_hip.h against tests/pack_ref.py, byte for byte and over the whole
buffer they are given (padding included).  They are pure host functions: no GPU is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import pack_ref as R
from vcm_ts_amd import lib

FILL = 0xA5  # the buffers handed to the library start out as garbage: padding must be WRITTEN as zero


def _weights(Cout, Cin, ks, bias, seed=0):
    rng = np.random.default_rng([seed, Cout, Cin, ks])
    w = rng.normal(0.0, 0.1, (Cout, Cin, ks, ks)).astype(np.float32)
    w.reshape(-1)[:4] = [0.0, -0.0, 1e-6, -3e-6]  # zeros and values whose lo part is an fp16 subnormal
    return w, (rng.normal(0.0, 0.1, Cout).astype(np.float32) if bias else None)


def _segs(seg_C):
    return (C.c_int32 * len(seg_C))(*seg_C)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _same_bytes(got, want):
    assert got.nbytes == want.nbytes
    g, w = got.view(np.uint8), want.view(np.uint8)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"


def _call_plain(w, b, seg_C, ps, prec):
    L = lib.hip()
    Cout, ks = w.shape[0], w.shape[2]
    cp = C.c_int32(0)
    total = L.dcvc_conv_pack_size(Cout, ks, len(seg_C), _segs(seg_C), C.byref(cp))
    assert (total, cp.value) == R.plain_size(Cout, ks, seg_C)
    wp, bp = np.full(total * 4, FILL, np.uint8), np.full(cp.value * 4, FILL, np.uint8)
    rc = L.dcvc_conv_pack_weights(_ptr(w), _ptr(b), Cout, ks, len(seg_C), _segs(seg_C), ps, prec, _ptr(wp), _ptr(bp))
    return wp, bp, rc


def _call_paired(w, b):
    L = lib.hip()
    Cout, Cin = w.shape[0], w.shape[1]
    cp = C.c_int32(0)
    total = L.dcvc_conv_pack_size_paired(Cout, Cin, C.byref(cp))
    assert (total, cp.value) == R.paired_size(Cout)
    wp, bp = np.full(total * 4, FILL, np.uint8), np.full(cp.value * 4, FILL, np.uint8)
    rc = L.dcvc_conv_pack_weights_paired(_ptr(w), _ptr(b), Cout, Cin, _ptr(wp), _ptr(bp))
    return wp, bp, rc


def _call_small(w, b, seg_C):
    L = lib.hip()
    Cout, ks = w.shape[0], w.shape[2]
    total = L.dcvc_conv_small_pack_bytes(Cout, ks, len(seg_C), _segs(seg_C))
    assert total == R.small_size(ks, seg_C)
    wp, bp = np.full(total, FILL, np.uint8), np.full(16 * 4, FILL, np.uint8)
    rc = L.dcvc_conv_small_pack_weights(_ptr(w), _ptr(b), Cout, ks, len(seg_C), _segs(seg_C), _ptr(wp), _ptr(bp))
    return wp, bp, rc


def _call_k32(w, b, seg_C, ps):
    L = lib.hip()
    Cout, ks = w.shape[0], w.shape[2]
    cp = C.c_int32(0)
    total = L.dcvc_conv_k32_pack_bytes(Cout, ks, len(seg_C), _segs(seg_C), C.byref(cp))
    assert (total, cp.value) == R.k32_size(Cout, ks, seg_C)
    wp, bp = np.full(total, FILL, np.uint8), np.full(cp.value * 4, FILL, np.uint8)
    rc = L.dcvc_conv_k32_pack_weights(_ptr(w), _ptr(b), Cout, ks, len(seg_C), _segs(seg_C), ps, _ptr(wp), _ptr(bp))
    return wp, bp, rc


def _check(got, want):
    (wp, bp, rc), (wref, bref, rcref) = got, want
    assert rc == rcref
    _same_bytes(wp, wref)
    _same_bytes(bp, bref)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("prec", [R.FP32, R.FP16X3], ids=["fp32", "fp16x3"])
@pytest.mark.parametrize("seg_C", [(3,), (16,), (17, 5, 32)], ids=str)
@pytest.mark.parametrize("Cout", [5, 33])
@pytest.mark.parametrize("ks", [1, 3, 7])
def test_plain_layout(ks, Cout, seg_C, prec, bias):
    w, b = _weights(Cout, sum(seg_C), ks, bias)
    _check(_call_plain(w, b, seg_C, 0, prec), R.plain(w, b, seg_C, 0, prec))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("prec", [R.FP32, R.FP16X3], ids=["fp32", "fp16x3"])
@pytest.mark.parametrize("seg_C", [(16,), (17, 5, 32)], ids=str)
def test_plain_layout_pixel_shuffle(seg_C, prec, bias):
    w, b = _weights(8, sum(seg_C), 3, bias)
    _check(_call_plain(w, b, seg_C, 1, prec), R.plain(w, b, seg_C, 1, prec))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("Cout", [17, 64])
@pytest.mark.parametrize("Cin", [3, 8])
def test_tap_paired_layout(Cin, Cout, bias):
    w, b = _weights(Cout, Cin, 7, bias)
    got = _call_paired(w, b)
    _check(got, R.paired(w, b))
    rows = got[0].view(np.float16).reshape(7, 4, 4, -1, 8)  # [ky][pair][hi h0, hi h1, lo h0, lo h1][n][8]
    assert not rows[:, 3, 1].view(np.uint16).any() and not rows[:, 3, 3].view(np.uint16).any()  # the partner of kx = 6
    assert rows[:, 3, 0, :Cout, :Cin].any()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("seg_C", [(3,), (20, 16)], ids=str)
@pytest.mark.parametrize("ks", [3, 7])
@pytest.mark.parametrize("Cout", [2, 16])
def test_small_layout(Cout, ks, seg_C, bias):
    w, b = _weights(Cout, sum(seg_C), ks, bias)
    _check(_call_small(w, b, seg_C), R.small(w, b, seg_C))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("Cout,ps", [(64, 0), (12, 1)])
@pytest.mark.parametrize("seg_C", [(32,), (64, 32)], ids=str)
@pytest.mark.parametrize("ks", [1, 3])
def test_k32_layout(ks, seg_C, Cout, ps, bias):
    w, b = _weights(Cout, sum(seg_C), ks, bias)
    _check(_call_k32(w, b, seg_C, ps), R.k32(w, b, seg_C, ps))


# ---- range and non-finite weights: one each, in input channels 0..4 of output channel 0, tap 0.  In all four layouts
# the hi parts of those channels are the first five fp16 of the buffer; LO is where their lo parts start.
SPECIAL = np.array([1024.0, -1024.0, np.inf, np.nan, -0.0], np.float32)
H_MAX, H_NEG0 = 0x7BFF, 0x8000  # fp16 bit patterns of 65504 and -0.0


def _special(Cout, Cin, ks):
    w = np.zeros((Cout, Cin, ks, ks), np.float32)
    w[0, :5, 0, 0] = SPECIAL
    return w


def _hi_lo(wp, lo_at):
    h = wp.view(np.uint16)
    return h[:5], h[lo_at:lo_at + 5]


def _is_nan16(bits):
    return (bits & 0x7C00) == 0x7C00 and (bits & 0x03FF) != 0


def test_plain_packer_clamps_silently_and_keeps_nan():
    w = _special(5, 16, 3)
    got = _call_plain(w, None, (16,), 0, R.FP16X3)
    _check(got, R.plain(w, None, (16,), 0, R.FP16X3))
    assert got[2] == R.OK
    hi, lo = _hi_lo(got[0], 2 * 32 * 8)
    assert list(hi[:3]) == [H_MAX, H_MAX | 0x8000, H_MAX] and _is_nan16(hi[3]) and hi[4] == H_NEG0
    assert list(lo[:3]) == [0, 0, 0] and _is_nan16(lo[3]) and lo[4] == 0
    # the fp32 layout carries every value as it is
    got = _call_plain(w, None, (16,), 0, R.FP32)
    _check(got, R.plain(w, None, (16,), 0, R.FP32))
    first = got[0].view(np.float32)[[0, 1, 2, 3, 32 * 4]]  # channels 0..3 are j of kq 0, channel 4 is kq 1
    assert first.tobytes() == SPECIAL.tobytes() and got[2] == R.OK


@pytest.mark.parametrize("packer", ["paired", "small", "k32"])
def test_reporting_packers_return_e_range_and_turn_nan_into_minus_max(packer):
    if packer == "paired":
        w = _special(17, 8, 7)
        got, want, lo_at = _call_paired(w, None), R.paired(w, None), 2 * 32 * 8
    elif packer == "small":
        w = _special(2, 16, 3)
        got, want, lo_at = _call_small(w, None, (16,)), R.small(w, None, (16,)), 2 * 16 * 8
    else:
        w = _special(64, 32, 1)
        got, want, lo_at = _call_k32(w, None, (32,), 0), R.k32(w, None, (32,), 0), 4 * 64 * 8
    _check(got, want)
    assert got[2] == R.E_RANGE == -3
    hi, lo = _hi_lo(got[0], lo_at)
    assert list(hi) == [H_MAX, H_MAX | 0x8000, H_MAX, H_MAX | 0x8000, H_NEG0]
    assert list(lo) == [0, 0, 0, 0, 0]


def test_size_functions_refuse_what_their_kernels_do_not_take():
    L = lib.hip()
    assert L.dcvc_conv_small_pack_bytes(17, 3, 1, _segs((16,))) == R.E_ARG  # more than 16 output channels
    assert L.dcvc_conv_k32_pack_bytes(64, 3, 1, _segs((48,)), None) == R.E_ARG  # a segment that is no multiple of 32
    assert L.dcvc_conv_pack_size_paired(32, 9, None) == R.E_ARG  # more than 8 input channels
    assert L.dcvc_conv_pack_size(32, 5, 1, _segs((16,)), None) == R.E_ARG  # kernel size 5
    assert L.dcvc_conv_small_pack_bytes(16, 5, 1, _segs((16,))) == R.E_ARG
    assert L.dcvc_conv_k32_pack_bytes(64, 5, 1, _segs((32,)), None) == R.E_ARG
    # ... and the packers pass the refusal on before they touch a buffer
    w = np.zeros((17, 16, 3, 3), np.float32)
    wp, bp = np.full(64, FILL, np.uint8), np.full(64, FILL, np.uint8)
    assert L.dcvc_conv_small_pack_weights(_ptr(w), None, 17, 3, 1, _segs((16,)), _ptr(wp), _ptr(bp)) == R.E_ARG
    assert L.dcvc_conv_pack_weights(_ptr(w), None, 17, 5, 1, _segs((16,)), 0, R.FP16X3, _ptr(wp), _ptr(bp)) == R.E_ARG
    assert (wp == FILL).all() and (bp == FILL).all()
