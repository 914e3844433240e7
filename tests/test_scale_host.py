"""The base layer's resampler, the parts that need no GPU: the tap tables of vcm_ts_amd/scale.py against the rule of
include/dcvc_hip_scale.h (tests/scale_ref.py restates it), base_size, every refusal by name, scale.json, the restatement
against Pillow's LANCZOS and against a float64 fold, and the entry point's refusals (a refused call launches nothing).
"""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import scale_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import scale as SC

AXES = [(40, 20), (52, 26), (96, 64), (160, 107), (75, 56), (107, 80), (100, 25), (132, 33), (20, 40), (26, 52), (64, 96),
        (56, 75), (25, 100), (130, 65), (260, 130), (1080, 540), (1920, 960), (128, 64)]


def test_header_and_bindings_agree():
    text = open(os.path.join(os.path.dirname(lib.HERE), "include", "dcvc_hip_scale.h")).read()
    assert f"#define DCVC_SCALE_MAX_TAPS {SC.MAX_TAPS}" in text and f"#define DCVC_SCALE_UNIT {SC.UNIT}" in text
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "scale.hip" in mk and "dcvc_hip_scale.h" in mk
    assert "#pragma clang fp contract(off)" in open(os.path.join(lib.CSRC, "scale.hip")).read()


@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_table_invariants(axis):
    n_in, n_out = axis
    start, k = SC.taps(n_in, n_out)
    rs, rk = R.taps(n_in, n_out)
    assert start.dtype == np.int32 and k.dtype == np.int16 and start.shape == (n_out,) and k.shape[0] == n_out
    assert np.array_equal(start, rs) and np.array_equal(k, rk)
    T = k.shape[1]
    assert 1 <= T <= 32 and T <= n_in
    assert (k.astype(np.int64).sum(axis=1) == 16384).all()
    assert (start >= 0).all() and (start + T <= n_in).all() and (np.diff(start) >= 0).all()
    # what the kernel's tile stages is enough: 64 outputs need at most 64 * 4 + 32 + 8 inputs from the aligned start,
    # 16 outputs at most 16 * 4 + 32
    for tile, cap, align in ((64, 296, 4), (16, 96, 1)):
        for i0 in range(0, n_out, tile):
            last = min(i0 + tile, n_out) - 1
            assert start[last] + T - (start[i0] // align * align) <= cap


def test_tap_counts_and_symmetry():
    assert [SC.taps(*a)[1].shape[1] for a in ((128, 64), (128, 32), (96, 64), (64, 128))] == [12, 24, 9, 6]
    start, k = SC.taps(128, 64)
    interior = [i for i in range(64) if 2 * i + 1 - 6 >= 0 and 2 * i + 1 + 6 <= 128]
    assert len(interior) > 50
    for i in interior:
        assert start[i] == 2 * i - 5 and np.array_equal(k[i], k[i][::-1]) and np.array_equal(k[i], k[interior[0]])
    # the rows clipped by the ends mirror each other: the same windows, and the same weights but for the unit the row's
    # correction moves (it goes to the FIRST largest weight, which the mirror image makes the second)
    for i in range(64):
        assert start[i] == 128 - 12 - start[63 - i]
        assert np.abs(k[i].astype(int) - k[63 - i][::-1].astype(int)).max() <= 2


def test_base_size():
    assert SC.base_size(40, 52, "1/2") == (20, 26)
    assert SC.base_size(96, 160, (2, 3)) == (64, 107)
    assert SC.base_size(75, 107, Fraction(3, 4)) == (56, 80)
    assert SC.base_size(100, 132, "1/4") == (25, 33)
    assert SC.base_size(2160, 3840, "1/2") == (1080, 1920) and SC.base_size(1080, 1920, "2/4") == (540, 960)
    assert SC.base_size(128, 128, "1/2") == SC.base_size(96, 96, "2/3") == (64, 64)
    assert SC.base_size(5, 7, "1/2") == (3, 4)  # halves round up
    for h, w, n, d in ((75, 107, 3, 4), (1080, 1920, 2, 3), (33, 47, 1, 3)):
        assert SC.base_size(h, w, (n, d)) == R.base_size(h, w, n, d)


def test_refusals_by_name():
    with pytest.raises(ValueError, match="n_in == n_out"):
        SC.taps(64, 64)
    for n_in, n_out in ((65, 16), (16, 65), (1000, 100)):
        with pytest.raises(ValueError, match=r"outside \[1/4, 4\]"):
            SC.taps(n_in, n_out)
    # (T > 32 and n_in < T cannot come out of the rule -- a window is clipped to the axis, and 1/4 gives 24 taps -- so
    # taps() keeps them as guards and the entry point's refusals below are what tests them)
    assert SC.taps(4, 2)[1].shape == (2, 4) and SC.taps(5, 10)[1].shape == (10, 5)
    for n_in, n_out in ((40000, 20000), (0, 5), (20, 0), (32769, 32768)):
        with pytest.raises(ValueError, match="within 1..32768"):
            SC.taps(n_in, n_out)
    assert SC.taps(32768, 8192)[1].shape[1] == 24  # the most taps the ratio range gives: DCVC_SCALE_MAX_TAPS is never met
    for bad in ("1/5", "1/1", "3/2", (0, 1), Fraction(1, 8), Fraction(1)):
        with pytest.raises(ValueError, match="1/4 <= n/d < 1"):
            SC.as_ratio(bad)
    for bad in ("half", "1:2", 0.5, (1, 2, 3), "1/0", None, (1.0, 2.0)):
        with pytest.raises(ValueError, match="expected a ratio n/d"):
            SC.as_ratio(bad)
    with pytest.raises(ValueError, match="within 1..32768"):
        SC.base_size(40000, 64, "1/2")
    with pytest.raises(ValueError, match="no CPU fallback"):
        SC.Scale((64, 64), "1/2", "cpu")


class _HostScale:
    """what write_scale needs of a Scale, without a device"""

    def __init__(self, full, ratio):
        self.full, self.ratio = full, SC.as_ratio(ratio)
        self.base = SC.base_size(*full, self.ratio)
        self.tables = SC._tables(self.full, self.base)

    to_json = SC.Scale.to_json


def test_scale_json_round_trips_and_a_flipped_digest_is_refused(tmp_path):
    assert SC.read_scale(str(tmp_path)) is None
    info = SC.write_scale(str(tmp_path), _HostScale((96, 160), "2/3"))
    assert sorted(os.listdir(tmp_path)) == ["scale.json"]
    assert info == json.loads((tmp_path / "scale.json").read_text())
    assert (info["version"], info["filter"], info["unit"], info["full"], info["base"], info["ratio"]) == \
        (1, "lanczos3", 16384, [96, 160], [64, 107], [2, 3])
    assert sorted(info["tables"]) == ["down_x", "down_y", "up_x", "up_y"] and len(set(info["tables"].values())) == 4
    assert SC.read_scale(str(tmp_path)) == {"full": (96, 160), "base": (64, 107), "ratio": Fraction(2, 3)}

    def refused(match, **edit):
        (tmp_path / "scale.json").write_text(json.dumps(dict(info, **edit)))
        with pytest.raises(ValueError, match=match):
            SC.read_scale(str(tmp_path))

    d = info["tables"]["up_x"]
    refused("up_x table built on this host", tables=dict(info["tables"], up_x=d[:3] + ("0" if d[3] != "0" else "1") + d[4:]))
    refused("unknown version", version=2)
    refused("unknown filter", filter="bicubic")
    refused("unknown filter", unit=4096)
    refused("gives a base of 80x48", ratio=[1, 2])
    refused("base must be two positive integers", base=[64])
    refused("1/4 <= n/d < 1", ratio=[3, 2])
    refused("tables must hold", tables={"down_x": d})
    (tmp_path / "scale.json").write_text("{")
    with pytest.raises(ValueError, match="not JSON"):
        SC.read_scale(str(tmp_path))
    # without the option a stale file is removed
    assert SC.write_scale(str(tmp_path), None) is None and os.listdir(tmp_path) == []
    SC.write_scale(str(tmp_path), None)


def _picture(seed, H, W):
    return np.random.default_rng(seed).random((H, W), dtype=np.float32)


@pytest.mark.parametrize("case", [((40, 52), (20, 26)), ((20, 26), (40, 52)), ((75, 107), (56, 80)), ((96, 160), (64, 107))],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_the_restatement_is_pillows_lanczos_resize(case):
    """Image.resize(..., LANCZOS) in mode F filters horizontally, then vertically, with float weights of the same rule;
    the restatement differs by the integer step of the weights alone: each of the T_x + T_y weights a sample passes
    through moves by at most 2^-15 (rounding) plus the row's correction on one weight (at most T 2^-15, on one tap), so
    |difference| <= (T_x + T_y) 2^-14 max|a|, plus 1e-5 for the float32 sums of both."""
    from PIL import Image

    (H, W), (Ho, Wo) = case
    a = _picture(H * W, H, W)
    want = np.asarray(Image.fromarray(a, "F").resize((Wo, Ho), Image.LANCZOS))
    got = R.resize(a, (Ho, Wo), clamp=False)
    T = SC.taps(W, Wo)[1].shape[1] + SC.taps(H, Ho)[1].shape[1]
    bound = T * 2.0 ** -14 * float(np.abs(a).max()) + 1e-5
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{case}: max |restatement - Pillow| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("case", [((40, 52), (20, 26)), ((100, 132), (25, 33)), ((25, 33), (100, 132)), ((75, 107), (56, 80))],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_the_float32_fold_against_the_float64_fold_of_the_same_tables(case):
    """A sum of T terms folded in float32 is within (T + 1) u sum |w x| of the exact one (u = 2^-24; one rounding per
    product and per sum); two passes: the vertical pass sees the horizontal error amplified by sum |w_y| and adds its own.
    With A_x = max sum_t |w_x|, A_y likewise and M = max|a|:  (T_x + 1 + T_y + 1) u A_x A_y M, and 1.01 for second order."""
    (H, W), (Ho, Wo) = case
    a = (_picture(7 * H + W, H, W) * 3.0 - 1.0).astype(np.float32)  # values outside [0, 1] too
    kx, ky = SC.taps(W, Wo)[1], SC.taps(H, Ho)[1]
    Ax, Ay = (np.abs(k.astype(np.float64)).sum(axis=1).max() / 16384 for k in (kx, ky))
    bound = 1.01 * (kx.shape[1] + ky.shape[1] + 2) * 2.0 ** -24 * Ax * Ay * float(np.abs(a).max())
    err = float(np.abs(R.resize(a, (Ho, Wo), clamp=False).astype(np.float64) - R.fold64(a, (Ho, Wo))).max())
    print(f"{case}: max |float32 - float64| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    # and the clamp: within [0, 1], a NaN gives 0
    a[3, 5] = np.nan
    out = R.resize(a, (Ho, Wo))
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0 and (out == 0).any() and (out == 1).any()


# ------------------------------------------------------------------------------------------------ the entry point
def _call(**edit):
    """dcvc_scale_planes on 40x52 -> 20x26 with aligned dummy pointers for the pictures and the device tables (a refused
    call returns before anything is launched or dereferenced) and real HOST tables; `edit` overrides arguments."""
    xs, xk = SC.taps(52, 26)
    ys, yk = SC.taps(40, 20)
    v = dict(src=0x10000, src_rs=52, src_ps=40 * 52, dst=0x20000, dst_rs=26, dst_ps=20 * 26, planes=3, H_in=40, W_in=52,
             H_out=20, W_out=26, xs=xs, xk=xk, xs_dev=0x30000, xk_dev=0x40000, xT=xk.shape[1], ys=ys, yk=yk, ys_dev=0x50000,
             yk_dev=0x60000, yT=yk.shape[1])
    v.update(edit)
    keep = [np.ascontiguousarray(v[n]) if v[n] is not None else None for n in ("xs", "xk", "ys", "yk")]
    ptr = lambda a: None if a is None else a.ctypes.data
    return lib.hip().dcvc_scale_planes(v["src"], v["src_rs"], v["src_ps"], v["dst"], v["dst_rs"], v["dst_ps"], v["planes"],
                                       v["H_in"], v["W_in"], v["H_out"], v["W_out"], ptr(keep[0]), ptr(keep[1]), v["xs_dev"],
                                       v["xk_dev"], v["xT"], ptr(keep[2]), ptr(keep[3]), v["ys_dev"], v["yk_dev"], v["yT"], None)


def test_entry_point_refusals():
    E_ARG = -1
    for name in ("src", "dst", "xs", "xk", "xs_dev", "xk_dev", "ys", "yk", "ys_dev", "yk_dev"):
        assert _call(**{name: None}) == E_ARG, name
    for name in ("H_in", "W_in", "H_out", "W_out", "planes"):
        for bad in (0, -1, 32769 if name != "planes" else 65536):
            assert _call(**{name: bad}) == E_ARG, (name, bad)
    # bad strides, either side
    for bad in (dict(src_rs=51), dict(src_rs=0), dict(src_rs=-52), dict(src_ps=39 * 52 + 51), dict(dst_rs=25),
                dict(dst_ps=19 * 26 + 25), dict(dst_ps=0), dict(src_ps=-1)):
        assert _call(**bad) == E_ARG, bad
    xs, xk = SC.taps(52, 26)
    ys, yk = SC.taps(40, 20)
    # a row that does not sum to 16384
    for table, key in ((xk, "xk"), (yk, "yk")):
        bad = table.copy()
        bad[7, 3] += 1
        assert _call(**{key: bad}) == E_ARG, key
    # a window outside the axis: before it, beyond it, and starts that go backwards
    for start, key, n_in, T in ((xs, "xs", 52, 12), (ys, "ys", 40, 12)):
        for i, v in ((0, -1), (len(start) - 1, n_in - T + 1), (5, int(start[4]) - 1)):
            bad = start.copy()
            bad[i] = v
            assert _call(**{key: bad}) == E_ARG, (key, i, v)
    # T = 33, T = 0, more taps than samples
    wide = np.zeros((26, 33), np.int16)
    wide[:, 0] = 16384
    assert _call(xk=wide, xT=33, xs=np.zeros(26, np.int32)) == E_ARG
    assert _call(xT=0) == E_ARG and _call(yT=-1) == E_ARG
    tall = np.zeros((20, 32), np.int16)
    tall[:, 0] = 16384
    assert _call(yk=tall, yT=32, ys=np.zeros(20, np.int32), H_in=31, src_ps=31 * 52) == E_ARG
    # a window that moves faster than 4 to 1: more than a tile stages
    fast = np.minimum(np.arange(26, dtype=np.int32) * 12, 300 - 12)
    assert _call(xs=fast, W_in=300, src_rs=300, src_ps=40 * 300) == E_ARG
