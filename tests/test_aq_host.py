"""Backward-adaptive quantisation, the parts that need no GPU: header against bindings, the activity's arithmetic
(tests/aq_ref.py restates include/dcvc_hip_aq.h), the two host-built tables, aq.json and its refusals by name, and the entry
points' refusals (a refused call launches nothing)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from tests import aq_ref as R
from vcm_ts_amd import aq as A
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X


def test_header_and_bindings_agree():
    text = open(os.path.join(os.path.dirname(lib.HERE), "include", "dcvc_hip_aq.h")).read()
    assert f"#define DCVC_AQ_MAX_L {A.MAX_L}" in text and f"#define DCVC_AQ_FTAB {A.FTAB}" in text
    assert f"#define DCVC_AQ_MAX_STRENGTH {A.MAX_STRENGTH}" in text and A.KTAB == 2 * A.MAX_L + 1 == 15871
    assert (A.CELL, A.MIN_Q, A.MAX_Q, A.MAX_SIDE) == (X.CELL, X.MIN_Q, X.MAX_Q, X.MAX_SIDE)
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "aq.hip" in mk and "dcvc_hip_aq.h" in mk
    assert "#pragma clang fp contract(off)" in open(os.path.join(lib.CSRC, "aq.hip")).read()


def test_activity_is_monotone_and_close_to_the_logarithm():
    """0 <= 256 log2(V + 1) - L < 256 (1 + log2(log2 e) - log2 e) + 1: with x = v / 2^e - 1 in [0, 1), L = 256 e +
    floor(256 x) for e >= 8 (exactly 256 (e + x) below), log2(1 + x) - x peaks at x = 1 / ln 2 - 1 with 0.0860713.., and the
    floor loses less than 1.  So floor(256 log2(V + 1)) - L is an integer within 0 .. 23."""
    peak = 1.0 + math.log2(math.log2(math.e)) - math.log2(math.e)
    assert abs(peak - 0.0860713) < 1e-6
    bound = 256.0 * peak + 1.0  # 23.03..
    g = np.random.default_rng(3)
    V = np.unique(np.concatenate([np.arange(0, 70000), 2 ** np.arange(0, 30) - 1, 2 ** np.arange(0, 30), 2 ** np.arange(1, 30) - 2,
                                  g.integers(0, 1065369601, 200000), [1065369600]]))
    L = R.log_activity(V)
    assert L[0] == 0 and (np.diff(L) >= 0).all() and L.max() <= A.MAX_L
    exact = 256.0 * np.log2((V + 1).astype(np.float64))
    diff = exact - L
    assert diff.min() > -1e-9 and diff.max() < bound
    assert (np.floor(exact).astype(np.int64) - L).max() <= 23
    assert diff.max() > 256.0 * peak - 0.5  # (the bound is sharp: the peak is reached)
    # powers of two are exact, and below 2^8 nothing is truncated
    for e in range(30):
        assert R.log_activity(np.array([2 ** e - 1]))[0] == 256 * e
    assert R.log_activity(np.array([2]))[0] == 256 + 128  # v = 3 = 2 * 1.5


def test_extremes_of_a_cell():
    flat = np.full((64, 64), 77)
    assert (R.variance256(flat) == 0).all() and (R.log_activity(R.variance256(flat)) == 0).all()
    half = np.zeros((64, 64), np.int64)
    half[:, ::2] = 255
    V = R.variance256(half)
    assert (V == 1065369600).all() and 1065369600 < 2 ** 30 and 2 ** 31 < 256 * 256 * 255 ** 2 < 2 ** 32  # (256 S2 of an all-255 cell)
    assert (R.log_activity(V) == 256 * 29 + ((1065369601 >> 21) & 255)).all()
    # luma: the weights sum to 256, so a grey pixel keeps its code, and the code of k / 255 is k
    k = np.arange(256)
    t = (k.astype(np.float32) / np.float32(255.0))
    assert np.array_equal(R.code(t), k) and np.array_equal(R.luma(np.stack([t, t, t])[:, None, :]).reshape(-1), k)
    assert R.code(np.float32("nan")) == 0 and R.code(np.float32(-3)) == 0 and R.code(np.float32("inf")) == 255


@pytest.mark.parametrize("strength", [1, 50, 100, 400])
def test_ktab(strength):
    k = A.AQ(strength).ktab().astype(np.int64)
    assert k.dtype == np.int64 and k.shape == (A.KTAB,) and np.array_equal(A.AQ(strength).ktab(), R.ktab(strength))
    assert A.AQ(strength).ktab().dtype == np.uint16
    assert k[A.MAX_L] == 100 and (np.diff(k) >= 0).all() and k.min() >= 10 and k.max() <= 1000
    # -d: k(d) k(-d) = 100^2 before rounding.  For d >= 0 (k >= 100) the larger side's rounding moves 10000 / k(d) by at
    # most 10000 * 0.5 / 100^2 = 0.5, the smaller side's own rounding by 0.5: within 1 wherever neither clamp acts
    d = np.arange(0, A.MAX_L + 1)
    up, down = k[A.MAX_L + d], k[A.MAX_L - d]
    free = (up < 1000) & (down > 10)
    assert free[: 2000 // strength + 2].all() and (np.abs(down - 10000.0 / up)[free] <= 1.0).all()
    # A: the exponent sees only the product A d, so strength 2 A at d is strength A at 2 d, exactly
    if 2 * strength <= A.MAX_STRENGTH:
        k2 = A.AQ(2 * strength).ktab().astype(np.int64)
        half = np.arange(-(A.MAX_L // 2), A.MAX_L // 2 + 1)
        assert np.array_equal(k2[half + A.MAX_L], k[2 * half + A.MAX_L])
    # clamps honoured, and the unclamped interior untouched
    c = A.AQ(strength, 50, 200).ktab().astype(np.int64)
    assert c.min() >= 50 and c.max() <= 200 and np.array_equal(c, np.clip(k, 50, 200))
    assert (A.AQ(strength, 100, 100).ktab() == 100).all() and A.AQ(strength, 100, 100).is_neutral()
    assert not A.AQ(strength).is_neutral()


def test_ktab_reaches_both_clamps_at_full_strength():
    k = A.AQ(400).ktab()
    assert k[0] == 10 and k[-1] == 1000
    k = A.AQ(1).ktab()  # 0.01 QP per doubling: 2^(+-7935 / 153600) = 1.0365 and 0.9648
    assert k[0] == 96 and k[-1] == 104


def test_ftab_holds_the_factors_of_roiq():
    f = A.AQ.ftab()
    assert f.dtype == np.float32 and f.shape == (A.FTAB,) and np.array_equal(f.view(np.uint32), R.ftab().view(np.uint32))
    for k in (10, 33, 60, 99, 100, 101, 140, 999, 1000):
        assert f[k - 10].tobytes() == X.RoiQ(k).factors()[0].tobytes()
    every = np.concatenate([X.RoiQ(100, tuple(range(k, min(k + 4, 1001)))).factors()[1:] for k in range(10, 1001, 4)])
    assert np.array_equal(f.view(np.uint32), every.view(np.uint32)) and f[90] == np.float32(1.0)


def test_settings_are_refused_by_name():
    assert A.AQ(np.int32(100), 50, 200) == A.AQ(100, 50, 200) and A.AQ.snapped(1.0, 0.5, 2.0) == A.AQ(100, 50, 200)
    assert A.AQ.snapped(0.004 + 0.01) == A.AQ(1) and A.AQ.hundredths(0.6) == 60
    for bad in (0, 401, -1, 1.0, True, "100", None):
        with pytest.raises(ValueError, match="strength"):
            A.AQ(bad)
    for lo, hi, name in ((9, 1000, "lo"), (101, 1000, "lo"), (10, 99, "hi"), (10, 1001, "hi"), (10.0, 1000, "lo")):
        with pytest.raises(ValueError, match=name):
            A.AQ(100, lo, hi)
    with pytest.raises(ValueError, match="finite"):
        A.AQ.snapped(float("nan"))
    with pytest.raises(ValueError, match="multiples of 64"):
        A.grid_of(72, 64)
    with pytest.raises(ValueError, match="multiples of 64"):
        A.grid_of(64, 0)
    assert A.grid_of(1088, 1920) == (68, 120)
    with pytest.raises(ValueError, match="GPU"):
        A.AqMaps(A.AQ(100), "cpu")
    with pytest.raises(ValueError, match="aq.AQ"):
        A.AqMaps(100, "cuda:0")


def test_aq_json_round_trips_and_refuses_by_name(tmp_path):
    aq = A.AQ(150, 40, 300)
    info = aq.to_json()
    assert set(info) == {"version", "cell", "strength", "clamp", "tables"} and info["strength"] == 150 and info["clamp"] == [40, 300]
    assert info["tables"] == {"ktab": "%08x" % __import__("zlib").crc32(R.ktab(150, 40, 300).tobytes()),
                              "ftab": "%08x" % __import__("zlib").crc32(R.ftab().tobytes())}
    assert A.AQ.from_json(json.loads(json.dumps(info))) == aq
    assert A.read_aq(str(tmp_path)) is None and A.write_aq(str(tmp_path), None) is None
    A.write_aq(str(tmp_path), aq)
    assert A.read_aq(str(tmp_path)) == aq and json.loads((tmp_path / A.AQ_JSON).read_text()) == info
    A.write_aq(str(tmp_path), None)  # (a stale file is removed)
    assert not (tmp_path / A.AQ_JSON).exists()

    def refused(match, **change):
        bad = dict(info, **change)
        (tmp_path / A.AQ_JSON).write_text(json.dumps(bad))
        with pytest.raises(ValueError, match=match):
            A.read_aq(str(tmp_path))

    flipped = ("0" if info["tables"]["ktab"][0] != "0" else "1") + info["tables"]["ktab"][1:]
    refused(r"aq\.json.*ktab table built on this host", tables=dict(info["tables"], ktab=flipped))
    refused(r"aq\.json.*ftab table built on this host", tables=dict(info["tables"], ftab="00000000"))
    refused(r"aq\.json.*unknown version 2", version=2)
    refused(r"aq\.json.*strength must be an integer within 1\.\.400", strength=401)
    refused(r"aq\.json.*strength", strength=1.5)
    refused(r"aq\.json.*lo must be", clamp=[5, 1000])
    refused(r"aq\.json.*hi must be", clamp=[10, 99])
    refused(r"aq\.json.*clamp must be two integers", clamp=[10])
    refused(r"aq\.json.*cell must be 16", cell=8)
    refused(r"aq\.json.*tables must hold", tables={"ktab": info["tables"]["ktab"]})
    refused(r"aq\.json.*expected the keys", extra=1)
    (tmp_path / A.AQ_JSON).write_text("{not json")
    with pytest.raises(ValueError, match="not JSON"):
        A.read_aq(str(tmp_path))
    (tmp_path / A.AQ_JSON).write_text("[1]")
    with pytest.raises(ValueError, match="JSON object"):
        A.read_aq(str(tmp_path))


def test_command_line_refusals(capsys):
    from vcm_ts_amd import run_codec as RC

    for argv, match in ((["--aq-clamp", "50", "200"], "--aq-clamp belongs to --aq-strength"),
                        (["--aq-strength", "0"], "strength must be an integer within 1..400"),
                        (["--aq-strength", "100", "--aq-clamp", "120", "200"], "lo must be"),
                        (["--aq-strength", "100", "--background-q", "0.5"], "belong to --roi-root")):
        with pytest.raises(SystemExit):
            RC.main(["encode", "--frames", "nowhere", "--bins", "nowhere"] + argv)
        assert match in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="aq.AQ"):
        RC._aq_args(100)


# ---------------------------------------------------------------------------------------------------- entry points
_KEEP = np.zeros(64, dtype=np.uint64)  # (an aligned address that is never dereferenced: a refused call launches nothing)
PTR = _KEEP.ctypes.data


def _activity(pic=PTR, rs=128, ps=64 * 128, Hp=64, Wp=128, L=PTR, total=PTR):
    return lib.hip().dcvc_aq_activity(pic, rs, ps, Hp, Wp, L, total, None)


def _map(L=PTR, total=PTR, hc=4, wc=8, ktab=PTR, ftab=PTR, roi=None, out=PTR):
    return lib.hip().dcvc_aq_map(L, total, hc, wc, ktab, ftab, roi, out, None)


def test_entry_point_refusals():
    E_ARG = -1
    base = PTR - PTR % 16 + 16  # 16-byte aligned inside _KEEP
    for name in ("pic", "L", "total"):
        assert _activity(**{name: None}) == E_ARG, name
    for name in ("Hp", "Wp"):
        for bad in (0, -64, 16, 32, 63, 65, 96, 32768 + 64, 2 ** 31 - 64):
            kw = {name: bad}
            if name == "Wp":
                kw["rs"] = max(bad, 128)
            assert _activity(ps=2 ** 40, **kw) == E_ARG, (name, bad)
    for bad in (dict(rs=127), dict(rs=0), dict(rs=-128), dict(ps=63 * 128 + 127), dict(ps=0), dict(ps=-1)):
        assert _activity(**bad) == E_ARG, bad
    for bad in (dict(total=base + 4), dict(total=base + 1), dict(L=base + 2), dict(pic=base + 1)):
        assert _activity(**bad) == E_ARG, bad
    for name in ("L", "total", "ktab", "ftab", "out"):
        assert _map(**{name: None}) == E_ARG, name
    for name in ("hc", "wc"):
        for bad in (0, -4, 1, 2, 6, 2048 + 4, 2 ** 31 - 4):
            assert _map(**{name: bad}) == E_ARG, (name, bad)
    for bad in (dict(total=base + 4), dict(L=base + 2), dict(ftab=base + 2), dict(roi=base + 1), dict(out=base + 3),
                dict(ktab=base + 1)):
        assert _map(**bad) == E_ARG, bad
