"""Rate control without a GPU: the restated ladder sweep (tests/ratectl_ref.py) against the bit map's
restatement, the controller against its restatement decision for decision, a plant whose rate curve the model represents
exactly, the refusals of the Python layer, of the C entry point (a refused call launches nothing) and of the command
line."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import bitmap_ref as B
from tests import ratectl_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import ratectl as RC

P = 0x10000  # an aligned dummy pointer: a refused call returns before anything is launched or dereferenced


def _edges(rng):
    e = np.sort(np.exp(rng.uniform(np.log(0.05), np.log(60.0), 255))).astype(np.float32)
    assert (np.diff(e) > 0).all()
    return np.concatenate([e, np.array([np.inf], dtype=np.float32)])


# ------------------------------------------------------------------------------------------------- the restated sweep
def test_restated_sweep_at_factor_100_is_the_bit_maps_sum():
    """With 100 hundredths the candidate is the coded symbol and the coded row: the sweep's sum is the sum of
    bitmap_ref.map_scale over the same symbols and rows, laid out as the two steps' planes."""
    rng = np.random.default_rng(7)
    N, Cc, H, W = 2, 6, 3, 5
    table = B.random_table(rng, 256)
    edges = _edges(rng)
    n = N * Cc * H * W
    res = (rng.standard_normal(n) * np.exp(rng.uniform(0, 6, n))).astype(np.float32)
    sc = np.exp(rng.uniform(np.log(0.02), np.log(90.0), n)).astype(np.float32)
    stats = {}
    est, status = R.sweep(res, sc, edges, (50, 100, 252), table, N, stats)
    assert status == 0 and est.shape == (N, 3) and stats["escapes"] > 0 and stats["below_lowest_edge"] > 0
    sym = np.rint(res).astype(np.int32).reshape(N, 2, Cc // 2, H, W)
    idx = np.array([R.row_of(v, edges) for v in sc], dtype=np.int32).reshape(N, 2, Cc // 2, H, W)
    m = B.map_scale(sym[:, 0], idx[:, 0], sym[:, 1], idx[:, 1], table, N, Cc, H, W)
    assert np.array_equal(est[:, 1], m.sum(axis=(1, 2)))
    assert est[0, 0] != est[0, 1] != est[0, 2]


def test_restated_sweep_rules():
    table = (np.array([[0, 65536, 0, 0], [0, 30000, 60000, 65536]], dtype=np.int32), np.array([2, 4], dtype=np.int32),
             np.array([0, -1], dtype=np.int32))
    edges = np.concatenate([np.array([1.0], np.float32), np.full(254, 1e30, np.float32), np.array([np.inf], np.float32)])
    # 2.5 / 1 -> 2 (half to even), 1.25 / 0.5 = 2.5 -> 2; a scale exactly on the edge belongs to the row above it
    assert R.candidate(2.5, 1.0, 100, edges) == (2, 1) and R.candidate(1.25, 0.5, 50, edges) == (2, 1)
    assert R.candidate(3.5, 0.999, 100, edges) == (4, 0)
    assert R.candidate(2.0 ** 30, 1.0, 50, edges) is None and R.candidate(-(2.0 ** 30), 1.0, 50, edges) is None
    assert R.candidate(2.0 ** 30, 1.0, 100, edges) == (2 ** 30, 1)
    est, status = R.sweep([0.0, np.inf, 0.0, 2.0 ** 30], [2.0, 2.0, np.nan, 2.0], edges, (50, 100), table, 1)
    want = B.symbol_cost(*table, 1, 0)[0]
    assert status == R.BAD_VALUE and est.tolist() == [[want, want]]  # (the last element is no int32 at 50: 0 at 100 too)
    est, status = R.sweep([0.0], [1e31], np.concatenate([np.arange(1, 256, dtype=np.float32), [np.inf]]), (100,), table, 1)
    assert status == R.BAD_INDEX and est.tolist() == [[0]]


# ------------------------------------------------------------------------------------------------------ the controller
def _random_row(rnd, K, shape):
    if shape == "monotone":
        steps = sorted((rnd.randrange(0, 40000 * 65536) for _ in range(K)), reverse=True)
        return tuple(steps)
    if shape == "flat":
        return (rnd.randrange(0, 40000 * 65536),) * K
    return tuple(rnd.randrange(0, 40000 * 65536) for _ in range(K))


def _random_ladder(rnd):
    K = rnd.randrange(2, 9)
    pts = set(rnd.sample(range(10, 1001), K - 1)) | {100}
    while len(pts) < K:
        pts.add(rnd.randrange(10, 1001))
    return tuple(sorted(pts))


@pytest.mark.parametrize("kind", ["mixed", "starved", "flooded", "narrow"])
def test_controller_equals_its_restatement(kind):
    """80 random GOPs per kind (320 logs): GOPs of 1 .. 12 pictures, random ladders, monotone, flat and non-monotone
    curves; `starved` / `flooded`: budgets below / above every ladder point; `narrow`: a q_range that clips."""
    decided = clipped = outside = 0
    for seed in range(80):
        rnd = random.Random(f"{kind}-{seed}")
        G = rnd.randrange(1, 13)
        ladder = RC.LADDER if seed % 3 == 0 else _random_ladder(rnd)
        b = {"starved": rnd.randrange(1, 50), "flooded": rnd.randrange(10 ** 6, 10 ** 8)}.get(kind, rnd.randrange(2000, 40000))
        if seed % 5 == 0:
            b = Fraction(b * 1000 + rnd.randrange(1000), 1000)
        q_range = (rnd.randrange(80, 100), rnd.randrange(100, 130)) if kind == "narrow" else (1, 65500)
        q_start = rnd.randrange(20, 400)
        rc = RC.RateControl(b, G, q_range, ladder)
        qs, As, Es = [rnd.randrange(1, 65501)], [], []
        pictures = G if seed % 4 else rnd.randrange(1, G + 1)  # (a GOP that a scene cut ended early)
        for j in range(pictures):
            if j:
                q = rc.decide(j, q_start)
                want_q, want_b = R.next_q(b, G, q_range, ladder, q_start, qs, As, Es, j)
                assert (q, rc._budget[j]) == (want_q, want_b), (kind, seed, j)
                qs.append(q)
                if j >= 3:
                    decided += 1
                    clipped += q in q_range
                    Ts = [As[j - 2] + Fraction(e - Es[j - 2][ladder.index(100)], 65536) for e in Es[j - 2]]
                    outside += not min(Ts) <= want_b <= max(Ts)
            A = rnd.randrange(100, 60000)
            row = _random_row(rnd, len(ladder), rnd.choice(("monotone", "monotone", "flat", "any"))) if j else None
            rc.record(j, qs[j], A, row)
            As.append(A)
            Es.append(row)
        log = rc.log
        assert [e[0] for e in log] == qs and [e[1] for e in log] == As and [e[3] for e in log] == Es
        assert R.replay(b, G, q_range, ladder, q_start, log) == [(e[0], e[2]) for e in log[1:]]
    print(kind, "decisions", decided, "clipped", clipped, "budget outside the curve", outside)
    assert decided > 100
    if kind in ("starved", "flooded"):
        assert outside > decided // 2
    if kind == "narrow":
        assert clipped > decided // 4


@pytest.mark.parametrize("G,decisions", [(3, 0), (4, 1)])
def test_short_gops(G, decisions):
    rc = RC.RateControl(5000, G)
    rc.record(0, 100, 30000)
    qs = []
    for j in range(1, G):
        qs.append(rc.decide(j, 120))
        rc.record(j, qs[-1], 9000, tuple(65536 * v for v in (9000, 8000, 7000, 6000, 5000, 4000, 3000, 2000)))
    assert qs[:2] == [120, 120] and sum(e[2] is not None for e in rc.log) == decisions
    if decisions:
        # picture 3 of 4 from picture 1: T_1 = 9000 + (E - 6000); picture 2 is taken to cost T_1(1) = 9000; the budget is
        # (4 * 5000 - 30000 - 9000 - 9000) / 1 < 0: below every ladder point -> the end with the nearer T, 252 hundredths
        assert rc.log[3][2] == -28000 and qs[2] == R.next_q(5000, 4, (1, 65500), RC.LADDER, 120, [100, 120, 120],
                                                            [30000, 9000], [None, rc.log[1][3]], 3)[0] == 302


def test_decisions_wait_for_their_pictures():
    rc = RC.RateControl(5000, 8)
    row = (8, 7, 6, 5, 4, 3, 2, 1)
    with pytest.raises(RuntimeError, match="not been decided"):
        rc.decide(2, 100)
    assert rc.decide(1, 100) == 100 and rc.decide(2, 100) == 100
    with pytest.raises(RuntimeError, match="not all been recorded"):
        rc.decide(3, 100)
    rc.record(0, 100, 20000)
    with pytest.raises(ValueError, match="sweep sums"):
        rc.record(1, 100, 5000)
    with pytest.raises(ValueError, match="decided with q index 100"):
        rc.record(1, 101, 5000, row)
    with pytest.raises(ValueError, match="8"):
        rc.record(1, 100, 5000, row[:7])
    rc.record(1, 100, 5000, row)
    with pytest.raises(ValueError, match="already recorded"):
        rc.record(1, 100, 5000, row)
    assert isinstance(rc.decide(3, 100), int)


# ------------------------------------------------------------------------------------------------------------ the plant
SLOPE = 25          # bits per hundredth of q: 25 * 65536 / 100 is an integer, so every sweep sum is one too
OTHER, TOP = 3000, 8500


def _plant_bits(q):
    """A P picture coded with q index `q`: the other components' constant bits plus a y part that is LINEAR in q -- hence
    piecewise linear on every ladder, with the same slope in every segment, and the model T_s represents it exactly."""
    return OTHER + TOP - SLOPE * q


def _plant_row(q, ladder):
    """Its sweep sums: the y part at q * h / 100, in 2^-16 bit (exact integers)."""
    return tuple(TOP * 65536 - (SLOPE * 65536 // 100) * q * h for h in ladder)


def test_plant_whose_curve_the_model_represents_exactly():
    """From the third P picture on the prediction is exact up to the snap of q to hundredths: b_j = T_s(m*) is the plant at
    q_s m*, the picture is coded at round(q_s m*), at most half a hundredth away, and the plant's largest slope is SLOPE
    bits per hundredth -- |A_j - b_j| <= SLOPE / 2.  The picture in flight is predicted exactly (its q is known), so the
    last budget is the whole remainder and the GOP total misses G b by the last picture's error alone; that lies inside
    the bound the issue states (the two uncontrolled pictures' excess plus the snap), which is asserted as well."""
    G, b, q_start, i_bits = 12, 8000, 100, 20000
    bound = Fraction(SLOPE, 2)
    rc = RC.RateControl(b, G)
    rc.record(0, 100, i_bits)
    bits, qs = [i_bits], [100]
    for j in range(1, G):
        q = rc.decide(j, q_start)
        A = _plant_bits(q)
        assert A > 0
        rc.record(j, q, A, _plant_row(q, rc.ladder))
        bits.append(A)
        qs.append(q)
    log = rc.log
    for j in range(3, G):
        budget, s = log[j][2], j - 2
        ratio = Fraction(qs[j], qs[s])
        assert Fraction(50, 100) < ratio < Fraction(252, 100), "the plant must keep every decision inside the ladder"
        assert 1 < qs[j] < 65500, "and away from q_range"
        print("picture", j, "q", qs[j], "bits", bits[j], "budget", float(budget), "error", float(bits[j] - budget))
        assert abs(bits[j] - budget) <= bound, (j, bits[j], budget)
    assert len(set(qs[3:])) > 1 and qs[3] > q_start  # (the I picture overspent: the step goes up, then settles)
    total, excess = sum(bits), sum(max(0, bits[j] - b) for j in (1, 2))
    print("total", total, "target", G * b, "excess of the two uncontrolled pictures", excess)
    assert abs(total - G * b) <= bound
    assert abs(total - G * b) <= excess + bound


# ------------------------------------------------------------------------------------------------------------- refusals
def test_ladders_targets_and_ranges_are_refused_by_name():
    assert RC.LADDER == (50, 63, 79, 100, 126, 159, 200, 252) and RC.check_ladder(list(RC.LADDER)) == RC.LADDER
    assert RC.check_ladder((10, 100, 1000)) == (10, 100, 1000)
    for ladder, word in (((50, 63, 200), "must contain 100"), ((100, 50, 200), "strictly increasing"),
                         ((50, 100, 100), "strictly increasing"), (tuple(range(96, 105)), "9 entries"), ((100,), "1 entries"),
                         ((9, 100), "10..1000"), ((100, 1001), "10..1000"), ((50.0, 100), "integers"), ((True, 100), "integers"),
                         (100, "sequence")):
        with pytest.raises(ValueError, match=f"ladder.*{word}"):
            RC.check_ladder(ladder)
        with pytest.raises(ValueError, match="ladder"):
            RC.RateControl(1000, 8, ladder=ladder)
    f = RC.ladder_factors(RC.LADDER)
    assert f.dtype == np.float32 and [float(v) for v in f] == [float(R.factor(h)) for h in RC.LADDER]
    for bad in (0, -5, float("nan"), float("inf"), "9", None, True):
        with pytest.raises(ValueError, match="target_bits"):
            RC.RateControl(bad, 8)
        with pytest.raises(ValueError, match="target_bpp"):
            RC.target_bits_of(bad, 64, 64)
    assert RC.target_bits_of(0.5, 72, 104) == Fraction(1, 2) * 72 * 104
    for bad in ((0, 100), (100, 65501), (200, 100), (1.0, 2), (1,), None, (True, 5)):
        with pytest.raises(ValueError, match="q_range"):
            RC.RateControl(1000, 8, q_range=bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="gop"):
            RC.RateControl(1000, bad)
    assert RC.q_index_range(None) == (1, 65500) and RC.q_index_range((0.5, 2)) == (50, 200)
    for bad, word in (((2.0, 1.0), "exceeds"), ((0.001, 1.0), "wire range"), ((1.0, 656.0), "wire range"),
                      ((float("nan"), 1.0), "wire range"), ((1.0,), "expected"), ("ab", "expected")):
        with pytest.raises(ValueError, match=f"q_range.*{word}"):
            RC.q_index_range(bad)
    with pytest.raises(ValueError, match="target_bits"):
        RC.factory(0, 8)
    assert isinstance(RC.factory(1000, 8)(), RC.RateControl)


def test_sweep_rows_decode_and_report_their_status():
    from vcm_ts_amd.bitmap import BitMapError

    row = np.arange(2 * 3 + 1, dtype=np.int64)
    row[-1] = 0
    sums = RC.RateSweep.decode(row, 2, 3)
    assert sums.shape == (2, 3) and sums.dtype == np.int64 and sums[1, 2] == 5
    for status, word in ((RC.BAD_VALUE, "not finite"), (1, "CDF row")):
        row[-1] = status
        with pytest.raises(BitMapError, match=word):
            RC.RateSweep.decode(row, 2, 3)
    # a log replayed into a fresh controller (no decide): predict() is T_s
    rc = RC.RateControl(5000, 8)
    rc.record(0, 100, 20000)
    rc.record(1, 120, 9000, tuple(65536 * v for v in (9000, 8000, 7000, 6000, 5000, 4000, 3000, 2000)))
    assert rc.predict(1, 120) == 9000 and rc.predict(1, 240) == 9000 + (3000 - 6000) and rc.predict(1, 12) == 9000 + 3000
    assert rc.predict(1, 135) == 9000 + Fraction(5000 - 6000, 1) * Fraction(1125 - 1000, 1260 - 1000)
    with pytest.raises(RuntimeError, match="no recorded sweep"):
        rc.predict(0, 100)


def test_file_loop_arguments():
    from vcm_ts_amd import run_codec as F

    assert F._rate_args(None, None, 64, 64, 8) is None
    with pytest.raises(ValueError, match="q_range= belongs to target_bpp="):
        F._rate_args(None, (1.0, 2.0), 64, 64, 8)
    with pytest.raises(ValueError, match="target_bpp"):
        F._rate_args(0.0, None, 64, 64, 8)
    with pytest.raises(ValueError, match="q_range.*exceeds"):
        F._rate_args(0.1, (3.0, 2.0), 64, 64, 8)
    rc = F._rate_args(0.25, (0.5, 4.0), 72, 104, 8)()
    assert (rc.b, rc.gop, rc.q_range, rc.ladder) == (Fraction(72 * 104, 4), 8, (50, 400), RC.LADDER)


_ORDER = "y_res scales_hat idx_edges factors K cost n_rows stride sizes offsets est N C H W status".split()


def _call(**over):
    fac = (C.c_float * 8)(0.5, 0.63, 0.79, 1.0, 1.26, 1.59, 2.0, 2.52)
    ok = dict(y_res=P, scales_hat=P, idx_edges=P, factors=C.cast(fac, C.c_void_p), K=8, cost=P, n_rows=64, stride=8, sizes=P,
              offsets=P, est=P, N=2, C=6, H=3, W=5, status=P)
    assert len(_ORDER) + 1 == len(lib._SIGS["dcvc_bits_sweep_scale"])  # the header's order, plus the stream
    if "factor" in over:
        k, v = over.pop("factor")
        fac[k] = v
    vals = dict(ok, **over)
    return lib.hip().dcvc_bits_sweep_scale(*[vals[k] for k in _ORDER], None)


def test_sweep_entry_point_refuses_bad_arguments():
    """DCVC_E_ARG before any launch; host-only, like the other refusal tests: a refused call touches no GPU."""
    for ptr in ("y_res", "scales_hat", "idx_edges", "factors", "cost", "sizes", "offsets", "est", "status"):
        assert _call(**{ptr: None}) == -1, ptr
    for over in (dict(K=0), dict(K=9), dict(K=-1), dict(factor=(0, 0.05)), dict(factor=(7, float("nan"))),
                 dict(factor=(3, float("inf"))), dict(factor=(2, 10.5)), dict(factor=(1, -1.0)), dict(C=5), dict(C=0), dict(C=514),
                 dict(stride=1), dict(stride=0), dict(n_rows=0), dict(n_rows=65537), dict(N=0), dict(N=65536), dict(H=0),
                 dict(W=0), dict(H=2049), dict(W=2049), dict(est=P + 4)):
        assert _call(**dict(over)) == -1, over
    # a factor beyond K is not looked at
    assert _call(K=3, factor=(5, float("nan")), y_res=None) == -1
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(lib.HERE), "include", "dcvc_hip_bits.h")).read()
    for macro, value in (("DCVC_BITS_BAD_VALUE", RC.BAD_VALUE), ("DCVC_BITS_MAX_LADDER", RC.MAX_LADDER),
                         ("DCVC_BITS_UNIT", RC.UNIT)):
        assert f"#define {macro} {value} " in hdr, macro
    assert "dcvc_bits_sweep_scale" in lib.BITS_SYMBOLS and "correctly rounded" in hdr and "fast-math" in hdr


# --------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("argv,word", [
    (["--target-bpp", "0"], "target_bpp"),
    (["--target-bpp", "-0.1"], "target_bpp"),
    (["--target-bpp", "0.1", "--q-range", "2", "1"], "exceeds"),
    (["--target-bpp", "0.1", "--q-range", "0.001", "1"], "wire range"),
    (["--target-bpp", "0.1", "--q-range", "1", "700"], "wire range"),
    (["--q-range", "1", "2"], "--q-range belongs to --target-bpp"),
    (["--target-bpp", "0.1", "--rate-count", "2", "--quality", "0"], "--rate-count selects several"),
], ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_command_line_refusals(argv, word, tmp_path, monkeypatch, capsys):
    from vcm_ts_amd import run_codec as F

    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ex:
        F.main(["encode", "--frames", "F", "--bins", "B"] + argv)
    err = capsys.readouterr().err
    assert ex.value.code == 2 and "error:" in err and word in err, err


def test_command_line_passes_the_target_on(tmp_path, monkeypatch):
    from vcm_ts_amd import run_codec as F

    monkeypatch.chdir(tmp_path)
    seen = {}

    def fake_encode(*args, **kw):
        seen.update(kw)
        return [8], (64, 64)

    monkeypatch.setattr(F, "encode_folder", fake_encode)
    F.main(["encode", "--frames", "F", "--bins", "B"])
    assert seen["target_bpp"] is None and seen["q_range"] is None
    F.main(["encode", "--frames", "F", "--bins", "B", "--target-bpp", "0.25", "--q-range", "0.5", "4", "--q", "1", "1", "1.5"])
    assert seen["target_bpp"] == 0.25 and seen["q_range"] == [0.5, 4.0]
    with pytest.raises(SystemExit):
        F.main(["decode", "--bins", "B", "--recon", "R", "--height", "64", "--width", "64", "--target-bpp", "0.25"])
