"""Film-grain synthesis without a GPU: the numpy restatement (tests/grain_ref.py) against a per-pixel statement in plain
Python loops, the white field's statistics, grain.params / grain.table against the restatement and their rules, what the
feature is for on the noisy clip, and every refusal that needs no launch: the two entry points with dummy pointers, the
record, the command line."""
import itertools
import math

import numpy as np
import pytest

from tests import grain_ref as G
from tests import tnr_ref as T
from vcm_ts_amd import grain as GR

F32 = np.float32


# ------------------------------------------------------------------------------------------ the per-pixel statement
def _code(v):
    v = F32(v)
    if v != v:
        return 0
    return int(np.rint(F32(255.0) * min(max(v, F32(0.0)), F32(1.0))))


def _luma(pic, y, x):
    return (54 * _code(pic[0, y, x]) + 183 * _code(pic[1, y, x]) + 19 * _code(pic[2, y, x]) + 128) >> 8


def _fmix(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _g(t, y, x):
    key = _fmix(t ^ 0x9E3779B9)
    w0 = _fmix((((y + 1) << 16) | (x + 1)) ^ key)
    w1 = _fmix(w0 ^ 0x9E3779B9)
    return sum((w >> s) & 255 for w in (w0, w1) for s in (0, 8, 16, 24)) - 1020


def _measure_loops(src, flt, held):
    H, W = src.shape[1:]
    wc = 4 * ((W + 63) // 64)
    acc = [0] * 32
    e = [[_luma(src, y, x) - _luma(flt, y, x) for x in range(W)] for y in range(H)]
    for y in range(H):
        for x in range(W):
            i, j = y // 16, x // 16
            if int(held.reshape(-1)[i * wc + j]) != min(16, H - 16 * i) * min(16, W - 16 * j):
                continue
            b = _luma(flt, y, x) >> 5
            acc[4 * b] += 1
            acc[4 * b + 1] += e[y][x] ** 2
            if x + 1 < W and (x + 1) // 16 == j:
                acc[4 * b + 2] += e[y][x] * e[y][x + 1]
            if y + 1 < H and (y + 1) // 16 == i:
                acc[4 * b + 3] += e[y][x] * e[y + 1][x]
    return acc


def _apply_loops(pic, t, kh, kv, stab):
    H, W = pic.shape[1:]
    out = pic.copy()
    th, tv = (kh, 64, kh), (kv, 64, kv)
    for y in range(H):
        for x in range(W):
            n = sum(tv[dy + 1] * th[dx + 1] * _g(t, y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
            s = int(stab[_luma(pic, y, x)])
            if s == 0:
                continue
            D = (n * s + (1 << 23)) >> 24  # (Python's >> floors)
            d = F32(D) * (F32(1.0) / F32(4080.0))
            for c in range(3):
                v = F32(pic[c, y, x] + d)
                v = F32(0.0) if v != v else max(v, F32(0.0))
                out[c, y, x] = min(v, F32(1.0))
    return out


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_the_per_pixel_statement(size):
    H, W = size
    g = np.random.default_rng(100 * H + W)
    src = g.integers(0, 256, (3, H, W)).astype(F32) / F32(255.0)
    flt = np.clip(src + g.integers(-6, 7, (3, H, W)).astype(F32) / F32(255.0), 0, 1).astype(F32)
    src[0, 0, 0], flt[1, H - 1, W - 1] = np.nan, F32(1.5)
    for name, held in G.held_cases(H, W).items():
        assert G.measure(src, flt, held).tolist() == _measure_loops(src, flt, held), name
    assert G.measure(src, flt, G.held_cases(H, W)["full"])[0::4].sum() == H * W
    assert not G.measure(src, flt, G.held_cases(H, W)["none"]).any()
    pic = src.copy()
    pic[:, 1, 1], pic[:, 2, 2], pic[2, 3, 3] = 0.0, 1.0, -0.25  # (the clamps; a sample below the range)
    stabs = G.stabs()
    for (kh, kv), t, name in zip(G.TAPS, [0, 1, 2 ** 31 - 1, 5], ["rising", "max", "even-zero", "zero"]):
        want = _apply_loops(pic, t, kh, kv, stabs[name])
        got = G.apply(pic, t, kh, kv, stabs[name])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, kh, kv, t)
        assert (name == "zero") == np.array_equal(got.view(np.uint32), pic.view(np.uint32))
    assert np.array_equal(G.white(3, H, W), [[_g(3, y, x) for x in range(-1, W + 1)] for y in range(-1, H + 1)])


@pytest.mark.parametrize("t", G.TIMES)
def test_white_field_is_white(t):
    """Conditions, not tuned figures: integers within +-1020, mean within 4 standard errors of 0, variance within 10 % of
    43690 (4096 samples: a standard error of about 2.2 %), lag-1 correlations below 4 / sqrt(4096)."""
    g = G.white(t, 64, 64)[1:-1, 1:-1]
    assert g.dtype == np.int64 and np.abs(g).max() <= 1020
    n, sd = g.size, math.sqrt(G.WHITE_VAR)
    assert abs(g.mean()) < 4 * sd / math.sqrt(n)
    assert abs(g.var() / G.WHITE_VAR - 1) < 0.10
    z = (g - g.mean()) / g.std()
    for a, b in ((z[:, :-1], z[:, 1:]), (z[:-1], z[1:]), (z[:-1, :-1], z[1:, 1:])):
        assert abs((a * b).mean()) < 4 / math.sqrt(n)
    other = G.white(t ^ 1, 64, 64)[1:-1, 1:-1]
    assert abs(((other - other.mean()) / other.std() * z).mean()) < 4 / math.sqrt(n)  # another picture, another field


def _acc(counts, var16=None, rho_h=0.0, rho_v=0.0):
    """32 sums of bins with `counts` pixels, the variance var16[b] / 256 codes^2 and the two correlations."""
    acc = []
    for b, c in enumerate(counts):
        s2 = c * (var16[b] if var16 else 400) // 256
        acc += [c, s2, int(rho_h * s2), int(rho_v * s2)]
    return acc


def test_params_rules():
    ms = 1000
    var16 = [(16 * (b + 1)) ** 2 for b in range(8)]  # standard deviations of 1, 2, ... 8 codes
    rec = GR.params(_acc([5000] * 8, var16), ms)
    assert rec == G.params(_acc([5000] * 8, var16), ms)
    assert rec["points"] == [16 * (b + 1) for b in range(8)] and rec["kh"] == rec["kv"] == 0 and rec["counts"] == [5000] * 8
    # a bin below min_samples takes its nearest populated neighbour's value, the lower one on a tie
    rec = GR.params(_acc([5000, 999, 5000, 0, 0, 5000, 10, 10], var16), ms)
    assert rec["points"] == [16, 16, 48, 48, 96, 96, 96, 96] and rec == G.params(_acc([5000, 999, 5000, 0, 0, 5000, 10, 10], var16), ms)
    assert GR.params(_acc([999] * 8, var16), ms) == {"points": [0] * 8, "kh": 0, "kv": 0, "counts": [999] * 8}
    assert GR.params([0] * 32, 1) == {"points": [0] * 8, "kh": 0, "kv": 0, "counts": [0] * 8}
    assert GR.params(_acc([1000] + [0] * 7, var16), ms)["points"] == [16] * 8  # (min_samples itself is enough)
    with pytest.raises(ValueError, match="32 sums"):
        GR.params([0] * 31, 1)
    # the tap inversion: monotone, 0 for no correlation, +-24 at and beyond the ends, exact at every tap's own correlation
    taps = []
    for r in np.linspace(-0.99, 0.99, 199):
        rec = GR.params(_acc([100000] * 8, [10 ** 6] * 8, r, -r), ms)
        assert rec["kh"] == -rec["kv"] == G.tap(int(r * 100000 * 10 ** 6 // 256) * 8, (100000 * 10 ** 6 // 256) * 8) or abs(r) < 1e-9
        taps.append(rec["kh"])
    assert taps == sorted(taps) and taps[0] == -24 and taps[-1] == 24 and taps[99] == 0 and set(taps) == set(range(-24, 25))
    for k in range(-24, 25):
        d = 4096 + 2 * k * k
        assert GR._tap(128 * k, d) == k == G.tap(128 * k, d)
    assert GR._tap(5, 0) == 0 and GR._tap(0, 7) == 0
    # the same sums in any accumulation order: integers, so every order is the same 32 words -- and the same record
    g = np.random.default_rng(3)
    parts = [g.integers(-10 ** 6, 10 ** 6, 32) for _ in range(6)]
    for p in parts:
        p[0::4], p[1::4] = np.abs(p[0::4]), np.abs(p[1::4]) * 50
    recs = {str(GR.params(sum(parts[i] for i in order).tolist(), ms)) for order in itertools.permutations(range(6))}
    assert len(recs) == 1


def test_table_values_and_range():
    points = [16, 32, 64, 16, 0, 160, 320, 4080]
    for kh, kv in G.TAPS:
        for percent in (1, 100, 200):
            tab = GR.table(points, kh, kv, percent)
            assert tab.dtype == np.uint16 and tab.shape == (256,) and np.array_equal(tab, G.table(points, kh, kv, percent))
    tab = GR.table(points, 0, 0, 100).astype(np.int64)
    root = math.isqrt(43690 * 4096 * 4096)
    assert root == 856152  # (209.02 * 4096)
    unit = (1 << 24) / root  # the entry of a standard deviation of 1/16 code
    assert (tab[:17] == tab[0]).all() and (tab[240:] == tab[255]).all() and tab[0] == round(16 * unit)
    for b, p in enumerate(points):
        assert tab[16 + 32 * b] == min(65535, round(p * unit)), b
    assert tab[32] == round(24 * unit) and tab[144] == 0 and tab[255] == 65535  # half way between centres; held to uint16
    assert (np.diff(tab[16:81]) >= 0).all() and (np.diff(tab[80:145]) <= 0).all()
    # the synthesised standard deviation is the measured one, whatever the taps: s * sqrt(variance of n) / 2^24 = points
    for kh, kv in G.TAPS:
        sd_n = math.sqrt(43690 * (4096 + 2 * kh * kh) * (4096 + 2 * kv * kv))
        assert abs(GR.table([160] * 8, kh, kv)[100] * sd_n / 2 ** 24 - 160) < 0.5
    one, two = GR.table([160] * 8, 7, 3, 1).astype(np.int64), GR.table([160] * 8, 7, 3, 200).astype(np.int64)
    assert (abs(one * 100 - GR.table([160] * 8, 7, 3).astype(np.int64)) <= 50).all() and (abs(two - 2 * GR.table([160] * 8, 7, 3)) <= 1).all()
    assert not GR.table([0] * 8, 24, -24, 200).any()
    for bad in (dict(points=[0] * 7), dict(points=[0] * 7 + [4081]), dict(points=[-1] + [0] * 7), dict(kh=25), dict(kv=-25),
                dict(percent=0), dict(percent=201), dict(points=[0.5] * 8)):
        with pytest.raises(ValueError):
            GR.table(**dict(dict(points=[0] * 8, kh=0, kv=0, percent=100), **bad))


@pytest.fixture(scope="module")
def clip():
    """The 70 x 100 noisy clip through the filter (T = 12, floor 64, P = 36), measured over its P pictures (one GOP)."""
    noisy, clean = T.clip(70, 100)
    gops, run = G.record(list(noisy), (12, 64, 36), {0}, 1024)
    return noisy, clean, gops, run


def test_grain_brings_the_noise_back(clip):
    """What the feature is for.  Over the fully held cells of pictures 5 .. 8, the luma variance of (picture - clean):
    noisy 3.948, filtered 1.010, grained 3.427 codes^2 (the restatement's, computed here on the CPU) -- the grained
    pictures' is nearer, in absolute log-ratio, to the noisy ones' than the filtered ones' is.  The test gates on the
    ordering, not on the figures."""
    noisy, clean, gops, run = clip
    rec = gops[0]
    assert sum(rec["counts"]) > 8 * 1024 and max(rec["points"]) > 0 and abs(rec["kh"]) <= 24 and abs(rec["kv"]) <= 24
    shown = G.grained([r[0] for r in run], gops, {0})
    assert np.array_equal(shown[0], noisy[0])
    diffs = {"noisy": [], "filtered": [], "grained": []}
    for t in range(5, 9):
        full = (run[t][2] == G.full_counts(70, 100)) & (G.full_counts(70, 100) > 0)
        part = np.repeat(np.repeat(full, 16, axis=0), 16, axis=1)[:70, :100]
        assert part.any()
        for name, pic in (("noisy", noisy[t]), ("filtered", run[t][0]), ("grained", shown[t])):
            diffs[name].append((G.luma(pic) - G.luma(clean[t]))[part])
    var = {name: float(np.concatenate(v).var()) for name, v in diffs.items()}
    print("luma variance over the fully held cells of pictures 5..8:", var)
    assert abs(math.log(var["grained"] / var["noisy"])) < abs(math.log(var["filtered"] / var["noisy"])), var


# ------------------------------------------------------------------------------------------------------------- refusals
def test_entry_points_refuse_before_any_launch():
    """Dummy pointers: a refused call returns before anything is launched or dereferenced."""
    from vcm_ts_amd import lib

    L = lib.hip()
    H, W, rs, ps = 70, 100, 104, 70 * 104
    m = dict(src=0x10000, srs=rs, sps=ps, flt=0x4000000, frs=rs, fps=ps, H=H, W=W, held=0x8000000, acc=0x9000000)
    order = ("src", "srs", "sps", "flt", "frs", "fps", "H", "W", "held", "acc")
    bad = [{k: None} for k in ("src", "flt", "held", "acc")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}] + \
          [{k: W - 1} for k in ("srs", "frs")] + [{k: (H - 1) * rs + W - 1} for k in ("sps", "fps")] + \
          [{k: m[k] + 2} for k in ("src", "flt")] + [{"held": m["held"] + 1}, {"acc": m["acc"] + 4}]
    for b in bad:
        v = dict(m, **b)
        assert L.dcvc_grain_measure(*[v[k] for k in order], None) == -1, b
    a = dict(inp=0x1000000, irs=rs, ips=ps, out=0x4000000, ors=rs, ops=ps, H=H, W=W, t=0, kh=0, kv=0, stab=0x8000000)
    order = ("inp", "irs", "ips", "out", "ors", "ops", "H", "W", "t", "kh", "kv", "stab")
    span = 4 * (2 * ps + (H - 1) * rs + W)
    bad = [{k: None} for k in ("inp", "out", "stab")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("irs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("ips", "ops")] + \
          [{k: a[k] + 2} for k in ("inp", "out")] + [{"stab": a["stab"] + 1}, {"kh": 25}, {"kh": -25}, {"kv": 25}, {"kv": -25},
                                                     {"t": -1}, {"t": -(2 ** 31)}] + \
          [{"out": a["inp"]}, {"out": a["inp"] + span - 4}, {"out": a["inp"] - span + 4}, {"inp": a["out"] + 4 * ps}]
    for b in bad:
        v = dict(a, **b)
        assert L.dcvc_grain_apply(*[v[k] for k in order], None) == -1, b


def _plan(n=8, gop=4):
    from vcm_ts_amd.scenecut import GopPlan

    return GopPlan.fixed(n, gop)


def _record():
    from vcm_ts_amd.tnr import TNR

    rec = {"points": [16] * 8, "kh": 3, "kv": -2, "counts": [2000] * 8}
    return GR.record_of(GR.Grain(), TNR(12), {0: rec, 4: dict(rec, kh=0)})


def test_record_refusals(tmp_path):
    import copy
    import json

    good = _record()
    assert good["version"] == 1 and good["min_samples"] == 1024 and good["tnr"] == {"threshold": 12, "floor": 64, "pixel": 36}
    assert list(good["gops"]) == ["0", "4"] and GR.check_record(good, _plan()) is good
    GR.write_grain(str(tmp_path), good)
    assert json.loads((tmp_path / "grain.json").read_text()) == good and GR.read_grain(str(tmp_path), _plan()) == good

    def broken(path, value, drop=False):
        rec = copy.deepcopy(good)
        at = rec
        for k in path[:-1]:
            at = at[k]
        if drop:
            del at[path[-1]]
        else:
            at[path[-1]] = value
        return rec

    cases = [(broken(["version"], 2), "version 2"), (broken(["version"], None, True), "version None"), ([], "version"),
             (broken(["min_samples"], 0), "min_samples"), (broken(["gops", "4"], None, True), "plan"),
             (broken(["gops"], [1, 2]), "plan"), (broken(["gops", "0", "kh"], 25), "GOP 0: kh"),
             (broken(["gops", "4", "kv"], "x"), "GOP 4: kv"), (broken(["gops", "0", "points"], [16] * 7), "GOP 0: .*8 points"),
             (broken(["gops", "0", "points", 3], 4081), "GOP 0: points"), (broken(["gops", "0", "counts"], [1] * 9), "GOP 0: .*8 counts"),
             (broken(["gops", "0", "counts", 0], -1), "GOP 0: counts"), (broken(["gops", "0"], 5), "GOP 0")]
    for rec, match in cases:
        with pytest.raises(ValueError, match=match):
            GR.check_record(rec, _plan())
    with pytest.raises(ValueError, match="plan"):
        GR.check_record(good, _plan(8, 8))
    with pytest.raises(ValueError, match="plan"):
        GR.check_record(good, _plan(12, 4))
    (tmp_path / "grain.json").write_text(json.dumps(broken(["version"], 7)))
    with pytest.raises(ValueError, match=r"grain\.json: version 7"):
        GR.read_grain(str(tmp_path), _plan())
    GR.write_grain(str(tmp_path), None)  # (a stale file is removed)
    assert not (tmp_path / "grain.json").exists()
    with pytest.raises(ValueError, match=r"no grain\.json"):
        GR.read_grain(str(tmp_path), _plan())
    for bad in (0, -5, True, 2.5, 2 ** 31):
        with pytest.raises(ValueError, match="min_samples"):
            GR.Grain(bad)


def test_file_loops_refuse_by_name_before_any_launch(tmp_path):
    """No GPU is touched: every refusal comes before the first launch (and before the device is looked at)."""
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd.tnr import TNR

    with pytest.raises(ValueError, match="grain= needs tnr="):
        RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), grain=GR.Grain())
    with pytest.raises(ValueError, match=r"expected a grain\.Grain"):
        RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), tnr=TNR(12), grain=True)
    assert not (tmp_path / "bins").exists()
    bins = tmp_path / "empty"
    bins.mkdir()
    for percent in (0, 201, True, 50.0):
        with pytest.raises(ValueError, match="grain must be an integer within 1..200"):
            RC.decode_folder(str(bins), str(tmp_path / "rec"), 64, 64, grain=percent)
    with pytest.raises(NotImplementedError, match="grain= with residuals= / residual_bins="):
        RC._decode_grain(100, str(bins), _plan(), None, str(tmp_path / "rl"), "file")  # (decode_folder wants a roi first)
    with pytest.raises(NotImplementedError, match="grain= with residuals= / residual_bins="):
        RC._decode_grain(100, str(bins), _plan(), str(tmp_path / "res.gbrp"), None, "file")
    with pytest.raises(ValueError, match="base-only decode .* takes no grain="):
        RC.decode_folder(str(bins), str(tmp_path / "rec"), 64, 64, grain=100, base_scale=None)
    with pytest.raises(ValueError, match=r"no grain\.json"):
        RC.decode_folder(str(bins), str(tmp_path / "rec"), 64, 64, grain=100)
    with pytest.raises(ValueError, match=r"no grain\.json"):
        RC.decode_video(str(bins), str(tmp_path / "rec.y4m"), 64, 64, grain=100)
    assert not (tmp_path / "rec").exists() and not (tmp_path / "rec.y4m").exists()


def test_command_line_refusals(tmp_path, capsys):
    from vcm_ts_amd import run_codec as RC

    enc = ["encode", "--frames", str(tmp_path / "png"), "--bins", str(tmp_path / "bins")]
    dec = ["decode", "--bins", str(tmp_path), "--recon", str(tmp_path / "rec"), "--height", "64", "--width", "64"]
    cases = [(enc + ["--grain"], "--grain needs --tnr"),
             (enc + ["--tnr", "12", "--grain-min-samples", "5"], "--grain-min-samples belongs to --grain"),
             (enc + ["--tnr", "12", "--grain", "--grain-min-samples", "0"], "--grain-min-samples: min_samples must be an integer"),
             (dec + ["--grain", "0"], "--grain: PERCENT must be within 1..200"),
             (dec + ["--grain", "201"], "--grain: PERCENT must be within 1..200"),
             (dec + ["--grain", "much"], "invalid int value"),
             (dec + ["--grain", "--base-only"], "--base-only takes no --grain"),
             (dec + ["--grain"], "--grain: no grain.json in")]
    for argv, message in cases:
        with pytest.raises(SystemExit) as ex:
            RC.main(argv)
        assert ex.value.code == 2 and message in capsys.readouterr().err, argv
    assert not (tmp_path / "bins").exists() and not (tmp_path / "rec").exists()
