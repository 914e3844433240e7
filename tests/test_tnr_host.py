"""The temporal noise prefilter without a GPU: the numpy restatement (tests/tnr_ref.py) against an independent per-pixel
statement of include/dcvc_hip_tnr.h, tnr.TNR and its table, what the filter is for on a noisy fixed-camera clip, the
entry point's host-side refusals, and the command line's parsing."""
import math

import numpy as np
import pytest

from tests import tnr_ref as R

F32 = np.float32


def _code(v):
    v = float(v)
    if math.isnan(v):
        return 0
    return int(np.rint(F32(255.0) * F32(min(max(v, 0.0), 1.0))))


def _luma(pic, y, x):
    r, g, b = (_code(pic[c, y, x]) for c in range(3))
    return (54 * r + 183 * g + 19 * b + 128) >> 8


def _independent(cur, ref, tab, P):
    """Per-pixel Python loops; the blend in float64, rounded to float32 after each operation."""
    _, H, W = cur.shape
    d = [[abs(_luma(cur, y, x) - _luma(ref, y, x)) for x in range(W)] for y in range(H)]
    out = np.empty_like(cur)
    hc, wc = R.grid(H, W)
    sad, held = np.zeros((hc, wc), np.int64), np.zeros((hc, wc), np.int64)
    for y in range(H):
        for x in range(W):
            S = 0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    S += d[min(max(y + dy, 0), H - 1)][min(max(x + dx, 0), W - 1)]
            w = 256 if d[y][x] > P else int(tab[S // 25])
            sad[y // 16, x // 16] += d[y][x]
            held[y // 16, x // 16] += w < 256
            for c in range(3):
                if w == 256:
                    out[c, y, x] = cur[c, y, x]
                    continue
                t = F32(np.float64(cur[c, y, x]) - np.float64(ref[c, y, x]))
                t = F32(np.float64(t) * np.float64(w))
                t = F32(np.float64(t) * 2.0 ** -8)
                out[c, y, x] = F32(np.float64(ref[c, y, x]) + np.float64(t))
    return out, sad, held


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_an_independent_statement(size):
    H, W = size
    g = np.random.default_rng(H * W)
    ref = g.uniform(-0.1, 1.1, (3, H, W)).astype(F32)
    # near the reference on the left (blended), far from it on the right (passed through), both kinds in between
    cur = (ref + g.normal(0.0, 1.0, (3, H, W)) * np.linspace(0.005, 0.2, W)[None, None, :]).astype(F32)
    classes = set()
    for T, floor, P in R.SETTINGS:
        tab = R.table(T, floor)
        want = _independent(cur, ref, tab, P)
        got = R.step(cur, ref, tab, P)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (T, floor, P)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (T, floor, P)
        assert got[1][(H + 15) // 16:].sum() == 0 and got[2][:, (W + 15) // 16:].sum() == 0  # the padding cells
        shares = R.classes(cur, ref, tab, P)
        classes |= {n for n, s in enumerate(shares) if s > 0}
    assert classes == {0, 1, 2}


def test_run_restarts_at_every_i_picture():
    pics = list(R.clip(17, 21)[0][:6])
    tnr = (12, 64, 36)
    got = R.run(pics, tnr, {0, 3})
    assert got[0][0] is not None and np.array_equal(got[3][0], pics[3]) and not got[3][1].any() and not got[3][2].any()
    tail = R.run(pics[3:], tnr, {0})
    for a, b in zip(got[3:], tail):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert not np.array_equal(got[4][0], pics[4])  # (a P picture is filtered)


def test_table_values_and_refusals():
    from vcm_ts_amd import tnr as N

    for T, floor in ((12, 64), (1, 1), (64, 255), (7, 200)):
        tab = N.TNR(T, floor).table()
        assert tab.dtype == np.uint16 and tab.shape == (256,) and np.array_equal(tab, R.table(T, floor))
        assert tab[0] == floor and tab[T] == 256 and tab[255] == 256
        assert tab[T - 1] == floor + ((256 - floor) * (T - 1)) // T and tab[T - 1] < 256
        assert (np.diff(tab.astype(np.int64)) >= 0).all() and tab.min() >= 1 and tab.max() == 256
    t = N.TNR(12)
    assert (t.threshold, t.floor, t.pixel) == (12, 64, 36) and N.TNR(64).pixel == 192 and N.TNR(12, pixel=0).pixel == 0
    assert N.TNR(12, 32, 255).to_json() == {"threshold": 12, "floor": 32, "pixel": 255}
    with pytest.raises(Exception):  # (frozen)
        t.threshold = 13
    for kw, name in ((dict(threshold=0), "threshold"), (dict(threshold=65), "threshold"), (dict(threshold=1.5), "threshold"),
                     (dict(threshold=True), "threshold"), (dict(threshold=8, floor=0), "floor"), (dict(threshold=8, floor=256), "floor"),
                     (dict(threshold=8, pixel=-1), "pixel"), (dict(threshold=8, pixel=256), "pixel")):
        with pytest.raises(ValueError, match=name):
            N.TNR(**kw)
    with pytest.raises(TypeError):
        N.TNR()  # (no default threshold exists)
    with pytest.raises(ValueError, match="tnr.TNR"):
        N.TnrFilter((12, 64, 36), (70, 100), "cuda:0")
    with pytest.raises(ValueError, match="no CPU fallback"):
        N.TnrFilter(t, (70, 100), "cpu")


def test_what_the_filter_is_for():
    """A noisy fixed camera with a block moving through.  The 0.5 and the 1 % are conditions, not measurements; the values
    the restatement gives on this clip are 0.196 for the ratio and, over pictures 5 .. 8, 0.908 .. 0.926 blended, 0.057
    guarded and 0.017 .. 0.035 passed through by the window alone.  (Recursive averaging with weight 1/4 leaves about
    alpha / (2 - alpha) = 0.14 of the noise's variance.)"""
    H, W, tnr = 70, 100, (12, 64, 36)
    noisy, clean = R.clip(H, W)
    assert len(noisy) == 9
    got = R.run(list(noisy), tnr, {0})
    tab = R.table(12, 64)
    sse = lambda a, b: float(((a[:, 45:].astype(np.float64) - b[:, 45:]) ** 2).sum())
    ratio = sse(got[8][0], clean[8]) / sse(noisy[8], clean[8])
    print("sse ratio", ratio)
    assert ratio < 0.5
    for t in range(5, 9):
        blended, guarded, window = R.classes(noisy[t], got[t - 1][0], tab, 36)
        print(t, blended, guarded, window)
        assert blended >= 0.01 and guarded >= 0.01 and window >= 0.01, t
        assert abs(blended + guarded + window - 1.0) < 1e-12
        assert int(got[t][2].sum()) == round(blended * H * W)  # held counts exactly the blended pixels
        # the block itself is handed to the codec untouched
        x = R.BLOCK_STEP * (t - R.BLOCK_FROM)
        assert (got[t][0][:, R.BLOCK_Y:R.BLOCK_Y + R.BLOCK, x:x + R.BLOCK] == F32(0.95)).all()


def test_entry_point_refuses_on_the_host():
    """Every refusal of include/dcvc_hip_tnr.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU."""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)  # bytes of a picture's extent
    good = dict(cur=0x10000000, crs=rs, cps=ps, ref=0x20000000, rrs=rs, rps=ps, out=0x30000000, ors=rs, ops=ps, H=H, W=W,
                wtab=0x40000000, P=36, sad=0x50000000, held=0x60000000)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "wtab", "P", "sad", "held")
    bad = [{k: None} for k in ("cur", "ref", "out", "wtab", "sad", "held")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"P": -1}, {"P": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("cps", "rps", "ops")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "out", "sad")] + [{k: good[k] + 1} for k in ("wtab", "held")] + \
          [{"out": good["cur"]}, {"out": good["ref"]}, {"out": good["cur"] + span - 4}, {"out": good["cur"] - span + 4},
           {"out": good["ref"] + 4 * ps}, {"out": good["ref"] - span + 4}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_tnr_step(*[v[k] for k in order], None) == -1, b


def test_cli_refuses_floor_and_pixel_without_tnr(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    for extra, name in ((["--tnr-floor", "32"], "--tnr-floor"), (["--tnr-pixel", "9"], "--tnr-pixel")):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and name in err and "--tnr" in err
    for extra, name in ((["--tnr", "0"], "threshold"), (["--tnr", "65"], "threshold"), (["--tnr", "8", "--tnr-floor", "256"], "floor"),
                        (["--tnr", "8", "--tnr-pixel", "256"], "pixel")):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        assert ex.value.code == 2 and name in capsys.readouterr().err
    assert not (tmp_path / "bins").exists()
