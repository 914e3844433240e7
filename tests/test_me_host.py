"""The motion search and compensation without a GPU: the numpy restatement (tests/me_ref.py) against an independent
per-cell statement of include/dcvc_hip_me.h, the tie rules of the key, tnr.TNR's two new fields, the command line's parsing,
the entry points' host-side refusals, and what the search is for on a noisy clip with a moving object."""
import math

import numpy as np
import pytest

from tests import me_ref as R
from tests import tnr_ref as T

F32 = np.float32


def _code(v):
    v = float(v)
    if math.isnan(v):
        return 0
    return int(np.rint(F32(255.0) * F32(min(max(v, 0.0), 1.0))))


def _luma(pic, y, x):
    r, g, b = (_code(pic[c, y, x]) for c in range(3))
    return (54 * r + 183 * g + 19 * b + 128) >> 8


def _independent(cur, ref, R_, lam):
    """Per-cell Python loops: every candidate's SAD over the cell's pixels, the smallest (J, length, dy, dx) tuple."""
    _, H, W = cur.shape
    hc, wc = R.grid(H, W)
    yc = [[_luma(cur, y, x) for x in range(W)] for y in range(H)]
    yr = [[_luma(ref, y, x) for x in range(W)] for y in range(H)]
    mv, cost, zero = np.zeros((hc, wc, 2), np.int64), np.zeros((hc, wc), np.int64), np.zeros((hc, wc), np.int64)
    for i in range(hc):
        for j in range(wc):
            pixels = [(y, x) for y in range(16 * i, min(16 * i + 16, H)) for x in range(16 * j, min(16 * j + 16, W))]
            if not pixels:
                continue
            keys = {}
            for dy in range(-R_, R_ + 1):
                for dx in range(-R_, R_ + 1):
                    sad = sum(abs(yc[y][x] - yr[min(max(y + dy, 0), H - 1)][min(max(x + dx, 0), W - 1)]) for y, x in pixels)
                    keys[sad + lam * (abs(dy) + abs(dx)), abs(dy) + abs(dx), dy, dx] = sad
            best = min(keys)
            mv[i, j], cost[i, j] = best[2:], keys[best]
            zero[i, j] = next(sad for key, sad in keys.items() if key[2:] == (0, 0))
    return mv, cost, zero


def _independent_compensate(ref, mv):
    _, H, W = ref.shape
    out = np.empty_like(ref)
    for y in range(H):
        for x in range(W):
            dy, dx = (int(v) for v in mv[y // 16, x // 16])
            out[:, y, x] = ref[:, min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
    return out


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_an_independent_statement(size):
    H, W = size
    g = np.random.default_rng(H * W)
    ref = g.uniform(-0.1, 1.1, (3, H, W)).astype(F32)
    ref[0, 0, 0] = np.nan
    yy, xx = np.mgrid[0:H, 0:W]
    cur = (ref[:, np.clip(yy + 1, 0, H - 1), np.clip(xx - 2, 0, W - 1)] + g.normal(0, 0.01, (3, H, W))).astype(F32)
    for lam in R.LAMBDAS:
        got, want = R.search(cur, ref, 2, lam), _independent(cur, ref, 2, lam)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), lam
        assert not got[1][(H + 15) // 16:].any() and not got[0][:, (W + 15) // 16:].any() and not got[2][(H + 15) // 16:].any()
    assert tuple(R.search(cur, ref, 2, 0)[0][0, 0]) == (1, -2)  # (the translation the picture was made with)
    for mv in (R.search(cur, ref, 2, 0)[0], R.wild_vectors(H, W)):
        for pic in (ref, R.odd_bits(H, W)):
            assert np.array_equal(R.compensate(pic, mv).view(np.uint32), _independent_compensate(pic, mv).view(np.uint32))
    assert np.array_equal(R.compensate(ref, np.zeros(R.grid(H, W) + (2,), np.int64)).view(np.uint32), ref.view(np.uint32))


def test_tie_rules():
    H, W = 48, 64
    # nothing differs anywhere: every candidate of a flat picture has SAD 0, the shortest vector wins
    flat = R.grey(np.full((H, W), 77))
    mv, cost, zero = R.search(flat, flat, 8, 0)
    assert not mv.any() and not cost.any() and not zero.any()
    # (0, -2) and (0, +2) both match a period-4 pattern shifted by 2: equal J, equal length, equal dy: the smaller dx
    cur, ref = R.period4(H, W)
    mv, cost, zero = R.search(cur, ref, 8, 0)
    inner = mv[:3, 1:3]  # (the cells two columns or more from the picture's left and right edge)
    assert (inner[..., 0] == 0).all() and (inner[..., 1] == -2).all() and not cost[:3, 1:3].any() and zero[:3, 1:3].all()
    plus = R.sads(cur, ref, 8)
    assert not plus[0, 2][:3, 1:3].any() and not plus[0, -2][:3, 1:3].any()  # (both are exact matches there)
    # a translation by (0, 3): found at lambda = 0, given up for (0, 0) once 3 lambda exceeds SAD(0, 0)
    g = np.random.default_rng(1)
    ref = g.integers(100, 104, (H, W))  # (a faint texture: SAD(0, 0) of a cell is a few hundred)
    yy, xx = np.mgrid[0:H, 0:W]
    cur = ref[yy, np.clip(xx - 3, 0, W - 1)]  # cur(y, x) = ref(y, x - 3)
    cur, ref = R.grey(cur), R.grey(ref)
    mv, cost, zero = R.search(cur, ref, 8, 0)
    assert (mv[:3, 1:4, 0] == 0).all() and (mv[:3, 1:4, 1] == -3).all() and not cost[:3, 1:4].any()
    worst = int(zero[:3, :4].max())
    assert 0 < worst < 3 * 255
    lam = worst // 3 + 1  # 3 lambda > SAD(0, 0) in every cell
    mv2, cost2, zero2 = R.search(cur, ref, 8, lam)
    assert not mv2[:3, 1:4].any() and np.array_equal(cost2[:3, 1:4], zero[:3, 1:4]) and np.array_equal(zero2, zero)
    if worst >= 6:  # and a lambda that keeps 3 lambda below every inner cell's SAD(0, 0) keeps the vector
        low = int(zero[:3, 1:4].min()) // 3 - 1
        if low > 0:
            assert (R.search(cur, ref, 8, low)[0][:3, 1:4, 1] == -3).all()


def test_tnr_setting_refusals_and_json():
    from vcm_ts_amd import tnr as N

    t = N.TNR(12)
    assert (t.search, t.penalty) == (None, 4) and t.to_json() == {"threshold": 12, "floor": 64, "pixel": 36}
    s = N.TNR(12, search=8)
    assert (s.search, s.penalty) == (8, 4)
    assert s.to_json() == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4}
    assert N.TNR(6, 32, 255, 32, 0).to_json() == {"threshold": 6, "floor": 32, "pixel": 255, "search": 32, "penalty": 0}
    assert N.TNR(12, search=1, penalty=255).penalty == 255 and list(N.TNR(12, search=1).to_json())[-2:] == ["search", "penalty"]
    for kw, name in ((dict(search=0), "search"), (dict(search=33), "search"), (dict(search=1.5), "search"), (dict(search=True), "search"),
                     (dict(search=8, penalty=-1), "penalty"), (dict(search=8, penalty=256), "penalty"),
                     (dict(search=8, penalty=2.0), "penalty"), (dict(penalty=3), "penalty belongs to search"),
                     (dict(penalty=0), "penalty belongs to search")):
        with pytest.raises(ValueError, match=name):
            N.TNR(12, **kw)
    assert np.array_equal(s.table(), t.table())  # the search changes nothing about the weights


def test_cli_refusals(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    for extra, names in ((["--tnr-search", "8"], ("--tnr-search", "--tnr")), (["--tnr-penalty", "4"], ("--tnr-penalty", "--tnr")),
                         (["--tnr-search", "8", "--tnr-penalty", "4"], ("--tnr-search", "--tnr")),
                         (["--tnr", "8", "--tnr-penalty", "4"], ("--tnr-penalty", "--tnr-search")),
                         (["--tnr", "8", "--tnr-search", "0"], ("search",)), (["--tnr", "8", "--tnr-search", "33"], ("search",)),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-penalty", "256"], ("penalty",)),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-penalty", "-1"], ("penalty",))):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and all(n in err for n in names), (extra, err)
    assert not (tmp_path / "bins").exists()


def test_entry_points_refuse_on_the_host():
    """Every refusal of include/dcvc_hip_me.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU."""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)
    good = dict(cur=0x10000000, crs=rs, cps=ps, ref=0x20000000, rrs=rs, rps=ps, H=H, W=W, R=8, lam=4, mv=0x40000000, cost=0x50000000,
                zero=0x60000000)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "R", "lam", "mv", "cost", "zero")
    bad = [{k: None} for k in ("cur", "ref", "mv", "cost", "zero")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"R": 0}, {"R": 33}, {"R": -1}, {"lam": -1}, {"lam": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * rs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost", "zero")] + [{"mv": good["mv"] + 1}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_search(*[v[k] for k in order], None) == -1, b
    good = dict(ref=0x20000000, rrs=rs, rps=ps, out=0x30000000, ors=rs, ops=ps, H=H, W=W, mv=0x40000000)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"W": -1}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"out": good["ref"] + 4 * ps},
           {"ref": good["out"] + 4 * (H - 1) * rs}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate(*[v[k] for k in order], None) == -1, b


def test_run_restarts_at_every_i_picture():
    pics = list(R.clip(17, 21)[0][:6])
    tnr = (12, 64, 36)
    got = R.run(pics, tnr, {0, 3}, 2, 4)
    assert np.array_equal(got[3][0], pics[3]) and not any(a.any() for a in got[3][1:])
    tail = R.run(pics[3:], tnr, {0}, 2, 4)
    for a, b in zip(got[3:], tail):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    # a step's sad is the search's cost, cell for cell: the step measures against the compensated picture
    for step in got:
        assert np.array_equal(step[1], step[4])
    assert R.totals(got[3], 17, 21) == (0, 0, 0, 0) and R.totals(got[4], 17, 21)[0] > 0


def test_what_the_search_is_for():
    """A 96 x 128 fixed-camera clip, a textured 48 x 48 object moving (2, 6) pixels a picture, +-4 codes of fresh noise on
    everything; T = 12, floor 64, P = 36, R = 8, lambda = 4.  The bounds are conditions, not measurements; the restatement's
    own figures on this clip: squared error to the clean picture as a fraction of the noisy source's over the four cells
    wholly inside the object, 0.270 (picture 5) and 0.308 (picture 6) with the search against 1.000 and 1.000 without (the
    plain filter passes every such pixel through); every interior cell finds (-2, -6); on the rows below the object's path
    0.226 and 0.218 with the search against 0.212 and 0.200 without, x1.07 and x1.09."""
    H, W = R.CLIP_SIZE
    tnr = (12, 64, 36)
    noisy, clean = R.clip(H, W)
    cells = R.object_cells(5)
    assert cells == R.object_cells(6) == R.object_cells(4) and len(cells) == 4  # the same four, covered at picture 4 already
    with_search = R.run(list(noisy), tnr, {0}, 8, 4)
    plain = T.run(list(noisy), tnr, {0})

    def sse(a, b, where):
        return sum(float(((a[:, ys, xs].astype(np.float64) - b[:, ys, xs]) ** 2).sum()) for ys, xs in where)

    inside = [(slice(16 * i, 16 * i + 16), slice(16 * j, 16 * j + 16)) for i, j in cells]
    bottom = R.OBJECT_AT[0] + R.OBJECT_STEP[0] * (R.CLIP_FRAMES - 1) + R.OBJECT
    below = [(slice(-(-bottom // 16) * 16, H), slice(0, W))]
    assert below[0][0].start < H
    for t in (5, 6):
        source = sse(noisy[t], clean[t], inside)
        searched, passed = sse(with_search[t][0], clean[t], inside) / source, sse(plain[t][0], clean[t], inside) / source
        print(t, "inside the object: with search", searched, "plain", passed)
        assert searched < 0.5 and passed > 0.9, t
        for i, j in cells:
            assert tuple(with_search[t][3][i, j]) == (-2, -6), (t, i, j)
        source = sse(noisy[t], clean[t], below)
        searched, passed = sse(with_search[t][0], clean[t], below) / source, sse(plain[t][0], clean[t], below) / source
        print(t, "below the object's path: with search", searched, "plain", passed)
        assert searched <= 1.25 * passed, t
