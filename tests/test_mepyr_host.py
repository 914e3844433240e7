"""The hierarchical motion search without a GPU: the numpy restatement (tests/mepyr_ref.py) against an independent per-cell,
per-candidate, per-pixel statement of include/dcvc_hip_mepyr.h in Python loops, the identities that tie it to
tests/me_ref.py, what it is for on the fast clip, tnr.TNR's new field, the command line's parsing, and the entry points'
host-side refusals."""
import math

import numpy as np
import pytest

from tests import me_ref as M
from tests import mepyr_ref as R
from tests import mesub_ref as S

F32 = np.float32
CASES = ((1, 2), (1, 7), (1, 64), (2, 4), (2, 9), (2, 128))  # (levels, R)


# --------------------------------------------------------------------------------------------- an independent statement
def _code(v):
    v = float(v)
    if math.isnan(v):
        return 0
    return int(np.rint(F32(255.0) * F32(min(max(v, 0.0), 1.0))))


def _levels(pic, levels):
    """[level][y][x] as lists of Python integers, pixel by pixel."""
    _, H, W = pic.shape
    out = [[[(54 * _code(pic[0, y, x]) + 183 * _code(pic[1, y, x]) + 19 * _code(pic[2, y, x]) + 128) >> 8 for x in range(W)] for y in range(H)]]
    for _ in range(levels):
        a = out[-1]
        h, w = len(a), len(a[0])
        out.append([[(a[min(2 * y, h - 1)][min(2 * x, w - 1)] + a[min(2 * y, h - 1)][min(2 * x + 1, w - 1)] +
                      a[min(2 * y + 1, h - 1)][min(2 * x, w - 1)] + a[min(2 * y + 1, h - 1)][min(2 * x + 1, w - 1)] + 2) >> 2
                     for x in range((w + 1) // 2)] for y in range((h + 1) // 2)])
    return out


def _sad(c, r, pixels, dy, dx):
    h, w = len(r), len(r[0])
    return sum(abs(c[y][x] - r[min(max(y + dy, 0), h - 1)][min(max(x + dx, 0), w - 1)]) for y, x in pixels)


class _Independent:
    """One pair of pictures: every SAD is computed once per (level, support, cell, candidate) and kept, so that the three
    penalties share them.  A choice of more than LOOPS pixel differences a cell takes the SADs of a row of candidates (one
    dy, every dx of the range) as ONE numpy expression over the support's slices of an edge-padded plane instead of the
    pixel loops; a test below holds the two against each other."""
    LOOPS = 2000

    def __init__(self, cur, ref, levels):
        self.H, self.W = cur.shape[1:]
        self.cur, self.ref = cur, ref
        self.c, self.r = _levels(cur, levels), _levels(ref, levels)
        self.np_c = [np.array(a, dtype=np.int64) for a in self.c]
        self.np_r = [np.array(a, dtype=np.int64) for a in self.r]
        self.kept, self.rows, self.squares = {}, {}, {}

    def pixels(self, level, i, j, coarse):
        h, w = len(self.c[level]), len(self.c[level][0])
        side = 16 >> level
        y0, x0, size = (4 * i - 2, 4 * j - 2, 8) if coarse and level == 2 else (side * i, side * j, side)
        return [(y, x) for y in range(max(y0, 0), min(y0 + size, h)) for x in range(max(x0, 0), min(x0 + size, w))]

    def row(self, level, i, j, coarse, dy, pixels):
        """The SADs of the candidates (dy, -RL .. RL), by slices."""
        RL, pad = self.pad[level]
        at = (level, i, j, coarse, dy, RL)
        if at not in self.rows:
            (ya, xa), (yb, xb) = pixels[0], pixels[-1]
            rows = pad[ya + RL + dy:yb + 1 + RL + dy, xa:xb + 1 + 2 * RL]  # (the columns of every dx = -RL .. RL)
            moved = np.lib.stride_tricks.sliding_window_view(rows, xb + 1 - xa, axis=1)  # [y, dx + RL, x]
            self.rows[at] = np.abs(self.np_c[level][ya:yb + 1, None, xa:xb + 1] - moved).sum(axis=(0, 2))
        return self.rows[at]

    def sad(self, level, i, j, coarse, dy, dx, pixels, fast=False):
        if fast:
            return int(self.row(level, i, j, coarse, dy, pixels)[dx + self.pad[level][0]])
        at = (level, i, j, coarse, dy, dx)
        if at not in self.kept:
            self.kept[at] = _sad(self.c[level], self.r[level], pixels, dy, dx)
        return self.kept[at]

    def choose(self, level, i, j, coarse, cands, lam, pixels):
        mul = 2 if level == 1 else 1
        fast = len(pixels) * len(cands) > self.LOOPS
        if fast and coarse:  # (the whole square of candidates: the smallest J by numpy, the rest of the key among those that reach it)
            RL = self.pad[level][0]
            if (level, i, j, RL) not in self.squares:
                self.squares[level, i, j, RL] = np.stack([self.row(level, i, j, True, dy, pixels) for dy in range(-RL, RL + 1)])
            length = np.abs(np.arange(-RL, RL + 1))[:, None] + np.abs(np.arange(-RL, RL + 1))[None]
            J = mul * self.squares[level, i, j, RL] + lam * length
            ties = np.argwhere(J == J.min())  # (in the order of dy, then dx: the first of the shortest)
            return tuple(int(v) - RL for v in ties[np.argmin(length[ties[:, 0], ties[:, 1]])])
        keys = {(mul * self.sad(level, i, j, coarse, dy, dx, pixels, fast) + lam * (abs(dy) + abs(dx)), abs(dy) + abs(dx), dy, dx)
                for dy, dx in cands}
        return min(keys)[2:]

    def search(self, R_, lam, levels):
        hc, wc = R.grid(self.H, self.W)
        vec = [np.zeros((hc, wc, 2), np.int64) for _ in range(levels + 1)]
        cost, zero = np.zeros((hc, wc), np.int64), np.zeros((hc, wc), np.int64)
        RL = -(-R_ // (1 << levels))
        self.pad = [(-(-R_ // (1 << level)), np.pad(self.np_r[level], -(-R_ // (1 << level)), mode="edge")) for level in range(levels + 1)]
        for i in range(hc):
            for j in range(wc):
                if 16 * i >= self.H or 16 * j >= self.W:
                    continue
                px = self.pixels(levels, i, j, True)
                cands = [(dy, dx) for dy in range(-RL, RL + 1) for dx in range(-RL, RL + 1)]
                vec[levels][i, j] = self.choose(levels, i, j, True, cands, lam, px)
                for level in range(levels - 1, -1, -1):
                    Rl, E = -(-R_ // (1 << level)), 2 if level == 0 else 1
                    p = [int(v) for v in vec[level + 1][i, j]]
                    cands = [(min(max(2 * p[0] + ey, -Rl), Rl), min(max(2 * p[1] + ex, -Rl), Rl)) for ey in range(-E, E + 1) for ex in range(-E, E + 1)]
                    px = self.pixels(level, i, j, False)
                    vec[level][i, j] = self.choose(level, i, j, False, cands + [(0, 0)], lam, px)
                cost[i, j] = self.sad(0, i, j, False, int(vec[0][i, j, 0]), int(vec[0][i, j, 1]), px)
                zero[i, j] = self.sad(0, i, j, False, 0, 0, px)
        return [vec[level] for level in range(levels, 0, -1)] + [(vec[0], cost, zero)]


def _same(got, want, where):
    assert len(got) == len(want), where
    for a, b in zip(got[:-1], want[:-1]):
        assert np.array_equal(a, b), where
    for a, b in zip(got[-1], want[-1]):
        assert np.array_equal(a, b), where


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_an_independent_statement(size):
    H, W = size
    made = {}  # (the pairs differ between the cases only where min(R, 7) does: their levels and SADs are kept)
    for levels, R_ in CASES:
        for name, todo in M.pairs(H, W, R_).items():
            for n, (cur, ref) in enumerate(todo):
                if (name, n, min(R_, 7)) not in made:
                    made[name, n, min(R_, 7)] = _Independent(cur, ref, 2)
                ind = made[name, n, min(R_, 7)]
                assert np.array_equal(ind.cur, cur, equal_nan=True) and np.array_equal(ind.ref, ref, equal_nan=True)
                for a, b in zip(R.pyramid(cur, levels), ind.np_c):
                    assert np.array_equal(a, b), (name, n, levels)
                table = R.coarse_sads(cur, ref, R_, levels)
                for lam in M.LAMBDAS:
                    got = R.stages(cur, ref, R_, lam, levels, table)
                    _same(got, ind.search(R_, lam, levels), (name, n, levels, R_, lam))
                    for a in got[:-1] + list(got[-1]):  # a cell that holds no pixel is 0 in every array of every level
                        assert not a[(H + 15) // 16:].any() and not a[:, (W + 15) // 16:].any()


def test_the_slices_of_the_independent_statement_equal_its_pixel_loops():
    H, W = 17, 21
    cur, ref = M.pairs(H, W, 9)["clip"][0]
    slow, fast = _Independent(cur, ref, 2), _Independent(cur, ref, 2)
    slow.LOOPS, fast.LOOPS = 1 << 30, 0
    for lam in (0, 4):
        _same(fast.search(9, lam, 2), slow.search(9, lam, 2), lam)
    assert any(k[3] for k in slow.kept) and fast.rows
    for (level, i, j, coarse, dy, dx), v in slow.kept.items():
        assert fast.rows[level, i, j, coarse, dy, fast.pad[level][0]][dx + fast.pad[level][0]] == v


# ------------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("size", [(33, 259), (70, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identities(size):
    H, W = size
    pairs = M.pairs(H, W, 8)
    for levels, R_ in ((1, 16), (2, 16), (2, 128)):
        for name, todo in pairs.items():
            for cur, ref in todo[:1]:
                for lam in (0, 4):
                    *upper, (mv, cost, zero) = R.stages(cur, ref, R_, lam, levels)
                    assert np.array_equal(zero, M.search(cur, ref, 1, lam)[2]), (name, levels, R_)  # SAD(0, 0) is the full search's
                    at = np.unravel_index(M.cells_of(H, W), mv.shape[:2])
                    moved = np.abs(R.pyramid(cur, 0)[0] - R._moved(R.pyramid(ref, 0)[0], mv[..., 0][at], mv[..., 1][at]))
                    assert np.array_equal(cost, M.T.cell_sums(moved)), (name, levels, R_)  # the level-0 SAD of the returned vector
                    assert (cost + lam * np.abs(mv).sum(axis=2) <= zero).all()  # (0, 0) is always a candidate
                    assert all(np.abs(v).max() <= R.level_range(R_, levels - k) for k, v in enumerate(upper + [mv]))
                    if name == "flat":  # every candidate of every level matches: the shortest
                        assert not mv.any() and not cost.any() and not any(v.any() for v in upper)


def test_the_tie_falls_as_the_key_says():
    """A period-4 pattern of columns 40, 80, 120, 160 against itself two columns on.  Its 2 x 2 means are 60, 140 repeating
    against 140, 60: (0, -1) and (0, +1) both match at level 1, equal J, equal length, equal dy: the smaller dx.  The descent
    from (0, -1) finds (0, -2) at SAD 0 among (0, -4) .. (0, 0), which is what the full search chooses between (0, -2) and
    (0, +2).  The means of means are 100 everywhere: level 2 is flat, every candidate ties and the shortest wins."""
    H, W = 64, 96
    cur, ref = M.period4(H, W)
    up, (mv, cost, zero) = R.stages(cur, ref, 8, 0, 1)
    assert (up[:4, 1:5, 1] == -1).all() and not up[..., 0].any()
    two, one, (mv2, _, _) = R.stages(cur, ref, 8, 0, 2)
    assert not two.any() and (one[:4, 1:5, 1] == -1).all() and np.array_equal(mv2[:4, 1:5], mv[:4, 1:5])
    assert (mv[:4, 1:5, 1] == -2).all() and not mv[..., 0].any() and not cost[:4, 1:5].any() and zero[:4, 1:5].all()
    assert np.array_equal(mv[:4, 1:5], M.search(cur, ref, 8, 0)[0][:4, 1:5])


def test_incoming_vectors_are_bounded_by_the_clamps():
    H, W = 33, 70
    for level, bound in ((0, 24), (1, 12)):
        yc, yr = R.random_planes(H, W, level)
        p = R.wild_vectors(H, W, bound)
        assert np.abs(p).max() == 32768
        mv, cost, zero = R.descend(yc, yr, H, W, 24, 4, level, p)
        assert np.abs(mv).max() <= R.level_range(24, level) and (np.abs(mv) == R.level_range(24, level)).any()


# ------------------------------------------------------------------------------------------------- what it is for
@pytest.fixture(scope="module")
def fast():
    """step -> (noisy, clean, the run of the full search at R = 32, of L = 1 and of L = 2 at R = 64) on the fast clip at
    T = 12, floor 64, P = 36, lambda = 4."""
    out = {}
    for step in R.FAST_STEPS:
        noisy, clean = R.fast_clip(step)
        pics = list(noisy)
        out[step] = (noisy, clean, M.run(pics, R.SETTING, {0}, 32, R.PENALTY), R.run(pics, R.SETTING, {0}, 64, R.PENALTY, 1),
                     R.run(pics, R.SETTING, {0}, 64, R.PENALTY, 2))
    return out


@pytest.mark.parametrize("step", R.FAST_STEPS, ids=str)
def test_what_the_hierarchical_search_is_for(fast, step):
    """A 128 x 320 fixed-camera clip of band-limited texture (0.02 .. 0.08 cycles a pixel), a 48 x 48 object moving 39 .. 61
    pixels a picture, +-4 codes of fresh noise.  The bounds are conditions; the restatement's own figures, P pictures 1 .. 4
    of the three steps: the full search at R = 32 finds the true vector in 0 of the 4 (once 6) cells wholly inside the object
    and leaves 6.58 .. 14.75 of the noisy source's squared error there; L = 1 finds it in every such cell at 0.31 .. 1.51,
    L = 2 in all of them but for 5 of 6 and 3 of 4 in one picture each, at 0.42 .. 1.23 and once 3.40 (against 14.75: the
    worst ratio, 0.23); 0 of the 128 .. 136 untouched cells a picture have a nonzero vector."""
    noisy, clean, full, one, two = fast[step]
    true = (-step[0], -step[1])
    for t in range(1, R.FAST_FRAMES):
        inside, ground = R.object_cells(step, t), R.untouched_cells(step, t)
        assert len(inside) >= 4 and len(ground) >= 100
        found = [sum(tuple(run[t][3][i, j]) == true for i, j in inside) for run in (full, one, two)]
        error = [S.relative_error(run[t][0], noisy[t], clean[t], inside) for run in (full, one, two)]
        still = [sum(tuple(run[t][3][i, j]) != (0, 0) for i, j in ground) for run in (one, two)]
        print(step, t, "cells inside", len(inside), "found", found, "error", error, "ground", len(ground), "moved", still)
        assert found[0] == 0 and found[1] == len(inside) and 3 * found[2] >= 2 * len(inside), t
        assert still == [0, 0], t
        assert error[1] < 0.5 * error[0] and error[2] < 0.5 * error[0], t
        assert R.far(one[t][3]) >= len(inside) and R.totals(one[t], *R.FAST_SIZE)[4] == R.far(one[t][3])


def test_run_restarts_at_every_i_picture():
    pics = list(M.clip(17, 21)[0][:6])
    got = R.run(pics, R.SETTING, {0, 3}, 4, 4, 2)
    assert np.array_equal(got[3][0], pics[3]) and not any(a.any() for a in got[3][1:])
    tail = R.run(pics[3:], R.SETTING, {0}, 4, 4, 2)
    for a, b in zip(got[3:], tail):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    for step in got:  # a step's sad is the search's cost, cell for cell
        assert np.array_equal(step[1], step[4])
    assert R.totals(got[3], 17, 21) == (0, 0, 0, 0, 0) and R.totals(got[4], 17, 21)[0] > 0


# ------------------------------------------------------------------------------------------------------- the setting
def test_tnr_setting_refusals_and_json():
    from vcm_ts_amd import tnr as N

    plain = {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4}
    assert N.TNR(12, search=8).levels is None and N.TNR(12, search=8).to_json() == plain and "levels" not in N.TNR(12).to_json()
    assert N.TNR(12, search=8, levels=1).to_json() == dict(plain, levels=1) and list(N.TNR(12, search=8, levels=2).to_json())[-1] == "levels"
    assert N.TNR(12, search=16, intra=2, subpel=True, split=True, levels=2).to_json() == dict(plain, search=16, intra=2, subpel=4, split=8, levels=2)
    for levels, (lo, hi) in ((1, (2, 64)), (2, (4, 128))):
        assert N.TNR(12, search=lo, levels=levels).search == lo and N.TNR(12, search=hi, levels=levels).search == hi
        for bad in (lo - 1, hi + 1, 0, -4, 2.0, True):
            with pytest.raises(ValueError, match="search"):
                N.TNR(12, search=bad, levels=levels)
    assert N.TNR(12, search=32).search == 32 and N.TNR(12, search=1).search == 1  # without levels: as it always was
    with pytest.raises(ValueError, match="search must be an integer within 1..32"):
        N.TNR(12, search=33)
    for kw, name in ((dict(levels=1), "levels belongs to search: got levels=1 without search"), (dict(levels=2, intra=2), "levels belongs to search"),
                     (dict(search=8, levels=0), "levels"), (dict(search=8, levels=3), "levels"), (dict(search=8, levels=True), "levels"),
                     (dict(search=8, levels=1.0), "levels"),
                     (dict(search=33, levels=1, subpel=True), "subpel stops at search=32"), (dict(search=64, levels=2, split=True), "split stops at search=32"),
                     (dict(search=128, levels=2, subpel=True, split=True), "subpel stops at search=32")):
        with pytest.raises(ValueError, match=name):
            N.TNR(12, **kw)
    assert N.TNR(12, search=32, levels=2, subpel=True, split=True).search == 32  # at 32 both work behind the pyramid
    assert np.array_equal(N.TNR(12, search=64, levels=1).table(), N.TNR(12).table())


def test_cli_parsing_and_refusals(capsys, tmp_path, monkeypatch):
    from vcm_ts_amd import run_codec as RC

    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    for extra, names in ((["--tnr", "8", "--tnr-levels", "2"], ("--tnr-levels", "--tnr-search")), (["--tnr-levels", "1"], ("--tnr-levels", "--tnr-search")),
                         (["--tnr-search", "64", "--tnr-levels", "1"], ("--tnr-search", "--tnr")),
                         (["--tnr", "8", "--tnr-search", "64"], ("search",)), (["--tnr", "8", "--tnr-search", "65", "--tnr-levels", "1"], ("search",)),
                         (["--tnr", "8", "--tnr-search", "3", "--tnr-levels", "2"], ("search",)),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-levels", "3"], ("levels",)),
                         (["--tnr", "8", "--tnr-search", "64", "--tnr-levels", "2", "--tnr-subpel"], ("subpel stops at search=32",)),
                         (["--tnr", "8", "--tnr-search", "64", "--tnr-levels", "2", "--tnr-split"], ("split stops at search=32",)),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-levels"], ("expected one argument",))):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and all(n in err for n in names), (extra, err)
    assert not (tmp_path / "bins").exists()
    seen = {}
    monkeypatch.setattr(RC, "encode_folder", lambda *a, **kw: seen.update(kw) or ([8], (1, 1)))  # (the parsed setting, nothing coded)
    RC.main(base + ["--tnr", "8", "--tnr-search", "128", "--tnr-levels", "2"])
    assert seen["tnr"].to_json() == {"threshold": 8, "floor": 64, "pixel": 24, "search": 128, "penalty": 4, "levels": 2}
    RC.main(base + ["--tnr", "8", "--tnr-search", "16", "--tnr-levels", "1", "--tnr-subpel", "--tnr-split"])
    assert seen["tnr"].to_json()["levels"] == 1 and seen["tnr"].subpel and seen["tnr"].split


def test_entry_points_refuse_on_the_host():
    """Every refusal of include/dcvc_hip_mepyr.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU."""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)
    good = dict(pic=0x10000000, rs=rs, ps=ps, H=H, W=W, L=2, y0=0x20000000, s0=100, y1=0x28000000, s1=52, y2=0x2c000000, s2=28)
    order = ("pic", "rs", "ps", "H", "W", "L", "y0", "s0", "y1", "s1", "y2", "s2")
    bad = [{k: None} for k in ("pic", "y0", "y1", "y2")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"L": 0}, {"L": 3}, {"L": -1}] + \
          [{"rs": W - 1}, {"ps": (H - 1) * rs + W - 1}, {"pic": good["pic"] + 2}] + \
          [{k: good[k] + n} for k in ("y0", "y1", "y2") for n in (1, 2)] + \
          [{"s0": 96}, {"s0": 102}, {"s1": 48}, {"s1": 50}, {"s1": 51}, {"s2": 24}, {"s2": 25}, {"s2": 26}, {"s2": 0}, {"s0": -100}] + \
          [{"y1": good["y0"]}, {"y1": good["y0"] + 69 * 100 + 96}, {"y2": good["y1"] + 34 * 52 + 48}, {"y2": good["y0"] - 17 * 28 - 20},
           {"y0": good["y1"] - 69 * 100 - 96}, {"y0": good["pic"]}, {"y1": good["pic"] + span - 4}, {"y2": good["pic"] + 4 * ps},
           {"y0": good["pic"] - 69 * 100 - 96}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_pyramid(*[v[k] for k in order], None) == -1, b

    good = dict(cur=0x20000000, cs=28, ref=0x28000000, rs=28, H=H, W=W, R=64, L=2, lam=4, mv=0x40000000)
    order = ("cur", "cs", "ref", "rs", "H", "W", "R", "L", "lam", "mv")
    bad = [{k: None} for k in ("cur", "ref", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"W": -1}] + \
          [{"L": 0}, {"L": 3}, {"R": 3}, {"R": 129}, {"R": 0}, {"R": -8}, {"L": 1}, {"lam": -1}, {"lam": 256}] + \
          [{k: v} for k in ("cs", "rs") for v in (24, 26, 27, 0, -28)] + [{k: good[k] + n} for k in ("cur", "ref") for n in (1, 2)] + \
          [{"mv": good["mv"] + 1}]
    for b in bad:  # ({"L": 1}: R = 64 is within L = 1's range, but the strides of level 2 are below level 1's width)
        v = dict(good, **b)
        assert lib.hip().dcvc_me_coarse(*[v[k] for k in order], None) == -1, b
    for b in ({"R": 1}, {"R": 65}):
        v = dict(good, L=1, cs=52, rs=52, **b)
        assert lib.hip().dcvc_me_coarse(*[v[k] for k in order], None) == -1, b

    good = dict(cur=0x20000000, cs=100, ref=0x28000000, rs=100, H=H, W=W, R=64, L=2, level=0, lam=4, mv_in=0x40000000, mv=0x48000000,
                cost=0x50000000, zero=0x60000000)
    order = ("cur", "cs", "ref", "rs", "H", "W", "R", "L", "level", "lam", "mv_in", "mv", "cost", "zero")
    bad = [{k: None} for k in ("cur", "ref", "mv_in", "mv", "cost", "zero")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}] + \
          [{"L": 0}, {"L": 3}, {"level": -1}, {"level": 2}, {"R": 3}, {"R": 129}, {"lam": -1}, {"lam": 256}] + \
          [{k: v} for k in ("cs", "rs") for v in (96, 98, 99, 0)] + [{k: good[k] + n} for k in ("cur", "ref") for n in (1, 2)] + \
          [{"mv": good["mv"] + 1}, {"mv_in": good["mv_in"] + 1}, {"cost": good["cost"] + 2}, {"zero": good["zero"] + 2}, {"mv": good["mv_in"]}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_descend(*[v[k] for k in order], None) == -1, b
    for b in ({"level": 1}, {"level": 1, "cs": 48}, {"R": 65}, {"R": 1}):  # one level: no level 1 to descend to, R within 2 .. 64
        v = dict(good, L=1, **b)
        assert lib.hip().dcvc_me_descend(*[v[k] for k in order], None) == -1, b
    v = dict(good, level=1, cs=48, rs=52, cost=None, zero=None)  # level 1 needs no cost or zero, but its own strides
    assert lib.hip().dcvc_me_descend(*[v[k] for k in order], None) == -1
