"""Quarter-pel motion without a GPU: the numpy restatement (tests/mesub_ref.py) against an independent per-cell statement
of include/dcvc_hip_mesub.h in Python loops, the tie rules of the key, the interpolating compensation at every phase and at
the int16 extremes, tnr.TNR's new field, the command line's parsing, the entry points' host-side refusals, and what the
refinement is for on a noisy clip whose object moves by a fraction of a pixel."""
import math

import numpy as np
import pytest

from tests import me_ref as M
from tests import mesub_ref as R

F32 = np.float32
# the filters once more, typed in from the header on their own: phase -> (first offset, taps)
TAPS = {0: (0, [64]), 1: (-3, [-1, 4, -10, 58, 17, -5, 1]), 2: (-3, [-1, 4, -11, 40, 40, -11, 4, -1]), 3: (-2, [1, -5, 17, 58, -10, 4, -1])}


def _code(v):
    v = float(v)
    if math.isnan(v):
        return 0
    return int(np.rint(F32(255.0) * F32(min(max(v, 0.0), 1.0))))


def _luma_rows(pic):
    _, H, W = pic.shape
    return [[(54 * _code(pic[0, y, x]) + 183 * _code(pic[1, y, x]) + 19 * _code(pic[2, y, x]) + 128) >> 8 for x in range(W)] for y in range(H)]


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


def _yi(yr, H, W, y, x, vy, vx):
    """The interpolated luma of one pixel, tap by tap."""
    iy, py, ix, px = vy >> 2, vy & 3, vx >> 2, vx & 3
    (oy, ty), (ox, tx) = TAPS[py], TAPS[px]
    s = 0
    for j, tj in enumerate(ty):
        row = yr[_clamp(y + iy + oy + j, 0, H - 1)]
        h = sum(tk * row[_clamp(x + ix + ox + k, 0, W - 1)] for k, tk in enumerate(tx))
        assert -32768 <= h <= 32767
        s += tj * h
    return _clamp((s + 2048) >> 12, 0, 255)


def _independent_refine(cur, ref, lam, mv_in):
    _, H, W = cur.shape
    hc, wc = R.grid(H, W)
    yc, yr = _luma_rows(cur), _luma_rows(ref)
    mvq, cost = np.zeros((hc, wc, 2), np.int64), np.zeros((hc, wc), np.int64)
    for i in range(hc):
        for j in range(wc):
            pixels = [(y, x) for y in range(16 * i, min(16 * i + 16, H)) for x in range(16 * j, min(16 * j + 16, W))]
            if not pixels:
                continue
            dy, dx = (_clamp(int(v), -32, 32) for v in mv_in[i, j])
            keys = {}
            for fy in range(-3, 4):
                for fx in range(-3, 4):
                    vy, vx = 4 * dy + fy, 4 * dx + fx
                    sad = sum(abs(yc[y][x] - _yi(yr, H, W, y, x, vy, vx)) for y, x in pixels)
                    keys[4 * sad + lam * (abs(vy) + abs(vx)), abs(vy) + abs(vx), vy, vx] = sad
            best = min(keys)
            mvq[i, j], cost[i, j] = best[2:], keys[best]
    return mvq, cost


def _independent_compensate(ref, mvq):
    """Pixel by pixel, scalar float32 operations in the header's order."""
    _, H, W = ref.shape
    out = np.empty_like(ref)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                vy, vx = (int(v) for v in mvq[y // 16, x // 16])
                iy, py, ix, px = vy >> 2, vy & 3, vx >> 2, vx & 3
                (oy, ty), (ox, tx) = TAPS[py], TAPS[px]
                for c in range(3):
                    if py == 0 and px == 0:
                        out[c, y, x] = ref[c, _clamp(y + iy, 0, H - 1), _clamp(x + ix, 0, W - 1)]
                        continue
                    rows = []
                    for j in range(len(ty)):
                        row = ref[c, _clamp(y + iy + oy + j, 0, H - 1)]
                        if px == 0:
                            rows.append(row[_clamp(x + ix, 0, W - 1)])
                            continue
                        a = F32(tx[0] / 64) * row[_clamp(x + ix + ox, 0, W - 1)]
                        for k in range(1, len(tx)):
                            a = F32(a + F32(F32(tx[k] / 64) * row[_clamp(x + ix + ox + k, 0, W - 1)]))
                        rows.append(a)
                    a = rows[0]
                    if py != 0:
                        a = F32(ty[0] / 64) * rows[0]
                        for j in range(1, len(ty)):
                            a = F32(a + F32(F32(ty[j] / 64) * rows[j]))
                    a = F32(0) if np.isnan(a) else min(max(a, F32(0)), F32(1))
                    out[c, y, x] = F32(0) if a == 0 else a
    return out


def _pair(H, W):
    g = np.random.default_rng(H * W)
    ref = g.uniform(-0.1, 1.1, (3, H, W)).astype(F32)
    ref[0, 0, 0] = np.nan
    yy, xx = np.mgrid[0:H, 0:W]
    cur = (ref[:, np.clip(yy + 1, 0, H - 1), np.clip(xx - 2, 0, W - 1)] + g.normal(0, 0.01, (3, H, W))).astype(F32)
    return cur, ref


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_an_independent_statement(size):
    H, W = size
    cur, ref = _pair(H, W)
    found = M.search(cur, ref, 2, 0)[0]
    wild = M.wild_vectors(H, W)
    for lam in M.LAMBDAS:
        for mv_in in ((found, wild) if lam == 4 else (found,)):  # (the clamp of d once: the loops are slow)
            got, want = R.refine(cur, ref, lam, mv_in), _independent_refine(cur, ref, lam, mv_in)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), lam
            assert not got[0][(H + 15) // 16:].any() and not got[0][:, (W + 15) // 16:].any() and not got[1][(H + 15) // 16:].any()
            assert (np.abs(got[0] - 4 * np.clip(mv_in, -32, 32))[:(H + 15) // 16, :(W + 15) // 16] <= 3).all()
    assert (np.abs(wild) > 32).any()
    # the interpolated luma of a whole picture is the per-pixel statement's
    yr = _luma_rows(ref)
    for v in ((0, 0), (1, -2), (-5, 7), (6, 3), (-400, 129)):
        got = R.interp_picture(ref, *v)
        assert all(got[y, x] == _yi(yr, H, W, y, x, *v) for y in range(H) for x in range(W)), v
    assert np.array_equal(R.interp_picture(ref, 0, 0), R.luma(ref))


def test_sad_at_the_whole_vector_is_the_searchs():
    H, W = 33, 40
    noisy = M.clip(H, W)[0]
    cur, ref = noisy[5], noisy[4]
    whole = M.sads(cur, ref, 8)
    for lam in (0, 4):
        mv, cost, _ = M.search(cur, ref, 8, lam, whole)
        table = R.sad_table(cur, ref, mv)
        for (i, j), sads in table.items():
            d = tuple(int(v) for v in mv[i, j])
            assert sads[4 * d[0], 4 * d[1]] == whole[d][i, j] == cost[i, j], (i, j)
        mvq, costq = R.refine(cur, ref, lam, mv, table)
        yc = R.luma(cur)
        for v in ((4 * 3 - 1, 4 * -2 + 2), (4 * 3 + 3, 4 * -2 - 3)):  # one vector for the whole picture: the table is interp_picture's
            diff = np.abs(yc - R.interp_picture(ref, *v))
            uniform = R.sad_table(cur, ref, np.broadcast_to(np.array([3, -2]), mv.shape))
            assert all(sads[v] == diff[16 * i:16 * i + 16, 16 * j:16 * j + 16].sum() for (i, j), sads in uniform.items()), v
        if lam == 0:  # (J = 4 SAD: the refinement can only find a smaller SAD)
            assert (costq <= cost).all() and (costq < cost).any()


def test_tie_rules():
    H, W = 48, 64
    flat = M.grey(np.full((H, W), 77))
    mv = M.search(flat, flat, 8, 0)[0]
    assert not mv.any()
    for lam in (0, 4):  # every candidate matches: the shortest, which around d = 0 is 4 d itself
        mvq, cost = R.refine(flat, flat, lam, mv)
        assert not mvq.any() and not cost.any()
    # around another d the shortest of the 49 is three quarters nearer to zero in both directions
    d = np.zeros(R.grid(H, W) + (2,), np.int64)
    d[..., 0], d[..., 1] = 5, -2
    mvq, cost = R.refine(flat, flat, 0, d)
    assert (mvq[:3, :4] == (17, -5)).all() and not cost.any()
    # a picture made by the restatement's own interpolation at (0, +2) quarters: found again at cost 0
    cur, ref = R.shifted_pair(H, W, (0, 2))
    # (searched within +-2 and +-4: the texture is a sum of sinusoids, and a wide search can prefer an alias of a blurred copy)
    for lam in (0, 4):
        mv = M.search(cur, ref, 2, lam)[0]
        assert (np.abs(mv[:3, :4]) <= 1).all()
        mvq, cost = R.refine(cur, ref, lam, mv)
        assert (mvq[:3, :4] == (0, 2)).all() and not cost[:3, :4].any(), lam
    cur, ref = R.shifted_pair(H, W, (-7, 13))
    mvq, cost = R.refine(cur, ref, 0, M.search(cur, ref, 4, 0)[0])
    assert (mvq[1:2, 1:3] == (-7, 13)).all() and not cost[1:2, 1:3].any()


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_compensation_equals_an_independent_statement(size):
    H, W = size
    _, ref = _pair(H, W)
    odd = M.odd_bits(H, W)
    # whole vectors: the bits of me_ref.compensate, whatever the samples are
    wild = M.wild_vectors(H, W)
    assert np.array_equal(R.compensate_sub(odd, 4 * wild).view(np.uint32), M.compensate(odd, wild).view(np.uint32))
    fields = {"random": R.random_quarters(H, W), "far": R.far_quarters(H, W)}
    assert {-32768, 32767} <= set(fields["far"].reshape(-1).tolist())
    for name, mvq in fields.items():
        for kind, pic in (("plain", ref), ("odd bits", odd)):
            got = R.compensate_sub(pic, mvq)
            assert np.array_equal(got.view(np.uint32), _independent_compensate(pic, mvq).view(np.uint32)), (name, kind)
            frac = np.repeat(np.repeat(((mvq & 3) != 0).any(axis=2), 16, axis=0), 16, axis=1)[:H, :W]
            assert frac.any() and (got[:, frac] >= 0).all() and (got[:, frac] <= 1).all(), (name, kind)  # (a NaN became 0)
            assert not np.signbit(got[:, frac]).any()


def test_all_sixteen_phases_and_specials():
    H, W = 96, 96  # the sixteen inner cells (1 .. 4, 1 .. 4) take a phase pair each: no tap of theirs is clamped
    g = np.random.default_rng(3)
    ref = g.uniform(0, 1, (3, H, W)).astype(F32)
    mvq = np.zeros(R.grid(H, W) + (2,), np.int64)
    for n in range(16):
        mvq[1 + n // 4, 1 + n % 4] = (4 * (n % 3 - 1) + n // 4, 4 * (1 - n % 2) + n % 4)
    assert {(int(v[0]) & 3, int(v[1]) & 3) for v in mvq.reshape(-1, 2)} == {(a, b) for a in range(4) for b in range(4)}
    got = R.compensate_sub(ref, mvq)
    assert (got >= 0).all() and (got <= 1).all()
    assert tuple(mvq[1, 1]) == (-4, 4) and np.array_equal(got[:, 16:32, 16:32], ref[:, 15:31, 17:33])  # (phases 0, 0: a copy)
    # a ramp is followed by every phase pair: the taps sum to 64, and their first moment is 15, 32 and 49 sixty-fourths for
    # the phases 1, 2, 3 (16 and 48 would be exact), so the position is off by 1 / 64 pixel at the most in each direction
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.broadcast_to(((64 + yy + 2 * xx) / 512).astype(F32), (3, H, W)).copy()
    got = R.compensate_sub(ramp, mvq)
    for n in range(16):
        vy, vx = mvq[1 + n // 4, 1 + n % 4]
        ys, xs = slice(16 * (1 + n // 4), 16 * (2 + n // 4)), slice(16 * (1 + n % 4), 16 * (2 + n % 4))
        want = (64 + (yy[ys, xs] + vy / 4) + 2 * (xx[ys, xs] + vx / 4)) / 512
        assert np.abs(got[0, ys, xs] - want).max() <= (1 + 2) / 64 / 512 + 2e-6, n  # (fp32 rounding of ~16 operations near 0.5)
    # NaN and infinities: copied in a whole cell, inside [0, 1] in fractional cells
    special = ref.copy()
    special[0, 20, 20], special[0, 20, 40], special[1, 40, 21], special[2, 40, 40], special[1, 70, 70] = np.nan, np.nan, np.inf, -np.inf, np.inf
    got = R.compensate_sub(special, mvq)
    frac = np.repeat(np.repeat(((mvq & 3) != 0).any(axis=2), 16, axis=0), 16, axis=1)[:H, :W]
    assert (got[:, frac] >= 0).all() and (got[:, frac] <= 1).all() and np.isnan(got[0, 16:32, 16:32]).sum() == 1
    assert (got[:, frac] != R.compensate_sub(ref, mvq)[:, frac]).sum() > 100  # (and the specials were met there)


def test_tnr_setting_refusals_and_json():
    from vcm_ts_amd import tnr as N

    assert N.TNR(12, search=8).subpel is False and "subpel" not in N.TNR(12, search=8).to_json()
    s = N.TNR(12, search=8, subpel=True)
    assert s.to_json() == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4, "subpel": 4}
    assert N.TNR(12, search=8, intra=2, subpel=True).to_json() == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4,
                                                                  "intra": 2, "subpel": 4}
    for kw, name in ((dict(subpel=True), "subpel belongs to search"), (dict(subpel=True, intra=2), "subpel belongs to search"),
                     (dict(search=8, subpel=1), "subpel"), (dict(search=8, subpel=None), "subpel"), (dict(search=8, subpel=4), "subpel")):
        with pytest.raises(ValueError, match=name):
            N.TNR(12, **kw)
    assert np.array_equal(s.table(), N.TNR(12).table())


def test_cli_refusals(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    for extra, names in ((["--tnr", "8", "--tnr-subpel"], ("--tnr-subpel", "--tnr-search")), (["--tnr-subpel"], ("--tnr-subpel", "--tnr-search")),
                         (["--tnr-search", "8", "--tnr-subpel"], ("--tnr-search", "--tnr")),
                         (["--tnr", "8", "--tnr-intra", "2", "--tnr-subpel"], ("--tnr-subpel", "--tnr-search")),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-subpel", "4"], ("unrecognized arguments",))):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and all(n in err for n in names), (extra, err)
    assert not (tmp_path / "bins").exists()


def test_entry_points_refuse_on_the_host():
    """Every refusal of include/dcvc_hip_mesub.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU."""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)
    words = 2 * 2 * 8 * 8  # the bytes of mv_in and of mvq: 2 hc wc int16
    good = dict(cur=0x10000000, crs=rs, cps=ps, ref=0x20000000, rrs=rs, rps=ps, H=H, W=W, lam=4, mv=0x40000000, mvq=0x48000000,
                cost=0x50000000)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "lam", "mv", "mvq", "cost")
    bad = [{k: None} for k in ("cur", "ref", "mv", "mvq", "cost")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"lam": -1}, {"lam": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * rs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost")] + [{"mv": good["mv"] + 1}, {"mvq": good["mvq"] + 1}] + \
          [{"mvq": good["mv"]}, {"mvq": good["mv"] + words - 2}, {"mvq": good["mv"] - words + 2}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_refine(*[v[k] for k in order], None) == -1, b
    good = dict(ref=0x20000000, rrs=rs, rps=ps, out=0x30000000, ors=rs, ops=ps, H=H, W=W, mv=0x40000000)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"W": -1}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"out": good["ref"] + 4 * ps},
           {"ref": good["out"] + 4 * (H - 1) * rs}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate_sub(*[v[k] for k in order], None) == -1, b


# ------------------------------------------------------------------------------------------------- what it is for
FRACTION, INTEGER = (0.5, 0.75), (2, 6)


@pytest.fixture(scope="module")
def clips():
    """step -> (noisy, clean, the whole-pel run or None, the quarter-pel run) of the 96 x 128 sub-pel clip."""
    out = {}
    for step, both in ((FRACTION, True), (INTEGER, False)):
        noisy, clean = R.subpel_clip(step)
        whole = R.run(list(noisy), R.SETTING, {0}, R.SEARCH, R.PENALTY, subpel=False) if both else None
        out[step] = (noisy, clean, whole, R.run(list(noisy), R.SETTING, {0}, R.SEARCH, R.PENALTY))
    return out


def test_what_the_refinement_is_for(clips):
    """The 96 x 128 clip of tests/mesub_ref.py, its object moving (0.5, 0.75) pixels a picture; T = 12, floor 64, P = 36,
    R = 8, lambda = 4.  The bounds are conditions, not measurements; the restatement's own figures on this clip: the squared
    error to the clean picture as a fraction of the noisy source's over the four cells wholly inside the object, pictures
    3 .. 6: 2.097, 2.929, 2.174, 1.903 with the whole-pel search against 0.319, 0.303, 0.320, 0.320 with the refinement,
    which finds (-2, -3) quarters in every such cell.  (The plain filter without a search passes these pixels through: 1.0.)"""
    noisy, clean, whole, quarter = clips[FRACTION]
    for t in (3, 4, 5, 6):
        cells = R.object_cells(FRACTION, t)
        assert len(cells) == 4
        a, b = R.relative_error(whole[t][0], noisy[t], clean[t], cells), R.relative_error(quarter[t][0], noisy[t], clean[t], cells)
        print(t, "inside the object: whole-pel", a, "quarter-pel", b)
        assert a > 1.0 and b < 0.5, t
        for i, j in cells:
            assert tuple(quarter[t][3][i, j]) == (-2, -3), (t, i, j)
        assert R.totals(quarter[t], *R.CLIP_SIZE)[4] >= 4 and R.totals(quarter[t], *R.CLIP_SIZE)[2] >= R.totals(quarter[t], *R.CLIP_SIZE)[4]


def test_static_ground_is_the_same_with_and_without(clips):
    noisy, clean, whole, quarter = clips[FRACTION]
    ground = R.ground_cells(FRACTION)
    assert len(ground) >= 16
    for t in range(R.CLIP_FRAMES):
        for i, j in ground:
            ys, xs = slice(16 * i, 16 * i + 16), slice(16 * j, 16 * j + 16)
            assert np.array_equal(whole[t][0][:, ys, xs].view(np.uint32), quarter[t][0][:, ys, xs].view(np.uint32)), (t, i, j)
            assert not quarter[t][3][i, j].any(), (t, i, j)
    assert R.relative_error(quarter[6][0], noisy[6], clean[6], ground) < 0.3  # (and it is filtered: 0.204)


def test_integer_motion_takes_no_fractional_vector(clips):
    noisy, clean, _, quarter = clips[INTEGER]
    for t in (3, 4, 5, 6):
        cells = R.object_cells(INTEGER, t)
        assert len(cells) == 4
        for i, j in cells:
            assert tuple(quarter[t][3][i, j]) == (-8, -24), (t, i, j)
        assert R.relative_error(quarter[t][0], noisy[t], clean[t], cells) < 0.5, t  # (0.347, 0.328, 0.296, 0.309)


def test_run_without_subpel_is_me_refs_run():
    pics = list(M.clip(17, 21)[0][:4])
    a, b = R.run(pics, R.SETTING, {0}, 2, 4, subpel=False), M.run(pics, R.SETTING, {0}, 2, 4)
    for x, y in zip(a, b):
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[3], 4 * y[3])
        assert all(np.array_equal(x[k], y[k]) for k in (1, 2, 4, 5))
    c = R.run(pics, R.SETTING, {0, 2}, 2, 4)
    assert np.array_equal(c[2][0], pics[2]) and R.totals(c[2], 17, 21) == (0, 0, 0, 0, 0) and R.totals(c[3], 17, 21)[0] > 0
