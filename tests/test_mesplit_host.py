"""Vectors per 8 x 8 sub-cell without a GPU: the numpy restatement (tests/mesplit_ref.py) against an independent per-pixel
statement of include/dcvc_hip_mesplit.h in Python loops, the identities that tie it to tests/mesub_ref.py and
tests/me_ref.py, tnr.TNR's new field, the command line's parsing, the entry points' host-side refusals, and what the
re-selection is for -- and is not -- on the noisy clips of tests/mesub_ref.py."""
import numpy as np
import pytest

from tests import me_ref as M
from tests import mesplit_ref as R
from tests import mesub_ref as S
from tests.test_mesub_host import TAPS, _clamp, _luma_rows, _pair, _yi

F32 = np.float32


def _independent_split(cur, ref, lam, mv_in, unit):
    """Sub-cell by sub-cell, candidate by candidate, pixel by pixel."""
    _, H, W = cur.shape
    hc, wc = R.grid(H, W)
    rows, cols = -(-H // 16), -(-W // 16)
    yc, yr = _luma_rows(cur), _luma_rows(ref)
    lim = 32 if unit == 1 else 131
    mv8, cost8 = np.zeros((2 * hc, 2 * wc, 2), np.int64), np.zeros((2 * hc, 2 * wc), np.int64)
    for a in range(2 * hc):
        for b in range(2 * wc):
            pixels = [(y, x) for y in range(8 * a, min(8 * a + 8, H)) for x in range(8 * b, min(8 * b + 8, W))]
            if not pixels:
                continue
            keys = {}
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    word = mv_in[_clamp((a >> 1) + di, 0, rows - 1), _clamp((b >> 1) + dj, 0, cols - 1)]
                    vy, vx = (_clamp(int(v), -lim, lim) * (4 // unit) for v in word)
                    sad = sum(abs(yc[y][x] - _yi(yr, H, W, y, x, vy, vx)) for y, x in pixels)
                    keys[4 * sad + lam * (abs(vy) + abs(vx)), abs(vy) + abs(vx), vy, vx] = sad
            best = min(keys)
            mv8[a, b], cost8[a, b] = best[2:], keys[best]
    return mv8, cost8


def _independent_compensate_split(ref, mv8):
    """Pixel by pixel, scalar float32 operations in the header's order, the vector that of the pixel's 8 x 8 sub-cell."""
    _, H, W = ref.shape
    out = np.empty_like(ref)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                vy, vx = (int(v) for v in mv8[y // 8, x // 8])
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


@pytest.mark.parametrize("size", [(7, 9), (17, 21)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_an_independent_statement(size):
    H, W = size
    cur, ref = _pair(H, W)
    found = M.search(cur, ref, 2, 0)[0]
    fields = {1: (found, M.wild_vectors(H, W)), 4: (S.refine(cur, ref, 0, found)[0], S.far_quarters(H, W), R.distinct_vectors(H, W))}
    assert (np.abs(fields[1][1]) > 32).any() and (np.abs(fields[4][1]) > 131).any()  # (words far outside the clamp)
    for unit, todo in fields.items():
        for mv_in in todo:
            table = R.sad8_table(cur, ref, mv_in, unit)
            for lam in M.LAMBDAS:
                got, want = R.split(cur, ref, lam, mv_in, unit, table), _independent_split(cur, ref, lam, mv_in, unit)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b), (unit, lam)
                assert not got[0][-(-H // 8):].any() and not got[0][:, -(-W // 8):].any() and not got[1][-(-H // 8):].any()
                assert (np.abs(got[0]) <= 131).all() and (unit == 4 or not (got[0] & 3).any())
    for seed in (1, 2):
        mv8 = R.sub_vectors(H, W, seed, whole=0.25 * (seed - 1))
        for pic in (ref, M.odd_bits(H, W)):
            assert np.array_equal(R.compensate_split(pic, mv8).view(np.uint32), _independent_compensate_split(pic, mv8).view(np.uint32)), seed
    assert {-32768, 32767} <= set(R.sub_vectors(H, W, 1).reshape(-1).tolist())


def test_nine_equal_candidates_return_the_vector_and_the_cells_sad():
    H, W = 33, 40
    noisy = M.clip(H, W)[0]
    cur, ref = noisy[5], noisy[4]
    hc, wc = R.grid(H, W)
    for d, f in (((3, -2), (0, 0)), ((3, -2), (-1, 2)), ((0, 0), (0, 0)), ((-32, 32), (-3, 3))):
        v = (4 * d[0] + f[0], 4 * d[1] + f[1])
        sads = S.sad_table(cur, ref, np.broadcast_to(np.array(d), (hc, wc, 2)))  # (the cells' SADs of the 49 around d)
        todo = [(np.broadcast_to(np.array(v), (hc, wc, 2)), 4)] + ([(np.broadcast_to(np.array(d), (hc, wc, 2)), 1)] if f == (0, 0) else [])
        for mv_in, unit in todo:
            for lam in M.LAMBDAS:
                mv8, cost8 = R.split(cur, ref, lam, mv_in, unit)
                assert (mv8[:-(-H // 8), :-(-W // 8)] == v).all(), (v, unit, lam)
                for (i, j), cell in sads.items():
                    assert cost8[2 * i:2 * i + 2, 2 * j:2 * j + 2].sum() == cell[v], (v, unit, i, j)


def test_compensation_with_repeated_vectors_is_the_cells_compensation():
    for H, W in ((17, 21), (33, 40)):
        _, ref = _pair(H, W)
        odd = M.odd_bits(H, W)
        for pic in (ref, odd):
            for mvq in (S.random_quarters(H, W), S.far_quarters(H, W)):
                assert np.array_equal(R.compensate_split(pic, R.repeated(mvq)).view(np.uint32), S.compensate_sub(pic, mvq).view(np.uint32))
            wild = M.wild_vectors(H, W)
            assert np.array_equal(R.compensate_split(pic, R.repeated(4 * wild)).view(np.uint32), M.compensate(pic, wild).view(np.uint32))


def test_without_a_penalty_the_sub_cells_cost_no_more_than_their_cell():
    H, W = 70, 100
    noisy = S.subpel_clip((2.25, 5.5), size=(H, W))[0]
    cur, ref = noisy[4], noisy[3]
    mv, cost, _ = M.search(cur, ref, 8, 0)
    mvq, costq = S.refine(cur, ref, 0, mv)
    for mv_in, unit, whole in ((mv, 1, cost), (mvq, 4, costq)):
        mv8, cost8 = R.split(cur, ref, 0, mv_in, unit)
        hc, wc = R.grid(H, W)
        sums = cost8.reshape(hc, 2, wc, 2).sum(axis=(1, 3))
        assert (sums <= whole).all() and (sums < whole).any(), unit
        assert R.left(mv8, 4 * mv if unit == 1 else mvq, H, W) > 0


def test_tnr_setting_refusals_and_json():
    from vcm_ts_amd import tnr as N

    assert N.TNR(12, search=8).split is False and "split" not in N.TNR(12, search=8).to_json()
    assert "split" not in N.TNR(12, search=8, subpel=True).to_json()
    assert N.TNR(12, search=8, split=True).to_json() == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4, "split": 8}
    assert N.TNR(12, search=8, intra=2, subpel=True, split=True).to_json() == {"threshold": 12, "floor": 64, "pixel": 36, "search": 8, "penalty": 4,
                                                                              "intra": 2, "subpel": 4, "split": 8}
    for kw, name in ((dict(split=True), "split belongs to search: got split=True without search"), (dict(split=True, intra=2), "split belongs to search"),
                     (dict(search=8, split=1), "split must be True or False"), (dict(search=8, split=None), "split"), (dict(search=8, split=8), "split")):
        with pytest.raises(ValueError, match=name):
            N.TNR(12, **kw)
    assert np.array_equal(N.TNR(12, search=8, split=True).table(), N.TNR(12).table())


def test_cli_refusals(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    base = ["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins")]
    for extra, names in ((["--tnr", "8", "--tnr-split"], ("--tnr-split", "--tnr-search")), (["--tnr-split"], ("--tnr-split", "--tnr-search")),
                         (["--tnr-search", "8", "--tnr-split"], ("--tnr-search", "--tnr")),
                         (["--tnr", "8", "--tnr-intra", "2", "--tnr-split"], ("--tnr-split", "--tnr-search")),
                         (["--tnr", "8", "--tnr-search", "8", "--tnr-split", "8"], ("unrecognized arguments",))):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(base + extra)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and all(n in err for n in names), (extra, err)
    assert not (tmp_path / "bins").exists()


def test_entry_points_refuse_on_the_host():
    """Every refusal of include/dcvc_hip_mesplit.h with aligned dummy pointers: a refused call returns before anything is
    launched or dereferenced, so this needs no GPU."""
    from vcm_ts_amd import lib

    H, W, rs = 70, 100, 128
    ps = 128 * rs
    span = 4 * (2 * ps + (H - 1) * rs + W)
    cells = 8 * 8
    good = dict(cur=0x10000000, crs=rs, cps=ps, ref=0x20000000, rrs=rs, rps=ps, H=H, W=W, lam=4, unit=4, mv=0x40000000, mv8=0x48000000,
                cost=0x50000000)
    order = ("cur", "crs", "cps", "ref", "rrs", "rps", "H", "W", "lam", "unit", "mv", "mv8", "cost")
    bad = [{k: None} for k in ("cur", "ref", "mv", "mv8", "cost")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"H": -1}, {"lam": -1}, {"lam": 256}] + \
          [{"unit": u} for u in (0, 2, 3, 5, 8, -1, -4)] + \
          [{k: W - 1} for k in ("crs", "rrs")] + [{k: (H - 1) * rs + W - 1} for k in ("cps", "rps")] + \
          [{k: good[k] + 2} for k in ("cur", "ref", "cost")] + [{"mv": good["mv"] + 1}, {"mv8": good["mv8"] + 1}] + \
          [{"mv8": good["mv"]}, {"mv8": good["mv"] + 4 * cells - 2}, {"mv8": good["mv"] - 16 * cells + 2}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_split(*[v[k] for k in order], None) == -1, b
    good = dict(ref=0x20000000, rrs=rs, rps=ps, out=0x30000000, ors=rs, ops=ps, H=H, W=W, mv=0x40000000)
    order = ("ref", "rrs", "rps", "out", "ors", "ops", "H", "W", "mv")
    bad = [{k: None} for k in ("ref", "out", "mv")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"W": -1}] + \
          [{k: W - 1} for k in ("rrs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("rps", "ops")] + \
          [{k: good[k] + 2} for k in ("ref", "out")] + [{"mv": good["mv"] + 1}] + \
          [{"out": good["ref"]}, {"out": good["ref"] + span - 4}, {"out": good["ref"] - span + 4}, {"out": good["ref"] + 4 * ps},
           {"ref": good["out"] + 4 * (H - 1) * rs}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_compensate_split(*[v[k] for k in order], None) == -1, b


# ------------------------------------------------------------------------------------------------- what it is for
FAST, INTEGER, SLOW = (2.25, 5.5), (2, 6), (0.5, 0.75)
PICTURES = (3, 4, 5, 6)


@pytest.fixture(scope="module")
def clips():
    """step -> (noisy, clean, {(subpel, split): the run}) of the 96 x 128 sub-pel clip at T = 12, floor 64, P = 36, R = 8,
    lambda = 4."""
    out = {}
    for step, whole in ((FAST, False), (INTEGER, True), (SLOW, False)):
        noisy, clean = S.subpel_clip(step)
        runs = {(sub, spl): R.run(list(noisy), S.SETTING, {0}, S.SEARCH, S.PENALTY, sub, spl)
                for sub in ((True, False) if whole else (True,)) for spl in (False, True)}
        out[step] = (noisy, clean, runs)
    return out


def _errors(clip, step, key, cells_of):
    noisy, clean, runs = clip
    return [S.relative_error(runs[key][t][0], noisy[t], clean[t], cells_of(step, t)) for t in PICTURES]


def _edge_sse(clip, step, key):
    noisy, clean, runs = clip
    return sum(float(((runs[key][t][0][:, 16 * i:16 * i + 16, 16 * j:16 * j + 16].astype(np.float64)
                       - clean[t][:, 16 * i:16 * i + 16, 16 * j:16 * j + 16]) ** 2).sum()) for t in PICTURES for i, j in R.edge_cells(step, t))


def test_a_fast_object_keeps_its_texture(clips):
    """Clip (2.25, 5.5).  The bounds are conditions; the restatement's own figures, squared error to the clean picture as a
    fraction of the noisy source's, pictures 3 .. 6: the cells wholly inside the object 0.518, 0.725, 0.374, 1.736 with
    subpel alone and 0.298, 0.439, 0.294, 0.496 with split; the cells on its edge 2.094, 1.656, 2.826, 3.638 and 1.050,
    1.185, 1.672, 2.443 -- still above the unfiltered source's 1.0."""
    alone, both = _errors(clips[FAST], FAST, (True, False), S.object_cells), _errors(clips[FAST], FAST, (True, True), S.object_cells)
    print("inside the object: subpel", alone, "subpel + split", both)
    assert all(b < 0.6 for b in both) and alone[1] > 0.7 and alone[3] > 0.7
    a, b = _edge_sse(clips[FAST], FAST, (True, False)), _edge_sse(clips[FAST], FAST, (True, True))
    print("edge cells, squared error summed over the pictures: subpel", a, "subpel + split", b)
    assert b < a
    edge = _errors(clips[FAST], FAST, (True, True), R.edge_cells)
    print("edge cells: subpel + split", edge)
    assert all(len(R.edge_cells(FAST, t)) in (6, 12) for t in PICTURES)
    assert all(R.totals(clips[FAST][2][True, True][t], *S.CLIP_SIZE)[5] > 0 for t in PICTURES)


def test_integer_motion_is_no_worse_with_or_without_subpel(clips):
    """Clip (2, 6): inside the object 0.347, 0.328, 0.296, 0.309 -> 0.267, 0.278, 0.211, 0.251 with subpel, and 0.340, 0.328,
    0.295, 0.308 -> 0.269, 0.278, 0.211, 0.244 on whole-pel vectors."""
    for subpel in (True, False):
        alone, both = _errors(clips[INTEGER], INTEGER, (subpel, False), S.object_cells), _errors(clips[INTEGER], INTEGER, (subpel, True), S.object_cells)
        print("subpel", subpel, "inside the object: without split", alone, "with", both)
        assert all(b <= a for a, b in zip(alone, both)), subpel
    assert not any((w[6] & 3).any() for w in clips[INTEGER][2][False, True])  # (whole-pel vectors stay whole)


def test_a_slow_object_is_left_as_it_was_and_its_edge_is_not_helped(clips):
    """Clip (0.5, 0.75): inside the object 0.319, 0.303, 0.320, 0.320 -> 0.312, 0.301, 0.316, 0.314; the cells on its edge
    1.480, 1.244, 1.272, 1.538 -> 1.903, 1.317, 1.404, 1.522: slightly WORSE, which the documents state."""
    alone, both = _errors(clips[SLOW], SLOW, (True, False), S.object_cells), _errors(clips[SLOW], SLOW, (True, True), S.object_cells)
    print("inside the object: subpel", alone, "subpel + split", both)
    assert all(abs(a - b) <= 0.03 for a, b in zip(alone, both))
    print("edge cells: subpel", _errors(clips[SLOW], SLOW, (True, False), R.edge_cells), "subpel + split", _errors(clips[SLOW], SLOW, (True, True), R.edge_cells))


def test_static_ground_is_bit_identical(clips):
    for step, (noisy, clean, runs) in clips.items():
        ground = S.ground_cells(step)
        assert len(ground) >= 12
        for subpel in {k[0] for k in runs}:
            for t in range(S.CLIP_FRAMES):
                for i, j in ground:
                    ys, xs = slice(16 * i, 16 * i + 16), slice(16 * j, 16 * j + 16)
                    assert np.array_equal(runs[subpel, False][t][0][:, ys, xs].view(np.uint32), runs[subpel, True][t][0][:, ys, xs].view(np.uint32)), (step, t, i, j)
                    assert not runs[subpel, True][t][6][2 * i:2 * i + 2, 2 * j:2 * j + 2].any(), (step, t, i, j)


def test_overlapped_blocks_were_measured_and_are_worse(clips):
    """Why they were not built: on clip (2.25, 5.5) the 32 x 32 linear window leaves the cells inside the object at 1.825,
    1.850, 1.666, 2.347 of the unfiltered source's error -- it blends the wrong vector of an edge cell into its neighbours."""
    noisy, clean, _ = clips[FAST]
    got = R.run_overlapped(list(noisy), S.SETTING, {0}, S.SEARCH, S.PENALTY)
    inside = [S.relative_error(got[t], noisy[t], clean[t], S.object_cells(FAST, t)) for t in PICTURES]
    print("overlapped blocks, inside the object:", inside)
    assert all(v > 1.0 for v in inside)
    # with one vector everywhere the window's weights add up to one and the blend is the plain compensation
    H, W = 33, 40
    ref = np.random.default_rng(5).uniform(0, 1, (3, H, W)).astype(F32)
    mvq = np.broadcast_to(np.array([5, -6]), R.grid(H, W) + (2,))
    assert np.abs(R.overlapped(ref, mvq) - S.compensate_sub(ref, mvq)).max() <= 2e-7


def test_run_without_split_is_mesub_refs_run():
    pics = list(M.clip(17, 21)[0][:4])
    for subpel in (True, False):
        a, b = R.run(pics, S.SETTING, {0, 2}, 2, 4, subpel, False), S.run(pics, S.SETTING, {0, 2}, 2, 4, subpel)
        for x, y in zip(a, b):
            assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and all(np.array_equal(x[k], y[k]) for k in range(1, 6))
            assert np.array_equal(x[6], R.repeated(y[3]))
    c = R.run(pics, S.SETTING, {0, 2}, 2, 4)
    assert np.array_equal(c[2][0], pics[2]) and R.totals(c[2], 17, 21) == (0, 0, 0, 0, 0, 0) and R.totals(c[3], 17, 21)[0] > 0
    assert len(R.totals(c[3], 17, 21, subpel=False)) == 5
