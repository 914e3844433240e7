"""The camera-shake registration without a GPU: tests/shake_ref.py (the numpy restatement of include/dcvc_hip_shake.h) held
against brute-force properties, the two integer host functions of vcm_ts_amd/shake.py against their restatements, and what
registration buys the two scans, measured with the project's own restatements of them (tests/motion_ref.py,
tests/noise_ref.py)."""
import numpy as np
import pytest

from tests import me_ref as ME
from tests import motion_ref as MR
from tests import noise_ref as NR
from tests import shake_ref as R
from vcm_ts_amd import shake as SH

F32 = np.float32


def _grey(values):
    return ME.grey(np.asarray(values))


def _shifted(world, sy, sx, H, W, m=16):
    return world[m + sy:m + sy + H, m + sx:m + sx + W]


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("move", [(0, 0), (3, -5), (-8, 8), (7, 1)])
def test_a_pure_shift_of_a_random_picture_gives_that_vector_in_every_tile(move):
    H, W, Rr = 128, 192, 8
    world = np.random.default_rng(1).integers(0, 256, (H + 32, W + 32))
    anchor, cur = _shifted(world, 0, 0, H, W), _shifted(world, *move, H, W)
    t = R.tiles(_grey(cur), anchor, Rr)
    assert t.shape == (6, 5) and (t[:, :2] == move).all() and (t[:, 3] > 2 * 1024 * 40).all() and (4 * t[:, 2] < t[:, 3]).all()
    for a in range(2):  # a tile whose moved samples all lie inside the anchor finds them exactly; the others see the clamp
        for b in range(3):
            inside = 64 * a + move[0] >= 0 and 64 * a + 60 + move[0] < H and 64 * b + move[1] >= 0 and 64 * b + 63 + move[1] < W
            assert (t[3 * a + b, 2] == 0) == inside, (a, b)
    # SAD(0, 0) by hand for one tile: rows 64, 68, ... of tile (1, 2)
    d = np.abs(cur.astype(np.int64) - anchor)[64:128:4, 128:192].sum()
    assert t[1 * 3 + 2, 4] == d and (d == 0) == (move == (0, 0))
    rec = R.vote(t, Rr, 6)
    want_status = R.EDGE if 8 in (abs(move[0]), abs(move[1])) else 0
    assert rec == [0 if want_status else move[0], 0 if want_status else move[1], 6, 6, 6, want_status, move[0], move[1]]
    # the registered picture is the anchor wherever the source pixel lay inside the picture
    reg = R.register(_grey(cur), rec)
    if want_status:  # (lost: passed on unmoved)
        assert np.array_equal(R.luma(reg), cur)
        return
    keep = ~np.repeat(np.repeat(R.border_cells(rec[0], rec[1], H, W), 16, 0), 16, 1)[:H, :W]
    assert np.array_equal(R.luma(reg)[keep], anchor[keep])


def test_an_all_equal_picture_votes_in_no_tile_and_zeros_do_not_vote():
    H, W = 64, 128
    flat = np.full((H, W), 77)
    t = R.tiles(_grey(flat), flat, 4)
    assert (t == [0, 0, 0, 0, 0]).all()  # every SAD 0: the key order answers (0, 0)
    assert R.vote(t, 4, 1) == [0, 0, 0, 0, 2, R.FEW, 0, 0]
    t = R.tiles(_grey(flat), flat + 3, 4)  # a flat tile under another light: every SAD 3072, twice the choice exceeds the largest
    assert (t == [0, 0, 3072, 3072, 3072]).all() and R.vote(t, 4, 1)[2] == 0
    ones = R.tiles(np.ones((3, H, W), F32), np.zeros((H, W), np.int64), 16)
    assert (ones == [0, 0, 261120, 261120, 261120]).all()


def test_a_picture_periodic_in_x_gives_the_tie_the_key_order_decides():
    cur, ref = ME.period4(64, 192)  # SAD is 0 at dx = +-2 (mod 4) inside the picture: (0, -2) and (0, 2) tie, the smaller dx wins
    t = R.tiles(cur, R.luma(ref), 3)
    assert t[1, :3].tolist() == [0, -2, 0] and t[1, 4] > 0  # the middle tile, whose windows all lie inside
    table = R.tile_sads(cur, R.luma(ref), 3)
    assert table[0, -2][0, 1] == 0 and table[0, 2][0, 1] == 0 and table[0, 0][0, 1] == t[1, 4]
    # the outer tiles see the clamp on one side, and no tie
    assert t[0, :3].tolist() == [0, 2, 0] and t[2, :3].tolist() == [0, -2, 0] and table[0, -2][0, 0] > 0 and table[0, 2][0, 2] > 0


def test_lower_medians_status_bits_and_agreement():
    def rec(dy, dx, s=10, top=100):
        return [dy, dx, s, top, 50]

    # an even count: the LOWER of the two middle elements, per axis
    t = [rec(1, 5), rec(2, 6), rec(3, 7), rec(4, 8)]
    assert R.vote(t, 8, 1) == [2, 6, 4, 1, 4, 0, 2, 6]
    # the two medians from different tiles: nobody agrees
    t = [rec(0, 3), rec(1, 0), rec(2, 1)]
    assert R.vote(t, 8, 1) == [1, 1, 3, 0, 3, 0, 1, 1]
    # too few votes: the flat, the zero and the doubtful tile have no opinion; the vector is zeroed, the medians are kept
    t = [rec(2, -3), rec(2, -3), rec(5, 5, 0, 0), rec(5, 5, 51, 100), rec(5, 5, 100, 100)]
    assert R.vote(t, 8, 3) == [0, 0, 2, 2, 5, R.FEW, 2, -3]
    assert R.vote(t, 8, 2) == [2, -3, 2, 2, 5, 0, 2, -3]
    assert R.vote([rec(5, 5, 50, 100)], 8, 1)[2] == 1  # twice the choice EQUAL to the largest still votes
    # a median at the radius: the true motion may lie beyond
    assert R.vote([rec(-8, 1)] * 3, 8, 1) == [0, 0, 3, 3, 3, R.EDGE, -8, 1]
    assert R.vote([rec(1, 8)] * 3, 8, 4) == [0, 0, 3, 3, 3, R.EDGE | R.FEW, 1, 8]
    assert R.vote([rec(9, 0), rec(0, -9)], 8, 1) == [0, 0, 0, 0, 2, R.FEW, 0, 0]  # words beyond the range are not counted
    assert R.vote(np.zeros((0, 5)), 8, 1) == [0, 0, 0, 0, 0, R.FEW, 0, 0]


# ---------------------------------------------------------------------------------------------------- host functions
def test_summary_and_border_cells_equal_their_restatements():
    g = np.random.default_rng(5)
    for n in (1, 2, 9):
        log = np.zeros((n, 8), dtype=np.int64)
        log[:, 4] = 24
        log[1:, 0:2] = g.integers(-6, 7, (n - 1, 2))
        log[1:, 2] = g.integers(0, 25, n - 1)
        log[1:, 3] = np.minimum(g.integers(0, 25, n - 1), log[1:, 2])
        log[1:, 5] = g.integers(0, 4, n - 1) * (g.random(n - 1) < 0.3)
        log[1:, 6:8] = log[1:, 0:2]
        log[log[:, 5] != 0, 0:2] = 0
        assert SH.summary(log) == R.summary(log) == SH.summary(log.astype(np.int32)), n
    hand = [[0, 0, 0, 0, 6, 0, 0, 0], [2, -3, 6, 4, 6, 0, 2, -3], [0, 0, 1, 1, 6, 1, 5, 5], [-1, 0, 3, 2, 6, 0, -1, 0], [0, 0, 0, 0, 6, 1, 0, 0]]
    assert SH.summary(np.array(hand)) == {"pictures": 5, "moved": 2, "lost": 2, "max_dy": 2, "max_dx": 3, "min_agree": [4, 6]}
    assert SH.summary(np.array(hand[:1])) == {"pictures": 1, "moved": 0, "lost": 0, "max_dy": 0, "max_dx": 0, "min_agree": [0, 0]}
    for H, W in ((128, 192), (70, 100), (16, 16), (1, 1), (250, 33)):
        for dy, dx in ((0, 0), (1, 0), (0, -1), (-6, 5), (16, -16), (-16, 16), (15, 15), (-1, -1)):
            got = SH.border_cells(dy, dx, H, W)
            assert got.dtype == bool and np.array_equal(got, R.border_cells(dy, dx, H, W)), (H, W, dy, dx)
    assert not SH.border_cells(0, 0, 128, 192).any() and SH.border_cells(1, 0, 128, 192).sum() == 12
    for bad in (dict(radius=0), dict(radius=17), dict(radius=8, min_votes=0), dict(radius=8, max_lost=101), dict(radius=True),
                dict(radius=8.0)):
        with pytest.raises(ValueError):
            SH.ShakeParams(**bad)
    with pytest.raises(TypeError):
        SH.ShakeParams()  # no default radius
    assert SH.ShakeParams(8).to_json() == {"radius": 8, "min_votes": 8, "max_lost": 25}
    with pytest.raises(ValueError, match="the camera moves.*--tnr T"):
        SH.check_lost({"lost": 3, "pictures": 10}, SH.ShakeParams(8))
    SH.check_lost({"lost": 2, "pictures": 8}, SH.ShakeParams(8))  # 25 % is not MORE than 25 %


# ------------------------------------------------------------------------------------------------ the six conditions
BIG = (256, 384)
MOVES = R.shifts(10, 6)


@pytest.mark.parametrize("name", list(R.CONDITIONS))
def test_every_picture_of_every_condition_gives_the_exact_vector(name):
    """256 x 384, R = 8, shifts within +-6: 9 pictures after the anchor in each of the six conditions, 54 in all."""
    pics = R.condition(name, *BIG, MOVES)
    log, _ = R.run(pics, 8)
    found = [tuple(r[:2]) for r in log.tolist()]
    print(name, "exact:", sum(a == b for a, b in zip(found[1:], MOVES[1:])), "of", len(MOVES) - 1, "votes", log[1:, 2].tolist(),
          "agree", log[1:, 3].tolist())
    assert found == MOVES and (log[:, 5] == 0).all(), (name, found, MOVES)
    assert (log[1:, 4] == 24).all() and (log[1:, 2] >= 8).all()


@pytest.mark.parametrize("name", list(R.CONDITIONS))
def test_six_tiles_give_the_exact_vector_or_lose_the_picture_by_name(name):
    """128 x 192 has six tiles (min_votes 3): every picture is exact or LOST (status set, the vector zeroed, the picture passed
    on unmoved); none is wrong.  The counts are printed: the README's figure for this size."""
    pics = R.condition(name, 128, 192, MOVES)
    log, reg = R.run(pics, 8, 3)
    exact = lost = 0
    for t in range(1, len(MOVES)):
        dy, dx, n, agree, n_tiles, status, my, mx = log[t].tolist()
        assert n_tiles == 6 and (status != 0 or (dy, dx) == MOVES[t]), (name, t, log[t].tolist(), MOVES[t])
        if status:
            assert (dy, dx) == (0, 0) and status == R.FEW and n < 3 and np.array_equal(reg[t], pics[t]), (name, t)
        exact, lost = exact + (status == 0), lost + (status != 0)
    print(name, "at 128 x 192: exact", exact, "lost", lost, "of", len(MOVES) - 1, "votes", log[1:, 2].tolist())


# ------------------------------------------------------------------------------------------------ what it buys the scans
@pytest.fixture(scope="module")
def clips():
    still = R.clip(*BIG, None, n=10)
    shaken = R.clip(*BIG, R.shifts(10, 4))
    log, registered = R.run(shaken, 8)
    return still, shaken, log, registered


def test_the_motion_scan_sees_the_registered_clip_as_the_still_one(clips):
    still, shaken, log, registered = clips
    H, W = BIG
    assert [tuple(r[:2]) for r in log.tolist()] == R.shifts(10, 4)

    def active(pics):
        return np.stack([c >= 8 for _, c in MR.run(pics, 12, 4, 8)])

    a_still, a_shaken, a_reg = active(still), active(shaken), active(registered)
    cells = (H // 16) * (W // 16)
    full = [int(a.sum()) == cells for a in a_shaken[1:]]
    print("active cells: still", [int(a.sum()) for a in a_still[1:]], "shaken", [int(a.sum()) for a in a_shaken[1:]],
          "registered", [int(a.sum()) for a in a_reg[1:]])
    assert sum(full) * 2 >= len(full)  # every cell active in at least half the pictures
    spurious = []
    for t in range(1, 10):
        off = ~R.border_cells(log[t][0], log[t][1], H, W)
        spurious.append(int((a_reg[t] & ~off).sum()))
        assert abs(int((a_reg[t] & off).sum()) - int((a_still[t] & off).sum())) <= 1, t
    print("active border cells of the registered clip:", spurious)
    masked = R.masked_counts(np.stack([c for _, c in MR.run(registered, 12, 4, 8)]), log, H, W)
    assert np.array_equal(masked, SH.mask_border(np.stack([c for _, c in MR.run(registered, 12, 4, 8)]), log, H, W))


def test_the_noise_scan_measures_the_noise_of_the_registered_clip_and_texture_of_the_shaken_one(clips):
    still, shaken, log, registered = clips
    want = 32.0 * NR.expected_mad(2.0)
    got = {name: NR.estimate(NR.histogram(pics), 1024, 9)["mad32"] for name, pics in (("still", still), ("shaken", shaken), ("registered", registered))}
    print("mad32: expected %.1f" % want, got)
    assert 0.90 * want <= got["still"] <= 1.05 * want and 0.90 * want <= got["registered"] <= 1.05 * want
    assert got["shaken"] > 5 * want
