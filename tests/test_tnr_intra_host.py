"""The look-ahead filter of I pictures without a GPU: tnr.TNR(intra=) and its reciprocal table, the look-ahead iterator of
the file loops on plain lists, the numpy restatement (tests/tnr_fuse_ref.py) of include/dcvc_hip_tnr_fuse.h -- its own
properties and what the fusion is for on the noisy fixed-camera clip -- the record of the film grain, and the command
line's parsing."""
import json

import numpy as np
import pytest

from tests import tnr_fuse_ref as FR
from tests import tnr_ref as R

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the setting
def test_setting_validates_intra_and_writes_it_only_when_set():
    from vcm_ts_amd import tnr as N

    assert N.TNR(8).intra is None and N.MAX_REFS == FR.MAX_REFS and N.RCP == FR.RCP
    for k in (1, 2, 3, 4):
        assert N.TNR(8, intra=k).intra == k
    for bad in (0, 5, -1, 2.5, "2", True):
        with pytest.raises(ValueError, match="intra"):
            N.TNR(8, intra=bad)
    # the JSON of every existing setting is what it was, byte for byte
    assert json.dumps(N.TNR(12).to_json()) == '{"threshold": 12, "floor": 64, "pixel": 36}'
    assert json.dumps(N.TNR(6, 32, 255).to_json()) == '{"threshold": 6, "floor": 32, "pixel": 255}'
    assert json.dumps(N.TNR(8, search=16).to_json()) == '{"threshold": 8, "floor": 64, "pixel": 24, "search": 16, "penalty": 4}'
    assert json.dumps(N.TNR(8, search=4, penalty=0).to_json()) == \
        '{"threshold": 8, "floor": 64, "pixel": 24, "search": 4, "penalty": 0}'
    assert N.TNR(8, intra=2).to_json() == {"threshold": 8, "floor": 64, "pixel": 24, "intra": 2}
    assert N.TNR(8, search=16, intra=4).to_json() == {"threshold": 8, "floor": 64, "pixel": 24, "search": 16, "penalty": 4, "intra": 4}
    assert list(N.TNR(8, search=16, intra=4).to_json())[-1] == "intra"


def test_rcp_table_is_the_restatements_bit_for_bit():
    from vcm_ts_amd import tnr as N

    got, want = N.TNR(8, intra=1).rcp_table(), FR.rcp_table()
    assert got.dtype == F32 and got.shape == (1021,) and np.array_equal(_bits(got), _bits(want))
    assert got[0] == F32(2.0 ** -8) and got[256] == F32(2.0 ** -9) and got[1020] == F32(1.0 / 1276.0)
    for U in (1, 3, 255, 510, 1019):  # the float32 nearest the float64 quotient
        q = 1.0 / (256.0 + U)
        assert abs(float(got[U]) - q) <= min(abs(float(np.nextafter(got[U], F32(0))) - q), abs(float(np.nextafter(got[U], F32(1))) - q))


# --------------------------------------------------------------------------------------------------- the look-ahead iterator
class _Counted:
    """A source of 0 .. n - 1 that counts what has been pulled from it."""

    def __init__(self, n):
        self.n, self.pulled = n, 0

    def __iter__(self):
        for i in range(self.n):
            self.pulled += 1
            yield i


def _walk(n, intra, K, hold=None):
    from vcm_ts_amd.run_codec import _LookAhead

    src = _Counted(n)
    look = _LookAhead(src, intra, K, n, hold)
    seen = []
    for item in look:
        seen.append((item, list(look.ahead), src.pulled))
    assert src.pulled == n
    return seen


@pytest.mark.parametrize("n,intra,K", [(9, {0, 4}, 2), (9, {0, 8}, 4), (9, {0, 4}, 4), (9, {0, 4, 8}, 1), (5, {0, 1, 2, 3, 4}, 3),
                                       (1, {0}, 2), (6, {0, 2, 3}, 2), (7, {0}, 3)])
def test_look_ahead_yields_once_in_order_and_stays_inside_the_gop(n, intra, K):
    seen = _walk(n, intra, K)
    assert [s[0] for s in seen] == list(range(n))  # exactly once, in order
    for t, ahead, pulled in seen:
        want = FR.ahead_of(t, n, intra, K) if t in intra else []
        assert ahead == want, t
        nxt = min([s for s in intra if s > t] + [n])
        assert len(ahead) == (min(K, nxt - t - 1) if t in intra else 0)
        # never past the next I picture or the end: what has been pulled are the pictures up to the last one shown ahead
        assert pulled <= nxt and pulled >= t + 1
        if t in intra:
            assert pulled == t + 1 + len(ahead)


def test_look_ahead_edge_cases():
    # K larger than the GOP: every picture of the GOP, none of the next
    assert [a for _, a, _ in _walk(9, {0, 4}, 4)] == [[1, 2, 3], [], [], [], [5, 6, 7, 8], [], [], [], []]
    # GOPs of one picture: nothing ahead, nothing pulled ahead
    assert [(a, p) for _, a, p in _walk(4, {0, 1, 2, 3}, 2)] == [([], 1), ([], 2), ([], 3), ([], 4)]
    assert [(a, p) for _, a, p in _walk(9, {0, 8}, 2)][8] == ([], 9)
    # K unset: one item pulled per item yielded, as the plain loop does
    for K in (None, 0):
        assert [(a, p) for _, a, p in _walk(6, {0, 3}, K)] == [([], t + 1) for t in range(6)]
    # what is held ahead goes through hold(), and what hold() gave is what is yielded later; an item that is not pulled
    # ahead is yielded as the source gave it
    seen = _walk(6, {0, 3}, 1, hold=lambda i: i + 100)
    assert [(i, a) for i, a, _ in seen] == [(0, [101]), (101, []), (2, []), (3, [104]), (104, []), (5, [])]


# ------------------------------------------------------------------------------------------- the restatement's own properties
def test_identical_references_return_the_picture_and_hold_everything():
    H, W = 33, 67
    same = R.sequences(H, W)["equal"][0]
    tab = R.table(12, 64)
    for n in (1, 2, 3, 4):
        out, sad, held = FR.fuse(same, [same.copy() for _ in range(n)], tab, 36)
        assert np.array_equal(out, same) and not sad.any() and int(held.sum()) == H * W, n


def test_flip_returns_the_bits_of_cur_and_holds_nothing():
    H, W = 33, 67
    zeros, ones = np.zeros((3, H, W), F32), np.ones((3, H, W), F32)
    zeros[0, 0, 0] = F32(-0.0)
    for T, floor, P in R.SETTINGS:
        for n in (1, 2, 3, 4):
            out, sad, held = FR.fuse(zeros, [ones] * n, R.table(T, floor), P)
            assert np.array_equal(_bits(out), _bits(zeros)) and not held.any() and int(sad.sum()) == 255 * H * W, (T, n)


def test_a_nan_reference_that_weighs_nothing_changes_nothing():
    H, W = 33, 67
    pics = R.clip(H, W)[0]
    tab, P = R.table(12, 64), 36
    want = FR.fuse(pics[0], [pics[1], pics[2]], tab, P)
    nan = np.full((3, H, W), np.nan, F32)  # (a NaN codes as 0: against the clip's 51 .. 204 every pixel is guarded)
    d, _, w = R.weights(pics[0], nan, tab, P)
    assert (w == 256).all()
    for refs in ([pics[1], nan, pics[2]], [pics[1], pics[2], nan], [nan, pics[1], pics[2], nan]):
        got = FR.fuse(pics[0], refs, tab, P)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[2], want[2]), len(refs)
        assert not np.isnan(got[0]).any()
    assert np.array_equal(FR.fuse(pics[0], [nan, pics[1], pics[2]], tab, P)[1], R.cell_sums(d))  # sad speaks of reference 0


def test_run_follows_the_stream_rule():
    H, W = 17, 67
    pics, setting = list(R.clip(H, W)[0]), R.SETTINGS[0]
    tab = R.table(*setting[:2])
    got = FR.run(pics, setting, {0, 4, 8}, 2)
    assert [g[3] for g in got] == [2, 1, 1, 1, 2, 1, 1, 1, 0]
    first = FR.fuse(pics[0], pics[1:3], tab, setting[2])
    assert np.array_equal(_bits(got[0][0]), _bits(first[0]))
    assert np.array_equal(_bits(got[1][0]), _bits(R.step(pics[1], first[0], tab, setting[2])[0]))  # from the FILTERED I picture
    assert np.array_equal(_bits(got[8][0]), _bits(pics[8])) and not got[8][1].any() and not got[8][2].any()
    assert [g[3] for g in FR.run(pics, setting, {0, 7}, 4)] == [4, 1, 1, 1, 1, 1, 1, 1, 1]
    assert [g[3] for g in FR.run(pics, setting, {0, 6}, 4)] == [4, 1, 1, 1, 1, 1, 2, 1, 1]


# ------------------------------------------------------------------------------------------------- what the fusion is for
@pytest.mark.parametrize("size", [(70, 100), (33, 259)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_more_references_take_more_noise_out_and_leave_the_moving_block_alone(size):
    H, W = size
    noisy, clean = R.clip(H, W)

    def mse(a, b):
        return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()) * 255.0 ** 2

    source = mse(noisy[0], clean[0])
    for T, floor, P in R.SETTINGS:
        tab = R.table(T, floor)
        errs = [mse(FR.fuse(noisy[0], list(noisy[1:1 + n]), tab, P)[0], clean[0]) for n in (1, 2, 3, 4)]
        print(size, (T, floor, P), "source", source, "n = 1 .. 4", errs)
        assert source > errs[0] > errs[1] > errs[2] > errs[3], (T, floor, P, source, errs)
        assert errs[3] < source / 3, (T, floor, P, source, errs)
        # picture 5, where the block stands at columns 0 .. 19, against pictures 6 .. 8, where it has moved on
        out = FR.fuse(noisy[5], list(noisy[6:9]), tab, P)[0]
        block = (slice(None), slice(R.BLOCK_Y, min(R.BLOCK_Y + R.BLOCK, H)), slice(0, R.BLOCK))
        assert np.array_equal(_bits(out[block]), _bits(noisy[5][block])), (T, floor, P)
        assert not np.array_equal(out, noisy[5])


# ------------------------------------------------------------------------------------------------------ grain and the CLI
def test_grain_record_accepts_and_checks_intra():
    from vcm_ts_amd import grain as GR
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.scenecut import GopPlan

    plan = GopPlan.fixed(8, 4)
    gops = {g: GR.params([0] * GR.WORDS, 1024) for g in plan.i_pictures}
    plain = GR.record_of(GR.Grain(), N.TNR(8), gops)
    assert plain["tnr"] == {"threshold": 8, "floor": 64, "pixel": 24} and GR.check_record(plain, plan) is plain
    rec = GR.record_of(GR.Grain(), N.TNR(8, intra=2), gops)
    assert rec["tnr"]["intra"] == 2 and GR.check_record(rec, plan) is rec
    for bad in (0, 5, "2"):
        with pytest.raises(ValueError, match="intra"):
            GR.check_record(dict(rec, tnr=dict(rec["tnr"], intra=bad)), plan)


def test_command_line_refuses_intra_without_tnr(capsys):
    from vcm_ts_amd import run_codec as RC

    for argv, word in ((["--tnr-intra", "2"], "--tnr-intra belongs to --tnr"), (["--tnr", "8", "--tnr-intra", "5"], "intra"),
                       (["--tnr", "8", "--tnr-intra", "0"], "intra")):
        with pytest.raises(SystemExit) as ex:
            RC.main(["encode", "--frames", "nowhere", "--bins", "nowhere"] + argv)
        assert ex.value.code == 2 and word in capsys.readouterr().err, argv
