"""The hierarchical motion search on a real MI355X: dcvc_me_pyramid, dcvc_me_coarse and dcvc_me_descend bit for bit against
the numpy restatement (tests/mepyr_ref.py) in tests/test_gpu_me.py's strided, offset, NaN-surrounded layouts with guarded
outputs and guarded byte planes, the chain of launches on the fast clip, TnrFilter(levels=...) with and without the
look-ahead, the refinement and the re-selection, TnrFilter without it, and the file loops end to end: the pictures the codec
is handed, an unchanged decoder, the report, two GOP streams, the command line."""
import json

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import me_ref as M
from tests import mepyr_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from tests.test_gpu_me import LAYOUTS, SENT16, SENT32, _cells, _handed, _padded, _spy, _tensors
from vcm_ts_amd import devargs, lib
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
SENT8 = 0xA5
CASES = ((1, 2), (1, 7), (1, 64), (2, 4), (2, 9), (2, 128))  # (levels, R)


def _sides(H, W, level):
    for _ in range(level):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W


class _Plane:
    """One level's byte plane on the device inside guard bytes of its own: rows of stride = the width rounded up to 4 plus
    4 * pad bytes, the first pixel 4 * shift bytes further into the buffer; every byte that is no pixel holds SENT8."""

    def __init__(self, H, W, level, pad, shift, values=None):
        self.h, self.w = _sides(H, W, level)
        self.stride = -(-self.w // 4) * 4 + 4 * pad
        self.buf, self.first = U.guarded(self.h * self.stride, 4 * shift, np.uint8, SENT8, DEV)
        if values is not None:
            rows = self.buf[self.first:self.first + self.h * self.stride].view(self.h, self.stride)
            rows[:, :self.w] = torch.from_numpy(np.asarray(values).astype(np.uint8).view(np.int8)).to(DEV)
        self.ptr = self.buf.data_ptr() + self.first

    def holds(self, want, where):
        """The pixels are `want` (None: untouched), and nothing beside them was written."""
        got = U.words(self.buf)
        rows = got[self.first:self.first + self.h * self.stride].reshape(self.h, self.stride)
        assert np.array_equal(rows[:, :self.w], np.full((self.h, self.w), SENT8) if want is None else want), where
        assert (rows[:, self.w:] == SENT8).all() and U.guards_intact(self.buf, self.first, self.h * self.stride, SENT8), where


def _planes(H, W, levels, layout, values=None):
    shift = layout[3]
    return [_Plane(H, W, level, (shift + level) % 3, shift, None if values is None else values[level]) for level in range(levels + 1)]


def _pyramid(pic, H, W, levels, layout, where):
    """One dcvc_me_pyramid in `layout`, held against the restatement on the bits the device holds."""
    row_pad, plane_pad, offset, _ = layout
    kp, vp, rs, ps, mask = U.strided(pic, H, W, row_pad, plane_pad, offset, DEV)
    before = kp.cpu().numpy()
    want = R.pyramid(before[mask].reshape(3, H, W), levels)
    y = _planes(H, W, 2, layout)
    lib.check(lib.hip().dcvc_me_pyramid(vp.data_ptr(), rs, ps, H, W, levels, y[0].ptr, y[0].stride, y[1].ptr, y[1].stride,
                                        y[2].ptr if levels == 2 else None, y[2].stride if levels == 2 else 0, U.stream(DEV)), "me_pyramid")
    for level in range(3):
        y[level].holds(want[level] if level <= levels else None, (where, level))
    assert np.array_equal(kp.cpu().numpy().view(np.uint32), before.view(np.uint32)), where  # the picture is only read
    return want


@pytest.mark.parametrize("size", list(M.SIZES) + [(48, 600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_equals_the_restatement(size):
    H, W = size
    g = np.random.default_rng(H + 1000 * W)
    pics = {"random": g.uniform(-0.1, 1.1, (3, H, W)).astype(F32), "odd bits": M.odd_bits(H, W), "clip": M.clip(H, W)[0][5],
            "period4": M.period4(H, W)[0], "ones": np.ones((3, H, W), F32)}
    for name, pic in pics.items():
        for levels in (1, 2):
            for k, layout in enumerate(LAYOUTS):
                if name not in ("random", "odd bits") and k != (levels + len(name)) % 4:
                    continue
                want = _pyramid(pic, H, W, levels, layout, (name, levels, layout))
                assert [a.shape for a in want] == [_sides(H, W, level) for level in range(levels + 1)]
                if name == "ones":
                    assert all((a == 255).all() for a in want)
                if name == "period4" and W >= 8:  # the means of 40, 80 and of 120, 160; their mean
                    assert set(np.unique(want[1][:, :W // 2])) == {60, 140} and (levels == 1 or (want[2][:, :W // 4] == 100).all())


def _vectors(values, n, shift):
    mv, m0 = U.guarded(2 * n, shift, np.uint16, SENT16, DEV)
    if values is not None:
        mv[m0:m0 + 2 * n] = torch.from_numpy(np.asarray(values).astype(np.int16).reshape(-1)).to(DEV)
    return mv, m0


def _coarse(yc, yr, H, W, radius, levels, lam, layout, want, where):
    """One dcvc_me_coarse on the level's planes yc, yr (arrays of codes), held against want (hc, wc, 2)."""
    n = int(np.prod(R.grid(H, W)))
    pc, pr = (_Plane(H, W, levels, k, layout[3], v) for k, v in ((1, yc), (2, yr)))
    mv, m0 = _vectors(None, n, layout[3])
    lib.check(lib.hip().dcvc_me_coarse(pc.ptr, pc.stride, pr.ptr, pr.stride, H, W, radius, levels, lam, mv.data_ptr() + 2 * m0, U.stream(DEV)),
              "me_coarse")
    _cells(mv, m0, 2 * n, want, SENT16, where)
    pc.holds(yc, where), pr.holds(yr, where)  # the planes are only read


def _descend(yc, yr, H, W, radius, levels, level, lam, p, layout, want, where):
    """One dcvc_me_descend to `level` from the vectors p, held against want = (mv, cost, zero)."""
    n = int(np.prod(R.grid(H, W)))
    pc, pr = (_Plane(H, W, level, k, layout[3], v) for k, v in ((2, yc), (0, yr)))
    mv_in, i0 = _vectors(p, n, layout[3])
    mv, m0 = _vectors(None, n, layout[3])
    cost, c0 = U.guarded(n, layout[3], np.uint32, SENT32, DEV)
    zero, z0 = U.guarded(n, layout[3], np.uint32, SENT32, DEV)
    lib.check(lib.hip().dcvc_me_descend(pc.ptr, pc.stride, pr.ptr, pr.stride, H, W, radius, levels, level, lam, mv_in.data_ptr() + 2 * i0,
                                        mv.data_ptr() + 2 * m0, cost.data_ptr() + 4 * c0, zero.data_ptr() + 4 * z0, U.stream(DEV)), "me_descend")
    _cells(mv, m0, 2 * n, want[0], SENT16, where)
    if level == 0:
        _cells(cost, c0, n, want[1], SENT32, where)
        _cells(zero, z0, n, want[2], SENT32, where)
    else:  # at level 1 cost and zero are ignored
        assert (U.words(cost) == SENT32).all() and (U.words(zero) == SENT32).all(), where
    _cells(mv_in, i0, 2 * n, p, SENT16, where)
    pc.holds(yc, where), pr.holds(yr, where)


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coarse_and_descents_equal_the_restatement(size):
    H, W = size
    for levels, radius in CASES:
        pairs = M.pairs(H, W, radius)
        if radius >= 64:  # (the brute force over 4225 candidates: one pair of each kind)
            pairs = {name: todo[:1] for name, todo in pairs.items()}
        for name, todo in pairs.items():
            for n, (cur, ref) in enumerate(todo):
                yc, yr = R.pyramid(cur, levels), R.pyramid(ref, levels)
                table = R.coarse_sads(cur, ref, radius, levels)
                for lam in M.LAMBDAS:
                    layout = LAYOUTS[(lam + n + len(name) + levels) % 4]
                    want = R.stages(cur, ref, radius, lam, levels, table)
                    where = (name, n, levels, radius, lam, layout)
                    _coarse(yc[levels], yr[levels], H, W, radius, levels, lam, layout, want[0], where)
                    if levels == 2:
                        _descend(yc[1], yr[1], H, W, radius, 2, 1, lam, want[0], layout, (want[1], None, None), where)
                    _descend(yc[0], yr[0], H, W, radius, levels, 0, lam, want[-2], layout, want[-1], where)
                    if name == "flat":
                        assert not any(v.any() for v in want[:-1]) and not want[-1][0].any()


@pytest.mark.parametrize("size", [(17, 67), (33, 259), (70, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_planes_and_incoming_vectors_that_the_clamps_must_bound(size):
    H, W = size
    for levels, radius in ((1, 24), (2, 24), (2, 128), (1, 64)):
        yc, yr = R.random_planes(H, W, levels)
        h, w = _sides(H, W, levels)
        edge = np.pad(yr, R.level_range(radius, levels), mode="edge")
        RL, sup = R.level_range(radius, levels), R.supports(H, W, levels, True)
        table = {(dy, dx): R.support_sums(np.abs(yc - edge[RL + dy:RL + dy + h, RL + dx:RL + dx + w]), sup) for dy, dx in M.candidates(RL)}
        for lam in (0, 4):
            want = R.coarse(table, H, W, radius, lam, levels)
            assert np.abs(want).max() >= 2
            _coarse(yc, yr, H, W, radius, levels, lam, LAYOUTS[lam % 4], want, ("random", levels, radius, lam))
        for level in range(levels):
            yc, yr = R.random_planes(H, W, level)
            for k, p in enumerate((R.wild_vectors(H, W, R.level_range(radius, level + 1)), R.wild_vectors(H, W, 3, seed=37))):
                for lam in (0, 255):
                    want = R.descend(yc, yr, H, W, radius, lam, level, p)
                    assert np.abs(p).max() == 32768 and np.abs(want[0]).max() <= R.level_range(radius, level)
                    _descend(yc, yr, H, W, radius, levels, level, lam, p, LAYOUTS[(k + lam + level) % 4], want, ("wild", levels, radius, level, lam, k))


def _chain(cur, ref, radius, levels, lam):
    """The launches TnrFilter makes in place of dcvc_me_search, on dense pictures: (mv, cost, zero) as int64 arrays."""
    H, W = cur.shape[1:]
    hc, wc = R.grid(H, W)
    hip, st = lib.hip(), U.stream(DEV)
    pics = [U.to_dev(p, DEV) for p in (cur, ref)]
    y = [[torch.empty((_sides(H, W, l)[0], -(-_sides(H, W, l)[1] // 4) * 4), dtype=torch.uint8, device=DEV) for l in range(levels + 1)] for _ in pics]
    for pic, planes in zip(pics, y):
        extra = (planes[2].data_ptr(), planes[2].shape[1]) if levels == 2 else (None, 0)
        lib.check(hip.dcvc_me_pyramid(pic.data_ptr(), W, H * W, H, W, levels, planes[0].data_ptr(), planes[0].shape[1], planes[1].data_ptr(),
                                      planes[1].shape[1], *extra, st), "me_pyramid")
    vec = [torch.empty(2 * hc * wc, dtype=torch.int16, device=DEV) for _ in range(levels + 1)]
    cost, zero = (torch.empty(hc * wc, dtype=torch.int32, device=DEV) for _ in range(2))
    lib.check(hip.dcvc_me_coarse(y[0][levels].data_ptr(), y[0][levels].shape[1], y[1][levels].data_ptr(), y[1][levels].shape[1], H, W, radius,
                                 levels, lam, vec[levels].data_ptr(), st), "me_coarse")
    for level in range(levels - 1, -1, -1):
        out = (cost.data_ptr(), zero.data_ptr()) if level == 0 else (None, None)
        lib.check(hip.dcvc_me_descend(y[0][level].data_ptr(), y[0][level].shape[1], y[1][level].data_ptr(), y[1][level].shape[1], H, W, radius,
                                      levels, level, lam, vec[level + 1].data_ptr(), vec[level].data_ptr(), *out, st), "me_descend")
    return vec[0].cpu().numpy().astype(np.int64).reshape(hc, wc, 2), U.words(cost).reshape(hc, wc), U.words(zero).reshape(hc, wc)


@pytest.mark.parametrize("case", [(1, 64), (2, 64), (2, 128)], ids=lambda c: f"L{c[0]}-R{c[1]}")
def test_the_chain_of_launches_on_the_fast_clip(case):
    levels, radius = case
    step = R.FAST_STEPS[1]  # (3, 61) pixels a picture
    noisy = R.fast_clip(step)[0]
    for t in (2, 3):
        want = R.search(noisy[t], noisy[t - 1], radius, R.PENALTY, levels)
        for a, b in zip(_chain(noisy[t], noisy[t - 1], radius, levels, R.PENALTY), want):
            assert np.array_equal(a, b), t
        assert R.far(want[0]) > 0  # (the object's cells, 61 pixels a picture)


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    n = int(np.prod(R.grid(H, W)))
    noisy = M.clip(H, W)[0]
    kp, vp, rs, ps, _ = U.strided(noisy[5], H, W, 8, 24, 12, DEV)
    y = _planes(H, W, 2, LAYOUTS[0])
    good = dict(pic=vp.data_ptr(), rs=rs, ps=ps, H=H, W=W, L=2, y0=y[0].ptr, s0=y[0].stride, y1=y[1].ptr, s1=y[1].stride, y2=y[2].ptr, s2=y[2].stride)
    order = ("pic", "rs", "ps", "H", "W", "L", "y0", "s0", "y1", "s1", "y2", "s2")
    bad = [{k: None} for k in ("pic", "y0", "y1", "y2")] + [{"H": 0}, {"W": 32769}, {"L": 0}, {"L": 3}, {"rs": W - 1}, {"ps": (H - 1) * rs + W - 1}] + \
          [{k: good[k] + 2} for k in ("pic", "y0", "y1", "y2")] + [{"s0": 96}, {"s1": 50}, {"s2": 24}, {"s2": 26}] + \
          [{"y1": good["y0"]}, {"y2": good["y0"] + 4 * 25}, {"y1": good["y0"] + 69 * good["s0"] + 96}, {"y0": good["pic"]}, {"y2": good["pic"] + 4 * ps}]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_pyramid(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    for p in y:
        p.holds(None, "refused")
    assert lib.hip().dcvc_me_pyramid(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.pyramid(noisy[5], 2)
    for level in range(3):
        y[level].holds(want[level], "good")
    mv, m0 = _vectors(None, n, 0)
    mv1, i0 = _vectors(np.zeros((n, 2)), n, 0)
    cost, c0 = U.guarded(n, 0, np.uint32, SENT32, DEV)
    good = dict(cur=y[2].ptr, cs=y[2].stride, ref=y[2].ptr, rs=y[2].stride, H=H, W=W, R=64, L=2, lam=4, mv=mv.data_ptr() + 2 * m0)
    order = ("cur", "cs", "ref", "rs", "H", "W", "R", "L", "lam", "mv")
    for b in [{k: None} for k in ("cur", "ref", "mv")] + [{"R": 3}, {"R": 129}, {"L": 1}, {"L": 3}, {"lam": 256}, {"cs": 24}, {"rs": 26},
                                                          {"cur": good["cur"] + 2}, {"mv": good["mv"] + 1}, {"H": 0}]:
        v = dict(good, **b)
        assert lib.hip().dcvc_me_coarse(*[v[k] for k in order], U.stream(DEV)) == -1, b
    good = dict(cur=y[0].ptr, cs=y[0].stride, ref=y[0].ptr, rs=y[0].stride, H=H, W=W, R=64, L=2, level=0, lam=4, mv_in=mv1.data_ptr() + 2 * i0,
                mv=mv.data_ptr() + 2 * m0, cost=cost.data_ptr() + 4 * c0, zero=cost.data_ptr() + 4 * c0)
    order = ("cur", "cs", "ref", "rs", "H", "W", "R", "L", "level", "lam", "mv_in", "mv", "cost", "zero")
    for b in [{k: None} for k in ("cur", "ref", "mv_in", "mv", "cost", "zero")] + [{"R": 3}, {"level": 2}, {"level": -1}, {"level": 1, "cs": 48}, {"lam": -1},
                                                                                 {"cs": 96}, {"mv": good["mv_in"]}, {"cost": good["cost"] + 2}]:
        v = dict(good, **b)  # (48: below level 1's width)
        assert lib.hip().dcvc_me_descend(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(mv) == SENT16).all() and (U.words(cost) == SENT32).all()


# ------------------------------------------------------------------------------------------------------------ TnrFilter
PLAIN = ["bufs", "wtab", "sad", "held", "_rows", "comp", "mv", "cost", "zero"]


@pytest.mark.parametrize("case", [(1, 16), (2, 64)], ids=lambda c: f"L{c[0]}-R{c[1]}")
def test_filter_with_levels_equals_the_restatement(case):
    levels, radius = case
    H, W, Hp, Wp = 70, 100, 128, 128
    pics, setting, intra = list(M.clip(H, W)[0]), R.SETTING, {0, 4}
    want = R.run(pics, setting, intra, radius, R.PENALTY, levels)
    f = N.TnrFilter(N.TNR(*setting, search=radius, levels=levels), (H, W), DEV)
    assert f.launches == 0 and f.untouched == (0,) * 5 and _tensors(f) == sorted(PLAIN + ["ycur", "yref", "mvl"])
    assert [tuple(p.shape) for p in f.ycur] == [(70, 100), (35, 52), (18, 28)][:levels + 1] and len(f.mvl) == levels
    got, launches = [], []
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        y = f.step(x, t in intra)
        assert (y is x) == (t in intra), t
        launches.append(f.launches)
        got.append(y.cpu().numpy())
        if t not in intra:
            assert np.array_equal(f.mv.cpu().numpy().astype(np.int64), want[t][3].reshape(-1)), t
            assert np.array_equal(U.words(f.cost), want[t][4].reshape(-1)) and np.array_equal(U.words(f.zero), want[t][5].reshape(-1)), t
            for level, plane in enumerate(f.ycur):  # the byte planes of the picture just filtered
                h, w = _sides(H, W, level)
                assert np.array_equal(U.words(plane)[:, :w], R.pyramid(pics[t], levels)[level]), (t, level)
    per = 5 + levels  # a P picture: pyramid, pyramid, coarse, [descend,] descend, compensate, step
    assert launches == [0, per, 2 * per, 3 * per, 3 * per, 4 * per, 5 * per, 6 * per]
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [R.totals(w, H, W) for w in want] and f.totals()[4] == (0,) * 5 and f.totals()[5][2] > 0
    bare = N.TnrFilter(N.TNR(*setting, search=radius, levels=levels), (H, W), DEV, totals=False)
    for t, pic in enumerate(pics[:3]):
        y = bare.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), got[t].view(np.uint32)), t
    assert bare.launches == 2 * per and bare._rows is None


def test_far_counts_the_cells_beyond_the_full_searchs_reach():
    H, W = R.FAST_SIZE
    Hp, Wp = 128, 320
    step = R.FAST_STEPS[0]
    pics = list(R.fast_clip(step)[0][:3])
    want = R.run(pics, R.SETTING, {0}, 128, R.PENALTY, 2)
    f = N.TnrFilter(N.TNR(*R.SETTING, search=128, levels=2), (H, W), DEV)
    for t, pic in enumerate(pics):
        y = f.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t == 0)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [R.totals(w, H, W) for w in want]
    assert [row[4] for row in f.totals()][0] == 0 and all(row[4] >= 3 for row in f.totals()[1:])  # the object's cells, 50 pixels a picture


def test_filter_with_levels_and_look_ahead_equals_the_restatement():
    H, W, Hp, Wp, K, levels, radius = 70, 100, 128, 128, 2, 2, 64
    pics, setting, intra = list(M.clip(H, W)[0]), R.SETTING, {0, 4}
    want = R.run_intra(pics, setting, intra, K, radius, R.PENALTY, levels)
    f = N.TnrFilter(N.TNR(*setting, search=radius, intra=K, levels=levels), (H, W), DEV)
    assert f.untouched == (0,) * 6 and len(f.yrefs) == 4 and len(f.mvls) == 4 and f.yref is f.yrefs[0] and f.mvl is f.mvls[0]
    xs = [torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV) for pic in pics]
    launches, got = [], []
    for t, x in enumerate(xs):
        ahead = []
        for s in range(t + 1, len(xs)):
            if s in intra:
                break
            ahead.append(xs[s])
        before = f.launches
        got.append(f.step(x, t in intra, ahead).cpu().numpy())
        launches.append(f.launches - before)
    assert [w[3] for w in want] == [2, 1, 1, 1, 2, 1, 1, 1]
    # the I source's pyramid once; per reference pyramid, coarse, descend, descend, compensate; ONE blend
    assert launches == [1 + (3 + levels) * w[3] + 1 for w in want]
    for t in range(len(pics)):
        assert np.array_equal(got[t].view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
    assert f.totals() == [(int(w[2].sum()), int(w[1].sum())) + tuple(w[4:]) + (w[3],) for w in want]


def test_the_refinement_and_the_re_selection_work_unchanged_behind_the_pyramid():
    from tests import mesplit_ref as P
    from tests import mesub_ref as S

    H, W, Hp, Wp, levels, radius = 70, 100, 128, 128, 2, 16
    pics, intra = list(S.subpel_clip((2.25, 5.5), size=(H, W))[0][:6]), {0, 4}
    want = R.run_refined(pics, R.SETTING, intra, radius, R.PENALTY, levels)
    f = N.TnrFilter(N.TNR(*R.SETTING, search=radius, subpel=True, split=True, levels=levels), (H, W), DEV)
    assert f.untouched == (0,) * 7
    for t, pic in enumerate(pics):
        y = f.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t in intra)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(want[t][0], Hp, Wp).view(np.uint32)), t
        if t not in intra:
            assert np.array_equal(f.mv8.cpu().numpy().astype(np.int64), want[t][6].reshape(-1)), t
    assert f.launches == 4 * (7 + levels)  # pyramid, pyramid, coarse, descend, descend, refine, split, compensate_split, step
    assert f.totals() == [P.totals(w, H, W) + (R.far(w[8]),) for w in want]
    assert any(w[3].any() for w in want)


def test_filter_without_levels_owns_and_launches_what_it_did(monkeypatch):
    H, W, Hp, Wp = 70, 100, 128, 128
    names = []
    launch = devargs.launch
    monkeypatch.setattr(devargs, "launch", lambda name, *a, **kw: names.append(name) or launch(name, *a, **kw))
    pics = M.clip(H, W)[0][:3]
    for kw, step in ((dict(), ["dcvc_tnr_step"]), (dict(search=8), ["dcvc_me_search", "dcvc_me_compensate", "dcvc_tnr_step"]),
                     (dict(search=8, subpel=True, split=True),
                      ["dcvc_me_search", "dcvc_me_refine", "dcvc_me_split", "dcvc_me_compensate_split", "dcvc_tnr_step"]),
                     (dict(search=8, levels=1), ["dcvc_me_pyramid", "dcvc_me_pyramid", "dcvc_me_coarse", "dcvc_me_descend", "dcvc_me_compensate",
                                                 "dcvc_tnr_step"])):
        del names[:]
        f = N.TnrFilter(N.TNR(*R.SETTING, **kw), (H, W), DEV)
        if "levels" not in kw:
            assert not any(hasattr(f, k) for k in ("ycur", "yref", "yrefs", "mvl", "mvls"))
            assert _tensors(f) == sorted((PLAIN if kw else PLAIN[:5]) + (["mvq", "costq", "mv8", "cost8"] if "split" in kw else []))
        for t, pic in enumerate(pics):
            f.step(torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV), t == 0)
        assert names == 2 * step and f.launches == len(names), kw
        assert len(f.totals()[1]) == len(f.untouched) == {0: 2, 1: 4, 3: 6, 2: 5}[len(kw)]


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW, RH, RW = 4, 8, 96, 128, 176, 192
SEARCH, LEVELS = 64, 2
SETTING = N.TNR(8, search=SEARCH, levels=LEVELS)
TUPLE = (8, 64, 24)  # (T, floor, P = min(255, 3 T)) of --tnr 8
INTRA = {0, 4}


def _write_pngs(folder, size):
    """The noisy clip as PNGs -> what u8_to_unit_float uploads of them, (3, H, W) float32 each."""
    u8 = np.rint(M.clip(*size)[0][:N_FRAMES] * 255).astype(np.uint8)
    U.write_pngs(folder, u8.transpose(0, 2, 3, 1))
    return [a.astype(F32) / F32(255.0) for a in u8]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the 96 x 128 clip as PNGs, coded with the hierarchical search in front of the prefilter"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("mepyr_e2e")
    pics = _write_pngs(tmp / "png", (FH, FW))
    with _spy() as seen:
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "pyr"), str(tmp / "pyr_rec"), gop=GOP, nets=file_nets, picture_hash=True, tnr=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, seen=seen, want=R.run(pics, TUPLE, INTRA, SEARCH, R.PENALTY, LEVELS))


def test_the_codec_is_handed_the_restatements_pictures(e2e):
    _handed(e2e["seen"], e2e["want"], FH, FW)
    assert any(w[3].any() for w in e2e["want"])  # (and the search found the object)


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert U.others(tmp / "pyr") == ["hashes.json"]  # no side file of the filter or the search
    assert RC.decode_folder(str(tmp / "pyr"), str(tmp / "pyr_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "pyr_dec", tmp / "pyr_rec", N_FRAMES)


def test_two_gop_streams_and_the_command_line_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spy() as seen:
        RC.encode_folder(str(tmp / "png"), str(tmp / "pyr2"), gop=GOP, nets=file_nets, gop_streams=2, tnr=SETTING)
    assert U.bins(tmp / "pyr2") == U.bins(tmp / "pyr")
    _handed(seen, e2e["want"], FH, FW)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "8", "--tnr-search", "64",
             "--tnr-levels", "2", "--picture-hash"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "pyr")
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "pyr_rec", N_FRAMES)


def test_report_speaks_of_the_far_cells(tmp_path, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path
    pics = _write_pngs(tmp / "png", (RH, RW))
    want = R.run(pics, TUPLE, INTRA, SEARCH, R.PENALTY, LEVELS)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "8", "--tnr-search", "64",
             "--tnr-levels", "2", "--report", str(tmp / "cli.json")])
    rd = json.loads((tmp / "cli.json").read_text())
    cells = M.cells_with_a_pixel(RH, RW)
    assert rd["tnr"] == {"threshold": 8, "floor": 64, "pixel": 24, "search": 64, "penalty": 4, "levels": 2}
    for key, column, per in (("frame_tnr_held", 0, RH * RW), ("frame_tnr_mad", 1, RH * RW), ("frame_tnr_moved", 2, cells),
                             ("frame_tnr_mad_zero", 3, RH * RW), ("frame_tnr_far", 4, cells)):
        assert rd[key] == [R.totals(w, RH, RW)[column] / per for w in want], key
    assert all(rd["frame_tnr_far"][t] == 0.0 for t in INTRA) and any(v > 0 for v in rd["frame_tnr_moved"])
    with _spy() as seen:
        _, _, full_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "full"), gop=GOP, nets=file_nets, report=True, tnr=N.TNR(8, search=8))
    assert set(rd) - set(full_rd) == {"frame_tnr_far"} and set(full_rd) <= set(rd) and "levels" not in full_rd["tnr"]
    _handed(seen, M.run(pics, TUPLE, INTRA, 8, R.PENALTY), RH, RW)  # without the option: the full search's pictures, as ever
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "pyr2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, tnr=SETTING)
    assert U.bins(tmp / "pyr2") == U.bins(tmp / "cli")
    for key in ("tnr", "frame_tnr_held", "frame_tnr_mad", "frame_tnr_moved", "frame_tnr_mad_zero", "frame_tnr_far", "frame_bpp"):
        assert rd2[key] == rd[key], key
