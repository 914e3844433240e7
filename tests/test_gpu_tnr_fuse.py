"""dcvc_tnr_fuse on a real MI355X: the kernel bit for bit against the numpy restatement (tests/tnr_fuse_ref.py) at n = 1 .. 4
in strided, offset, NaN-surrounded layouts with guarded outputs, in the manner of tests/test_gpu_tnr.py (whose sizes,
settings, layouts and sequences these are), on odd bit patterns, with unused references absent or poisoned, and its
refusals."""
import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import tnr_fuse_ref as FR
from tests import tnr_ref as R
from tests.test_gpu_tnr import LAYOUTS, SENT16, SENT32, _check_cells
from vcm_ts_amd import lib
from vcm_ts_amd import tnr as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
ORDER = ("cur", "crs", "cps", "ref0", "ref1", "ref2", "ref3", "rrs", "rps", "n", "out", "ors", "ops", "H", "W", "wtab", "rtab", "P",
         "sad", "held")


@pytest.fixture(scope="module")
def rtab():
    table = N.TNR.rcp_table()
    assert np.array_equal(table.view(np.uint32), FR.rcp_table().view(np.uint32))
    return torch.from_numpy(table).to(DEV)


def _tab(tab):
    return torch.from_numpy(np.asarray(tab, dtype=np.uint16).view(np.int16)).to(DEV)


def _fuse(cur, refs, tab_dev, rtab, P, H, W, layout, want, where, spare=None, any_nan=None):
    """One dcvc_tnr_fuse with n = len(refs) in `layout`, held against want = (out, sad, held).  spare: what the unused
    ref_j point at (None: NULL).  any_nan: a (3, H, W) mask of the samples where a NaN of the restatement need only be a
    NaN of the kernel (the header leaves the sign and payload of a NaN that arithmetic made to the machine)."""
    row_pad, plane_pad, offset, shift = layout
    hc, wc = R.grid(H, W)
    kc, vc, crs, cps, mask = U.strided(cur, H, W, row_pad, plane_pad, offset, DEV)
    held_refs = [U.strided(r, H, W, row_pad, plane_pad, offset, DEV) for r in refs]
    ko, vo, ors, ops, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    sad, s0 = U.guarded(hc * wc, shift, np.uint32, SENT32, DEV)  # (fresh sentinels every call: every cell is WRITTEN)
    held, h0 = U.guarded(hc * wc, shift, np.uint16, SENT16, DEV)
    ptrs = [r[1].data_ptr() for r in held_refs] + [spare] * (FR.MAX_REFS - len(refs))
    lib.check(lib.hip().dcvc_tnr_fuse(vc.data_ptr(), crs, cps, *ptrs, held_refs[0][2], held_refs[0][3], len(refs), vo.data_ptr(), ors, ops,
                                      H, W, tab_dev.data_ptr(), rtab.data_ptr(), P, sad.data_ptr() + 4 * s0, held.data_ptr() + 2 * h0,
                                      U.stream(DEV)), "tnr_fuse")
    got = ko.cpu().numpy()
    same = got[mask].view(np.uint32) == want[0].reshape(-1).view(np.uint32)
    if any_nan is not None:
        same |= any_nan.reshape(-1) & np.isnan(got[mask]) & np.isnan(want[0].reshape(-1))
    assert same.all(), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    _check_cells(sad, s0, hc * wc, want[1], SENT32, where)
    _check_cells(held, h0, hc * wc, want[2], SENT16, where)
    for k, pic in [(kc, cur)] + [(r[0], p) for r, p in zip(held_refs, refs)]:  # the inputs are only read
        assert np.array_equal(k.cpu().numpy()[mask].view(np.uint32), np.asarray(pic, F32).reshape(-1).view(np.uint32)), where


def _following(pics, t, n):
    """The n pictures that follow picture t, going round the sequence where it is shorter."""
    return [pics[(t + 1 + j) % len(pics)] for j in range(n)]


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_bit_for_bit(size, rtab):
    H, W = size
    seqs = R.sequences(H, W)
    for T, floor, P in R.SETTINGS:
        tab = N.TNR(T, floor, P).table()
        tab_dev = _tab(tab)
        for name, pics in seqs.items():
            for n in (1, 2, 3, 4):
                starts = (0, 5) if name == "clip" else (0,)  # (picture 5: the block stands where it will not stand again)
                for t in starts:
                    refs = _following(pics, t, n)
                    want = FR.fuse(pics[t], refs, tab, P)
                    for at, layout in enumerate(LAYOUTS):
                        if name != "clip" and at not in (0, 1 + (T + n + len(name)) % 3):  # (every layout on the clip, two on the others)
                            continue
                        _fuse(pics[t], refs, tab_dev, rtab, P, H, W, layout, want, (name, T, floor, P, n, t, layout))
                    out, sad, held = want
                    assert not sad[(H + 15) // 16:].any() and not sad[:, (W + 15) // 16:].any() and not held[(H + 15) // 16:].any()
                    if name == "equal":  # nothing differs: every reference weighs 256 - floor, and the mean of equals is the picture
                        assert not sad.any() and int(held.sum()) == H * W and np.array_equal(out, pics[t])
                    if name == "flip" and n == 1:  # everything differs by 255 codes: the bits of cur
                        assert not held.any() and int(sad.sum()) == 255 * H * W and np.array_equal(out, pics[t])
        # a at T - 1 | T and d at P | P + 1 side by side, written by the host.  The pattern lives in the difference: cur is
        # the zero picture, and each of the n references is a different such picture, the pattern moved on by j columns
        zero = np.zeros((3, H, W), F32)
        patterns = [np.roll(R.edge_case(H, W, T, P)[0], j, axis=2) for j in range(4)]
        for n in (1, 2, 3, 4):
            want = FR.fuse(zero, patterns[:n], tab, P)
            for layout in LAYOUTS[:2]:
                _fuse(zero, patterns[:n], tab_dev, rtab, P, H, W, layout, want, ("edge", T, floor, P, n, layout))
        d, a, w = R.weights(zero, patterns[0], tab, P)
        if H >= 6 and W >= 9:
            assert {T - 1, T} <= set(a[:(H + 1) // 2].ravel().tolist())
        if H >= 2 and W >= 2 and P < 255:
            low = d[(H + 1) // 2:]
            assert set(low.ravel().tolist()) == {P, P + 1} and (w[(H + 1) // 2:][low > P] == 256).all()


def _odd(H, W, seed):
    """A noisy clip picture with NaN, -0.0, values outside [0, 1], infinities and float32 subnormals sprinkled over it."""
    g = np.random.default_rng(seed)
    pic = R.clip(H, W, seed=seed)[0][0].copy()
    special = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000],
                       dtype=np.uint32).view(F32)
    special = np.concatenate([special, np.array([-0.25, 1.5, 3.0e38, -7.0], F32)])
    at = g.random(pic.shape) < 0.02
    pic[at] = g.choice(special, int(at.sum()))
    return pic


def test_odd_bit_patterns_in_cur_and_in_single_references(rtab):
    """T = 64 and P = 255: nothing is guarded and a window with an odd sample or two in it still blends, so odd samples
    take part in the arithmetic and are not only copied.  Every bit is the restatement's, but for a NaN that the blend
    itself made or passed on (a pixel with U > 0): IEEE 754 leaves its sign and payload open, the header says nothing of
    them, and numpy on the host and the GPU choose differently (inf - inf is one such).  Where U == 0 the bits of cur are
    held, NaNs included."""
    H, W = 33, 259
    clean = list(R.clip(H, W)[0][:5])
    T, floor, P = 64, 32, 255
    tab = R.table(T, floor)
    tab_dev = _tab(tab)
    cases = {"cur": (_odd(H, W, 21), clean[1:5])}
    for j in range(4):
        refs = list(clean[1:5])
        refs[j] = _odd(H, W, 30 + j)
        cases[f"ref{j}"] = (clean[0], refs)
    cases["all"] = (_odd(H, W, 21), [_odd(H, W, 30 + j) for j in range(4)])
    for name, (cur, refs) in cases.items():
        for n in (1, 4) if name in ("cur", "all") else (4,):
            want = FR.fuse(cur, refs[:n], tab, P)
            blended = sum(256 - R.weights(cur, r, tab, P)[2] for r in refs[:n]) > 0
            odd = ~np.isfinite(cur) | (np.abs(cur) < F32(1e-37)) | (cur < 0) | (cur > 1)
            for r in refs[:n]:
                odd |= ~np.isfinite(r) | (np.abs(r) < F32(1e-37)) | (r < 0) | (r > 1)
            assert (odd & blended[None]).sum() > 20, name  # odd samples do take part
            assert np.array_equal(want[0].view(np.uint32)[:, ~blended], np.ascontiguousarray(cur).view(np.uint32)[:, ~blended])
            for layout in LAYOUTS[:2]:
                _fuse(cur, refs[:n], tab_dev, rtab, P, H, W, layout, want, (name, n, layout),
                      any_nan=np.broadcast_to(blended[None], cur.shape).copy())


def test_unused_references_are_ignored_and_a_full_table_copies_cur(rtab):
    H, W = 17, 67
    pics = R.sequences(H, W)["clip"]
    T, floor, P = R.SETTINGS[0]
    tab = R.table(T, floor)
    nan_buf = torch.full((8 * (H + 2) * (W + 16),), float("nan"), device=DEV)  # (room for three planes in either layout)
    for n in (1, 2, 3):
        want = FR.fuse(pics[0], pics[1:1 + n], tab, P)
        for spare in (None, nan_buf.data_ptr()):
            _fuse(pics[0], pics[1:1 + n], _tab(tab), rtab, P, H, W, LAYOUTS[0], want, (n, spare is None), spare=spare)
    full = np.full(256, 256, np.uint16)  # every weight 256: no reference weighs anything
    for n in (1, 4):
        want = FR.fuse(pics[0], pics[1:1 + n], full, P)
        assert np.array_equal(want[0].view(np.uint32), pics[0].view(np.uint32)) and not want[2].any() and want[1].any()
        _fuse(pics[0], pics[1:1 + n], _tab(full), rtab, P, H, W, LAYOUTS[1], want, ("full", n))


def test_entry_point_refusals_leave_the_outputs_alone(rtab):
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    pics = R.sequences(H, W)["clip"]
    kc, vc, crs, cps, mask = U.strided(pics[0], H, W, 8, 24, 12, DEV)
    refs = [U.strided(pics[1 + j], H, W, 8, 24, 12, DEV) for j in range(4)]
    ko, vo, ors, ops, _ = U.strided(None, H, W, 8, 24, 12, DEV)
    sad, s0 = U.guarded(hc * wc, 0, np.uint32, SENT32, DEV)
    held, h0 = U.guarded(hc * wc, 0, np.uint16, SENT16, DEV)
    tab = _tab(R.table(12, 64))
    good = dict(cur=vc.data_ptr(), crs=crs, cps=cps, ref0=refs[0][1].data_ptr(), ref1=refs[1][1].data_ptr(), ref2=refs[2][1].data_ptr(),
                ref3=refs[3][1].data_ptr(), rrs=refs[0][2], rps=refs[0][3], n=4, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W,
                wtab=tab.data_ptr(), rtab=rtab.data_ptr(), P=36, sad=sad.data_ptr() + 4 * s0, held=held.data_ptr() + 2 * h0)
    span = 4 * (2 * cps + (H - 1) * crs + W)
    names = ("ref0", "ref1", "ref2", "ref3")
    bad = [{k: None} for k in ("cur", "out", "wtab", "rtab", "sad", "held") + names] + \
          [{"n": 0}, {"n": 5}, {"n": -1}, {"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"P": -1}, {"P": 256}] + \
          [{k: W - 1} for k in ("crs", "rrs", "ors")] + [{k: (H - 1) * crs + W - 1} for k in ("cps", "rps", "ops")] + \
          [{k: good[k] + 2} for k in ("cur", "out", "sad", "rtab") + names] + [{k: good[k] + 1} for k in ("wtab", "held")] + \
          [{"out": good["cur"]}, {"out": good["cur"] + span - 4}, {"cur": good["out"] + 4 * ops}] + \
          [{"out": good[k]} for k in names] + [{"out": good[k] - span + 4} for k in names] + \
          [{k: good["out"] + 4 * (H - 1) * ors} for k in names] + \
          [{"n": 2, "ref1": None}, {"n": 3, "ref2": good["out"]}]  # (what n leaves out is not looked at; what it takes in is)
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_tnr_fuse(*[v[k] for k in ORDER], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(sad) == SENT32).all() and (U.words(held) == SENT16).all()
    assert np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_tnr_fuse(*[good[k] for k in ORDER], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = FR.fuse(pics[0], pics[1:5], R.table(12, 64), 36)
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), want[0].reshape(-1).view(np.uint32))
    _check_cells(sad, s0, hc * wc, want[1], SENT32, "good")
    _check_cells(held, h0, hc * wc, want[2], SENT16, "good")
    # an unused reference may be anything, out itself included; the references may alias each other and cur
    v = dict(good, n=2, ref2=good["out"], ref3=None)
    assert lib.hip().dcvc_tnr_fuse(*[v[k] for k in ORDER], U.stream(DEV)) == 0
    want = FR.fuse(pics[0], pics[1:3], R.table(12, 64), 36)
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), want[0].reshape(-1).view(np.uint32))
    v = dict(good, n=3, ref0=good["cur"], ref2=good["ref1"])
    assert lib.hip().dcvc_tnr_fuse(*[v[k] for k in ORDER], U.stream(DEV)) == 0
    want = FR.fuse(pics[0], [pics[0], pics[2], pics[2]], R.table(12, 64), 36)
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), want[0].reshape(-1).view(np.uint32))
    _check_cells(sad, s0, hc * wc, np.zeros(hc * wc), SENT32, "ref0 is cur")
    _check_cells(held, h0, hc * wc, want[2], SENT16, "ref0 is cur")
