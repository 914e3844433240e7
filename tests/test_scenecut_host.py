"""Scene-cut I pictures, the parts that need no GPU: the numpy restatement of include/dcvc_hip_scene.h
(tests/scenecut_ref.py) against itself, vcm_ts_amd/scenecut.py's plan rule and GopPlan, the entry point's refusals (a refused
call launches nothing), and the separation of the pictures tests/test_gpu_scenecut.py relies on.
"""
import os

import numpy as np
import pytest

from tests import scenecut_ref as R
from vcm_ts_amd import scenecut as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 5), (65, 63), (64, 96)]


# ------------------------------------------------------------------------------------------------------- restatement
def test_restatement_distance_of_a_picture_with_itself_and_of_black_with_white():
    for H, W in SIZES:
        p = R.wide_picture(3, H, W)
        assert R.distance(R.hist(p), R.hist(p), H, W) == 0.0
        zero, one = np.zeros((3, H, W), np.float32), np.ones((3, H, W), np.float32)
        assert R.distance(R.hist(zero), R.hist(one), H, W) == 1.0
    assert R.luma(255, 255, 255) == 255 and R.luma(0, 0, 0) == 0
    assert 54 + 183 + 19 == 256
    # rint is round-half-to-even on the float32 product, and both clamps act
    assert R.code(np.float32([-0.5, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1.0, 1.5])).tolist() == [0, 0, 0, 2, 2, 255, 255]


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_restatement_histograms_sum_to_the_pixel_counts(size):
    H, W = size
    h = R.hist(R.wide_picture(5, H, W))
    assert h.shape == (512,) and h.sum() == H * W
    cells = R.cell_pixels(H, W)
    assert np.array_equal(h.reshape(16, 32).sum(axis=1), cells) and cells.sum() == H * W
    # the header's closed form of a cell's rows: ceil(c n / 4) .. ceil((c + 1) n / 4) - 1
    for n, axis in ((H, 0), (W, 1)):
        per = cells.reshape(4, 4).sum(axis=1 - axis) // (W if axis == 0 else H)
        assert per.tolist() == [-(-(c + 1) * n // 4) - -(-c * n // 4) for c in range(4)]
    if (H, W) == (3, 5):
        assert (cells == 0).any()  # empty cells
    assert np.array_equal(SC.distances([h, h], H, W), [0.0, 0.0])


# -------------------------------------------------------------------------------------------------------------- plan
def test_plan_without_a_threshold_is_the_multiples_of_gop():
    for n in (1, 7, 31, 33, 100):
        for gop in (8, 32):
            d = np.random.default_rng(n).random(n)
            assert SC.plan(d, gop, None, 1) == list(range(0, n, gop)) == R.plan(d, gop, None, 1)
    assert SC.plan([], 8, None) == []
    # a threshold that can never be exceeded gives the same
    assert SC.plan(np.ones(40), 8, 1.0, 1) == list(range(0, 40, 8))


def test_plan_forces_an_i_picture_gop_after_the_last_one_whatever_caused_it():
    d = np.zeros(40)
    d[5] = d[21] = 0.9
    assert SC.plan(d, 8, 0.5, 1) == [0, 5, 13, 21, 29, 37]
    assert SC.plan(d, 8, 0.5, 1) == R.plan(d, 8, 0.5, 1)
    rng = np.random.default_rng(0)
    for _ in range(50):
        d = rng.random(60)
        gop, mg = int(rng.integers(1, 12)), 1
        mg = int(rng.integers(1, gop + 1))
        got = SC.plan(d, gop, 0.7, mg)
        assert got == R.plan(d, gop, 0.7, mg)
        gaps = np.diff(got + [60])
        assert got[0] == 0 and gaps.max() <= gop and (np.diff(got) >= mg).all()


def test_plan_min_gop_suppresses_a_cut_and_does_not_defer_it():
    d = np.zeros(20)
    d[2] = 0.9
    assert SC.plan(d, 8, 0.5, 1) == [0, 2, 10, 18]
    assert SC.plan(d, 8, 0.5, 2) == [0, 2, 10, 18]
    assert SC.plan(d, 8, 0.5, 3) == [0, 8, 16]  # not [0, 3, ...]: the cut stays a P picture
    d[9] = 0.9  # one picture behind the forced I at 8
    assert SC.plan(d, 8, 0.5, 2) == [0, 2, 9, 17]
    assert SC.plan(d, 8, 0.5, 8) == [0, 8, 16]


def test_plan_comparison_is_strict_and_a_cut_at_frame_one_is_taken():
    d = np.zeros(10)
    d[4] = 0.5
    assert SC.plan(d, 8, 0.5, 1) == [0, 8]
    d[4] = np.nextafter(0.5, 1.0)
    assert SC.plan(d, 8, 0.5, 1) == [0, 4]
    d = np.zeros(10)
    d[1] = 0.9
    assert SC.plan(d, 8, 0.5, 1) == [0, 1, 9]
    assert SC.plan(d, 8, 0.5, 2) == [0, 8]


def test_plan_refuses_bad_options_by_name():
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            SC.plan(np.zeros(4), 8, bad, 1)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError, match="min_gop"):
            SC.plan(np.zeros(4), 8, 0.5, bad)
    with pytest.raises(ValueError, match="gop"):
        SC.plan(np.zeros(4), 0, 0.5, 1)


# ----------------------------------------------------------------------------------------------------------- GopPlan
def _old_order(n_frames, gop, k, K):
    """_EncodeRun.order as it was before GopPlan: the closed form of `GOP g -> stream g mod K`"""
    n_gops = (n_frames + gop - 1) // gop
    index = lambda t: ((t // gop) * K + k) * gop + t % gop
    return [g for g in (index(t) for t in range(((n_gops - k + K - 1) // K) * gop)) if g < n_frames]


def test_fixed_plan_orders_equal_the_closed_form():
    for n in (1, 31, 32, 33, 100):
        for gop in (8, 32):
            plan = SC.GopPlan.fixed(n, gop)
            assert plan.i_pictures == list(range(0, n, gop)) and plan.n_gops == (n + gop - 1) // gop
            for K in (1, 2, 3):
                K_eff = max(1, min(K, plan.n_gops))
                for k in range(K_eff):
                    assert plan.order(k, K_eff) == _old_order(n, gop, k, K_eff), (n, gop, k, K_eff)
            assert [plan.is_intra(g) for g in range(n)] == [g % gop == 0 for g in range(n)]
            assert [plan.is_gop_end(g) for g in range(n)] == [g % gop == gop - 1 or g == n - 1 for g in range(n)]


def test_orders_partition_the_frames_into_whole_gops_in_increasing_order():
    plan = SC.GopPlan(40, [0, 5, 13, 14, 22, 30, 38])
    assert [plan.gop_of(g) for g in (0, 4, 5, 12, 13, 14, 39)] == [0, 0, 1, 1, 2, 3, 6]
    assert list(plan.gop_range(2)) == [13] and list(plan.gop_range(6)) == [38, 39]
    with pytest.raises(IndexError):
        plan.gop_of(40)
    for K in (1, 2, 3):
        orders = [plan.order(k, K) for k in range(K)]
        assert sorted(g for o in orders for g in o) == list(range(40))
        for k, o in enumerate(orders):
            assert o == sorted(o)
            gops = sorted({plan.gop_of(g) for g in o})
            assert gops == list(range(k, plan.n_gops, K))
            assert o == [g for j in gops for g in plan.gop_range(j)]


def test_json_round_trip_and_refusals_by_name():
    plan = SC.GopPlan(16, [0, 5, 13])
    assert plan.to_json() == {"frames": 16, "i_pictures": [0, 5, 13]}
    assert SC.GopPlan.from_json(plan.to_json()) == plan
    assert SC.GopPlan.from_json(dict(plan.to_json(), gop=8, scenecut=0.5, min_gop=2)) == plan  # gops.json's other keys
    for bad, name in (([1, 5], "start at 0"), ([], "start at 0"), ([0, 5, 5], "strictly increasing"), ([0, 7, 6], "strictly increasing"),
                      ([0, 5, 16], "reaches"), ([0, 99], "reaches")):
        with pytest.raises(ValueError, match=name):
            SC.GopPlan.from_json({"frames": 16, "i_pictures": bad})
    with pytest.raises(ValueError, match="frames"):
        SC.GopPlan.from_json({"i_pictures": [0]})
    with pytest.raises(ValueError, match="list of frame numbers"):
        SC.GopPlan(4, [0, "x"])


def test_gop_plan_files_are_refused_by_name(tmp_path):
    import json

    from vcm_ts_amd import run_codec as RC

    for t in range(6):
        (tmp_path / f"im{t + 1:05d}.bin").write_bytes(b"")
    plan, gop = RC.read_gop_plan(str(tmp_path), None)
    assert plan == SC.GopPlan.fixed(6, 32) and gop == 32
    assert RC.read_gop_plan(str(tmp_path), 4)[0] == SC.GopPlan.fixed(6, 4)
    RC.write_gop_plan(str(tmp_path), SC.GopPlan(6, [0, 2]), 4, 0.5, 2)
    assert json.loads((tmp_path / "gops.json").read_text()) == {"frames": 6, "gop": 4, "min_gop": 2, "scenecut": 0.5,
                                                                "i_pictures": [0, 2]}
    assert RC.read_gop_plan(str(tmp_path), None) == (SC.GopPlan(6, [0, 2]), 4)
    assert RC.read_gop_plan(str(tmp_path), 4) == (SC.GopPlan(6, [0, 2]), 4)
    with pytest.raises(ValueError, match="gop 4, not 8"):
        RC.read_gop_plan(str(tmp_path), 8)
    (tmp_path / "im00007.bin").write_bytes(b"")
    with pytest.raises(ValueError, match="6 frames beside 7"):
        RC.read_gop_plan(str(tmp_path), None)
    (tmp_path / "gops.json").write_text(json.dumps({"frames": 7, "i_pictures": [0, 3, 3]}))
    with pytest.raises(ValueError, match="strictly increasing"):
        RC.read_gop_plan(str(tmp_path), None)
    RC.write_gop_plan(str(tmp_path), SC.GopPlan.fixed(7, 4), 4, None, 1)  # no scan: no file (a stale one goes)
    assert not (tmp_path / "gops.json").exists()


# --------------------------------------------------------------------------------------------------------------- ABI
def test_header_symbols_are_bound_and_built():
    mk = open(os.path.join(ROOT, "vcm_ts_amd", "csrc", "Makefile")).read()
    assert "scene.hip" in [ln for ln in mk.splitlines() if ln.startswith("HIPSRC")][0].split()
    assert "dcvc_hip_scene.h" in [ln for ln in mk.splitlines() if ln.startswith("$(HERE)build/%.o")][0]
    src = open(os.path.join(ROOT, "vcm_ts_amd", "csrc", "scene.hip")).read()
    assert "__launch_bounds__" in src


def test_entry_point_refuses_each_bad_argument_before_any_launch():
    """Pointers are aligned dummies: a refused call returns before anything is launched or dereferenced."""
    from vcm_ts_amd import lib

    L, E_ARG = lib.hip(), -1
    good = dict(rgb=0x10000, rs=96, ps=64 * 96, H=64, W=96, hist=0x20000)

    def call(**over):
        a = dict(good, **over)
        return L.dcvc_scene_hist(a["rgb"], a["rs"], a["ps"], a["H"], a["W"], a["hist"], None)

    assert call(rgb=None) == E_ARG and call(hist=None) == E_ARG
    for side in ("H", "W"):
        for bad in (0, -1, 32769, -(2 ** 31)):
            assert call(**{side: bad}, rs=40000, ps=2 ** 40) == E_ARG, (side, bad)
    assert call(rs=95) == E_ARG and call(rs=0) == E_ARG and call(rs=-96) == E_ARG
    assert call(ps=63 * 96 + 95) == E_ARG and call(ps=0) == E_ARG and call(ps=-1) == E_ARG
    assert call(rs=128, ps=63 * 128 + 95) == E_ARG  # the rows of a padded picture need (H - 1) * row_stride + W
    assert call(rgb=0x10002) == E_ARG and call(hist=0x20001) == E_ARG  # not 4-byte aligned


def test_scan_refuses_cpu_tensors_by_name():
    import torch

    with pytest.raises(ValueError, match="GPU"):
        SC.SceneScan(torch.device("cpu"), 8, 8, 2)


# ------------------------------------------------------------------------------- the inputs of the GPU tests separate
@pytest.mark.parametrize("size", [(64, 64), (65, 63), (128, 192)], ids=["64x64", "65x63", "128x192"])
def test_synthetic_scenes_are_separated_by_wide_margins_around_the_test_threshold(size):
    """Scene A = 0.5 + 0.5 frames(seed), scene B = 0.35 frames(seed'): consecutive frames within a scene stay below 0.25,
    the transitions A -> B and B -> A are above 0.75 (measured with this restatement, 8 seeds per size: within <= 0.091,
    across = 1.000 -- A's luma codes are all >= 127, B's all <= 90, so no bin is shared).  The threshold 0.5 of
    tests/test_gpu_scenecut.py therefore has wide margins on both sides."""
    H, W = size
    for seed in range(8):
        a, b = R.scene_a(seed, 4, H, W), R.scene_b(100 + seed, 4, H, W)
        d = R.distances(list(a) + list(b) + list(a[:1]))
        within = np.delete(d, [0, 4, 8])
        assert within.max() < 0.25, (seed, within.max())
        assert d[4] > 0.75 and d[8] > 0.75, (seed, d[4], d[8])
    clip = R.cut_clip(64, 64).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    assert SC.plan(R.distances(list(clip)), 8, 0.5, 2) == [0, 5, 13]
