"""Rate control on a real MI355X: the ladder-sweep kernel bit for bit against the restatement
(tests/ratectl_ref.py) inside guarded, offset buffers; DMC.compress(sweep=) against the bit map's y total with the bytes
and the DPB left alone; a rate-controlled GOP against the restated controller replayed on the run's own log and against
the decoder; the direction of the control; GOP streams; the file loop; the refusals."""
import ctypes as C
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import bitmap_ref as B
from tests import gpu_util as U
from tests import ratectl_ref as R
from tests.gpu_util import seeded_nets  # noqa: F401 (fixture)
from vcm_ts_amd import bitmap as BM
from vcm_ts_amd import lib
from vcm_ts_amd import ratectl as RC
from vcm_ts_amd.pipeline import ConcurrentGopEncoder, GopEncoder, pad_frame
from vcm_ts_amd.synthetic import frames

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, FILL = 64, 0x5A5A5A5A5A5A5A5A
LADDERS = {1: (100,), 3: (63, 100, 159), 8: RC.LADDER}
I100 = RC.LADDER.index(100)


def _offset(a, lead):
    """`a` on the device as a view that starts `lead` elements into its buffer."""
    buf = torch.zeros(a.size + lead + 5, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    buf[lead:lead + a.size] = U.to_dev(a.reshape(-1), DEV)
    return buf[lead:lead + a.size]


def _edges(rng):
    e = np.sort(np.exp(rng.uniform(np.log(0.05), np.log(60.0), 255))).astype(np.float32)
    assert (np.diff(e) > 0).all()
    return np.concatenate([e, np.array([np.inf], dtype=np.float32)])


def _case(shape):
    """Residuals and scales of an (N, C, H, W) latent with the corner cases the kernel can get wrong, a 256-row table whose
    row 0 holds only its sentinel, and 256 edges."""
    N, Cc, H, W = shape
    rng = np.random.default_rng(1000 + Cc * H + W)
    table, edges = B.random_table(rng, 256), _edges(rng)
    n = N * Cc * H * W
    res = (rng.standard_normal(n) * np.exp(rng.uniform(0, 3, n))).astype(np.float32)
    big = rng.random(n) < 0.08  # escapes of both signs, up to 8 nibbles (|v| up to 4e8; 4e8 / 0.5 stays below 2^31)
    res[big] = (np.exp(rng.uniform(np.log(10.0), np.log(4e8), n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)[big]
    sc = np.exp(rng.uniform(np.log(0.02), np.log(90.0), n)).astype(np.float32)
    res[:6] = [3e8, -3e8, 2.5, -3.5, 1.25, 0.5]                    # 8 nibbles of both signs; quotients exactly on .5
    sc[6:9] = [edges[40], edges[100], np.float32(edges[17] * np.float32(0.5))]  # exactly on an edge (at 100, 100, 50)
    sc[9:13] = [edges[0] * np.float32(0.4), 1e-6, 0.0, -1.0]       # under the lowest edge: row 0, sentinel only
    assert float(np.float32(sc[8]) / R.factor(50)) == float(edges[17])
    return table, edges, res, sc


_REF = {}


def _reference(shape):
    """The restated sweep of _case(shape) for the whole LADDER, once per shape.  It meets no bad value, so the sums of a
    ladder that is a subset of LADDER are its columns."""
    if shape not in _REF:
        table, edges, res, sc = _case(shape)
        stats = {}
        est, status = R.sweep(res, sc, edges, RC.LADDER, table, shape[0], stats)
        assert status == 0
        assert stats["escapes"] >= 0.05 * stats["candidates"] and stats["signs"] == {-1, 1} and 8 in stats["nibbles"]
        assert stats["sentinel_only"] >= 4 and stats["below_lowest_edge"] >= 4
        _REF[shape] = est
    return _REF[shape]


def _run_kernel(table, edges, res, sc, ladder, shape):
    N, Cc, H, W = shape
    K = len(ladder)
    cost, sizes, offsets = U.to_dev(BM.cost_array(*table), DEV), U.to_dev(table[1], DEV), U.to_dev(table[2], DEV)
    r, s, e = _offset(res, 3), _offset(sc, 1), _offset(edges, 5)
    buf = torch.full((N * K + 2 * GUARD,), FILL, dtype=torch.int64, device=DEV)
    view = buf[GUARD:GUARD + N * K]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    fac = np.array([R.factor(h) for h in ladder], dtype=np.float32)
    lib.check(lib.hip().dcvc_bits_sweep_scale(r.data_ptr(), s.data_ptr(), e.data_ptr(), fac.ctypes.data_as(C.c_void_p), K,
                                              cost.data_ptr(), table[0].shape[0], table[0].shape[1], sizes.data_ptr(),
                                              offsets.data_ptr(), view.data_ptr(), N, Cc, H, W, status.data_ptr(), U.stream(DEV)),
              "bits_sweep_scale")
    h = buf.cpu().numpy()
    intact = bool((h[:GUARD] == FILL).all() and (h[GUARD + N * K:] == FILL).all())
    return h[GUARD:GUARD + N * K].reshape(N, K), int(status.item()), intact


# ----------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("shape", [(2, 6, 3, 5), (1, 96, 4, 8), (2, 96, 9, 15)], ids=lambda s: "x".join(map(str, s)))
def test_sweep_kernel_equals_the_restatement_bit_for_bit(shape, K):
    """N=2 C=6 3x5: 90 elements per sample, a partial wave.  C=96 4x8: 3072, whole workgroups of 1024.  N=2 C=96 9x15:
    12960, 13 workgroups per sample, the last one ragged."""
    ladder = LADDERS[K]
    want = _reference(shape)[:, [RC.LADDER.index(h) for h in ladder]]
    got, status, intact = _run_kernel(*_case(shape), ladder, shape)
    assert status == 0 and intact
    assert np.array_equal(got, want), (got - want)


def test_values_that_are_not_finite_cost_nothing_and_set_the_status():
    shape, ladder = (2, 6, 3, 5), LADDERS[3]
    table, edges, res, sc = _case(shape)
    clean, status = R.sweep(res, sc, edges, ladder, table, 2)
    assert status == 0
    spots = (20, 90 + 33, 40)  # (sample 0, sample 1, sample 0)
    taken = [R.sweep(res[e:e + 1], sc[e:e + 1], edges, ladder, table, 1)[0][0] for e in spots]
    res, sc = res.copy(), sc.copy()
    res[spots[0]], sc[spots[1]] = np.inf, np.nan
    res[spots[2]] = 2e9  # finite, and an int32 at 100 and 159 hundredths but not at 63: nothing for any of the three
    want, status = R.sweep(res, sc, edges, ladder, table, 2)
    assert status == R.BAD_VALUE and np.array_equal(want, clean - np.array([taken[0] + taken[2], taken[1]]))
    got, status, intact = _run_kernel(table, edges, res, sc, ladder, shape)
    assert status == RC.BAD_VALUE and intact and np.array_equal(got, want)


def test_a_row_outside_the_table_costs_nothing_and_sets_the_status():
    """A table of 200 rows under 256 edges: scales in the rows 200 .. 255 are compared, never used as an address."""
    shape, ladder = (2, 6, 3, 5), LADDERS[3]
    table, edges, res, sc = _case(shape)
    table = tuple(t[:200] for t in table)
    want, status = R.sweep(res, sc, edges, ladder, table, 2)
    assert status == R.BAD_INDEX
    got, status, intact = _run_kernel(table, edges, res, sc, ladder, shape)
    assert status == BM.BAD_INDEX and intact and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ the codec
def _clip(h, w, batch, n=3, seed=31):
    fr = frames(seed, n, h, w)
    xs = [pad_frame(torch.from_numpy(fr[t:t + 1]).to(DEV)) for t in range(n)]
    return [x.expand(batch, -1, -1, -1).contiguous() for x in xs]


def _q(batch, a, b):
    return a if batch == 1 else torch.tensor([a, b], device=DEV)


@pytest.mark.parametrize("case", ["64x64", "72x104", "72x104-qmap", "64x64-batch2"])
def test_compress_with_a_sweep_prices_the_coded_symbols_and_leaves_the_bytes_alone(seeded_nets, case):
    """I + 2 P: compress(sweep=LADDER) returns the bytes and every DPB tensor of the call without it; the column of 100
    hundredths is the y total of the picture's bit map, exactly; the whole row is the restatement applied to the residual
    and scale planes the picture left on the device."""
    from vcm_ts_amd.entropy import scale_index_edges

    d, i = seeded_nets
    size, *opt = case.split("-")
    h, w = (int(v) for v in size.split("x"))
    batch = 2 if "batch2" in opt else 1
    xs = _clip(h, w, batch)
    Hp, Wp = xs[0].shape[2:]
    q_map = None
    if "qmap" in opt:
        q_map = torch.full((1, 1, Hp // 16, Wp // 16), 1.4, device=DEV)
        q_map[:, :, 1:4, 2:6] = 0.6
    qm, qy = _q(batch, 1.0, 1.3), _q(batch, 1.0, 0.7)
    dpb = U.intra_dpb(i.compress(xs[0], _q(batch, 1.0, 0.6), q_map=q_map)["x_hat"].clone())
    edges = scale_index_edges("laplace").numpy()
    for t in (1, 2):
        plain = d.compress(xs[t], dpb, qm, qy, q_map=q_map)
        assert "rate_sweep" not in plain
        keep = (plain["bit_streams"], {k: v.clone() for k, v in plain["dpb"].items()})
        res = d.compress(xs[t], dpb, qm, qy, q_map=q_map, sweep=RC.LADDER, bit_map=True)
        assert res["bit_streams"] == keep[0] and all(torch.equal(res["dpb"][k], keep[1][k]) for k in keep[1])
        assert set(res) == set(plain) | {"bit_map", "rate_sweep"}
        sweep = res["rate_sweep"]
        assert isinstance(sweep, RC.RateSweep) and sweep.ladder == RC.LADDER
        sums, totals = sweep.sums(), res["bit_map"].totals()
        assert sums.shape == (batch, 8) and sums.dtype == np.int64 and (sums > 0).all()
        assert np.array_equal(sums[:, I100], totals[:, 3])
        r = res["_views"]["r_y"]
        want, status = R.sweep(r["y_res"].cpu().numpy(), r["scales_hat"].cpu().numpy(), edges, RC.LADDER, d._tables["scale"], batch)
        assert status == 0 and np.array_equal(sums, want)
        print(case, "picture", t, "bits of y per ladder point", (sums / B.UNIT).round(1).tolist())
        assert (sums[:, 0] > sums[:, -1]).all()  # (half the step costs more than 2.52 times the step)
        if batch == 2:
            assert sums[0].tolist() != sums[1].tolist()
        # without a bit map, deferred, and with the device coder: the same sums
        r2 = d.compress(xs[t], dpb, qm, qy, q_map=q_map, sweep=RC.LADDER, defer=True)
        assert set(r2) == (set(plain) - {"bit_stream", "bit_streams"}) | {"pending", "rate_sweep"}
        assert r2["pending"].finish_all() == keep[0] and np.array_equal(r2["rate_sweep"].sums(), sums)
        if batch == 1:
            r3 = d.compress(xs[t], dpb, qm, qy, q_map=q_map, sweep=(50, 100, 200), coder="device")
            assert np.array_equal(r3["rate_sweep"].sums(), sums[:, [0, I100, 6]])
        dpb = keep[1]


# -------------------------------------------------------------------------------------------------------------- the GOP
GOP, SIZE, START = 8, 64, (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def clip8():
    fr = frames(21, GOP, SIZE, SIZE)
    return [pad_frame(torch.from_numpy(fr[t:t + 1]).to(DEV)) for t in range(GOP)]


def _coded_bits(coded):
    return [(len(p) + (14 if kind == "I" else 8)) * 8 for kind, _, p in coded]


@pytest.fixture(scope="module")
def free_run(seeded_nets, clip8):
    """The 8 pictures coded without rate control: (coded, bits per picture)."""
    coded, bits, _ = GopEncoder(seeded_nets[1], seeded_nets[0], gop_size=GOP).encode_gop(clip8, *START)
    per = _coded_bits(coded)
    assert sum(per) == bits
    return coded, per


def _controlled(seeded_nets, clip8, target_bits, q_range=(1, 65500)):
    recons, res = [], {}
    enc = GopEncoder(seeded_nets[1], seeded_nets[0], gop_size=GOP)
    coded, bits, _ = enc.encode_gop(clip8, *START, on_recon=lambda t, x: recons.append(x.clone()), res=res,
                                    rate=RC.factory(target_bits, GOP, q_range))
    assert sum(_coded_bits(coded)) == bits
    return enc, coded, recons, res["rate_log"]


def test_a_controlled_gop_follows_the_restated_controller_and_decodes(seeded_nets, clip8, free_run):
    """8 pictures at 64x64, target 0.7 of the free run's average: the q indexes in the headers are what the restated
    controller decides when replayed on the run's own log, and the decoder reproduces the encoder's reconstructions."""
    target = Fraction(7 * sum(free_run[1]), 10 * GOP)
    enc, coded, recons, log = _controlled(seeded_nets, clip8, target)
    assert [k for k, _, _ in coded] == ["I"] + ["P"] * 7 and len(log) == GOP
    assert [e[1] for e in log] == _coded_bits(coded)
    assert log[0][0] == 100 and log[0][2] is None and log[0][3] is None
    assert all(len(e[3]) == 8 and e[3][I100] > 0 for e in log[1:])
    want = R.replay(target, GOP, (1, 65500), RC.LADDER, 100, log)
    print("q_y", [q[-1] for _, q, _ in coded], "bits", _coded_bits(coded), "budgets", [e[2] and round(float(e[2])) for e in log])
    assert [q for _, q, _ in coded[1:]] == [(100, w[0]) for w in want]
    assert [e[2] for e in log[1:]] == [w[1] for w in want]
    assert [q[1] for _, q, _ in coded[1:3]] == [100, 100] and any(q[1] != 100 for _, q, _ in coded[3:])
    decoded = enc.decode_gop(coded, SIZE, SIZE)
    assert len(decoded) == GOP and all(torch.equal(a, b) for a, b in zip(decoded, recons))


@pytest.mark.parametrize("factor,sign", [(Fraction(1, 2), -1), (2, 1)], ids=["half", "twice"])
def test_direction_of_the_control(seeded_nets, clip8, free_run, factor, sign):
    """A target of half the free run's average bits per picture must cost fewer bits from the third P picture on than
    the free run's same pictures, a target of twice must cost more.  The sign only: how close a GOP lands to its target
    is measured (profiles/ratectl_1080p.txt), not asserted."""
    free = free_run[1]
    target = factor * Fraction(sum(free), GOP)
    _, coded, _, log = _controlled(seeded_nets, clip8, target)
    got = _coded_bits(coded)
    print("target", float(target), "free", free, "controlled", got, "q_y", [q[-1] for _, q, _ in coded])
    assert got[:3] == free[:3]  # (the I picture and the first two P pictures are not controlled)
    assert (sum(got[3:]) - sum(free[3:])) * sign > 0


def test_q_range_bounds_every_decision(seeded_nets, clip8, free_run):
    target = Fraction(sum(free_run[1]), 4 * GOP)
    _, coded, _, _ = _controlled(seeded_nets, clip8, target, q_range=(90, 130))
    qs = [q[1] for _, q, _ in coded[1:]]
    assert qs[:2] == [100, 100] and all(90 <= q <= 130 for q in qs) and 130 in qs


def test_two_gops_on_two_streams_give_the_bytes_of_sequential_coding(seeded_nets, clip8, free_run):
    from vcm_ts_amd.dmc import DMC
    from vcm_ts_amd.intra import IntraNoAR

    target = Fraction(6 * sum(free_run[1]), 10 * GOP)
    rate = RC.factory(target, 4)
    res = {}
    seq, _, _ = GopEncoder(seeded_nets[1], seeded_nets[0], gop_size=4).encode_gop(clip8, *START, rate=rate, res=res)
    assert [k for k, _, _ in seq] == ["I", "P", "P", "P"] * 2 and len(R.split_gops(res["rate_log"])) == 2
    assert any(q[1] != 100 for _, q, _ in seq[3::4])

    def make():
        d, i = DMC().to(DEV).eval(), IntraNoAR().to(DEV).eval()
        return i, d

    cenc = ConcurrentGopEncoder(make, gop_size=4, streams=2)
    out = cenc.encode_gops([clip8[:4], clip8[4:]], *START, rate=rate)
    assert [c for coded, _, _ in out for c in coded] == seq
    assert [e for log in cenc.rate_logs for e in log] == res["rate_log"]


# ------------------------------------------------------------------------------------------------------------ file loop
N_FRAMES, FGOP, FH, FW = 6, 5, 176, 192  # (a report takes MS-SSIM, whose five levels need sides above 160)


def _write_clip(folder, h, w):
    U.write_pngs(folder, np.rint(frames(21, N_FRAMES, h, w) * 255).astype(np.uint8).transpose(0, 2, 3, 1))


def test_file_loop_with_a_target(tmp_path):
    from PIL import Image

    from vcm_ts_amd import run_codec as F
    from vcm_ts_amd import stream as S

    file_nets = F._nets(DEV, None)
    _write_clip(tmp_path / "png", FH, FW)
    common = dict(gop=FGOP, nets=file_nets)
    bits, size, plain = F.encode_folder(str(tmp_path / "png"), str(tmp_path / "plain"), report=True, **common)
    assert "frame_q_y" not in plain and "frame_bits_target" not in plain
    # without the option: the bytes of the GOP loop called directly
    xs = [pad_frame(F.u8_to_unit_float(torch.from_numpy(a).to(DEV))) for a in
          np.rint(frames(21, N_FRAMES, FH, FW) * 255).astype(np.uint8).transpose(0, 2, 3, 1)]
    coded, _, _ = GopEncoder(*file_nets, gop_size=FGOP).encode_gop(xs, 1.0, 1.0, 1.0)
    for g, (kind, q, payload) in enumerate(coded):
        got = (S.decode_i if kind == "I" else S.decode_p)(str(tmp_path / "plain" / f"im{g + 1:05d}.bin"))
        assert got[-1] == payload and tuple(got[-1 - len(q):-1]) == q
    bpp = 0.5 * sum(bits) / (N_FRAMES * FH * FW)
    report = str(tmp_path / "report.json")
    cbits, _, rd = F.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), str(tmp_path / "recon"), report=report,
                                   target_bpp=bpp, q_range=(0.5, 3.0), **common)
    assert set(rd) == set(plain) | {"frame_q_y", "frame_bits_target"} and json.loads(open(report).read()) == rd
    q_y, target = rd["frame_q_y"], rd["frame_bits_target"]
    print("bits", cbits, "q_y", q_y, "targets", target)
    assert rd["frame_type"] == [0, 1, 1, 1, 1, 0] and q_y[:3] == [1.0, 1.0, 1.0] and q_y[5] == 1.0
    assert [t is None for t in target] == [True, True, True, False, False, True]
    assert all(0.5 <= q <= 3.0 for q in q_y[3:5]) and q_y[3] > 1.0 and cbits[:3] == bits[:3] and cbits[5] == bits[5]
    for g in (1, 2, 3, 4):  # every header carries its picture's own index
        assert S.decode_p(str(tmp_path / "bins" / f"im{g + 1:05d}.bin"))[:2] == (100, round(q_y[g] * 100))
    n = F.decode_folder(str(tmp_path / "bins"), str(tmp_path / "dec"), FH, FW, FGOP)
    assert n == N_FRAMES
    for g in range(N_FRAMES):
        a, b = (np.asarray(Image.open(tmp_path / d / f"im{g + 1:05d}.png")) for d in ("recon", "dec"))
        assert np.array_equal(a, b), g
    # two GOP streams: the same bytes
    F.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins2"), gop=FGOP, nets=[file_nets, F._nets(DEV, None)], gop_streams=2,
                    target_bpp=bpp, q_range=(0.5, 3.0))
    assert U.bins(tmp_path / "bins2") == U.bins(tmp_path / "bins")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(seeded_nets, tmp_path, monkeypatch, capsys):
    d, i = seeded_nets
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    with pytest.raises(NotImplementedError, match="sweep.*graph"):
        d.compress(x, U.intra_dpb(x), 1.0, 1.0, graph=True, sweep=RC.LADDER)
    with pytest.raises(ValueError, match="ladder.*must contain 100"):
        d.compress(x, U.intra_dpb(x), 1.0, 1.0, sweep=(50, 200))
    d.train()
    try:
        with pytest.raises(ValueError, match="sweep.*eval"):
            d.compress(x, U.intra_dpb(x), 1.0, 1.0, sweep=RC.LADDER)
    finally:
        d.eval()
    enc = GopEncoder(i, d, gop_size=2, graphs=True)
    with pytest.raises(NotImplementedError, match="rate.*graph"):
        enc.encode_gop([x, x], 1.0, 1.0, 1.0, rate=RC.factory(1000, 2))
    from vcm_ts_amd import run_codec as F

    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ex:
        F.main(["encode", "--frames", "F", "--bins", "B", "--target-bpp", "0.1", "--rate-count", "2", "--quality", "1"])
    err = capsys.readouterr().err
    assert ex.value.code == 2 and "--target-bpp" in err and "--rate-count" in err
