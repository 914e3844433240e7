"""Per-cell bit maps on a real MI355X: the map and region kernels bit for bit against the restatement
(tests/bitmap_ref.py) inside guarded buffers, the codecs' maps against the restatement applied to their own staged symbol
planes and against the length of the byte string the host coder writes (the bound of DESIGN.md 4i), and the file loops."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import bitmap_ref as R
from tests import gpu_util as U
from tests.gpu_util import seeded_nets  # noqa: F401 (fixture: the name-seeded weights the CPU oracle's tests use)
from vcm_ts_amd import bitmap as B
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X
from vcm_ts_amd.pipeline import pad_frame
from vcm_ts_amd.synthetic import frames

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL = 0x5A5A5A5A


def _table_on_device(table):
    cdf, sizes, offsets = table
    return U.to_dev(B.cost_array(cdf, sizes, offsets), DEV), U.to_dev(sizes, DEV), U.to_dev(offsets, DEV), cdf.shape[0], cdf.shape[1]


def _guarded(n, dtype=np.uint32):
    buf, at = U.guarded(n, 0, dtype, FILL, DEV)
    return buf, buf[at:at + n]


def _guards_intact(buf, n):
    return U.guards_intact(buf, U.GUARD, n, FILL)


# ----------------------------------------------------------------------------------------------------- the map kernels
def _scale_case(seed, N, Cc, H, W, rows=9):
    rng = np.random.default_rng(seed)
    table = R.random_table(rng, rows)
    n = N * (Cc // 2) * H * W
    planes = [R.random_symbols(rng, table, n) for _ in (0, 1)]
    # every row in both planes (the smallest case has 90 entries per plane), and escapes among them
    for sym, idx in planes:
        idx[:rows] = np.arange(rows)
        sym[:rows] = R.random_symbols(rng, table, rows, rows=np.arange(rows))[0]
    return table, planes


def _run_scale(table, planes, N, Cc, H, W):
    cost, sizes, offsets, rows, stride = _table_on_device(table)
    (s0, i0), (s1, i1) = [(U.to_dev(s, DEV), U.to_dev(i, DEV)) for s, i in planes]
    buf, view = _guarded(N * H * W)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(lib.hip().dcvc_bits_map_scale(s0.data_ptr(), i0.data_ptr(), s1.data_ptr(), i1.data_ptr(), cost.data_ptr(), rows,
                                            stride, sizes.data_ptr(), offsets.data_ptr(), view.data_ptr(), N, Cc, H, W,
                                            status.data_ptr(), U.stream(DEV)), "bits_map_scale")
    return buf, view.cpu().numpy().reshape(N, H, W), int(status.item())


@pytest.mark.parametrize("shape", [(2, 6, 3, 5), (1, 96, 4, 8), (2, 96, 9, 15)], ids=lambda s: "x".join(map(str, s)))
def test_scale_map_kernel_equals_the_restatement_bit_for_bit(shape):
    """N=2 C=6 3x5 (fewer channels than channel slices, fewer positions than lanes), C=96 4x8 (the codec's y), and C=96
    9x15 with N=2: 135 positions, more than one workgroup per sample and a ragged last one."""
    N, Cc, H, W = shape
    table, planes = _scale_case(11 + Cc + H, N, Cc, H, W)
    buf, got, status = _run_scale(table, planes, N, Cc, H, W)
    want = R.map_scale(planes[0][0], planes[0][1], planes[1][0], planes[1][1], table, N, Cc, H, W)
    assert want.max() < 2 ** 31 and want.min() >= 0
    assert status == 0 and got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want)
    assert _guards_intact(buf, N * H * W)


def test_factorized_map_kernel_equals_the_restatement_bit_for_bit():
    N, Cc, H, W = 2, 64, 1, 2
    rng = np.random.default_rng(3)
    table = R.random_table(rng, Cc)
    chan = np.broadcast_to(np.arange(Cc)[None, :, None, None], (N, Cc, H, W)).reshape(-1)
    sym, _ = R.random_symbols(rng, table, chan.size, rows=chan, escapes=0.2)
    cost, sizes, offsets, rows, stride = _table_on_device(table)
    s = U.to_dev(sym, DEV)
    buf, view = _guarded(N * H * W)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(lib.hip().dcvc_bits_map_factorized(s.data_ptr(), cost.data_ptr(), rows, stride, sizes.data_ptr(),
                                                 offsets.data_ptr(), view.data_ptr(), N, Cc, H, W, status.data_ptr(),
                                                 U.stream(DEV)), "bits_map_factorized")
    want = R.map_factorized(sym, table, N, Cc, H, W)
    assert int(status.item()) == 0 and np.array_equal(view.cpu().numpy().reshape(N, H, W).astype(np.int64), want)
    assert _guards_intact(buf, N * H * W)


def test_an_index_out_of_range_costs_nothing_and_sets_the_status():
    """Two bad rows as DATA (n_rows and -1): they are compared, never used as an address; their symbols cost 0."""
    N, Cc, H, W = 2, 6, 3, 5
    table, planes = _scale_case(5, N, Cc, H, W)
    rows = table[0].shape[0]
    planes[0][1][17] = rows
    planes[1][1][40] = -1
    buf, got, status = _run_scale(table, planes, N, Cc, H, W)
    # the restatement with the two symbols taken out: replace them by a symbol of known cost and subtract it
    fixed = [(s.copy(), i.copy()) for s, i in planes]
    fixed[0][1][17], fixed[0][0][17] = 1, table[2][1]      # row 1 {1, 65535}: its only coded symbol, frequency 1
    fixed[1][1][40], fixed[1][0][40] = 1, table[2][1]
    want = R.map_scale(fixed[0][0], fixed[0][1], fixed[1][0], fixed[1][1], table, N, Cc, H, W)
    per = (Cc // 2) * H * W
    for e in (17, 40):
        n, pos = divmod(e, per)
        want[n].reshape(-1)[pos % (H * W)] -= R.lut(1)
    assert status == B.BAD_INDEX
    assert np.array_equal(got.astype(np.int64), want) and _guards_intact(buf, N * H * W)


# --------------------------------------------------------------------------------------------------- the region kernel
@pytest.mark.parametrize("grid", [(4, 4, 4, 4), (8, 8, 8, 8), (5, 7, 8, 8)], ids=["4x4", "8x8", "5x7-in-8x8"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_region_kernel_equals_the_restatement_bit_for_bit(grid, K):
    """5x7: the cells of an 80 x 112 picture, whose z grid would not divide evenly -- the cell grid is the PADDED
    picture's (128 x 128: 8 x 8), labels beyond the 5 x 7 cells are the background's."""
    used_h, used_w, hc, wc = grid
    assert (hc, wc) == X.grid_of(16 * used_h, 16 * used_w)
    N = 2
    rng = np.random.default_rng(K * 100 + used_h)
    maps = [rng.integers(0, 2 ** 31 - 1, (N, hc // 4, wc // 4)), rng.integers(0, 2 ** 31 - 1, (N, hc, wc)),
            rng.integers(0, 2 ** 26, (N, hc // 4, wc // 4)), rng.integers(0, 2 ** 26, (N, hc, wc))]
    maps = [m.astype(np.int32) for m in maps]
    labels = np.zeros((N, hc, wc), dtype=np.uint8)
    labels[:, :used_h, :used_w] = rng.integers(0, K, (N, used_h, used_w))
    lab = U.to_dev(labels, DEV)
    for absent in ((), (0, 1), (2,), (0, 1, 2)):
        present = [None if c in absent else m for c, m in enumerate(maps)]
        on_dev = [None if m is None else U.to_dev(m, DEV) for m in present]
        ptrs = (C.c_void_p * 4)(*[None if m is None else m.data_ptr() for m in on_dev])
        buf, view = _guarded(N * K * 4, np.uint64)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        lib.check(lib.hip().dcvc_bits_regions(ptrs, lab.data_ptr(), K, view.data_ptr(), N, hc, wc, status.data_ptr(),
                                              U.stream(DEV)), "bits_regions")
        want = R.region_sums(present, labels, K)
        assert int(status.item()) == 0
        assert np.array_equal(view.cpu().numpy().reshape(N, K, 4), want), absent
        assert _guards_intact(buf, N * K * 4)
        # the Python layer on the same maps
        bm = B.BitMap(dict(zip(B.COMPONENTS, on_dev)), torch.zeros(2, dtype=torch.int32, device=DEV), N, hc, wc)
        assert np.array_equal(bm.regions(lab, K), want)
        assert np.array_equal(bm.totals() * 16, want.sum(axis=1))
        cells = bm.cells()
        assert cells.shape == (N, hc, wc) and cells.dtype == np.float64
        assert np.array_equal(cells.sum(axis=(1, 2)) * R.REGION_UNIT, want.sum(axis=(1, 2)).astype(np.float64))


def test_a_label_out_of_range_adds_nothing_and_sets_the_status():
    hc = wc = 4
    y = np.full((1, hc, wc), 5, dtype=np.int32)
    labels = np.zeros((1, hc, wc), dtype=np.uint8)
    labels[0, 1, 2] = 2
    bm = B.BitMap({"y": U.to_dev(y, DEV)}, torch.zeros(2, dtype=torch.int32, device=DEV), 1, hc, wc)
    row = bm.regions_enqueue(U.to_dev(labels, DEV), 2).cpu().numpy()
    assert row[:8].tolist() == [0, 0, 0, 15 * 16 * 5, 0, 0, 0, 0] and int(row[8:].view(np.int32)[0]) == B.BAD_LABEL
    with pytest.raises(B.BitMapError, match="label"):
        B.BitMap.decode(row, 1, 2)


def test_labels_from_boxes_follow_the_touch_rule():
    H, W = 72, 104                                   # padded 128 x 128: 8 x 8 cells
    boxes = np.array([[17, 0, 33, 16, 0], [90, 60, 104, 72, 3], [5, 40, 5, 60, 1]])  # the last one is empty
    for grow in (0, 1, 20):
        got = B.labels_from_boxes(boxes, H, W, grow)
        want = np.zeros((8, 8), dtype=np.uint8)
        for x1, y1, x2, y2, _ in boxes:
            if x2 <= x1 or y2 <= y1:
                continue
            x1, y1, x2, y2 = max(x1 - grow, 0), max(y1 - grow, 0), min(x2 + grow, W), min(y2 + grow, H)
            for i in range(8):
                for j in range(8):
                    if x1 < 16 * j + 16 and x2 > 16 * j and y1 < 16 * i + 16 and y2 > 16 * i:
                        want[i, j] = 1
        assert got.dtype == torch.uint8 and got.device == DEV and tuple(got.shape) == (1, 8, 8)
        assert np.array_equal(got.cpu().numpy()[0], want), grow
    assert int(B.labels_from_boxes(np.zeros((0, 5), np.int32), H, W).sum()) == 0


# ---------------------------------------------------------------------------------------------------------- the codecs
def _np(t):
    return t.detach().cpu().numpy()


def _i_groups(net, v):
    return [("z", "bit_estimator_z", v["sym_z"], v["r"], net.N, net.N, v["z_hat"])]


def _p_groups(v):
    return [("mv_z", "bit_estimator_z_mv", v["sym_mv_z"], v["r_mv"], 64, 64, v["mv_z_hat"]),
            ("z", "bit_estimator_z", v["sym_z"], v["r_y"], 64, 96, v["z_hat"])]


def _check_picture(net, groups, res, N):
    """The maps of res["bit_map"] against the restatement applied to the staged planes; returns per element the
    restatement's (units, records) of the whole picture, in bitstream order."""
    bm = res["bit_map"]
    assert isinstance(bm, B.BitMap) and bm.N == N
    per_element = [[0, 0] for _ in range(N)]
    for zname, ztable, zsym, r, Cz, Cy, zv in groups:
        yname = {"z": "y", "mv_z": "mv_y"}[zname]
        zh, zw = zv.H, zv.W
        H, W = 4 * zh, 4 * zw
        zs, s0, s1, i0, i1 = (_np(t) for t in (zsym, r["sym"][0], r["sym"][1], r["idx"][0], r["idx"][1]))
        want_z = R.map_factorized(zs, net._tables[ztable], N, Cz, zh, zw)
        want_y = R.map_scale(s0, i0, s1, i1, net._tables["scale"], N, Cy, H, W)
        assert np.array_equal(_np(bm.maps[zname]).astype(np.int64), want_z), zname
        assert np.array_equal(_np(bm.maps[yname]).astype(np.int64), want_y), yname
        assert want_y.max() > 0 and want_z.max() > 0
        chan = np.broadcast_to(np.arange(Cz)[:, None, None], (Cz, zh, zw)).reshape(-1)
        for b in range(N):
            for sym, idx, table in ((zs.reshape(N, -1)[b], chan, ztable), (s0.reshape(N, -1)[b], i0.reshape(N, -1)[b], "scale"),
                                    (s1.reshape(N, -1)[b], i1.reshape(N, -1)[b], "scale")):
                u, n = R.stream_cost(sym, idx, net._tables[table])
                per_element[b][0] += u
                per_element[b][1] += n
    totals = bm.totals()
    assert totals.shape == (N, 4) and totals.dtype == np.int64
    streams = res["bit_streams"]
    assert len(streams) == N
    for b in range(N):
        units, records = per_element[b]
        assert int(totals[b].sum()) == units
        diff, lo, hi = R.bound(len(streams[b]), int(totals[b].sum()), records)
        print("element", b, "bytes", len(streams[b]), "bits of the map", units / R.UNIT, "difference", diff, "bound", lo, hi)
        assert lo <= diff <= hi, (b, diff, lo, hi)
    cells = bm.cells()
    assert cells.shape == (N, bm.hc, bm.wc)
    assert np.allclose(cells.sum(axis=(1, 2)), totals.sum(axis=1) / R.UNIT, rtol=1e-12, atol=0)
    return totals


def _clip(h, w, batch):
    fr = frames(31, 3, h, w)
    xs = [pad_frame(torch.from_numpy(fr[t:t + 1]).to(DEV)) for t in range(3)]
    return [x.expand(batch, -1, -1, -1).contiguous() for x in xs]


def _q(batch, a, b):
    return a if batch == 1 else torch.tensor([a, b], device=DEV)


@pytest.mark.parametrize("case", ["64x64", "72x104", "72x104-qmap", "64x64-batch2"])
def test_codecs_bit_maps_equal_the_restatement_and_leave_the_bytes_alone(seeded_nets, case):
    """I + 2 P: compress(bit_map=True) returns the bytes and the DPB of bit_map=False; the six maps are the restatement
    applied to the staged symbol planes; 8 * len(bit_stream) - totals.sum() / 65536 lies in the coder's bound.  With a
    q-scale map; with a batch of two rate points: one stream and one total per element."""
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
    qi, qm, qy = _q(batch, 1.0, 0.6), _q(batch, 1.0, 1.3), _q(batch, 1.0, 0.7)
    plain = i.compress(xs[0], qi, q_map=q_map)
    assert "bit_map" not in plain
    keep = (plain["bit_streams"], plain["x_hat"].clone())
    res = i.compress(xs[0], qi, q_map=q_map, bit_map=True)
    assert res["bit_streams"] == keep[0] and torch.equal(res["x_hat"], keep[1])
    assert set(res) == set(plain) | {"bit_map"}
    tot = _check_picture(i, _i_groups(i, res["_views"]), res, batch)
    assert (tot[:, :2] == 0).all() and res["bit_map"].maps["mv_y"] is None  # an I picture has no mv maps
    if batch == 2:
        assert tot[0].sum() != tot[1].sum()
    dpb = U.intra_dpb(keep[1])
    for t in (1, 2):
        plain = d.compress(xs[t], dpb, qm, qy, q_map=q_map)
        assert "bit_map" not in plain
        keep = (plain["bit_streams"], {k: v.clone() for k, v in plain["dpb"].items()})
        res = d.compress(xs[t], dpb, qm, qy, q_map=q_map, bit_map=True)
        assert res["bit_streams"] == keep[0] and all(torch.equal(res["dpb"][k], keep[1][k]) for k in keep[1])
        assert set(res) == set(plain) | {"bit_map"}
        tot = _check_picture(d, _p_groups(res["_views"]), res, batch)
        assert (tot > 0).all()
        dpb = keep[1]


def test_bit_maps_with_defer_and_the_device_coder(seeded_nets):
    """defer=True carries the map beside the pending stream; coder="device" codes other bytes from the same planes, so
    the maps are the host coder's."""
    d, i = seeded_nets
    xs = _clip(64, 64, 1)
    ref = i.compress(xs[0], 1.0, bit_map=True)
    want_i, x_hat = ref["bit_map"].totals(), ref["x_hat"].clone()
    r = i.compress(xs[0], 1.0, defer=True, bit_map=True)
    assert "bit_stream" not in r and np.array_equal(r["bit_map"].totals(), want_i)
    assert r["pending"].finish() == ref["bit_stream"]
    dpb = U.intra_dpb(x_hat)
    ref = d.compress(xs[1], dpb, 1.0, 1.0, bit_map=True)
    want_p = {k: v.clone() for k, v in ref["bit_map"].maps.items()}
    r = d.compress(xs[1], dpb, 1.0, 1.0, defer=True, bit_map=True)
    assert r["pending"].finish() == ref["bit_stream"]
    assert all(torch.equal(r["bit_map"].maps[k], want_p[k]) for k in want_p)
    r = d.compress(xs[1], dpb, 1.0, 1.0, coder="device", bit_map=True)
    assert r["bit_stream"][:4] == b"DGR1" and all(torch.equal(r["bit_map"].maps[k], want_p[k]) for k in want_p)
    r = i.compress(xs[0], 1.0, coder="device", bit_map=True)
    assert np.array_equal(r["bit_map"].totals(), want_i)


def test_graph_replay_with_a_bit_map_is_refused(seeded_nets):
    d, _ = seeded_nets
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    with pytest.raises(NotImplementedError, match="bit_map.*graph"):
        d.compress(x, U.intra_dpb(x), 1.0, 1.0, graph=True, bit_map=True)
    from vcm_ts_amd.pipeline import GopEncoder

    enc = GopEncoder(seeded_nets[1], seeded_nets[0], gop_size=2, graphs=True)
    with pytest.raises(NotImplementedError, match="bit_maps"):
        enc.encode_gop([x, x], 1.0, 1.0, 1.0, bit_maps=lambda t, b: None)


# ---------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW = 4, 6, 176, 192  # (a report takes MS-SSIM, whose five levels need sides above 160)
SH, SW = 64, 96
BOX = [[16, 16, 48, 40, 0]]
ROIQ = X.RoiQ(140, (60,), 8)
TODAY = {"frame_pixel_num", "i_frame_num", "p_frame_num", "frame_bpp", "frame_psnr", "frame_msssim", "frame_type",
         "frame_psnr_roi", "frame_psnr_bg", "frame_roi_pixels"} | \
        {f"ave_{k}_frame_{m}" for k in ("i", "p", "all") for m in ("bpp", "psnr", "msssim")}
NEW = set(("frame_bits_mv_z", "frame_bits_mv_y", "frame_bits_z", "frame_bits_y"))


def _roi():
    return X.Roi(lambda t: X.FrameBoxes(BOX), (X.RoiClass(0),), ("plate",))


def _write_clip(folder, h, w):
    U.write_pngs(folder, np.rint(frames(21, N_FRAMES, h, w) * 255).astype(np.uint8).transpose(0, 2, 3, 1))


def test_file_loop_reports_regional_bits_and_writes_the_same_bins(tmp_path):
    """6 pictures, GOP 4.  The report is taken at 176 x 192 -- the smallest kind of size a report exists for: it measures
    MS-SSIM, which refuses sides up to 160 -- and 6 pictures of 64 x 96 go through the loop with a folder and no report."""
    from vcm_ts_amd import run_codec as RC

    file_nets = RC._nets(DEV, None)
    _write_clip(tmp_path / "png", FH, FW)
    _write_clip(tmp_path / "small", SH, SW)
    small = dict(gop=GOP, nets=file_nets, roi=_roi(), roi_q=ROIQ)
    sbits, ssize = RC.encode_folder(str(tmp_path / "small"), str(tmp_path / "sbins"), bit_map=str(tmp_path / "smaps"), **small)
    RC.encode_folder(str(tmp_path / "small"), str(tmp_path / "splain"), **small)
    assert U.bins(tmp_path / "sbins") == U.bins(tmp_path / "splain") and ssize == (SH, SW)
    for g in range(N_FRAMES):
        cells = np.load(tmp_path / "smaps" / f"im{g + 1:05d}.npy")
        assert cells.shape == (1,) + X.grid_of(SH, SW) and float(cells.min()) > 0
        intra = g % GOP == 0
        symbols = 32 * 192 + 2 * 192 if intra else 32 * (96 + 64) + 2 * 128
        diff, lo, hi = R.bound((sbits[g] - 8 * (14 if intra else 8)) // 8, round(float(cells.sum()) * R.UNIT), 10 * symbols)
        assert lo <= diff <= hi, (g, diff, lo, hi)
    common = dict(gop=GOP, nets=file_nets, roi=_roi(), roi_q=ROIQ)
    _, _, plain = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "plain"), report=True, **common)
    assert set(plain) == TODAY  # without bit_map: exactly the keys there were
    report = str(tmp_path / "report.json")
    bits, size, rd = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), report=report,
                                      bit_map=str(tmp_path / "maps"), **common)
    assert U.bins(tmp_path / "bins") == U.bins(tmp_path / "plain") and len(bits) == N_FRAMES and size == (FH, FW)
    assert set(rd) == TODAY | NEW | {"frame_bits_roi", "frame_bits_bg", "frame_roi_cells"}
    assert json.loads(open(report).read()) == rd
    assert all(rd[k] == plain[k] for k in ("frame_bpp", "frame_type", "frame_roi_pixels", "frame_pixel_num"))
    hc, wc = X.grid_of(FH, FW)
    # box [16, 48) x [16, 40) grown by 8: columns [8, 56) -> cells 0..3, rows [8, 48) -> cells 0..2
    assert rd["frame_roi_cells"] == [12] * N_FRAMES
    assert rd["frame_type"] == [0, 1, 1, 1, 0, 1]
    for g in range(N_FRAMES):
        parts = [rd[k][g] for k in ("frame_bits_mv_z", "frame_bits_mv_y", "frame_bits_z", "frame_bits_y")]
        assert all(isinstance(p, float) for p in parts) and parts[2] > 0 and parts[3] > 0
        assert (parts[0] == 0 and parts[1] == 0) if rd["frame_type"][g] == 0 else (parts[0] > 0 and parts[1] > 0)
        # (every value is an integer number of 2^-20 bit far below 2^53 of them: float64 sums of them are exact)
        total = sum(parts)
        assert rd["frame_bits_roi"][g] > 0 and rd["frame_bits_bg"][g] > 0
        assert rd["frame_bits_roi"][g] + rd["frame_bits_bg"][g] == total
        cells = np.load(tmp_path / "maps" / f"im{g + 1:05d}.npy")
        assert cells.shape == (1, hc, wc) and cells.dtype == np.float64
        assert float(cells.sum()) == total
        assert float(cells[0, :3, :4].sum()) == rd["frame_bits_roi"][g]
        # the payload behind the header (14 bytes for an I picture, 8 for a P picture) against the map: the coder's bound
        # with the largest record count there can be -- every symbol of the picture an escape of 8 nibbles, 10 records
        cells_n = hc * wc
        symbols = cells_n * 192 + cells_n // 16 * 192 if rd["frame_type"][g] == 0 else cells_n * (96 + 64) + cells_n // 16 * 128
        diff, lo, hi = R.bound((bits[g] - 8 * (14 if rd["frame_type"][g] == 0 else 8)) // 8, round(total * R.UNIT), 10 * symbols)
        print("picture", g, "difference", diff, "bound", lo, hi)
        assert lo <= diff <= hi, (g, diff, lo, hi)
    assert sorted(os.listdir(tmp_path / "maps")) == [f"im{g + 1:05d}.npy" for g in range(N_FRAMES)]
    # a folder without a report: the maps only, the return value of a run without a report; two GOP streams, no ROI
    out = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins2"), gop=GOP, nets=[file_nets, RC._nets(DEV, None)],
                           gop_streams=2, bit_map=str(tmp_path / "maps2"))
    assert len(out) == 2
    _, _, rd2 = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins3"), gop=GOP, nets=file_nets, report=True, bit_map=True)
    assert set(rd2) == (TODAY - {"frame_psnr_roi", "frame_psnr_bg", "frame_roi_pixels"}) | NEW
    assert U.bins(tmp_path / "bins2") == U.bins(tmp_path / "bins3")
    for g in range(N_FRAMES):
        cells = np.load(tmp_path / "maps2" / f"im{g + 1:05d}.npy")
        assert float(cells.sum()) == sum(rd2[k][g] for k in NEW)
    with pytest.raises(ValueError, match="bit_map=True needs report"):
        RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "x"), gop=GOP, nets=file_nets, bit_map=True)
