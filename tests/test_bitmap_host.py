"""Per-cell bit maps without a GPU: the restatement the GPU tests compare with (tests/bitmap_ref.py) checked against the
entropy coders themselves -- the sum of the code lengths against the length of the byte string, inside the bound that
follows from the rANS update rule --, the host-built cost arrays, the argument checks of the Python layer,
the entry points' refusals (a refused call launches nothing) and the command line's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import rans_py
from tests import bitmap_ref as R
from vcm_ts_amd import bitmap as B
from vcm_ts_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000  # an aligned dummy pointer: a refused call returns before anything is launched or dereferenced


# ------------------------------------------------------------------------------------- the restatement against the coders
def _lib_encode(sym, idx, table):
    from vcm_ts_amd.entropy import BufferedRansEncoder

    enc = BufferedRansEncoder()
    enc.encode_with_indexes(sym, idx, *table)
    return enc.flush()


def _have_rans():
    return os.path.exists(os.path.join(lib.CSRC, "libdcvc_rans.so"))


CASES = [(seed, n) for seed, n in enumerate([1, 2, 3, 7, 50, 400, 3000, 20000])]


@pytest.mark.parametrize("seed,n", CASES, ids=lambda v: str(v))
def test_sum_of_code_lengths_against_the_coders_bytes(seed, n):
    """32 - t <= 8 * len(bytes) - sum_bits <= 64 + 1e-4 * records + t, t = records * 2^-17: the state starts at 2^31 and
    ends in [2^31, 2^63), every emitted word carries 32 bits, each division and each shift of the update loses at most
    log2(1 / (1 - 2^-15)) < 1e-4 bit, and the LUT rounds each cost to the nearest 2^-16 bit."""
    rng = np.random.default_rng(100 + seed)
    table = R.random_table(rng, 9)
    sym, idx = R.random_symbols(rng, table, n)
    if n >= 400:  # every row, the corner rows (sentinel only, frequencies 1 and 65535) and both signs of escape among them
        assert set(idx.tolist()) == set(range(9))
        v = sym - table[2][idx]
        assert (v < 0).any() and (v >= table[1][idx] - 2).any()
    units, records = R.stream_cost(sym, idx, table)
    assert records >= n
    streams = {"python": rans_py.encode([(sym, idx, *table)])}
    if _have_rans():
        streams["library"] = _lib_encode(sym, idx, table)
        assert streams["library"] == streams["python"]
    for name, data in streams.items():
        diff, lo, hi = R.bound(len(data), units, records)
        print(name, "symbols", n, "records", records, "bytes", len(data), "difference", diff, "bound", lo, hi)
        assert lo <= diff <= hi, (name, diff, lo, hi)


def test_escape_lengths_up_to_eight_nibbles():
    """Only escapes, of every nibble count and both signs, through a row whose sentinel has frequency 1."""
    table = (np.array([[0, 65535, 65536]], dtype=np.int32), np.array([3], dtype=np.int32), np.array([0], dtype=np.int32))
    sym = []
    for nib in range(0, 9):
        raw_lo = 1 << (4 * max(nib - 1, 0))
        for raw in ({raw_lo, raw_lo + 1, (1 << (4 * nib)) - 1, (1 << (4 * nib)) - 2} if nib else {0}):
            v = -(raw + 1) // 2 if raw & 1 else 1 + raw // 2
            if -2 ** 31 <= v < 2 ** 31:
                sym.append(v)
                assert R.symbol_cost(*table, 0, v) == (R.lut(1) + 4 * R.UNIT * (1 + nib), 2 + nib), (nib, raw)
    sym = np.array(sym, dtype=np.int32)
    idx = np.zeros(len(sym), dtype=np.int32)
    units, records = R.stream_cost(sym, idx, table)
    data = rans_py.encode([(sym, idx, *table)])
    assert rans_py.Decoder(data).decode(idx, *table) == sym.tolist()
    diff, lo, hi = R.bound(len(data), units, records)
    assert lo <= diff <= hi
    if _have_rans():
        assert _lib_encode(sym, idx, table) == data


def test_library_coder_codes_a_sentinel_only_row():
    """A frequency of 2^16 leaves the coder's state alone: the library writes what the pure-Python coder writes, and
    reads it back (its packed record has 16 bits for the frequency).  Escapes of up to 7 nibbles: the library's decoder
    takes the escape value as an int32, so one of 8 nibbles with its top bit set does not come back."""
    if not _have_rans():
        pytest.skip("libdcvc_rans.so not built")
    from vcm_ts_amd.entropy import RansDecoder

    rng = np.random.default_rng(5)
    table = R.random_table(rng, 4)
    sym, idx = R.random_symbols(rng, table, 300, rows=rng.integers(0, 2, 300), max_nib=7)
    assert (idx == 0).sum() > 50
    data = _lib_encode(sym, idx, table)
    assert data == rans_py.encode([(sym, idx, *table)])
    dec = RansDecoder()
    dec.set_stream(data)
    assert np.array_equal(dec.decode_stream(idx, *table), sym)


# --------------------------------------------------------------------------------------------------------- cost arrays
def test_cost_lut_and_cost_array_equal_the_restatement():
    lut = B.cost_lut()
    assert lut.dtype == np.int32 and lut.shape == (65537,)
    assert [int(lut[f]) for f in (1, 2, 3, 65535, 65536)] == [R.lut(f) for f in (1, 2, 3, 65535, 65536)]
    assert int(lut[1]) == 16 * R.UNIT and int(lut[65536]) == 0 and int(lut[65535]) == 1
    g = np.random.default_rng(0)
    for f in g.integers(1, 65537, 2000).tolist():
        assert int(lut[f]) == R.lut(f), f
    cdf, sizes, offsets = R.random_table(g, 12)
    cost = B.cost_array(cdf, sizes, offsets)
    assert cost.shape == cdf.shape and cost.dtype == np.int32
    for r in range(12):
        for s in range(cdf.shape[1]):
            want = R.lut(int(cdf[r, s + 1]) - int(cdf[r, s])) if s <= sizes[r] - 2 else 0
            assert int(cost[r, s]) == want, (r, s)


def test_cost_tables_refuse_bad_tables():
    cdf, sizes, offsets = R.random_table(np.random.default_rng(1), 12)
    assert set(B.CostTables({"a": (cdf, sizes, offsets)}).host) == {"a"}
    r = int(np.argmax(sizes))
    assert sizes[r] > 3 and r > 2
    zero = cdf.copy()
    zero[r, 2] = zero[r, 1]                       # a zero frequency inside the used part of a row
    with pytest.raises(ValueError, match=rf"a: row {r} slot 1 has frequency 0"):
        B.CostTables({"a": (zero, sizes, offsets)})
    big = cdf.copy()
    big[5, sizes[5] - 1] = 65536 + big[5, sizes[5] - 2] + 1  # above 65536
    with pytest.raises(ValueError, match="frequency"):
        B.CostTables({"a": (big, sizes, offsets)})
    down = cdf.copy()
    down[3, 1] = -5                               # a decreasing CDF: a negative frequency
    with pytest.raises(ValueError, match="frequency"):
        B.CostTables({"a": (down, sizes, offsets)})
    for bad in (1, 0, -3, cdf.shape[1] + 1):
        s = sizes.copy()
        s[2] = bad
        with pytest.raises(ValueError, match=rf"row 2 has size {bad}"):
            B.CostTables({"a": (cdf, s, offsets)})
    with pytest.raises(ValueError, match="sizes and offsets"):
        B.CostTables({"a": (cdf, sizes[:-1], offsets)})
    with pytest.raises(ValueError, match="integer CDF"):
        B.CostTables({"a": (cdf.astype(np.float32), sizes, offsets)})
    with pytest.raises(ValueError, match="integer CDF"):
        B.CostTables({"a": (cdf[:, :1], sizes, offsets)})
    # what lies beyond a row's size is not looked at
    junk = cdf.copy()
    junk[0, 2:] = -7
    assert np.array_equal(B.cost_array(junk, sizes, offsets), B.cost_array(cdf, sizes, offsets))


# ------------------------------------------------------------------------------------------------ Python argument checks
def _host_bitmap(N=1, hc=4, wc=8):
    maps = {"y": np.zeros((N, hc, wc), np.int32), "z": np.zeros((N, hc // 4, wc // 4), np.int32)}
    return B.BitMap(maps, None, N, hc, wc)


def test_bitmap_shapes_and_region_arguments():
    b = _host_bitmap(2, 4, 8)
    assert b.maps["mv_y"] is None and b.maps["mv_z"] is None and (b.N, b.hc, b.wc) == (2, 4, 8)
    good = np.zeros((4, 8), np.uint8)
    for labels, K, match in ((good, 0, "K"), (good, 9, "K"), (good, True, "K"), (good, 2.0, "K"),
                             (good.astype(np.int32), 2, "uint8"), ([[0] * 8] * 4, 2, "uint8"),
                             (np.zeros((8, 4), np.uint8), 2, "shape"), (np.zeros((3, 4, 8), np.uint8), 2, "shape"),
                             (np.zeros((1, 1, 4, 8), np.uint8), 2, "shape")):
        with pytest.raises(ValueError, match=match):
            b.regions(labels, K)
    for shape in ((4, 8), (1, 4, 8), (2, 4, 8)):
        with pytest.raises(ValueError, match="GPU"):  # the arguments are fine; maps on the host are not (no CPU fallback)
            b.regions(np.zeros(shape, np.uint8), 8)
    with pytest.raises(ValueError, match="GPU"):
        b.cells()
    with pytest.raises(ValueError, match="multiple of 4"):
        B.BitMap({"y": np.zeros((1, 5, 7), np.int32)}, None, 1, 5, 7)
    with pytest.raises(ValueError, match="at least one map"):
        B.BitMap({}, None, 1, 4, 4)
    with pytest.raises(ValueError, match="map z: expected shape"):
        B.BitMap({"y": np.zeros((1, 4, 8), np.int32), "z": np.zeros((1, 4, 8), np.int32)}, None, 1, 4, 8)
    with pytest.raises(ValueError, match="3 or 6"):
        B.BitMap.from_planes({}, [None] * 4, 1)


def test_bitmap_decode_reads_sums_and_status():
    row = np.arange(2 * 3 * 4 + 1, dtype=np.int64)
    row[-1] = 0
    sums = B.BitMap.decode(row, 2, 3)
    assert sums.shape == (2, 3, 4) and sums.dtype == np.int64 and sums[1, 2, 3] == 23
    for status, word in ((B.BAD_INDEX, "CDF row"), (B.BAD_LABEL, "label")):
        row[-1] = status
        with pytest.raises(B.BitMapError, match=word):
            B.BitMap.decode(row, 2, 3)


def test_labels_from_boxes_argument_checks():
    for grow in (-1, 256, 1.5, True):
        with pytest.raises(ValueError, match="grow"):
            B.labels_from_boxes(np.zeros((0, 5), np.int32), 64, 64, grow)
    with pytest.raises(ValueError, match="boxes"):
        B.labels_from_boxes(np.zeros((2, 4), np.int32), 64, 64)
    with pytest.raises(ValueError, match="sides"):
        B.labels_from_boxes(np.zeros((0, 5), np.int32), 0, 64)
    with pytest.raises(ValueError, match="out of range"):
        B.labels_from_boxes(np.array([[0, 0, 65, 10, 0]]), 64, 64)
    with pytest.raises(ValueError, match="unknown class"):
        B.labels_from_boxes(np.array([[0, 0, 64, 10, 4]]), 64, 64)


def test_file_loop_arguments():
    from vcm_ts_amd import run_codec as RC

    assert RC._bitmap_args(None, None) is None and RC._bitmap_args(False, "r.json") is None
    assert RC._bitmap_args(True, "r.json") is None and RC._bitmap_args(True, True) is None
    assert RC._bitmap_args("maps", None) == "maps"
    with pytest.raises(ValueError, match="bit_map=True needs report"):
        RC._bitmap_args(True, None)
    with pytest.raises(ValueError, match="bit_map"):
        RC._bitmap_args(3, "r.json")
    assert RC.BIT_KEYS == tuple(f"frame_bits_{c}" for c in B.COMPONENTS)


# ------------------------------------------------------------------------------------------------------------ the C ABI
_SCALE = "sym0 idx0 sym1 idx1 cost n_rows stride sizes offsets map N C H W status".split()
_FACT = "sym cost n_rows stride sizes offsets map N C H W status".split()
_REG = "maps labels K sums N hc wc status".split()


def _call(name, order, ok, over):
    vals = dict(ok, **over)
    assert len(order) + 1 == len(lib._SIGS[name])  # the header's order, plus the stream
    return getattr(lib.hip(), name)(*[vals[k] for k in order], None)


def test_map_entry_points_refuse_null_empty_and_odd_arguments():
    ok = dict(sym0=P, idx0=P, sym1=P, idx1=P, sym=P, cost=P, n_rows=64, stride=8, sizes=P, offsets=P, map=P, N=2, C=6, H=3, W=5,
              status=P)
    for ptr in ("sym0", "idx0", "sym1", "idx1", "cost", "sizes", "offsets", "map", "status"):
        assert _call("dcvc_bits_map_scale", _SCALE, ok, {ptr: None}) == -1, ptr
    for ptr in ("sym", "cost", "sizes", "offsets", "map", "status"):
        assert _call("dcvc_bits_map_factorized", _FACT, ok, {ptr: None}) == -1, ptr
    common = (dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=2049), dict(W=2049), dict(n_rows=0),
              dict(n_rows=65537), dict(stride=1), dict(C=0), dict(C=-2), dict(C=514))
    for over in common + (dict(C=5), dict(C=1), dict(C=511)):
        assert _call("dcvc_bits_map_scale", _SCALE, ok, over) == -1, over
    for over in common + (dict(C=65, n_rows=64), dict(C=513, n_rows=1024)):
        assert _call("dcvc_bits_map_factorized", _FACT, ok, over) == -1, over


def test_region_entry_point_refuses_null_empty_and_odd_arguments():
    four = (C.c_void_p * 4)(None, None, None, P)
    none = (C.c_void_p * 4)()
    ok = dict(maps=four, labels=P, K=2, sums=P, N=1, hc=4, wc=8, status=P)
    for over in (dict(maps=None), dict(maps=none), dict(labels=None), dict(sums=None), dict(status=None), dict(sums=P + 4),
                 dict(K=0), dict(K=9), dict(N=0), dict(N=65536), dict(hc=0), dict(wc=0), dict(hc=5), dict(wc=7), dict(hc=2),
                 dict(hc=2052), dict(wc=-4)):
        assert _call("dcvc_bits_regions", _REG, ok, over) == -1, over


def test_bindings_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "dcvc_hip_bits.h")).read()
    for macro, value in (("DCVC_BITS_UNIT", B.UNIT), ("DCVC_BITS_MAX_C", B.MAX_C), ("DCVC_BITS_MAX_LABELS", B.MAX_LABELS),
                         ("DCVC_BITS_BAD_INDEX", B.BAD_INDEX), ("DCVC_BITS_BAD_LABEL", B.BAD_LABEL)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert B.REGION_UNIT == 16 * B.UNIT == R.REGION_UNIT and B.UNIT == R.UNIT


# --------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("argv", [
    ["encode", "--frames", "F", "--bins", "B", "--bit-map"],
    ["decode", "--bins", "B", "--recon", "R", "--height", "64", "--width", "96", "--bit-map"],
    ["decode", "--bins", "B", "--recon", "R", "--height", "64", "--width", "96", "--bit-map", "D"],
], ids=lambda a: " ".join(a[0:1] + a[-2:]))
def test_command_line_refuses_bit_map_without_a_destination(argv, tmp_path, monkeypatch, capsys):
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ex:
        RC.main(argv)
    err = capsys.readouterr().err
    assert ex.value.code == 2 and "error:" in err and "--bit-map" in err


def test_command_line_passes_bit_map_on(tmp_path, monkeypatch):
    from vcm_ts_amd import run_codec as RC

    monkeypatch.chdir(tmp_path)
    seen = {}

    def fake_encode(*args, **kw):
        seen.update(kw)
        return [8], (64, 64)

    monkeypatch.setattr(RC, "encode_folder", fake_encode)
    RC.main(["encode", "--frames", "F", "--bins", "B"])
    assert seen["bit_map"] is None
    RC.main(["encode", "--frames", "F", "--bins", "B", "--bit-map", "--report", "r.json"])
    assert seen["bit_map"] is True and seen["report"] == "r.json"
    RC.main(["encode", "--frames", "F", "--bins", "B", "--bit-map", "MAPS"])
    assert seen["bit_map"] == "MAPS" and seen["report"] is None
