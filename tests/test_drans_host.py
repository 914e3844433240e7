"""Host side of the device entropy coder (include/dcvc_hip_rans.h) without a GPU: dcvc_drans_build_lut as the validity
check of a table (the kernels stage rows as 16-bit values and trust them: a row of one bin, an empty bin, a row that does
not span 0..65536 must never reach them), the LUT it builds against a plain search, the entry points' refusals (a
refused call launches nothing) and the synthetic tables of tests/drans_ref.py themselves."""
import numpy as np
import pytest

from tests import drans_ref as T
from tests.util import golden
from vcm_ts_amd import lib

P = 0x10000  # an aligned dummy pointer: a refused call returns before anything is launched or dereferenced
E_ARG = -1


def build_lut(cdf, sizes, stride=None):
    cdf, sizes = np.ascontiguousarray(cdf, np.int32), np.ascontiguousarray(sizes, np.int32)
    lut = np.zeros((cdf.shape[0], 256), np.uint8)
    rc = lib.hip().dcvc_drans_build_lut(cdf.ctypes.data, cdf.shape[0], stride or cdf.shape[1], sizes.ctypes.data, lut.ctypes.data)
    return rc, lut


def _model_tables():
    t = golden("tables")
    return {k: (t[k + "_cdf"], t[k + "_len"], t[k + "_off"]) for k in ("dmc_scale", "intra_scale", "dmc_z", "dmc_zmv", "intra_z")}


# ------------------------------------------------------------------------------------------------------------ the LUT
@pytest.mark.parametrize("name", T.NAMES + ("dmc_scale", "intra_scale", "dmc_z", "dmc_zmv", "intra_z"))
def test_lut_is_the_bin_of_every_bucket_start(name):
    tab = T.table(name) if name in T.NAMES else _model_tables()[name]
    rc, lut = build_lut(tab[0], tab[1])
    assert rc == 0
    np.testing.assert_array_equal(lut, T.lut_by_search(tab))
    assert lut.max() <= tab[1].max() - 2                       # never the entry behind the sentinel
    if name == "wide":
        assert lut.max() == 254 and (lut[0, 255], lut[1, 255]) == (254, 254)
    if name == "flat":
        assert lut[0, 0] == 0 and lut[0, 1] == 200             # bucket 0 starts 200 bins before bucket 1


def test_synthetic_tables_are_what_their_names_promise():
    tabs = T.tables()
    for name, (cdf, sizes, offsets) in tabs.items():
        assert cdf.dtype == sizes.dtype == offsets.dtype == np.int32 and cdf.shape[0] == sizes.size == offsets.size, name
        for r, s in enumerate(sizes.tolist()):
            row = cdf[r, :s].astype(np.int64)
            assert 3 <= s <= cdf.shape[1] and row[0] == 0 and row[-1] == 65536 and (np.diff(row) >= 1).all(), (name, r)
            assert not cdf[r, s:].any()
    w = np.diff(tabs["flat"][0][0].astype(np.int64))
    assert tabs["flat"][0].shape == (1, 203) and w.tolist() == [1] * 200 + [65335, 1]
    assert tabs["wide"][0].shape == (4, 256) and (tabs["wide"][1] == 256).all()
    in_bucket = [np.bincount(tabs["wide"][0][r, :255] >> 8, minlength=256).max() for r in range(4)]
    assert in_bucket[1] > 5 and max(in_bucket) < 255           # more than four bins behind one LUT byte
    assert tabs["tiny"][0].tolist() == [[0, 65535, 65536], [0, 1, 65536]]
    assert tabs["odd"][0].size == 21 and tabs["odd"][0].size % 4 == 1
    assert tabs["full"][0].size == 32768 and tabs["full"][0].shape == (256, 128)
    assert (tabs["full"][1].min(), tabs["full"][1].max()) == (3, 128)
    assert (tabs["full"][2].min(), tabs["full"][2].max()) == (-64, 5)
    assert tabs["one"][0].shape[0] == 1
    for name, tab in tabs.items():
        sym, idx = T.covering_symbols(tab)
        T.assert_covered(sym, idx, tab)
        assert sym.size <= 5000, (name, sym.size)


def test_escape_values_span_every_nibble_count():
    raws = T.escape_raws()
    assert raws[0] == (0, 0) and max(r for _, r in raws) == 2 ** 31 - 1
    for k in range(1, 9):
        mine = [r for kk, r in raws if kk == k]
        assert all(T.nibbles(r) == k for r in mine)
        assert {r & 1 for r in mine} == {0, 1} and min(mine) <= (1 << 4 * (k - 1)) + 1 and max(mine) == min(16 ** k, 2 ** 31) - 1
    cdf, sizes, offsets = T.table("full")
    for row in (31, 11):
        for _, raw in raws:
            s = T.escape_symbol(raw, sizes[row], offsets[row])
            assert -2 ** 31 <= s < 2 ** 31
            b, back = T.classify(np.array([s]), np.array([row]), sizes, offsets)
            assert back[0] == raw and b[0] == sizes[row] - 2


# ------------------------------------------------------------------------------------------------- refused tables
def test_build_lut_refuses_rows_the_kernels_cannot_code():
    good = np.array([[0, 10, 65536, 0], [0, 1, 2, 65536]], np.int32)
    sizes = np.array([3, 4], np.int32)
    assert build_lut(good, sizes)[0] == 0

    def refused(cdf, sz=sizes):
        return build_lut(np.array(cdf, np.int32), np.array(sz, np.int32))[0] == E_ARG

    assert refused([[0, 65536, 0, 0], [0, 1, 2, 65536]], [2, 4])        # ONE bin of width 65536: 0 in 16 bits, a division by it
    assert refused(good, [3, 1]) and refused(good, [0, 4]) and refused(good, [3, -1])
    assert refused(good, [3, 5])                                         # longer than the stride
    assert refused([[1, 10, 65536, 0], [0, 1, 2, 65536]])                # does not start at 0
    assert refused([[0, 10, 65535, 0], [0, 1, 2, 65536]])                # does not end at 65536
    assert refused([[0, 10, 65536, 0], [0, 1, 2, 65537]])
    assert refused([[0, 10, 65536, 0], [0, 1, 1, 65536]])                # an empty bin
    assert refused([[0, 10, 65536, 0], [0, 0, 2, 65536]])
    assert refused([[0, 10, 65536, 0], [0, 2, 65536, 65536]])            # an empty sentinel bin
    assert refused([[0, 10, 65536, 0], [0, 5, 3, 65536]])                # a decreasing row
    assert refused([[0, 10, 65536, 7], [0, 1, 2, 65536]]) is False       # what lies behind a row's size is not looked at
    L = lib.hip()
    ok = dict(cdfs=good.ctypes.data, n=2, stride=4, sizes=sizes.ctypes.data, lut=np.zeros(512, np.uint8).ctypes.data)
    for over in (dict(cdfs=None), dict(sizes=None), dict(lut=None), dict(n=0), dict(n=-1), dict(n=257), dict(stride=1),
                 dict(stride=257)):
        v = dict(ok, **over)
        assert L.dcvc_drans_build_lut(v["cdfs"], v["n"], v["stride"], v["sizes"], v["lut"]) == E_ARG, over


def test_device_coder_refuses_a_bad_table_before_any_launch():
    """DeviceCoder.__init__ builds the LUT first: a table the kernels cannot code raises there, whatever the device."""
    import torch

    from vcm_ts_amd import entropy as E

    bad = (np.array([[0, 65536]], np.int32), np.array([2], np.int32), np.array([0], np.int32))
    with pytest.raises(lib.KernelError, match="drans_build_lut"):
        E.DeviceCoder(torch.device("cpu"), {"bad": bad})


# ------------------------------------------------------------------------------------------------- the entry points
_ENC = "sym idx chan_hw chan_c n cdfs n_cdfs stride sizes offsets lanes scratch scratch_words payload payload_words cursor_in " \
       "cursor_out status".split()
_DEC = "payload payload_words cursor_in cursor_out idx chan_hw chan_c n cdfs n_cdfs stride sizes offsets lut lanes out " \
       "status".split()
_OK = dict(sym=P, idx=P, chan_hw=0, chan_c=0, n=1000, cdfs=P, n_cdfs=64, stride=103, sizes=P, offsets=P, lanes=64, scratch=P,
           scratch_words=1 << 20, payload=P, payload_words=1 << 20, cursor_in=P, cursor_out=P + 8, status=P + 4, lut=P, out=P)


def _call(name, order, over):
    vals = dict(_OK, **over)
    assert len(order) + 1 == len(lib._SIGS[name])  # the header's order, plus the stream
    return getattr(lib.hip(), name)(*[vals[k] for k in order], None)


_BOTH = (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(lanes=0), dict(lanes=-64), dict(lanes=8193), dict(cursor_out=P),
         dict(cursor_in=None), dict(cursor_out=None), dict(status=None), dict(cdfs=None), dict(sizes=None), dict(offsets=None),
         dict(payload=None), dict(n_cdfs=0), dict(n_cdfs=-1), dict(stride=1), dict(cdfs=P + 4),
         dict(n_cdfs=10923, stride=3),                    # 32769 entries
         dict(n_cdfs=255, stride=129),                    # 32895
         dict(idx=None), dict(idx=None, chan_hw=7, chan_c=0), dict(idx=None, chan_hw=0, chan_c=5))


def test_encode_entry_point_refuses_null_empty_and_oversized_arguments():
    for over in _BOTH + (dict(sym=None), dict(scratch=None),
                         dict(scratch_words=lib.hip().dcvc_drans_scratch_words(1000, 64) - 1)):
        assert _call("dcvc_drans_encode", _ENC, over) == E_ARG, over


def test_decode_entry_point_refuses_null_empty_and_oversized_arguments():
    for over in _BOTH + (dict(lut=None), dict(out=None), dict(lut=P + 2), dict(stride=257, n_cdfs=100), dict(n_cdfs=257, stride=100)):
        assert _call("dcvc_drans_decode", _DEC, over) == E_ARG, over


def test_scratch_words_and_default_lanes():
    L = lib.hip()
    for n, lanes in ((-1, 64), (10, 0), (10, -1), (10, 8193)):
        assert L.dcvc_drans_scratch_words(n, lanes) == E_ARG, (n, lanes)
    # 2 words per symbol of a lane + 8, and one word per lane for its size: the format's worst symbol is a sentinel of
    # width 1 (16 bits), the count nibble and eight value nibbles, 52 bits < 2 words
    for n, lanes in ((1, 1), (1, 64), (65, 64), (4096, 64), (9000, 8192), (1000, 1), (0, 64)):
        per_lane = -(-n // lanes)
        assert L.dcvc_drans_scratch_words(n, lanes) == lanes * (2 * per_lane + 8) + lanes, (n, lanes)
    assert L.dcvc_drans_scratch_words(10, 8192) > 0
    for n, want in ((1, 64), (512 * 64, 64), (512 * 64 + 1, 128), (10 ** 7, 1024)):
        assert L.dcvc_drans_default_lanes(n) == want
