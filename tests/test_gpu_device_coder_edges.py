"""The device entropy coder (vcm_ts_amd/csrc/rans_device.hip) at its edges on a real MI355X, with tables built for the
branches the model's own tables never or only by chance reach (tests/drans_ref.py): the decoder's bin search (bucket LUT,
four clamped probes, `while` loop), the 16-bit LDS image with a width of 65535, load_tables' scalar tail, the largest
accepted table (130 KB of LDS in the decoder), lane counts that are no multiple of 64 and up to 8192, 7 / 8 / 9 symbols
per lane around the batch of 8, escapes of every length, the worst-case plane that pins the scratch bound, the wrap of
channel-indexed rows and three sections with an odd word count in the middle.  Every case: the GPU's bytes equal the
format oracle's (oracle/drans_py.py), the GPU decodes them, and the oracle's decoder reads them."""
import numpy as np
import pytest
import torch

from oracle import drans_py as D
from tests import drans_ref as T
from tests.util import golden
from vcm_ts_amd import entropy as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def tabs():
    t = golden("tables")
    out = T.tables()
    out["scale"] = (t["dmc_scale_cdf"], t["dmc_scale_len"], t["dmc_scale_off"])
    return out


@pytest.fixture(scope="module")
def coder(tabs):
    return E.DeviceCoder(DEV, tabs, capacity_words=1 << 20)


def _host_lane_encoder(cdf, ln, off):
    enc = E.BufferedRansEncoder()

    def fn(s, i):  # the product's host coder: byte-identical to oracle/rans_py.py (tests/test_rans.py), but fast
        enc.reset()
        enc.encode_with_indexes(np.asarray(s, np.int32), np.asarray(i, np.int32), cdf, ln, off)
        return enc.flush()

    return fn


def run(coder, tabs, sections):
    """sections: [(table name, sym, idx or None, chan or None, lanes)].  Encode on the GPU (status 0, bytes == oracle),
    decode on the GPU (symbols, status 0), decode the GPU's bytes with the oracle."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
    coder.begin()
    plan = []
    for name, sym, idx, chan, lanes in sections:
        row = idx if idx is not None else (np.arange(sym.size) // chan[1]) % chan[0]
        plan.append((name, sym, row.astype(np.int32), None if idx is None else dev(idx), chan, lanes))
        coder.encode(name, dev(sym), plan[-1][3], chan=chan, lanes=lanes)
    got = coder.end().finish()                       # raises on a non-zero status (BAD_SPACE, BAD_INDEX)
    want = D.MAGIC
    for name, sym, row, _, _, lanes in plan:
        fn = None if sym.size <= 5000 else _host_lane_encoder(*tabs[name])
        want += D.encode_section(sym, row, *tabs[name], lanes=lanes, encode_fn=fn)
    assert len(got) == len(want) and got == want
    coder.set_stream(got)
    outs = [coder.decode(name, sym.size, idx=di, chan=chan, lanes=lanes) for name, sym, _, di, chan, lanes in plan]
    coder.check()
    coder.release()
    pos = 4
    for (name, sym, row, _, _, _), out in zip(plan, outs):
        np.testing.assert_array_equal(out.cpu().numpy(), sym, err_msg=name)
        assert sym.size <= 9000
        back, pos = D.decode_section(got, pos, row, *tabs[name])
        np.testing.assert_array_equal(back, sym, err_msg=name)
    assert pos == len(got)
    return got


# lanes: 64 (one full workgroup), 96 and 200 (a partial last workgroup), 33 (a partial only one), 1
@pytest.mark.parametrize("name,lanes,repeat", [("flat", 64, 8), ("wide", 96, 2), ("tiny", 33, 600), ("odd", 64, 150),
                                               ("full", 200, 1), ("one", 1, 100)])
def test_every_bin_of_every_synthetic_table(coder, tabs, name, lanes, repeat):
    sym, idx = T.covering_symbols(tabs[name], seed=1, repeat=repeat)
    T.assert_covered(sym, idx, tabs[name])
    assert 1000 <= sym.size <= 5000, sym.size
    run(coder, tabs, [(name, sym, idx, None, lanes)])


@pytest.mark.parametrize("n,lanes", [(1, 1), (1, 64), (63, 64), (64, 64), (65, 64), (7 * 65, 65), (8 * 65, 65), (8 * 65 + 1, 65),
                                     (9 * 100, 100), (1000, 1), (9000, 8192), (3 * 1000 + 17, 1000)])
def test_lane_and_length_edges_with_the_models_scale_table(coder, tabs, n, lanes):
    rng = np.random.default_rng(n * 10007 + lanes)
    idx = rng.integers(0, 256, n).astype(np.int32)
    sym = np.rint(rng.laplace(0, 6.0, n)).astype(np.int32)
    sym[::53] = 300
    sym[7 % n] = -100000
    run(coder, tabs, [("scale", sym, idx, None, lanes)])


@pytest.mark.parametrize("name,row", [("full", 31), ("full", 11), ("tiny", 0), ("tiny", 1)])
def test_escapes_of_every_length(coder, tabs, name, row):
    """0..8 value nibbles, both signs, the smallest and the largest value of each length (up to raw = 2^31 - 1), on a row
    with a negative offset (full 31: -64), one with a positive offset (full 11: +5) and the two rows of `tiny`."""
    _, sizes, offsets = tabs[name]
    assert (name, row) != ("full", 31) or offsets[row] < 0
    assert (name, row) != ("full", 11) or offsets[row] > 0
    sym = np.array([T.escape_symbol(raw, sizes[row], offsets[row]) for _, raw in T.escape_raws()], np.int64)
    assert sym.min() >= -2 ** 31 and sym.max() < 2 ** 31
    sym = np.concatenate([sym, [offsets[row]], sym[::-1]]).astype(np.int32)     # one ordinary symbol (bin 0) in between
    idx = np.full(sym.size, row, np.int32)
    _, raw = T.classify(sym, idx, sizes, offsets)
    assert {T.nibbles(r) for r in raw[raw >= 0].tolist()} == set(range(9)) and raw.max() == 2 ** 31 - 1
    for lanes in (1, 3):       # all of them in one stream, and spread over three
        run(coder, tabs, [(name, sym, idx, None, lanes)])


def test_worst_case_plane_fits_the_scratch_bound(coder, tabs):
    """4096 symbols on 64 lanes, every one the costliest the format has: the sentinel of `tiny` row 0 (width 1: 16 bits),
    the count nibble and eight value nibbles, 52 bits.  Two words per symbol + 8 per lane must hold them: status 0
    (DCVC_DRANS_BAD_SPACE would raise in finish()), the oracle's bytes, and the round trip."""
    cdf, sizes, offsets = tabs["tiny"]
    assert cdf[0, 2] - cdf[0, 1] == 1
    rng = np.random.default_rng(52)
    raw = rng.integers(1 << 28, 1 << 31, 4096)
    raw[:4] = [1 << 28, (1 << 28) + 1, (1 << 31) - 2, (1 << 31) - 1]
    sym = np.array([T.escape_symbol(int(r), sizes[0], offsets[0]) for r in raw], np.int32)
    idx = np.zeros(4096, np.int32)
    _, back = T.classify(sym, idx, sizes, offsets)
    assert all(T.nibbles(r) == 8 for r in back.tolist())
    got = run(coder, tabs, [("tiny", sym, idx, None, 64)])
    words = np.frombuffer(got[12:12 + 4 * 64], np.uint32)
    assert words.min() >= 64 * 52 // 32 and words.max() <= 64 * 52 // 32 + 3      # 104 words of records + the final state
    assert words.max() <= 2 * 64 + 8


def test_channel_indexed_rows_wrap(coder, tabs):
    """chan = (C, HW) with three pictures in the plane: row = (i // HW) % C."""
    C_, HW, N = 5, 7, 3
    n = N * C_ * HW
    row = (np.arange(n) // HW) % C_
    _, sizes, offsets = tabs["full"]
    rng = np.random.default_rng(5)
    sym = (offsets[row] + rng.integers(-2, sizes[row] + 1, n)).astype(np.int32)  # in-table and just outside, by row
    assert set(row[:C_ * HW].tolist()) == set(range(C_)) and (row[C_ * HW:2 * C_ * HW] == row[:C_ * HW]).all()
    assert len(set(offsets[:C_].tolist())) == C_ and len(set(sizes[:C_].tolist())) == C_   # a wrong row shows
    run(coder, tabs, [("full", sym, None, (C_, HW), 64)])
    run(coder, tabs, [("full", sym, None, (C_, HW), 3)])


def test_three_sections_with_an_odd_one_in_the_middle(coder, tabs):
    """Three tables in one payload; the middle section has 65 lanes, so the header and the position handed to the third
    section are odd word counts."""
    a = T.covering_symbols(tabs["flat"], seed=2)
    b = T.covering_symbols(tabs["odd"], seed=3, repeat=20)
    c = T.covering_symbols(tabs["wide"], seed=4)
    got = run(coder, tabs, [("flat", *a, None, 64), ("odd", *b, None, 65), ("wide", *c, None, 128)])
    first = 2 + 64 + int(np.frombuffer(got[12:12 + 4 * 64], np.uint32).sum())
    second = np.frombuffer(got[4 + 4 * first:4 + 4 * first + 8], np.uint32)
    assert second.tolist() == [b[0].size, 65]
