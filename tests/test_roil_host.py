"""The ROI residual layer without a GPU: the restatement (tests/roil_ref.py) against itself and against the header's
properties, the product's host half (active cells, record validation, argument refusals) against the restatement, and the
sanitizer fuzz of the record checker and the per-sample segment decoder (tests/fuzz/roil_fuzz.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import roi_ref as R
from tests import roil_ref as RL
from vcm_ts_amd import lib
from vcm_ts_amd import roi as X
from vcm_ts_amd import roilayer as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


@pytest.fixture(scope="module")
def coded():
    """{(H, W): {list name: (boxes, residual picture, {S: (record, modes, decoded picture)})}}, computed once"""
    out = {}
    for seed, (H, W) in enumerate(R.SIZES):
        src, rec = RL.pictures(seed, H, W)
        out[(H, W)] = {}
        for name, boxes in R.box_lists(H, W).items():
            res = R.residual(src, rec, boxes)
            out[(H, W)][name] = (boxes, res, {S: RL.encode_record(res, boxes, S) for S in RL.STEPS})
    return out


def test_restatement_round_trips_and_is_lossless_at_step_one(coded):
    for (H, W), lists in coded.items():
        for name, (boxes, res, by_step) in lists.items():
            cells, counts, mask = RL.active_cells(boxes, H, W)
            assert list(cells) == RL.touched_cells(boxes, H, W), (H, W, name)  # the two definitions of an active cell
            assert (counts >= 1).all() and int(counts.sum()) == int(mask.sum())
            for S, (record, modes, want) in by_step.items():
                assert RL.check_record(record, counts) is None
                got = RL.decode_record(record, boxes, H, W)
                assert got is not None and np.array_equal(got, want), (H, W, name, S)
                assert not got[:, ~mask].any()
                err = np.abs(got.astype(np.int64) - res.astype(np.int64))[:, mask]
                assert err.size == 0 or err.max() <= S // 2, (H, W, name, S)
                if S == 1:
                    assert np.array_equal(got, res)
                A = len(cells)
                entries = np.frombuffer(record, "<u2", 3 * A, 8).astype(np.int64)
                assert ((entries & 0xFFF) <= np.repeat(counts, 3)).all()  # L <= n
                assert len(record) == 8 + 6 * A + int((entries & 0xFFF).sum()) and len(record) <= 8 + 774 * A
            if not len(cells):
                assert by_step[1][0] == b"RL\x01\x01\x00\x00\x00\x00"


def test_quantiser_stays_within_half_a_step_for_every_value_and_step():
    r = np.arange(256)
    for S in range(1, 65):
        q = RL.quantise(r, S)
        u = RL.fold(q)
        assert u.min() >= 0 and u.max() <= 255 and np.array_equal(RL.unfold(u), q)
        assert np.abs(RL.reconstruct(q, S) - r).max() <= S // 2, S
    assert np.array_equal(RL.reconstruct(RL.quantise(r, 1), 1), r)


def test_the_inputs_make_the_encoder_choose_every_mode_it_can(coded):
    """A condition on the inputs.  Nine of the ten modes: mode 7 never has the fewest bits under the tie rule (the proof is
    beside roil_ref.REACHABLE_MODES and checked here on random segments); the decoders meet it in forced records."""
    seen = set()
    for lists in coded.values():
        for _, _, by_step in lists.values():
            for _, modes, _ in by_step.values():
                seen.update(modes)
    assert seen == RL.REACHABLE_MODES == set(range(10)) - {7}, sorted(seen)
    rng = np.random.default_rng(5)
    for trial in range(400):
        n, top = int(rng.integers(1, 257)), int(rng.choice([1, 2, 64, 100, 127, 128, 129, 200, 256]))
        u = rng.integers(max(0, top - int(rng.integers(1, 129))), top, n)
        assert RL.segment_bits(u, 7) >= min(RL.segment_bits(u, 6), RL.segment_bits(u, 8))
        assert RL.encode_segment(u)[0] != 7


def test_forced_mode_seven_records_decode(coded):
    H, W = 37, 131
    boxes, res, by_step = coded[(H, W)]["whole"]
    for S in (1, 7):
        record, modes, want = RL.encode_record(res, boxes, S, force7=True)
        assert 7 in modes and record != by_step[S][0]
        counts = RL.active_cells(boxes, H, W)[1]
        assert RL.check_record(record, counts) is None and Y.check_record(record, counts)["step"] == S
        assert np.array_equal(RL.decode_record(record, boxes, H, W), want) and np.array_equal(want, by_step[S][2])


def test_product_active_cells_are_the_restatements(coded):
    for (H, W), lists in coded.items():
        for name, (boxes, _, _) in lists.items():
            cells, counts = Y.active_cells(X.FrameBoxes(boxes), H, W)
            want_cells, want_counts, _ = RL.active_cells(boxes, H, W)
            assert cells.dtype == np.int32 and counts.dtype == np.int32
            assert np.array_equal(cells, want_cells) and np.array_equal(counts, want_counts), (H, W, name)
    with pytest.raises(ValueError, match="coordinates out of range"):
        Y.active_cells(X.FrameBoxes([[0, 0, 9, 8, 0]]), 8, 8)
    with pytest.raises(ValueError, match="picture sides"):
        Y.active_cells(X.FrameBoxes(), 0, 8)


def _entry(record, s, mode=None, L=None):
    """the record with table entry s changed"""
    e = int.from_bytes(record[8 + 2 * s:10 + 2 * s], "little")
    e = ((e >> 12 if mode is None else mode) << 12) | (e & 0xFFF if L is None else L)
    return record[:8 + 2 * s] + e.to_bytes(2, "little") + record[10 + 2 * s:]


def test_check_record_refuses_by_name(coded):
    H, W = 38, 518
    boxes, _, by_step = coded[(H, W)]["overlap"]
    record = by_step[1][0]
    cells, counts = Y.active_cells(X.FrameBoxes(boxes), H, W)
    A = len(cells)
    info = Y.check_record(record, counts)
    assert info["step"] == 1 and info["cells"] == A and info["modes"].shape == (A, 3)
    assert np.array_equal(info["offsets"].reshape(-1)[1:], (info["offsets"] + info["lengths"]).reshape(-1)[:-1])
    modes, lengths = info["modes"].reshape(-1), info["lengths"].reshape(-1)
    raw, zero, golomb = (int(np.flatnonzero(c)[0]) for c in (modes == 8, modes == 9, (modes < 8) & (lengths < np.repeat(counts, 3))))
    n_of = lambda s: int(counts[s // 3])
    cases = {
        "truncated record": (record[:-1], "truncated", -16),
        "truncated inside the table": (record[:8 + 6 * A - 1], "truncated", -16),
        "shorter than a header": (record[:5], "truncated", -16),
        "trailing bytes": (record + b"\0", "trailing", -23),
        "wrong A": (record[:4] + (A + 1).to_bytes(4, "little") + record[8:], "cells", -20),
        "mode 10": (_entry(record, golomb, mode=10), "mode", -21),
        "mode 9 with L = 1": (_entry(record, zero, L=1), "length", -22),
        "mode 8 with L != n": (_entry(record, raw, L=n_of(raw) - 1), "length", -22),
        "L beyond n": (_entry(record, golomb, L=n_of(golomb) + 1), "length", -22),
        "L below the low parts": (_entry(record, golomb, L=0), "length", -22),
        "bad magic": (b"RX" + record[2:], "magic", -17),
        "bad version": (record[:2] + b"\2" + record[3:], "version", -18),
        "step 0": (record[:3] + b"\0" + record[4:], "step", -19),
        "step 65": (record[:3] + b"\x41" + record[4:], "step", -19),
    }
    messages = {"truncated": "truncated record", "trailing": "trailing bytes", "cells": "wrong number of active cells",
                "mode": "mode 10 above 9", "magic": "bad magic", "version": "unknown version", "step": "out of range"}
    length_messages = {"mode 9 with L = 1": "mode 9 with a length", "mode 8 with L != n": "mode 8 with a length other than n",
                       "L beyond n": "length out of bounds", "L below the low parts": "length out of bounds"}
    L = lib.hip()
    for name, (bad, kind, status) in cases.items():
        assert RL.check_record(bad, counts) == kind, name
        assert L.dcvc_roil_check(bad, len(bad), counts.ctypes.data, A) == status, name
        with pytest.raises(Y.RoiLayerError, match=length_messages.get(name) or messages[kind]):
            Y.check_record(bad, counts)
    assert L.dcvc_roil_check(record, len(record), counts.ctypes.data, A) == 0
    assert L.dcvc_roil_check(None, len(record), counts.ctypes.data, A) == E_ARG
    assert L.dcvc_roil_check(record, -1, counts.ctypes.data, A) == E_ARG
    assert L.dcvc_roil_check(record, len(record), None, A) == E_ARG
    with pytest.raises(Y.RoiLayerError, match="wrong number of active cells"):
        Y.check_record(record, counts[:-1])
    # without the boxes parse_record still refuses what the record alone shows
    assert Y.parse_record(record)["cells"] == A
    for name in ("truncated record", "trailing bytes", "mode 10", "bad magic", "bad version", "step 0", "step 65"):
        with pytest.raises(Y.RoiLayerError):
            Y.parse_record(cases[name][0])
    empty = b"RL\x01\x07\x00\x00\x00\x00"
    assert Y.check_record(empty, np.zeros(0, np.int32))["step"] == 7
    for S in (0, 65, 1.0, True):
        with pytest.raises(ValueError, match="residual step"):
            Y.check_step(S)


def test_library_exports_what_the_header_declares():
    text = open(os.path.join(ROOT, "include", "dcvc_hip_roil.h")).read()
    mk = open(os.path.join(ROOT, "vcm_ts_amd", "csrc", "Makefile")).read()
    assert "roil.hip" in [ln for ln in mk.splitlines() if ln.startswith("HIPSRC")][0].split()
    assert "dcvc_hip_roil.h" in [ln for ln in mk.splitlines() if ln.startswith("$(HERE)build/%.o:")][0]
    for name, value in (("DCVC_ROIL_MAX_STEP", Y.MAX_STEP), ("DCVC_ROIL_HEADER", Y.HEADER), ("DCVC_ROIL_SLOT", Y.SLOT),
                        ("DCVC_ROIL_CELL_MAX", Y.CELL_MAX), ("DCVC_ROIL_VERSION", Y.VERSION)):
        assert re.search(rf"#define {name} {value}\b", text), name
    for status, phrase in Y._REFUSALS.items():
        assert f"({status})" in text, phrase


P = 0x100000  # an aligned dummy: a refused call returns before anything is launched or dereferenced


BOXES = (lib.RoiBox * 1025)()  # (module level: the calls below take its address)
for _i in range(1025):
    BOXES[_i].x1, BOXES[_i].y1, BOXES[_i].x2, BOXES[_i].y2, BOXES[_i].cls = 1, 1, 20, 18, _i % 2  # 2 x 2 cells


def _calls(**over):
    H, W, boxes = 32, 48, BOXES
    record = b"RL\x01\x01\x04\x00\x00\x00" + (9 << 12).to_bytes(2, "little") * 12
    a = dict(src=P, rs=W, ps=H * W, rec=P, H=H, W=W, bh=C.addressof(boxes), bd=P, n=2, step=1, table=P, A=4, staging=P, record=P,
             capacity=8 + 774 * 4, size_word=P, rec_host=record, rec_dev=P, size=len(record), out=P, cs=H * W, urs=W, px=1,
             order=(0, 1, 2), status=P)
    a.update(over)
    enc = [a["src"], a["rs"], a["ps"], a["rec"], a["rs"], a["ps"], a["H"], a["W"], a["bh"], a["bd"], a["n"], a["step"], a["table"],
           a["A"], a["staging"], a["record"], a["capacity"], a["size_word"], None]
    dec = [a["rec_host"], a["rec_dev"], a["size"], a["H"], a["W"], a["bh"], a["bd"], a["n"], a["table"], a["out"], a["cs"], a["urs"],
           a["px"], *a["order"], a["status"], None]
    return enc, dec, a


COMMON = {"null boxes on the host": dict(bh=None), "null boxes on the device": dict(bd=None), "zero height": dict(H=0),
          "width beyond the limit": dict(W=32769, rs=32769, urs=32769), "1025 boxes": dict(n=1025), "negative count": dict(n=-1),
          "null table": dict(table=None), "table not 8-byte aligned": dict(table=P + 4), "a box beyond the picture": dict(H=17)}
ENCODE = {"null source": dict(src=None), "null reconstruction": dict(rec=None), "row stride below the width": dict(rs=47),
          "plane stride too small": dict(ps=32 * 48 - 1), "step 0": dict(step=0), "step 65": dict(step=65),
          "wrong number of cells": dict(A=3), "negative number of cells": dict(A=-1), "null staging": dict(staging=None),
          "staging unaligned": dict(staging=P + 2), "null record": dict(record=None), "record unaligned": dict(record=P + 2),
          "capacity below 8 + 774 A": dict(capacity=8 + 774 * 4 - 1), "null size word": dict(size_word=None),
          "size word unaligned": dict(size_word=P + 2)}
DECODE = {"null host record": dict(rec_host=None), "null device record": dict(rec_dev=None), "odd device record": dict(rec_dev=P + 1),
          "size below the header": dict(size=7), "null output": dict(out=None), "pixel stride 2": dict(px=2),
          "pixel stride 3 with planes": dict(px=3), "interleaved row too short": dict(px=3, cs=1, urs=143),
          "planar row too short": dict(urs=47), "order repeats a channel": dict(order=(0, 1, 1)),
          "order out of range": dict(order=(0, 1, 3)), "null status": dict(status=None), "status unaligned": dict(status=P + 2)}


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = lib.hip()
    for name, over in {**COMMON, **ENCODE}.items():
        assert L.dcvc_roil_encode(*_calls(**over)[0]) == E_ARG, name
    for name, over in {**COMMON, **DECODE}.items():
        assert L.dcvc_roil_decode(*_calls(**over)[1]) == E_ARG, name
    # a record that disagrees with the boxes is refused with its own code before any launch
    good = _calls()[2]["rec_host"]
    for bad, status in ((good[:-2], -16), (good + b"\0", -23), (b"RL\x01\x01\x03\x00\x00\x00" + good[8:], -20),
                        (good[:8] + (10 << 12).to_bytes(2, "little") + good[10:], -21),
                        (good[:8] + ((9 << 12) | 1).to_bytes(2, "little") + good[10:], -22), (b"RL\x02" + good[3:], -18)):
        assert L.dcvc_roil_decode(*_calls(rec_host=bad, size=len(bad))[1]) == status, status
    cells, counts = (np.zeros(4, np.int32) for _ in range(2))
    boxes = _calls()[2]
    assert L.dcvc_roil_cells(32, 48, boxes["bh"], 2, cells.ctypes.data, counts.ctypes.data, 4) == 4
    assert cells.tolist() == [0, 1, 3, 4] and counts.tolist() == [15 * 15, 4 * 15, 15 * 2, 4 * 2]
    assert L.dcvc_roil_cells(32, 48, boxes["bh"], 2, None, None, 0) == 4
    for bad in ((32, 48, boxes["bh"], 2, cells.ctypes.data, None, 4), (32, 48, boxes["bh"], 2, cells.ctypes.data, counts.ctypes.data, 3),
                (32, 48, None, 2, None, None, 0), (0, 48, boxes["bh"], 2, None, None, 0), (32, 19, boxes["bh"], 2, None, None, 0)):
        assert L.dcvc_roil_cells(*bad) == E_ARG, bad


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_checker_and_segment_decoder_are_memory_safe_under_sanitizers(tmp_path):
    """tests/fuzz/roil_fuzz.cpp: dcvc_roil_check, dcvc_roil_cells (vcm_ts_amd/csrc/roil_check.cpp) and the per-sample segment
    decoder of the decode kernel (roil_segment.h) built with AddressSanitizer + UBSan as a stand-alone program; records of
    random samples round-trip, and truncated, extended, bit-flipped and zero-payload mutants are refused with a status or
    decode to samples within 0 .. 255 -- a sanitizer report aborts the run."""
    exe = tmp_path / "roil_fuzz"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vcm_ts_amd", "csrc"),
                            os.path.join(ROOT, "vcm_ts_amd", "csrc", "roil_check.cpp"),
                            os.path.join(ROOT, "tests", "fuzz", "roil_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    for seed in (1, 2, 3):
        run = subprocess.run([str(exe), "400", str(seed)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (seed, run.stdout[-500:], run.stderr[-3000:])
        assert "roil_fuzz: 400 rounds" in run.stdout and "refused with a status" in run.stdout


def test_file_loops_and_command_line_refuse_before_any_gpu_work(tmp_path, capsys):
    from vcm_ts_amd import run_codec as RC

    roi = X.Roi(lambda t: X.FrameBoxes(), (X.RoiClass(0),))
    with pytest.raises(ValueError, match="residual_bins= needs roi="):
        RC.encode_video(str(tmp_path / "none.y4m"), str(tmp_path / "b"), residual_bins=str(tmp_path / "b"))
    with pytest.raises(ValueError, match="residual_step= belongs to residual_bins="):
        RC.encode_video(str(tmp_path / "none.y4m"), str(tmp_path / "b"), roi=roi, residual_step=2)
    with pytest.raises(ValueError, match="residual step"):
        RC.encode_video(str(tmp_path / "none.y4m"), str(tmp_path / "b"), roi=roi, residual_bins=str(tmp_path / "b"), residual_step=0)
    with pytest.raises(ValueError, match="not both"):
        RC.decode_folder(str(tmp_path), str(tmp_path / "r"), 64, 64, roi=roi, residuals="x.gbrp", residual_bins=str(tmp_path))
    with pytest.raises(ValueError, match="not both"):
        RC.decode_video(str(tmp_path), str(tmp_path / "r.y4m"), 64, 64, roi=roi, residuals="x.gbrp", residual_bins=str(tmp_path))
    with pytest.raises(ValueError, match="residual_bins= needs roi="):
        RC.decode_folder(str(tmp_path), str(tmp_path / "r"), 64, 64, residual_bins=str(tmp_path))
    assert not (tmp_path / "b").exists() and not (tmp_path / "r").exists()
    (tmp_path / "boxes" / "faces_coords").mkdir(parents=True)
    for argv, said in (
            (["encode", "--frames", "f", "--bins", "b", "--residual-bins", "b"], "belong to --roi-root"),
            (["encode", "--frames", "f", "--bins", "b", "--roi-root", str(tmp_path / "boxes"), "--residual-step", "2"],
             "--residual-step belongs to --residual-bins"),
            (["encode", "--frames", "f", "--bins", "b", "--roi-root", str(tmp_path / "boxes"), "--residual-bins", "b",
              "--residual-step", "65"], "within 1..64"),
            (["decode", "--bins", "b", "--recon", "r", "--roi-root", str(tmp_path / "boxes"), "--residuals", "x.gbrp",
              "--residual-bins", "b"], "one of --residuals and --residual-bins"),
            (["decode", "--bins", "b", "--recon", "r", "--residual-bins", "b"], "belong to --roi-root")):
        with pytest.raises(SystemExit):
            RC.main(argv)
        assert said in capsys.readouterr().err, argv
