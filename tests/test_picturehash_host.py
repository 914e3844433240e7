"""Decoded-picture hashes, the parts that need no GPU: the combine algebra of include/dcvc_hip_hash.h against zlib.crc32,
hashes.json and its refusals, `run_codec verify` on a folder of PNGs, and every DCVC_E_ARG case of the two entry points
(a refused call returns before anything is launched or dereferenced: the pointers are aligned dummies).
"""
import json
import os
import zlib

import numpy as np
import pytest

from tests import gpu_util as U
from tests import picturehash_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import picturehash as PH
from vcm_ts_amd.scenecut import GopPlan

E_ARG = -1


def _constants():
    return lib.hash_constant("dcvc_hash_chunk_bytes"), lib.hash_constant("dcvc_hash_block_bytes")


def test_library_constants_are_the_headers():
    L, B = _constants()
    text = open(os.path.join(os.path.dirname(lib.HERE), "include", "dcvc_hip_hash.h")).read()
    assert f"#define DCVC_HASH_CHUNK_BYTES {L} " in text and L % 12 == 0 and B == 256 * L
    assert lib.hash_constant("dcvc_hash_scratch_bytes") == 4 * (0xFFFFFFFF // B + 1)


def test_the_algebra_equals_zlib():
    """mulmod / x8n / crc0 / finish, the identities the header states, for lengths 0 .. 80 and a few splits each."""
    g = np.random.default_rng(5)
    assert R.x8n(0) == R.ONE and R.x8n(1) == R.ONE >> 8 and R.mulmod(R.ONE, 0x12345678) == 0x12345678
    for n in range(0, 81):
        m = g.integers(0, 256, n, dtype=np.uint8).tobytes()
        c0 = R.crc0(m)
        assert c0 == zlib.crc32(m, 0xFFFFFFFF) ^ 0xFFFFFFFF
        assert R.finish(c0, n) == zlib.crc32(m)
        for cut in {0, n // 3, n // 2, n}:
            a, b = m[:cut], m[cut:]
            assert R.mulmod(R.crc0(a), R.x8n(len(b))) ^ R.crc0(b) == c0
        assert R.crc0(bytes(7) + m) == c0  # zero bytes in front change nothing


def test_chunked_combine_equals_zlib_across_every_seam():
    L, B = _constants()
    g = np.random.default_rng(6)
    lengths = {0, 1, 3, 4, 12}
    for seam in (L, B, 2 * B, 2 * B + L, 3 * B):
        lengths |= {seam + d for d in (-4, -3, -1, 0, 1, 3, 4) if seam + d >= 0}
    for n in sorted(lengths):
        m = g.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert R.chunked_crc32(m, L, B) == zlib.crc32(m), n
    # the procedure, not these constants: other chunk and block lengths
    m = g.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    for chunk, block in ((12, 48), (24, 24), (36, 360)):
        for n in (0, 11, 12, 13, 47, 48, 49, 359, 360, 361, 1000):
            assert R.chunked_crc32(m[:n], chunk, block) == zlib.crc32(m[:n]), (chunk, block, n)


def test_byte_strings_are_what_the_header_says():
    a = R.pixel_values(3, 5, 7)
    codes = R.code(a)
    m = R.pixel_bytes(a)
    assert len(m) == 3 * 5 * 7 and all(m[3 * (y * 7 + x) + c] == codes[c, y, x] for c in range(3) for y in range(5) for x in range(7))
    t = R.f32_values(4, 2, 3, 5)
    m = R.f32_bytes(t)
    bits = t.view(np.uint32)
    assert len(m) == 4 * 30 and int.from_bytes(m[4 * 17:4 * 18], "little") == int(bits.reshape(-1)[17])
    assert R.crc32_f32(np.float32([[[0.0]]])) != R.crc32_f32(np.float32([[[-0.0]]]))


# ---------------------------------------------------------------------------------------------------- hashes.json
def _digests(n, seed=1):
    g = np.random.default_rng(seed)
    return {t: (int(g.integers(0, 1 << 32)), int(g.integers(0, 1 << 32))) for t in range(n)}


def test_hashes_json_round_trips(tmp_path):
    d = _digests(5)
    d[2] = (0x0000000A, 0xFFFFFFFF)  # leading zeros survive
    assert PH.read_hashes(str(tmp_path)) is None
    info = PH.write_hashes(str(tmp_path), d, 60, 70, (64, 128), "fp16x3")
    on_disk = json.loads((tmp_path / "hashes.json").read_text())
    assert on_disk == info and list(on_disk) == ["version", "algorithm", "frames", "height", "width", "padded", "precision",
                                                 "pixels", "state"]
    assert on_disk["version"] == 1 and on_disk["algorithm"] == "crc32" and on_disk["pixels"][2] == "0000000a"
    back = PH.read_hashes(str(tmp_path))
    assert back["frames"] == 5 and (back["height"], back["width"], back["padded"], back["precision"]) == (60, 70, (64, 128), "fp16x3")
    assert {t: (back["pixels"][t], back["state"][t]) for t in range(5)} == d
    PH.remove_hashes(str(tmp_path))
    assert not (tmp_path / "hashes.json").exists()
    PH.remove_hashes(str(tmp_path))
    with pytest.raises(ValueError, match="frames"):
        PH.write_hashes(str(tmp_path), {0: (1, 2), 2: (3, 4)}, 60, 70, (64, 128), "fp32")


@pytest.mark.parametrize("edit, match", [
    (dict(version=2), "unknown version 2"),
    (dict(version=None), "unknown version"),
    (dict(algorithm="md5"), "unknown algorithm 'md5'"),
    (dict(pixels=["00000000"] * 2), "pixels holds 2 digests for 3 frames"),
    (dict(state=["00000000"] * 4), "state holds 4 digests for 3 frames"),
    (dict(state=None), "state holds no list of digests"),
    (dict(frames=4), "holds 3 digests for 4 frames"),
    (dict(pixels=["00000000", "0000000g", "00000000"]), r"pixels\[1\] is not a digest"),
    (dict(pixels=["00000000", "00000000", "ABCDEF01"]), r"pixels\[2\] is not a digest"),
    (dict(state=["0000000", "00000000", "00000000"]), r"state\[0\] is not a digest"),
    (dict(state=[1, "00000000", "00000000"]), r"state\[0\] is not a digest"),
    (dict(frames=-1), "frames must be"),
    (dict(height=0), "height must be"),
    (dict(padded=[64]), "padded must be"),
    (dict(padded=[32, 128]), "padded must be"),
    (dict(precision=None), "precision must be"),
])
def test_malformed_records_are_refused_by_name(tmp_path, edit, match):
    PH.write_hashes(str(tmp_path), _digests(3), 60, 70, (64, 128), "fp32")
    path = tmp_path / "hashes.json"
    info = json.loads(path.read_text())
    info.update(edit)
    path.write_text(json.dumps(info))
    with pytest.raises(ValueError, match=match) as ex:
        PH.read_hashes(str(tmp_path))
    assert "hashes.json" in str(ex.value)


def test_not_json_and_not_an_object_are_refused(tmp_path):
    (tmp_path / "hashes.json").write_text("{")
    with pytest.raises(ValueError, match="not JSON"):
        PH.read_hashes(str(tmp_path))
    (tmp_path / "hashes.json").write_text("[1]")
    with pytest.raises(ValueError, match="JSON object"):
        PH.read_hashes(str(tmp_path))


def test_modes_and_records_are_checked_before_any_launch(tmp_path):
    rec = PH.parse_hashes(PH.write_hashes(str(tmp_path), _digests(16), 64, 64, (64, 64), "fp32"))
    assert PH.verify_mode(None, rec, "d") == "pixels" and PH.verify_mode(None, None, "d") == "off"
    assert PH.verify_mode("off", None, "d") == "off" and PH.verify_mode("strict", rec, "d") == "strict"
    with pytest.raises(ValueError, match="expected one of"):
        PH.verify_mode("loose", rec, "d")
    for mode in ("strict", "pixels", "warn"):
        with pytest.raises(ValueError, match=f"verify='{mode}': there is no hashes.json in d"):
            PH.verify_mode(mode, None, "d")
    plan = GopPlan.fixed(16, 8)
    PH.check_record(rec, plan, 64, 64, (64, 64))
    with pytest.raises(ValueError, match="digests of 16 frames beside 15 .bin files"):
        PH.check_record(rec, GopPlan.fixed(15, 8), 64, 64, (64, 64))
    with pytest.raises(ValueError, match="64x64 pictures, decoding 48x64"):
        PH.check_record(rec, plan, 64, 48, (64, 64))
    with pytest.raises(ValueError, match=r"padded to \(64, 64\), this decoder pads to \(64, 128\)"):
        PH.check_record(rec, plan, 64, 64, (64, 128))


def test_mismatch_says_what_a_user_needs():
    m = PH.PictureHashMismatch(5, "pixels", 0x0000BEEF, 0xDEAD0001, "P", 0, "fp32", "fp16x3")
    assert (m.picture, m.name, m.which, m.expected, m.actual, m.kind, m.gop_start) == (5, "im00006.bin", "pixels", 0xBEEF,
                                                                                      0xDEAD0001, "P", 0)
    text = str(m)
    for part in ("picture 5", "im00006.bin", "a P picture", "began at picture 0", "pixels digest is dead0001",
                 "says 0000beef", "coded with precision fp32", "decoded with fp16x3"):
        assert part in text, part
    same = PH.PictureHashMismatch(8, "state", 1, 2, "I", 8, "fp32", "fp32")
    assert "precision" not in str(same) and "an I picture" in str(same) and "state digest" in str(same)
    assert (same.recorded_precision, same.decoding_precision) == ("fp32", "fp32")


# ------------------------------------------------------------------------------------------------ run_codec verify
def test_verify_names_the_first_changed_picture(tmp_path, capsys):
    from PIL import Image

    from vcm_ts_amd import run_codec as RC

    bins, recon, n, h, w = tmp_path / "bins", tmp_path / "recon", 4, 9, 13
    bins.mkdir()
    g = np.random.default_rng(7)
    pics = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    U.write_pngs(recon, pics)
    floats = [a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0) for a in pics]
    digests = {t: (R.crc32_pixels(f), 0) for t, f in enumerate(floats)}
    assert all(digests[t][0] == zlib.crc32(pics[t].tobytes()) for t in range(n))  # code(k / 255) == k
    PH.write_hashes(str(bins), digests, h, w, (64, 64), "fp32")
    assert PH.verify_pngs(str(bins), str(recon)) is None
    RC.main(["verify", "--bins", str(bins), "--recon", str(recon)])
    assert "4 pictures verified" in capsys.readouterr().out
    pics[2, 4, 5, 1] ^= 1  # one sample of one picture, by one code
    Image.fromarray(pics[2]).save(recon / "im00003.png")
    assert PH.verify_pngs(str(bins), str(recon)) == (2, "im00003.png", digests[2][0], zlib.crc32(pics[2].tobytes()))
    with pytest.raises(SystemExit) as ex:
        RC.main(["verify", "--bins", str(bins), "--recon", str(recon)])
    assert ex.value.code == 1
    out = capsys.readouterr().out
    assert "picture 2 (im00003.png)" in out and ("%08x" % digests[2][0]) in out
    os.remove(recon / "im00004.png")
    pics[2, 4, 5, 1] ^= 1
    Image.fromarray(pics[2]).save(recon / "im00003.png")
    with pytest.raises(ValueError, match="im00004.png: missing"):
        PH.verify_pngs(str(bins), str(recon))
    with pytest.raises(ValueError, match="no hashes.json"):
        PH.verify_pngs(str(recon), str(recon))
    with pytest.raises(SystemExit) as ex:
        RC.main(["verify", "--bins", str(recon), "--recon", str(recon)])
    assert ex.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit) as ex:
        RC.main(["verify", "--help"])
    assert ex.value.code == 0 and "unfused base-layer PNG folders only" in " ".join(capsys.readouterr().out.split())


# --------------------------------------------------------------------------------------------------- DCVC_E_ARG
_PTR = dict(src=0x10000, out=0x20000, scratch=0x30000)


def _pixels(**o):
    v = dict(_PTR, rs=24, ps=24 * 16, H=16, W=24)
    v.update(o)
    return lib.hip().dcvc_hash_pixels(v["src"], v["rs"], v["ps"], v["H"], v["W"], v["out"], v["scratch"], None)


def _f32(**o):
    v = dict(_PTR, rs=24, ps=24 * 16, C=3, H=16, W=24)
    v.update(o)
    return lib.hip().dcvc_hash_f32(v["src"], v["rs"], v["ps"], v["C"], v["H"], v["W"], v["out"], v["scratch"], None)


@pytest.mark.parametrize("call", [_pixels, _f32], ids=["pixels", "f32"])
def test_entry_points_refuse_every_bad_argument(call):
    """Host-only: a refused call launches nothing (and nothing else is tried here: the dummy pointers are not memory)."""
    for key in ("src", "out", "scratch"):
        assert call(**{key: None}) == E_ARG, key
        for off in (1, 2, 3):
            assert call(**{key: _PTR[key] + off}) == E_ARG, (key, off)
    sides = ("H", "W") + (("C",) if call is _f32 else ())
    for key in sides:
        for bad in (0, -1, 32769, -(2 ** 31)):
            assert call(**{key: bad, "rs": 40000, "ps": 1 << 40}) == E_ARG, (key, bad)
    assert call(rs=23) == E_ARG and call(rs=0) == E_ARG and call(rs=-24) == E_ARG
    assert call(ps=24 * 15 + 23) == E_ARG and call(ps=0) == E_ARG and call(ps=-1) == E_ARG
    assert call(H=1, ps=23) == E_ARG
    big = dict(rs=32768, ps=1 << 40)
    if call is _pixels:  # 3 H W >= 2^32 needs a side beyond 32768 (3 * 32768 * 32768 < 2^32): the side is what is refused
        assert 3 * 32768 * 32768 < 1 << 32 and call(H=32768, W=43691, **big) == E_ARG
    else:  # 4 C H W >= 2^32
        assert call(C=1, H=32768, W=32768, **big) == E_ARG and 4 * 32768 * 32768 == 1 << 32
        assert call(C=32768, H=32768, W=1, rs=1, ps=1 << 40) == E_ARG
        assert call(C=4, H=16384, W=16384, rs=16384, ps=1 << 40) == E_ARG
