"""The PNG writer without a GPU: the restatement (tests/pngdev_ref.py) against PIL and zlib, the built-in presets, the tie
rules, the tokens at the segments' seams, and every refusal of the two entry points, of pngdev and of the command line."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import pngdev_ref as R
from vcm_ts_amd import lib
from vcm_ts_amd import pngdev as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1, None), (1, 3, None), (3, 5, None), (16, 16, None), (17, 67, None), (64, 64, None), (2, 8191, 1), (40, 21, 1),
         (40, 21, 7), (40, 21, 40)]


@pytest.fixture(scope="module")
def words():
    return P.to_words(P.presets())


def inflate(file):
    """zlib's decompression of the concatenated IDAT data of a PNG file."""
    return zlib.decompress(b"".join(d for kind, d in R.chunks(file) if kind == b"IDAT"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}-R{s[2] or 'default'}")
def test_pil_and_zlib_read_what_the_restatement_writes(size, words):
    from PIL import Image

    H, W, rows = size
    rows = rows or R.default_rows(W)
    assert R.default_rows(W) == P.default_rows(W) and rows * (3 * W + 1) <= R.BAND_MAX
    for name, pic in R.contents(H, W).items():
        c = R.codes(pic)
        file, bands = R.encode(c, rows, words), R.bands(c, rows, words)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(file)).convert("RGB")), c), name
        assert inflate(file) == b"".join(s for s, _, _ in bands), name
        assert len(bands) == -(-H // rows) and all(len(d) <= 5 + len(s) for s, d, _ in bands)
        assert len(file) <= R.bound(H, W, rows) and len(file) == R.PREFIX + R.TRAILER + sum(12 + len(d) for _, d, _ in bands), name
        kinds = [k for k, _ in R.chunks(file)]
        assert kinds == [b"IHDR"] + [b"IDAT"] * (len(bands) + 2) + [b"IEND"]
        if name == "noise80" and H * W >= 256:  # nothing a table could gain on: a band really takes stored
            assert any(which == "stored" for _, _, which in bands)
        if name == "noise0" and H * W >= 256 and size[2] is None:
            assert all(which != "stored" for _, _, which in bands)


def test_a_flat_picture_is_small(words):
    c = R.codes(R.contents(64, 96)["flat"])
    file = R.encode(c, R.default_rows(96), words)
    assert len(file) * 16 < c.size and inflate(file) == b"".join(s for s, _, _ in R.bands(c, R.default_rows(96), words))


def test_every_preset_is_a_complete_code_that_zlib_accepts(words):
    fam = P.presets()
    assert len(fam) == len(P.THETAS) * len(P.RUNS) <= P.MAX_PRESETS and words.shape == (len(fam), R.PRESET_WORDS)
    assert np.array_equal(words, P.to_words(P.presets()))  # (a function of integers alone)
    assert lib.hip().dcvc_png_tables_check(words.ctypes.data, len(fam)) == 0
    pics = R.contents(17, 67)
    strings = [R.band_string(R.codes(pics[name]), 0, 17) for name in ("noise1.5", "flat", "ramp")]
    for k, p in enumerate(fam):
        lens, cds, hbits, header = R.preset_fields(words, k)
        assert lens == p.lengths and cds == p.codes and (header, hbits) == p.header and hbits <= 32 * R.HEADER_WORDS
        assert max(lens) <= 15 and min(lens) >= 1 and sum(2 ** (15 - n) for n in lens) == 2 ** 15  # Kraft: exactly 1
        for s in strings:  # a band forced onto the preset, inside a zlib stream of its own
            data, which = R.band_data(s, words, force=k)
            stream = b"\x78\x01" + data + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(s))
            assert which == k and zlib.decompress(stream) == s, k
    assert len({tuple(p.lengths) for p in fam}) == len(fam)


def test_ties_go_to_the_smaller_filter_type_and_to_stored(words):
    # the picture's first row: nothing above, so Sub and Paeth filter alike; on a steady slope both beat the rest
    c = np.zeros((1, 40, 3), np.uint8)
    c[0] = (10 + 5 * np.arange(40))[:, None]
    costs = R.row_costs(R.filtered_rows(c, 0))
    assert costs[1] == costs[4] == costs.min() and costs[0] > costs[1] and costs[2] > costs[1] and costs[3] > costs[1]
    assert R.band_string(c, 0, 1)[0] == 1
    assert R.band_string(np.zeros((2, 5, 3), np.uint8), 0, 2)[::16] == b"\x00\x00"  # all five tie: None
    # a string of expensive bytes, and cheap pairs in front of it until one preset costs exactly what stored costs
    k = len(P.presets()) - 1
    lens = R.preset_fields(words, k)[0]
    assert lens[0] + lens[1] < 16 and lens[128] > 8
    one = words[k:k + 1]
    tied = None
    for m in range(4000):
        s = bytes([0, 1]) * m + bytes([128, 127]) * 40
        size = R.dynamic_size(R.tokens(s), one, 0)
        if size == 5 + len(s) and tied is None:
            tied = s
        if size < 5 + len(s):
            cheaper = s
            break
    assert tied is not None
    assert R.band_data(tied, one)[1] == "stored" and R.band_data(cheaper, one)[1] == 0
    two = np.concatenate([one, one])  # equal presets: the smaller index
    assert R.band_data(cheaper, two)[1] == 0


def runs_rule(s):
    """The tokens by the header's second wording: maximal runs of "equals the byte before" of length >= 3 are matches."""
    out = []
    for s0 in range(0, len(s), R.SEG):
        seg = s[s0:s0 + R.SEG]
        e = [i > 0 and seg[i] == seg[i - 1] for i in range(len(seg))] + [False]
        i = 0
        while i < len(seg):
            L = 0
            while e[i + L]:
                L += 1
            if L >= 3:
                out.append(("match", L))
                i += L
            else:
                out.extend(("lit", b) for b in seg[i:i + max(L, 1)])
                i += max(L, 1)
    return out


def test_tokens_at_the_segments_seams(words):
    def with_run(at, n, total=192):  # `n` equal bytes from position `at` in a string without any other repeat
        s = bytearray((7 * i) % 251 + 1 for i in range(total))
        s[at:at + n] = bytes([255]) * n
        return bytes(s)

    lit, match = (lambda *b: [("lit", v) for v in b]), (lambda n: [("match", n)])
    a = 255
    assert R.tokens(with_run(0, 2, 8))[:3] == lit(a, a, 15)
    assert R.tokens(with_run(0, 3, 8))[:4] == lit(a, a, a, 22)       # two repeats behind the first byte: no match
    assert R.tokens(with_run(0, 4, 8))[:3] == lit(a) + match(3) + lit(29)
    assert R.tokens(with_run(1, 3, 8))[:5] == lit(1, a, a, a, 29)
    assert R.tokens(with_run(1, 4, 8))[:4] == lit(1, a) + match(3) + lit(36)
    assert R.tokens(with_run(0, 64))[:3] == lit(a) + match(63) + lit(with_run(0, 64)[64])
    assert R.tokens(with_run(0, 63))[:3] == lit(a) + match(62) + lit(with_run(0, 63)[63])
    assert R.tokens(with_run(1, 63))[:3] == lit(1, a) + match(62)
    assert R.tokens(with_run(1, 64))[:5] == lit(1, a) + match(62) + lit(a, with_run(1, 64)[65])  # cut by the segment's end
    assert R.tokens(with_run(63, 3))[63:67] == lit(a, a, a, with_run(63, 3)[66])                  # 1 + 2: no match either side
    assert R.tokens(with_run(60, 64))[60:64] == lit(a) + match(3) + lit(a) + match(59)            # straddles: 4 + 60
    assert R.tokens(with_run(61, 6))[61:67] == lit(a, a, a, a, a, a)                              # 3 + 3: one repeat short twice
    for n in (2, 3, 63, 64):
        for at in (0, 1, 63, 64, 65, 62, 127, 128 - n // 2):
            s = with_run(at, n)
            toks = R.tokens(s)
            assert toks == runs_rule(s), (n, at)
            assert sum(1 if t[0] == "lit" else t[1] for t in toks) == len(s)
            assert all(3 <= t[1] <= 63 for t in toks if t[0] == "match")
            for k in (0, len(words) - 1):
                data = R.band_data(s, words, force=k)[0]
                assert zlib.decompress(b"\x78\x01" + data + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(s))) == s
    assert [R.length_symbol(n) for n in (3, 10, 11, 12, 18, 19, 34, 35, 42, 43, 63)] == \
        [(257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (268, 1, 1), (269, 2, 0), (272, 2, 3), (273, 3, 0), (273, 3, 7),
         (274, 3, 0), (276, 3, 4)]


# -------------------------------------------------------------------------------------------------------------- refusals
def test_tables_check_refuses_what_is_not_a_preset(words):
    check = lib.hip().dcvc_png_tables_check
    K = len(words)
    assert check(words.ctypes.data, K) == 0 and check(words.ctypes.data, 1) == 0
    assert check(None, K) == -1 and check(words.ctypes.data, 0) == -1 and check(words.ctypes.data, 33) == -1
    odd = np.zeros(words.size * 4 + 8, np.uint8)
    odd[1:1 + words.size * 4] = words.view(np.uint8).reshape(-1)
    assert check(odd.ctypes.data + 1, K) == -1  # a misaligned pointer

    def refused(k, word, value):
        bad = words.copy()
        bad[k, word] = value
        return check(bad.ctypes.data, K) == -1

    w = words[2]
    assert refused(2, 7, int(w[7]) + (1 << 16))                        # a length longer: no longer complete
    assert refused(2, 7, int(w[7]) & 0xFFFF)                           # a length of 0
    assert refused(2, 7, (16 << 16) | (int(w[7]) & 0xFFFF))            # a length of 16
    assert refused(2, 7, int(w[7]) ^ 1)                                # not the canonical code
    assert refused(2, 7, int(w[7]) | 1 << 20)                          # bits above the fields
    assert refused(K - 1, R.NSYM, int(words[K - 1, R.NSYM]) + 1)       # a bit more than the header has
    assert refused(K - 1, R.NSYM, int(words[K - 1, R.NSYM]) - 1)       # a bit fewer: a set bit beyond, or a short decode
    assert refused(0, R.NSYM, 32 * R.HEADER_WORDS + 1)
    assert refused(0, R.NSYM + 1, int(words[0, R.NSYM + 1]) ^ 1)       # HLIT is not 29
    assert refused(0, R.NSYM + 1, int(words[0, R.NSYM + 1]) ^ (1 << 5))  # HDIST is not 0
    assert refused(0, R.NSYM + 2, int(words[0, R.NSYM + 2]) ^ (1 << 9))  # some length, or the code-length code itself
    assert refused(0, R.NSYM + R.HEADER_WORDS, 1 << 31)                # a bit set beyond the header
    assert refused(0, R.PRESET_WORDS - 1, 1)
    swapped = words.copy()  # two symbols of different lengths exchanged: codes and header of another table
    a, b = next((a, b) for a in range(256) for b in range(a + 1, 256) if words[1, a] >> 16 != words[1, b] >> 16)
    swapped[1, [a, b]] = swapped[1, [b, a]]
    assert check(swapped.ctypes.data, K) == -1


def test_encode_refuses_before_it_launches(words):
    L = lib.hip()
    H, W, rows = 17, 67, 4
    cap = R.bound(H, W, rows)
    assert L.dcvc_png_bound(H, W, rows) == cap == 80 + 17 * 202 + 17 * 5
    good = dict(rgb=0x1000, rs=W, ps=H * W, H=H, W=W, R=rows, th=words.ctypes.data, td=0x2000, K=len(words), staging=0x3000,
                file=0x4000, capacity=cap, size=0x5000)
    cases = [dict(rgb=None), dict(th=None), dict(td=None), dict(staging=None), dict(file=None), dict(size=None),
             dict(rgb=0x1002), dict(td=0x2001), dict(staging=0x3002), dict(file=0x4001), dict(size=0x5002),
             dict(H=0), dict(W=0), dict(H=32769, ps=32769 * W), dict(W=8192, rs=8192, ps=H * 8192, R=1, capacity=1 << 40),
             dict(rs=W - 1), dict(ps=H * W - 1), dict(R=0), dict(R=-1), dict(R=R.BAND_MAX // (3 * W + 1) + 1, capacity=1 << 40),
             dict(K=0), dict(K=33), dict(K=-1), dict(capacity=cap - 1), dict(capacity=0)]
    broken = words.copy()
    broken[len(words) - 1, 100] ^= 3
    cases.append(dict(th=broken.ctypes.data))
    for case in cases:
        v = dict(good, **case)
        assert L.dcvc_png_encode(v["rgb"], v["rs"], v["ps"], v["H"], v["W"], v["R"], v["th"], v["td"], v["K"], v["staging"],
                                 v["file"], v["capacity"], v["size"], None) == -1, case
    for H_, W_, R_ in ((0, 5, 1), (5, 0, 1), (5, 8192, 1), (32769, 5, 1), (5, 5, 0), (5, 5, R.BAND_MAX // 16 + 1)):
        assert L.dcvc_png_bound(H_, W_, R_) == -1
    assert L.dcvc_png_bound(32768, 8191, 1) == 80 + 32768 * 24574 + 17 * 32768
    assert L.dcvc_png_bound(5, 5, R.BAND_MAX // 16) == 80 + 5 * 16 + 17


def test_pngdev_refuses_by_name():
    fam = P.presets()
    for bad in ([8] * 286, [9] * 286, [8] * 285, [0] + [8] * 285, [16] * 286, [8.0] * 286):
        with pytest.raises(ValueError):
            P.Preset(bad)
    for bad in ([], fam + fam, [fam[0].lengths], fam[0]):
        with pytest.raises((ValueError, TypeError)):
            P.to_words(bad)
    for bad in ((0, 10), (100, 10), (50, 0), (50, 100), (50.0, 10)):
        with pytest.raises(ValueError):
            P.geometric_preset(*bad)
    with pytest.raises(ValueError):
        P.default_rows(8192)
    with pytest.raises(ValueError):
        P.bound(17, 67, 200)
    with pytest.raises(ValueError):
        P.checked_words(np.zeros((1, 360), np.uint32))
    with pytest.raises(ValueError):
        P.checked_words(np.zeros((2, 359), np.uint32))
    with pytest.raises(ValueError, match="GPU only"):
        P.PngDevice((64, 64), "cpu")
    assert P.default_rows(1920) == 4 and P.bound(1080, 1920, 4) == 80 + 1080 * 5761 + 17 * 270


def test_cli_refuses_png_device_without_recon(capsys, tmp_path):
    from vcm_ts_amd import run_codec as RC

    for argv in (["encode", "--frames", str(tmp_path / "none"), "--bins", str(tmp_path / "bins"), "--png-device"],
                 ["decode", "--bins", str(tmp_path / "bins"), "--recon-video", str(tmp_path / "out.y4m"), "--png-device",
                  "--height", "64", "--width", "64"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as ex:
            RC.main(argv)
        err = capsys.readouterr().err
        assert ex.value.code == 2 and "--png-device belongs to --recon" in err
    assert not (tmp_path / "bins").exists()
    with pytest.raises(ValueError, match="png_device belongs to recon_dir"):
        RC.encode_folder(str(tmp_path / "none"), str(tmp_path / "bins"), None, png_device=True)
    with pytest.raises(ValueError, match="png_device belongs to recon_dir"):
        RC.decode_folder(str(tmp_path / "bins"), None, 64, 64, png_device=True)
    assert not (tmp_path / "bins").exists()
    seen = {}
    with pytest.MonkeyPatch.context() as mp:  # the option reaches the loops
        mp.setattr(RC, "encode_folder", lambda *a, **k: seen.update(k) or ([1], (64, 64)))
        RC.main(["encode", "--frames", "f", "--bins", "b", "--recon", "r", "--png-device"])
        assert seen["png_device"] is True
        RC.main(["encode", "--frames", "f", "--bins", "b", "--recon", "r"])
        assert seen["png_device"] is False


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_tables_check_is_memory_safe_under_sanitizers(tmp_path):
    """tests/fuzz/png_fuzz.cpp: dcvc_png_tables_check and dcvc_png_bound (vcm_ts_amd/csrc/png_check.cpp) built with
    AddressSanitizer + UBSan as a stand-alone program; tables written from the header's text pass, and mutants of their
    codes, header counts and header bits in exactly sized arrays are accepted or refused with a status -- a sanitizer report
    aborts the run."""
    exe = tmp_path / "png_fuzz"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "vcm_ts_amd", "csrc", "png_check.cpp"),
                            os.path.join(ROOT, "tests", "fuzz", "png_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    for seed in (1, 2):
        run = subprocess.run([str(exe), "150", str(seed)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (seed, run.stdout[-500:], run.stderr[-3000:])
        assert "png_fuzz: 150 rounds" in run.stdout and "refused with a status" in run.stdout
