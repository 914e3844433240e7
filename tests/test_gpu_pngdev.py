"""The PNG writer on a real MI355X: dcvc_png_encode byte for byte against the restatement (tests/pngdev_ref.py, which
tests/test_pngdev_host.py holds against PIL and zlib) in strided, offset, NaN-surrounded layouts with guarded outputs, its
memory discipline and refusals, the pricing at K = 1 and 32 and with a hopeless table, PngDevice, and the file loops."""
import io
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import pngdev_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from vcm_ts_amd import lib
from vcm_ts_amd import pngdev as P

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
SENT = 0xABCD1234
# (row pad, plane pad, offset of the picture, shift in words of file / staging / size_word)
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]
SIZES = [(1, 1, None), (1, 3, None), (3, 5, None), (16, 16, None), (17, 67, None), (33, 259, 1), (33, 259, None), (2, 8191, None),
         (300, 8, 1)]


@pytest.fixture(scope="module")
def family():
    words = P.to_words(P.presets())
    return words, torch.from_numpy(words.view(np.int32)).to(DEV)


def _encode(pic, H, W, rows, words, words_dev, layout, capacity=None):
    """One dcvc_png_encode in `layout`: (status, the file's bytes or None, what the checks of memory need)."""
    row_pad, plane_pad, offset, shift = layout
    bands = -(-H // rows)
    cap = R.bound(H, W, rows) if capacity is None else capacity
    kp, vp, rs, ps, mask = U.strided(pic, H, W, row_pad, plane_pad, offset, DEV)
    fw, sw = -(-cap // 4), bands * R.SLOT_BYTES // 4
    file, f0 = U.guarded(fw, shift, np.uint32, SENT, DEV)
    staging, s0 = U.guarded(sw, shift, np.uint32, SENT, DEV)
    size, z0 = U.guarded(1, shift, np.uint32, SENT, DEV)
    status = lib.hip().dcvc_png_encode(vp.data_ptr(), rs, ps, H, W, rows, words.ctypes.data, words_dev.data_ptr(), len(words),
                                       staging.data_ptr() + 4 * s0, file.data_ptr() + 4 * f0, cap, size.data_ptr() + 4 * z0,
                                       U.stream(DEV))
    torch.cuda.synchronize(DEV)
    got = kp.cpu().numpy()  # the input is only read
    assert np.array_equal(got[mask].view(np.uint32), np.asarray(pic, np.float32).reshape(-1).view(np.uint32))
    assert np.isnan(got[~mask]).all()
    assert U.guards_intact(staging, s0, sw, SENT) and U.guards_intact(size, z0, 1, SENT)
    if status != 0:  # a refusal leaves the outputs alone
        assert U.guards_intact(file, f0, 0, SENT) and U.guards_intact(staging, s0, 0, SENT) and U.guards_intact(size, z0, 0, SENT)
        return status, None
    n = int(U.words(size)[z0])
    raw = file.cpu().numpy().view(np.uint8)
    data = raw[4 * f0:4 * f0 + n].tobytes()
    rest = raw[4 * f0 + n:]  # at and beyond `size`, the guard included: the fill
    assert np.array_equal(rest, np.frombuffer(np.full(1, SENT, np.uint32).tobytes() * (len(rest) // 4 + 1), np.uint8)[n % 4:][:len(rest)])
    assert (raw[:4 * f0].view(np.uint32) == SENT).all()
    return status, data


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}-R{s[2] or 'default'}")
def test_kernel_equals_the_restatement_byte_for_byte(size, family):
    from PIL import Image

    H, W, rows = size
    rows = rows or R.default_rows(W)
    assert rows == P.default_rows(W) or size[2]
    words, words_dev = family
    for n, (name, pic) in enumerate(R.contents(H, W).items()):
        c = R.codes(pic)
        want = R.encode(c, rows, words)
        for m, layout in enumerate(LAYOUTS):
            if name != "noise1.5" and m != n % 4:  # (every layout on one content, one on the others)
                continue
            status, got = _encode(pic, H, W, rows, words, words_dev, layout)
            assert status == 0 and len(got) == len(want) and got == want, (name, layout, len(got), len(want))
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), c), name


def test_pricing_with_one_with_32_and_with_a_hopeless_table():
    from PIL import Image

    H, W = 33, 259
    rows, pics = R.default_rows(W), R.contents(H, W)
    fam = P.presets()
    for tables in (fam[5:6], (fam + fam[:12])[:32]):
        words = P.to_words(tables)
        words_dev = torch.from_numpy(words.view(np.int32)).to(DEV)
        for name in ("noise0", "noise1.5", "flat"):
            status, got = _encode(pics[name], H, W, rows, words, words_dev, LAYOUTS[1])
            assert status == 0 and got == R.encode(R.codes(pics[name]), rows, words), (len(tables), name)
    # ten bits and more for every literal and every length: no band of a noisy picture is cheaper than stored
    hopeless = P.to_words([P.Preset([10] * 256 + [7] * 24 + [6] * 4 + [2] * 2)])
    c = R.codes(pics["noise80"])
    assert all(which == "stored" for _, _, which in R.bands(c, 4, hopeless))
    status, got = _encode(pics["noise80"], H, W, 4, hopeless, torch.from_numpy(hopeless.view(np.int32)).to(DEV), LAYOUTS[2])
    assert status == 0 and got == R.encode(c, 4, hopeless)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), c)


def test_refusals_leave_the_outputs_alone(family):
    words, words_dev = family
    H, W = 17, 67
    pic = R.contents(H, W)["noise1.5"]
    rows = R.default_rows(W)
    assert _encode(pic, H, W, rows, words, words_dev, LAYOUTS[0], capacity=R.bound(H, W, rows) - 1)[0] == -1
    assert _encode(pic, H, W, rows + 1, words, words_dev, LAYOUTS[0], capacity=1 << 20)[0] == -1
    bad = words.copy()
    bad[3, 40] ^= 1 << 16  # one length of one preset: no longer a complete code
    assert _encode(pic, H, W, rows, bad, words_dev, LAYOUTS[0])[0] == -1
    assert _encode(pic, H, W, rows, words, words_dev, LAYOUTS[0])[0] == 0


def test_png_device_hands_finished_files_to_writer_threads(tmp_path):
    from PIL import Image

    H, W = 40, 21
    pics = R.contents(H, W)
    dev = P.PngDevice((H, W), DEV, streams=2, ring=2)
    words = P.to_words(P.presets())
    big = torch.full((1, 3, 64, 64), 0.5, device=DEV)
    handles = []
    for n, (name, pic) in enumerate(pics.items()):  # (more pictures than ring buffers: a buffer returns on release)
        big[..., :H, :W] = torch.from_numpy(pic).to(DEV)
        h = dev.put(n % 2, big)
        path = str(tmp_path / f"{name}.png")
        h.save(path)
        assert open(path, "rb").read() == R.encode(R.codes(pic), dev.rows, words), name
        assert np.array_equal(U.png(path), R.codes(pic))
        handles.append(h)
    assert dev.launches == 2 * len(pics) and all(h.free.is_set() for h in handles)
    with pytest.raises(ValueError):
        dev.put(0, big.cpu())
    with pytest.raises(ValueError):
        dev.put(2, big)
    with pytest.raises(ValueError):
        dev.put(0, big[..., :H - 1, :W])


# ---------------------------------------------------------------------------------------------------------- file loops
FH, FW, FN, FGOP = 128, 192, 4, 2  # two GOPs of an I and a P picture


@pytest.fixture(scope="module")
def loops(tmp_path_factory, file_nets):
    """The clip as PNGs; encodes with picture_hash into PNG folders: the host's writer, the device's with one and with two
    GOP streams, each with the names of the launches that went through devargs."""
    from tests.pixel_ref import code
    from vcm_ts_amd import devargs
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd.synthetic import frames

    tmp = tmp_path_factory.mktemp("pngdev_loops")
    U.write_pngs(tmp / "png", [code(a).astype(np.uint8).transpose(1, 2, 0) for a in frames(0, FN, FH, FW)])
    launches, real = {}, devargs.launch
    for name, extra in (("host", {}), ("dev1", dict(png_device=True)), ("dev2", dict(png_device=True, gop_streams=2))):
        launches[name] = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(devargs, "launch", lambda n, *a, _log=launches[name], **k: _log.append(n) or real(n, *a, **k))
            RC.encode_folder(str(tmp / "png"), str(tmp / f"bins_{name}"), str(tmp / f"rec_{name}"), gop=FGOP, nets=file_nets,
                             picture_hash=True, **extra)
    return dict(tmp=tmp, launches=launches)


def test_encode_writes_the_same_pixels_in_the_restatements_files(loops):
    from vcm_ts_amd import picturehash as PH

    tmp, words = loops["tmp"], P.to_words(P.presets())
    names = [f"im{t + 1:05d}.png" for t in range(FN)]
    for run in ("dev1", "dev2"):
        assert sorted(os.listdir(tmp / f"rec_{run}")) == names and U.bins(tmp / f"bins_{run}") == U.bins(tmp / "bins_host")
        assert U.others(tmp / f"bins_{run}") == U.others(tmp / "bins_host")
        for name in names:
            c = U.png(tmp / "rec_host" / name)
            assert np.array_equal(U.png(tmp / f"rec_{run}" / name), c), (run, name)  # PIL reads the same pixels
            assert (tmp / f"rec_{run}" / name).read_bytes() == R.encode(c, R.default_rows(FW), words), (run, name)
        assert PH.verify_pngs(str(tmp / f"bins_{run}"), str(tmp / f"rec_{run}")) is None  # what `run_codec verify` does
        assert loops["launches"][run].count("dcvc_png_encode") == FN
        rest = [n for n in loops["launches"][run] if n != "dcvc_png_encode"]  # (two streams interleave their launches)
        assert (rest if run == "dev1" else sorted(rest)) == (loops["launches"]["host"] if run == "dev1" else sorted(loops["launches"]["host"]))


def test_without_the_option_nothing_changes(loops):
    from PIL import Image

    tmp = loops["tmp"]
    assert "dcvc_png_encode" not in loops["launches"]["host"]
    for t in range(FN):  # the files are PIL's own of those pixels, as they were before the option existed
        path = tmp / "rec_host" / f"im{t + 1:05d}.png"
        b = io.BytesIO()
        Image.fromarray(U.png(path)).save(b, format="PNG")
        assert path.read_bytes() == b.getvalue(), t
    assert sorted(os.listdir(tmp / "rec_host")) == [f"im{t + 1:05d}.png" for t in range(FN)]


def test_decode_writes_them_too_and_verify_passes(loops, file_nets):
    from vcm_ts_amd import devargs
    from vcm_ts_amd import picturehash as PH
    from vcm_ts_amd import run_codec as RC

    tmp, words = loops["tmp"], P.to_words(P.presets())
    launches, real = {}, devargs.launch
    for name, on in (("dec_host", False), ("dec_dev", True)):
        launches[name] = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(devargs, "launch", lambda n, *a, _log=launches[name], **k: _log.append(n) or real(n, *a, **k))
            mp.setattr(RC, "_nets", lambda *a, **k: file_nets[0])
            assert RC.decode_folder(str(tmp / "bins_host"), str(tmp / name), FH, FW, gop=FGOP, png_device=on) == FN
    assert "dcvc_png_encode" not in launches["dec_host"] and launches["dec_dev"].count("dcvc_png_encode") == FN
    assert [n for n in launches["dec_dev"] if n != "dcvc_png_encode"] == launches["dec_host"]
    U.same_pngs(str(tmp / "dec_host"), str(tmp / "rec_host"), FN)
    U.same_pngs(str(tmp / "dec_dev"), str(tmp / "rec_dev1"), FN)
    assert PH.verify_pngs(str(tmp / "bins_host"), str(tmp / "dec_dev")) is None
    RC.main(["verify", "--bins", str(tmp / "bins_dev2"), "--recon", str(tmp / "dec_dev")])  # (the command: SystemExit on a mismatch)
    assert (tmp / "dec_dev" / "im00003.png").read_bytes() == R.encode(U.png(tmp / "rec_host" / "im00003.png"), R.default_rows(FW), words)
    with pytest.raises(ValueError, match="8191"):  # (before any launch or file)
        RC._PngStage(str(tmp / "refused"), 2, "cuda:0").open((64, 8192))
    assert not (tmp / "refused").exists()
