"""ROI redaction on a real MI355X: the kernel bit for bit against the numpy restatement (tests/redact_ref.py) in strided,
offset, NaN-surrounded layouts with guarded outputs, its refusals, Redactor, and the file loops end to end: the pictures
the codec is handed, the bytes of a plain encode of those pictures, an unchanged decoder, the report, two GOP streams, a
Y4M file, a reduced base layer, the prefilter before it, the residual layer beside it, the command line."""
import contextlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import redact_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from vcm_ts_amd import lib
from vcm_ts_amd import redact as D
from vcm_ts_amd import roi as X

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
SENT16 = 0xABCD


def _box_pair(boxes):
    """(the host array kept alive, host pointer, the device tensor kept alive, device pointer, n) of a box list."""
    a = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
    if len(a) == 0:
        return a, None, None, None, 0
    dev = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
    return a, a.ctypes.data, dev, dev.data_ptr(), len(a)


# (row pad, plane pad, offset of src / out, shift of count): 16-byte accesses; an odd offset, an odd row stride, an odd
# plane stride -> 4-byte accesses; count at every 2-byte alignment
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]


def _run(pic, boxes, mask, grow, tile, fill, H, W, layout, want, where):
    """One dcvc_redact in `layout`, held against want = (out, count)."""
    row_pad, plane_pad, offset, shift = layout
    hc, wc = R.grid(H, W)
    ks, vs, srs, sps, smask = U.strided(pic, H, W, row_pad, plane_pad, offset, DEV)
    before = ks.cpu().numpy().view(np.uint32).copy()
    ko, vo, ors, ops, omask = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    count, c0 = U.guarded(hc * wc, shift, np.uint16, SENT16, DEV)  # (fresh sentinels every run: every cell is WRITTEN)
    keep, host, dev, devp, n = _box_pair(boxes)
    lib.check(lib.hip().dcvc_redact(vs.data_ptr(), srs, sps, vo.data_ptr(), ors, ops, H, W, host, devp, n, mask, grow, tile, fill,
                                    count.data_ptr() + 2 * c0, U.stream(DEV)), "redact")
    got = ko.cpu().numpy()
    assert np.array_equal(U.f32_bits(got[omask]), U.f32_bits(want[0].reshape(-1))), where
    assert np.isnan(got[~omask]).all(), where  # nothing outside the crop of out is touched
    words = U.words(count)
    assert np.array_equal(words[c0:c0 + hc * wc], np.asarray(want[1]).reshape(-1)), where
    assert U.guards_intact(count, c0, hc * wc, SENT16), where
    assert np.array_equal(ks.cpu().numpy().view(np.uint32), before), where  # the input is only read
    if dev is not None:
        assert np.array_equal(dev.cpu().numpy(), keep.reshape(-1)), where


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement_bit_for_bit(size):
    H, W = size
    assert X.grid_of(H, W) == R.grid(H, W)
    pic = R.picture(H, W)
    for c, (name, boxes, grow) in enumerate(R.cases(H, W)):
        for m, (tile, fill) in enumerate(R.MODES):
            want = R.expected(H, W, name, grow, tile, fill)
            for n, layout in enumerate(LAYOUTS):
                if name != "classes" and n not in (0, 1 + (c + m) % 3):  # (every layout on one set, two on the others)
                    continue
                _run(pic, boxes, R.MASK, grow, tile, fill, H, W, layout, want, (name, grow, tile, fill, layout))
    # what the sets are there for does happen at this size
    sets = R.box_sets(H, W)
    assert not R.region(sets["none"], H, W, R.MASK, R.GROW).any() and R.region(sets["whole"], H, W, R.MASK, 0).all()
    assert R.region(sets["pixel"], H, W, R.MASK, 0).sum() == 1
    both = R.region(sets["classes"], H, W, 0b111, 0)
    assert H < 7 or (R.region(sets["classes"], H, W, R.MASK, 0).sum() < both.sum())
    if "margin" in sets:
        assert not R.region(sets["margin"], H, W, R.MASK, 0)[:64, :64].any() and R.region(sets["margin"], H, W, R.MASK, R.GROW)[:64, :64].any()


def test_list_order_and_other_class_masks():
    H, W = 130, 200
    pic, boxes = R.picture(H, W), R.box_sets(H, W)["random300"]
    for mask in (0b001, 0b010, 0b110, 0b1111):
        want = R.redact(pic, boxes, mask, 3, 8, -1)
        _run(pic, boxes, mask, 3, 8, -1, H, W, LAYOUTS[0], want, ("mask", mask))
        _run(pic, boxes[::-1], mask, 3, 8, -1, H, W, LAYOUTS[1], want, ("reversed", mask))
    assert len(R.box_sets(H, W)["full1024"]) == X.MAX_BOXES == R.MAX_BOXES


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    hc, wc = R.grid(H, W)
    pic, boxes = R.picture(H, W), R.box_sets(H, W)["classes"]
    ks, vs, srs, sps, _ = U.strided(pic, H, W, 8, 24, 12, DEV)
    ko, vo, ors, ops, omask = U.strided(None, H, W, 8, 24, 12, DEV)
    count, c0 = U.guarded(hc * wc, 0, np.uint16, SENT16, DEV)
    keep, host, dev, devp, n = _box_pair(boxes)
    good = dict(src=vs.data_ptr(), srs=srs, sps=sps, out=vo.data_ptr(), ors=ors, ops=ops, H=H, W=W, host=host, dev=devp, n=n,
                mask=R.MASK, grow=R.GROW, tile=8, fill=-1, count=count.data_ptr() + 2 * c0)
    order = ("src", "srs", "sps", "out", "ors", "ops", "H", "W", "host", "dev", "n", "mask", "grow", "tile", "fill", "count")

    def with_box(row):
        a = keep.copy()
        a[0] = row
        return a

    bad_lists = [with_box(r) for r in ([-1, 0, 5, 5, 0], [0, 0, W + 1, 5, 0], [0, -1, 5, 5, 0], [0, 0, 5, H + 1, 0], [0, 0, 5, 5, -1],
                                       [0, 0, 5, 5, 4])]
    span = 4 * (2 * sps + (H - 1) * srs + W)
    bad = [{k: None} for k in ("src", "out", "count", "host", "dev")] + \
          [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}, {"srs": W - 1}, {"ors": W - 1}, {"sps": (H - 1) * srs + W - 1},
           {"ops": (H - 1) * ors + W - 1}, {"src": good["src"] + 2}, {"out": good["out"] + 2}, {"count": good["count"] + 1},
           {"n": -1}, {"n": 1025}, {"grow": -1}, {"grow": 256}, {"mask": 0}, {"mask": 16}, {"mask": -1},
           {"tile": 0, "fill": -1}, {"tile": 8, "fill": 0}, {"tile": 8, "fill": 255}, {"tile": 0, "fill": 256}, {"tile": 0, "fill": -2},
           {"tile": 8, "fill": -2}, {"tile": 1}, {"tile": 3}, {"tile": 12}, {"tile": 128}, {"tile": -8},
           {"out": good["src"]}, {"out": good["src"] + span - 4}, {"src": good["out"] + 4 * ops}, {"src": good["out"] + 4 * (H - 1) * ors}] + \
          [{"host": a.ctypes.data} for a in bad_lists]
    for b in bad:
        v = dict(good, **b)
        assert lib.hip().dcvc_redact(*[v[k] for k in order], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(count) == SENT16).all() and np.isnan(ko.cpu().numpy()).all()
    assert lib.hip().dcvc_redact(*[good[k] for k in order], U.stream(DEV)) == 0  # (and the arguments were good ones)
    want = R.expected(H, W, "classes", R.GROW, 8, -1)
    assert np.array_equal(U.f32_bits(ko.cpu().numpy()[omask]), U.f32_bits(want[0].reshape(-1)))
    assert np.array_equal(U.words(count)[c0:c0 + hc * wc], want[1].reshape(-1))
    # n == 0 needs no lists
    assert lib.hip().dcvc_redact(*[dict(good, host=None, dev=None, n=0)[k] for k in order], U.stream(DEV)) == 0
    assert np.array_equal(U.f32_bits(ko.cpu().numpy()[omask]), U.f32_bits(pic.reshape(-1))) and not U.words(count)[c0:c0 + hc * wc].any()


def _padded(pic, Hp, Wp):
    out = np.zeros((1, 3, Hp, Wp), F32)
    out[0, :, :pic.shape[1], :pic.shape[2]] = pic
    return out


def _roi(frames=None, names=R.NAMES):
    frames = frames or []
    return X.Roi(lambda g: X.FrameBoxes(frames[g]), tuple(X.RoiClass(0) for _ in names), names)


def test_redactor_launches_nothing_without_boxes_and_keeps_the_padding_zero():
    H, W, Hp, Wp = 70, 100, 128, 128
    pic, sets = R.picture(H, W), R.box_sets(H, W)
    setting = D.Redact(("liplates", "motion"), tile=8, grow=R.GROW)
    assert setting.mask(R.NAMES) == R.MASK
    f = D.Redactor(setting, _roi(), (H, W), DEV)
    assert f.padded == (Hp, Wp) and f.grid == R.grid(H, W) and f.launches == 0
    unselected = np.array([[3, 3, 30, 30, 1]])
    steps = ["classes", "none", "edges", unselected, "whole", "pixel"]
    x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
    source = x.clone()
    got, results, want_totals, launches = [], [], [], []
    for s in steps:
        boxes = sets[s] if isinstance(s, str) else s
        y = f.step(x, boxes)
        results.append(y)
        launches.append(f.launches)
        got.append(y.cpu().numpy())  # (a buffer of the redactor is valid until the step after the next: copy now)
        want, count = R.redact(pic, boxes, R.MASK, R.GROW, 8, -1)
        assert np.array_equal(U.f32_bits(got[-1]), U.f32_bits(_padded(want, Hp, Wp))), s  # (the padding: zeros)
        want_totals.append(int(count.sum()))
    assert launches == [1, 1, 2, 3, 4, 5]  # an empty list launches nothing ...
    assert results[1] is x and results[0] is not x  # ... and the picture is returned itself
    # a list of unselected classes only is not empty: it launches and copies (the file loops drop such boxes before)
    assert np.array_equal(U.f32_bits(got[3]), U.f32_bits(_padded(pic, Hp, Wp))) and want_totals[3] == 0
    assert results[0] is f.bufs[0] and results[2] is f.bufs[1] and results[3] is f.bufs[0] and results[4] is f.bufs[1]  # alternately
    assert torch.equal(x.view(torch.int32), source.view(torch.int32))  # the source is only read
    assert f.totals() == want_totals and want_totals[1] == 0 and want_totals[4] == H * W and not f._done
    f.flush()
    assert f.totals() == want_totals
    bare = D.Redactor(D.Redact(["liplates", "motion"], fill=17, grow=R.GROW), _roi(), (H, W), DEV, totals=False)
    y = bare.step(x, sets["classes"])
    assert np.array_equal(U.f32_bits(y.cpu().numpy()), U.f32_bits(_padded(R.redact(pic, sets["classes"], R.MASK, R.GROW, 0, 17)[0], Hp, Wp)))
    assert bare.launches == 1 and bare._rows is None and not bare._done
    with pytest.raises(ValueError, match="totals=False"):
        bare.totals()
    for bad in (x[0], x[:, :2], x.double(), x[..., :H, :W]):
        with pytest.raises(ValueError, match="expected a"):
            f.step(bad, sets["none"])
    with pytest.raises(ValueError, match="no CPU fallback"):
        f.step(x.cpu(), sets["none"])
    with pytest.raises(ValueError, match="no class 'motion'"):
        D.Redactor(setting, _roi(names=("liplates", "faces")), (H, W), DEV)
    with pytest.raises(ValueError, match="unknown class"):
        f.step(x, np.array([[0, 0, 4, 4, 3]]))
    # one picture, for library use
    out, count = D.redact_picture(x[..., :H, :W], sets["classes"], setting, R.NAMES)
    want = R.expected(H, W, "classes", R.GROW, 8, -1)
    assert np.array_equal(U.f32_bits(out.cpu().numpy()[0]), U.f32_bits(want[0])) and np.array_equal(count.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="no CPU fallback"):
        D.redact_picture(x.cpu()[..., :H, :W], sets["classes"], setting, R.NAMES)


# -------------------------------------------------------------------------------------------------------- file loops
# At 128 x 192 no report exists (MS-SSIM needs sides above 160): there the handed pictures, the bytes, the decoder, the
# hashes, the GOP streams, the residual layer and the command line are checked; everything about --report on a 176 x 192 clip.
GOP, N_FRAMES, FH, FW, RH = 4, 8, 128, 192, 176
SETTING = D.Redact(("liplates", "motion"), tile=8, grow=3, hold=2)
RESTORABLE = D.Redact(("liplates", "motion"), tile=8, grow=3, hold=2, restorable=True)


def _write_root(path, frames):
    """a PickleBoxes root with all three classes"""
    for cls, name in enumerate(R.NAMES):
        os.makedirs(path / f"{name}_coords")
        for t, a in enumerate(frames):
            with open(path / f"{name}_coords" / ("%05d" % (t + 1)), "wb") as f:
                pickle.dump(a[a[:, 4] == cls][:, :4].astype(np.uint16), f)
    boxes = X.PickleBoxes(str(path))
    assert boxes.names == R.NAMES
    return X.Roi(boxes, boxes.classes)


def _want(pics, frames, setting):
    """[(the picture the codec is handed, the counts)] by the restatement"""
    mask = setting.mask(R.NAMES)
    tile, fill = setting.mode()
    return [R.redact(pics[t], R.held_boxes(frames, t, mask, setting.hold), mask, setting.grow, tile, fill) for t in range(len(pics))]


def _handed(seen, want, H, W):
    """The pictures the codec was handed are the restatement's, bit for bit, in a padding of zeros."""
    assert sorted(seen) == list(range(N_FRAMES))
    for t in range(N_FRAMES):
        Hp, Wp = seen[t].shape[2:]
        assert (Hp, Wp) == ((H + 63) // 64 * 64, (W + 63) // 64 * 64)
        assert np.array_equal(U.f32_bits(seen[t]), U.f32_bits(_padded(want[t][0], Hp, Wp))), t


@contextlib.contextmanager
def _spies():
    """(the padded picture the codec was handed, the source the report measured against) by frame number, of the encodes
    run inside -- the technique of test_gpu_tnr.py."""
    from vcm_ts_amd import run_codec as RC

    seen, measured = {}, {}
    encode, add, add_yuv = RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv

    def spy_encode(self, frames, *a, **kw):
        def wrapped(k):
            for t, x in enumerate(frames(k)):
                seen[self.global_index(k, t)] = x.cpu().numpy()
                yield x
        return encode(self, wrapped, *a, **kw)

    def spy_add(self, g, recon, source, size):
        measured[g] = source.cpu().numpy()
        return add(self, g, recon, source, size)

    def spy_add_yuv(self, g, recon, source, size, sums):
        measured[g] = source.cpu().numpy()
        return add_yuv(self, g, recon, source, size, sums)

    RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv = spy_encode, spy_add, spy_add_yuv
    try:
        yield seen, measured
    finally:
        RC._EncodeRun.encode, RC._QualityLog.add, RC._VideoQualityLog.add_yuv = encode, add, add_yuv


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the clip as PNGs and its boxes as a root; the redacted encode -- the pictures its codec was handed captured on the
    way -- and a PLAIN encode of a folder holding the restatement's pictures"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("redact_e2e")
    pics, frames = list(R.clip(FH, FW)), R.clip_boxes(FH, FW)
    U.write_pngs(tmp / "png", pics)
    roi = _write_root(tmp / "root", frames)
    want = _want(pics, frames, SETTING)
    U.write_pngs(tmp / "want_png", [w[0] for w in want])
    RC.encode_folder(str(tmp / "want_png"), str(tmp / "plain_of_want"), gop=GOP, nets=file_nets)
    with _spies() as (seen, _):
        bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "red"), str(tmp / "red_rec"), gop=GOP, nets=file_nets,
                                      picture_hash=True, roi=roi, redact=SETTING)
    assert size == (FH, FW) and len(bits) == N_FRAMES
    return dict(tmp=tmp, pics=pics, frames=frames, roi=roi, seen=seen, want=want)


def test_the_codec_is_handed_the_restatements_pictures_and_writes_their_bytes(e2e):
    tmp, want, pics = e2e["tmp"], e2e["want"], e2e["pics"]
    _handed(e2e["seen"], want, FH, FW)
    touched = [int(w[1].sum()) for w in want]
    assert touched[0] > 0 and all(touched)  # picture 0 has no motion box of its own: hold reaches it from pictures 1 and 2
    for t in range(N_FRAMES):  # I pictures (0 and 4) and P pictures alike
        assert not np.array_equal(want[t][0], pics[t]), t
    # the plate the detector misses in pictures 3 and 4 is redacted there all the same, across the GOP boundary
    for t in (3, 4):
        assert not np.array_equal(want[t][0][:, 70:81, 62:80], pics[t][:, 70:81, 62:80]), t
    # the face (not selected) is untouched everywhere
    for t in range(N_FRAMES):
        assert np.array_equal(want[t][0][:, FH - 40:FH - 28, FW - 50:FW - 20], pics[t][:, FH - 40:FH - 28, FW - 50:FW - 20]), t
    assert U.bins(tmp / "red") == U.bins(tmp / "plain_of_want") and len(U.bins(tmp / "red")) == N_FRAMES
    assert sorted(n for n in os.listdir(tmp / "red") if not n.endswith(".bin")) == ["hashes.json", "redact.json"]
    assert json.loads((tmp / "red" / "redact.json").read_text()) == SETTING.to_json()


def test_an_unchanged_decoder_decodes_and_verifies(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    assert RC.decode_folder(str(tmp / "red"), str(tmp / "red_dec"), FH, FW, gop=GOP, verify="strict") == N_FRAMES
    U.same_pngs(tmp / "red_dec", tmp / "red_rec", N_FRAMES)


def test_two_gop_streams_write_the_same_bins(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "red2"), gop=GOP, nets=file_nets, gop_streams=2, roi=e2e["roi"], redact=SETTING)
    assert U.bins(tmp / "red2") == U.bins(tmp / "red")
    _handed(seen, e2e["want"], FH, FW)


def test_base_scale_codes_the_scaled_redacted_picture(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "want_png"), str(tmp / "half_of_want"), gop=GOP, nets=file_nets, base_scale="1/2")
    RC.encode_folder(str(tmp / "png"), str(tmp / "half"), gop=GOP, nets=file_nets, base_scale="1/2", roi=e2e["roi"], redact=SETTING)
    assert U.bins(tmp / "half") == U.bins(tmp / "half_of_want") and U.bins(tmp / "half") != U.bins(tmp / "red")
    assert (tmp / "half" / "scale.json").read_text() == (tmp / "half_of_want" / "scale.json").read_text()


def test_y4m_file(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp = e2e["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(pic, dtype=np.float64)) for pic in e2e["pics"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, FH, fps="30:1")
    # the 8-bit pictures the conversion gives, taken through the coding pass's own path
    with Y.open_video(str(tmp / "src.y4m")) as reader:
        src = [x.cpu().numpy()[0, :, :FH, :FW] for x, _ in RC._video_pictures(reader, range(N_FRAMES), reader.spec(), True, DEV)]
    want = _want(src, e2e["frames"], SETTING)
    with _spies() as (seen, _):
        RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), str(tmp / "enc.y4m"), quantize8=True, gop=GOP, nets=file_nets,
                        gop_streams=2, roi=e2e["roi"], redact=SETTING)
    _handed(seen, want, FH, FW)
    U.write_pngs(tmp / "vwant_png", [w[0] for w in want])
    RC.encode_folder(str(tmp / "vwant_png"), str(tmp / "plain_of_vwant"), gop=GOP, nets=file_nets)
    assert U.bins(tmp / "vbins") == U.bins(tmp / "plain_of_vwant")
    assert sorted(n for n in os.listdir(tmp / "vbins") if not n.endswith(".bin")) == ["redact.json", "sequence.json"]
    assert "redact" not in RC.read_sequence_info(str(tmp / "vbins"))
    assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == N_FRAMES
    assert (tmp / "dec.y4m").read_bytes() == (tmp / "enc.y4m").read_bytes()


def test_after_the_prefilter(e2e, file_nets):
    from tests import tnr_ref as TR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    tmp = e2e["tmp"]
    filtered = [w[0] for w in TR.run(e2e["pics"], (12, 64, 36), {0, 4})]  # (the filter's own state stays unredacted)
    want = _want(filtered, e2e["frames"], SETTING)
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "tnr_red"), gop=GOP, nets=file_nets, roi=e2e["roi"], redact=SETTING,
                         tnr=N.TNR(12, 64, 36))
    _handed(seen, want, FH, FW)
    assert U.bins(tmp / "tnr_red") != U.bins(tmp / "red")


def test_feature_off_and_refusals(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, roi = e2e["tmp"], e2e["roi"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets)
    plain = U.bins(tmp / "plain")
    os.makedirs(tmp / "none")
    (tmp / "none" / "redact.json").write_text("{}")  # a stale file of an earlier encode into the same folder
    RC.encode_folder(str(tmp / "png"), str(tmp / "none"), gop=GOP, nets=file_nets, roi=roi, redact=None)
    assert U.bins(tmp / "none") == plain and sorted(os.listdir(tmp / "none")) == sorted(plain) and plain != U.bins(tmp / "red")
    # a class no picture has a box of: nothing is launched, the plain bytes, but the file says what was asked for
    empty = _write_root(tmp / "root_faces_only", [f[f[:, 4] == 1] for f in e2e["frames"]])
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "untouched"), gop=GOP, nets=file_nets, roi=empty, redact=SETTING)
    assert U.bins(tmp / "untouched") == plain and (tmp / "untouched" / "redact.json").exists()
    for t in range(N_FRAMES):
        assert np.array_equal(U.f32_bits(seen[t][0, :, :FH, :FW]), U.f32_bits(e2e["pics"][t])), t
    for kw, name in ((dict(redact=SETTING), "needs roi="), (dict(redact=("motion", 8), roi=roi), "redact.Redact"),
                     (dict(redact=SETTING, roi=roi, residual_bins=str(tmp / "never_rl")), "restorable=True"),
                     (dict(redact=SETTING, roi=roi, residuals=str(tmp / "never.gbrp")), "restorable=True"),
                     (dict(redact=D.Redact(("plates",), fill=0), roi=roi), "no class 'plates'")):
        with pytest.raises(ValueError, match=name):
            RC.encode_folder(str(tmp / "png"), str(tmp / "never"), gop=GOP, nets=file_nets, **kw)
    assert not (tmp / "never").exists() and not (tmp / "never_rl").exists() and not (tmp / "never.gbrp").exists()
    many = X.Roi(lambda g: X.FrameBoxes(R.random_boxes(FH, FW, 600, g)), (X.RoiClass(0),) * 3, R.NAMES)
    with pytest.raises(ValueError, match="picture 0 .*boxes"):
        RC.encode_folder(str(tmp / "png"), str(tmp / "never"), gop=GOP, nets=file_nets, roi=many, redact=D.Redact(R.NAMES, fill=0, hold=1))
    assert not (tmp / "never").exists()


def test_restorable_residual_layer_holds_what_was_removed(e2e, file_nets):
    from tests import roi_ref as RR
    from tests import roil_ref as RL
    from vcm_ts_amd import roilayer as Y
    from vcm_ts_amd import run_codec as RC

    tmp, roi, pics = e2e["tmp"], e2e["roi"], e2e["pics"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "rest"), str(tmp / "rest_rec"), gop=GOP, nets=file_nets, gop_streams=2, roi=roi,
                     redact=RESTORABLE, residuals=str(tmp / "res.gbrp"), residual_bins=str(tmp / "rest"))
    assert U.bins(tmp / "rest") == U.bins(tmp / "red")  # the base layer is the redacted one, with or without the layer
    assert json.loads((tmp / "rest" / "redact.json").read_text())["restorable"] is True
    raw = np.frombuffer((tmp / "res.gbrp").read_bytes(), np.uint8).reshape(N_FRAMES, 3, FH, FW)
    assert RC.decode_folder(str(tmp / "rest"), str(tmp / "fused"), FH, FW, gop=GOP, roi=roi, residual_bins=str(tmp / "rest")) == N_FRAMES
    for t in range(N_FRAMES):
        boxes = roi.boxes(t).array  # the picture's OWN boxes, all classes: no grow, nothing held
        rec = U.png(tmp / "rest_rec" / f"im{t + 1:05d}.png", planar=True)
        want = RR.residual(pics[t], RR.T[rec], boxes)  # against the UNREDACTED source
        assert np.array_equal(raw[t], want[[1, 2, 0]]), t  # G, B, R planes
        record = (tmp / "rest" / f"im{t + 1:05d}{Y.FILE_EXT}").read_bytes()
        assert record == RL.encode_record(want, boxes, 1)[0], t
        # decode puts the content back wherever the residual was not clipped
        inside, fused = RR.binary_mask(boxes, FH, FW), U.png(tmp / "fused" / f"im{t + 1:05d}.png", planar=True)
        ok = inside[None] & (want > 0) & (want < 255)
        assert np.array_equal(fused[ok], R.code(pics[t])[ok]) and ok.any(), t
        assert np.array_equal(fused[:, ~inside], rec[:, ~inside]), t


@pytest.fixture(scope="module")
def reported(tmp_path_factory, file_nets):
    """the 176 x 192 clip coded with a report, plain and redacted"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("redact_report")
    pics, frames = list(R.clip(RH, FW)), R.clip_boxes(RH, FW)
    U.write_pngs(tmp / "png", pics)
    roi = _write_root(tmp / "root", frames)
    _, _, plain_rd = RC.encode_folder(str(tmp / "png"), str(tmp / "plain"), gop=GOP, nets=file_nets, report=True, roi=roi)
    with _spies() as (seen, measured):
        _, size, rd = RC.encode_folder(str(tmp / "png"), str(tmp / "red"), gop=GOP, nets=file_nets, report=str(tmp / "red.json"),
                                       roi=roi, redact=SETTING)
    assert size == (RH, FW)
    return dict(tmp=tmp, pics=pics, roi=roi, seen=seen, measured=measured, rd=rd, plain_rd=plain_rd, want=_want(pics, frames, SETTING))


def test_report_speaks_of_the_redaction_and_measures_against_the_source(reported, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, rd, want, pics, roi = reported["tmp"], reported["rd"], reported["want"], reported["pics"], reported["roi"]
    _handed(reported["seen"], want, RH, FW)
    assert rd["redact"] == SETTING.to_json()
    assert rd["frame_redacted"] == [int(w[1].sum()) / (RH * FW) for w in want] and all(v > 0 for v in rd["frame_redacted"])
    for t in range(N_FRAMES):
        assert int(want[t][1].sum()) == int(R.region(R.held_boxes(R.clip_boxes(RH, FW), t, 0b101, 2), RH, FW, 0b101, 3).sum()), t
    assert json.loads((tmp / "red.json").read_text()) == rd
    assert json.loads((tmp / "red" / "redact.json").read_text()) == SETTING.to_json()
    assert set(rd) - set(reported["plain_rd"]) == {"redact", "frame_redacted"} and set(reported["plain_rd"]) <= set(rd)
    assert sorted(n for n in os.listdir(tmp / "red") if not n.endswith(".bin")) == ["redact.json"]
    # PSNR, MS-SSIM and the ROI figures are measured against the UNREDACTED source, which is not what the codec was handed
    for t in range(N_FRAMES):
        assert np.array_equal(U.f32_bits(reported["measured"][t][0, :, :RH, :FW]), U.f32_bits(pics[t])), t
        assert not np.array_equal(reported["measured"][t], reported["seen"][t]), t
    assert len(rd["frame_psnr"]) == N_FRAMES and all(np.isfinite(rd["frame_psnr"]))
    assert len(rd["frame_psnr_roi"]) == N_FRAMES and rd["frame_roi_pixels"] == reported["plain_rd"]["frame_roi_pixels"]
    # two GOP streams: the same bytes and the same figures
    _, _, rd2 = RC.encode_folder(str(tmp / "png"), str(tmp / "red2"), gop=GOP, nets=file_nets, gop_streams=2, report=True, roi=roi,
                                 redact=SETTING)
    assert U.bins(tmp / "red2") == U.bins(tmp / "red")
    for key in ("redact", "frame_redacted", "frame_bpp", "frame_psnr_roi"):
        assert rd2[key] == rd[key], key
    # redact=None: the bytes and the report keys of a run without the argument, and no file
    _, _, rd0 = RC.encode_folder(str(tmp / "png"), str(tmp / "none"), gop=GOP, nets=file_nets, report=True, roi=roi, redact=None)
    assert U.bins(tmp / "none") == U.bins(tmp / "plain") and list(rd0) == list(reported["plain_rd"])
    assert rd0["frame_bpp"] == reported["plain_rd"]["frame_bpp"] and sorted(os.listdir(tmp / "none")) == sorted(U.bins(tmp / "plain"))


def test_command_line(e2e, file_nets, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--picture-hash", "--roi-root",
             str(tmp / "root"), "--redact", "liplates", "motion", "--redact-tile", "8", "--redact-grow", "3", "--redact-hold", "2"])
    assert U.bins(tmp / "cli") == U.bins(tmp / "red")
    assert (tmp / "cli" / "redact.json").read_text() == (tmp / "red" / "redact.json").read_text()
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_dec"), "--height", str(FH), "--width", str(FW),
             "--gop", str(GOP), "--verify", "strict"])
    U.same_pngs(tmp / "cli_dec", tmp / "red_rec", N_FRAMES)
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli2"), "--gop", str(GOP), "--roi-root", str(tmp / "root"),
             "--redact", "faces", "--redact-fill", "16", "--redact-restorable", "--residual-bins", str(tmp / "cli2")])
    fill = D.Redact(("faces",), fill=16, restorable=True)
    with _spies() as (seen, _):
        RC.encode_folder(str(tmp / "png"), str(tmp / "api2"), gop=GOP, nets=file_nets, roi=e2e["roi"], redact=fill)
    assert U.bins(tmp / "cli2") == U.bins(tmp / "api2") and U.bins(tmp / "cli2") != U.bins(tmp / "red")
    assert json.loads((tmp / "cli2" / "redact.json").read_text()) == fill.to_json()
    assert len([n for n in os.listdir(tmp / "cli2") if n.endswith(".rl")]) == N_FRAMES
    want = _want(e2e["pics"], e2e["frames"], fill)
    _handed(seen, want, FH, FW)
    assert (want[0][0][:, FH - 40:FH - 28, FW - 50:FW - 20] == R.T[16]).all()
