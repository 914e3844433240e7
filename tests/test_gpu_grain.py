"""Film-grain synthesis on a real MI355X: both kernels bit for bit against the numpy restatement (tests/grain_ref.py) in
strided, offset, NaN-surrounded layouts with guarded outputs, their refusals, GrainMeter and GrainSynth, and the file loops
end to end: grain.json, every other output unchanged, the grained pictures, the verifier, a base layer, a Y4M file, the
command line."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import grain_ref as G
from tests import tnr_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from vcm_ts_amd import grain as GR
from vcm_ts_amd import lib
from vcm_ts_amd import tnr as N

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
F32 = np.float32
SENT16, SENT64 = 0xABCD, 0x2BCD1234ABCD1234
# (row pad, plane pad, offset of the pictures, shift of acc / held): 16-byte accesses; an odd offset, an odd row stride, an
# odd plane stride -> 4-byte accesses; held at every alignment its type allows
LAYOUTS = [(8, 24, 12, 0), (8, 24, 13, 1), (5, 24, 12, 2), (8, 23, 12, 3)]
SETTING = (12, 64, 36)


def _pictures(H, W):
    """(source, filtered) of picture 2 of the noisy clip: the restatement's filter, so e is what the filter took out; with a
    NaN and a sample beyond the range in each."""
    pics = list(R.clip(H, W)[0][:3])
    run = R.run(pics, SETTING, {0})
    src, flt = pics[2].copy(), run[2][0].copy()
    src[0, 0, 0], flt[2, H - 1, W - 1] = np.nan, F32(1.25)
    src[1, H // 2, W // 2], flt[0, H // 2, 0] = F32(-0.5), np.nan
    return src, flt


def _measure(src, flt, held, start, H, W, layout, calls=1):
    """acc after `calls` launches in `layout`, starting from `start`; the guards and the inputs are checked here."""
    row_pad, plane_pad, offset, shift = layout
    hc, wc = G.grid(H, W)
    ks, vs, srs, sps, mask = U.strided(src, H, W, row_pad, plane_pad, offset, DEV)
    kf, vf, frs, fps, _ = U.strided(flt, H, W, row_pad, plane_pad, offset, DEV)
    hbuf, h0 = U.guarded(hc * wc, shift, np.uint16, SENT16, DEV)
    hbuf[h0:h0 + hc * wc] = torch.from_numpy(np.asarray(held, dtype=np.uint16).reshape(-1).view(np.int16)).to(DEV)
    abuf, a0 = U.guarded(G.WORDS, shift, np.uint64, SENT64, DEV)
    abuf[a0:a0 + G.WORDS] = torch.from_numpy(np.asarray(start, dtype=np.int64)).to(DEV)
    for _ in range(calls):
        lib.check(lib.hip().dcvc_grain_measure(vs.data_ptr(), srs, sps, vf.data_ptr(), frs, fps, H, W, hbuf.data_ptr() + 2 * h0,
                                               abuf.data_ptr() + 8 * a0, U.stream(DEV)), "grain_measure")
    got = abuf.cpu().numpy()[a0:a0 + G.WORDS].copy()
    assert U.guards_intact(abuf, a0, G.WORDS, SENT64) and U.guards_intact(hbuf, h0, hc * wc, SENT16)
    assert np.array_equal(U.words(hbuf)[h0:h0 + hc * wc], np.asarray(held, dtype=np.int64).reshape(-1))
    for k, pic in ((ks, src), (kf, flt)):  # the inputs are only read
        assert np.array_equal(k.cpu().numpy()[mask].view(np.uint32), pic.reshape(-1).view(np.uint32))
    return got


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_measure_equals_the_restatement_bit_for_bit(size):
    H, W = size
    src, flt = _pictures(H, W)
    start = np.random.default_rng(H + W).integers(-2 ** 40, 2 ** 40, G.WORDS)
    zeros = np.zeros(G.WORDS, dtype=np.int64)
    for name, held in G.held_cases(H, W).items():
        once = G.measure(src, flt, held)
        for n, layout in enumerate(LAYOUTS):
            begin = start if n % 2 else zeros
            assert np.array_equal(_measure(src, flt, held, begin, H, W, layout), begin + once), (name, layout)
        assert np.array_equal(_measure(src, flt, held, start, H, W, LAYOUTS[0], calls=2), start + 2 * once), name  # acc is ADDED TO
        if name == "full":
            assert once[0::4].sum() == H * W and once[1::4].sum() > 0
        if name == "none":  # a zeroed acc with no full cell stays zero
            assert not once.any() and not _measure(src, flt, held, zeros, H, W, LAYOUTS[1]).any()
        if name == "edge":
            assert once[0::4].sum() == H * W - int(G.full_counts(H, W)[(H - 1) // 16, (W - 1) // 16])
    # zeros against ones: e = 255 everywhere, the largest sums a strip can hold
    ones, none = np.ones((3, H, W), F32), np.zeros((3, H, W), F32)
    want = G.measure(ones, none, G.full_counts(H, W))
    assert want[1] == 255 * 255 * H * W and np.array_equal(_measure(ones, none, G.full_counts(H, W), zeros, H, W, LAYOUTS[0]), want)


def _apply(pic, t, taps, stab, H, W, layout, where):
    row_pad, plane_pad, offset, shift = layout
    ki, vi, irs, ips, mask = U.strided(pic, H, W, row_pad, plane_pad, offset, DEV)
    ko, vo, ors, ops, _ = U.strided(None, H, W, row_pad, plane_pad, offset, DEV)
    sbuf, s0 = U.guarded(256, shift, np.uint16, SENT16, DEV)
    sbuf[s0:s0 + 256] = torch.from_numpy(np.asarray(stab, dtype=np.uint16).view(np.int16)).to(DEV)
    lib.check(lib.hip().dcvc_grain_apply(vi.data_ptr(), irs, ips, vo.data_ptr(), ors, ops, H, W, t, taps[0], taps[1],
                                         sbuf.data_ptr() + 2 * s0, U.stream(DEV)), "grain_apply")
    got = ko.cpu().numpy()
    want = G.apply(pic, t, taps[0], taps[1], stab)
    assert np.array_equal(got[mask].view(np.uint32), want.reshape(-1).view(np.uint32)), where
    assert np.isnan(got[~mask]).all(), where  # nothing outside the crop of out is touched
    assert np.array_equal(ki.cpu().numpy()[mask].view(np.uint32), pic.reshape(-1).view(np.uint32)), where
    assert U.guards_intact(sbuf, s0, 256, SENT16), where
    return want


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_equals_the_restatement_bit_for_bit(size):
    H, W = size
    src, _ = _pictures(H, W)
    stabs = G.stabs()
    n = 0
    for t in G.TIMES:
        for taps in G.TAPS:
            for layout in (LAYOUTS if n % 4 == 0 else [LAYOUTS[n % 4]]):  # (every layout on every third case, one on the others)
                out = _apply(src, t, taps, stabs["rising"], H, W, layout, (t, taps, layout))
            n += 1
            if H * W > 64:
                assert not np.array_equal(out.view(np.uint32), src.view(np.uint32))
    for layout in LAYOUTS[:2]:
        same = _apply(src, 7, (7, 3), stabs["zero"], H, W, layout, ("zero", layout))  # s == 0 copies the bits, a NaN's too
        assert np.array_equal(same.view(np.uint32), src.view(np.uint32))
        for value in (0.0, 1.0):  # the clamps: the strongest grain on the range's two ends
            flat = np.full((3, H, W), value, F32)
            out = _apply(flat, 1, (24, -24), stabs["max"], H, W, layout, ("max", value, layout))
            assert out.min() >= 0.0 and out.max() <= 1.0 and (H * W < 64 or ((out == value).any() and (out != value).any()))
        ramp = G.ramp(H, W)
        if H * W >= 256:
            assert set(G.luma(ramp).ravel().tolist()) == set(range(256))  # every table entry is visited
        _apply(ramp, 2, (7, 3), stabs["rising"], H, W, layout, ("ramp", layout))
        half = _apply(ramp, 2 ** 31 - 1, (-24, 24), stabs["even-zero"], H, W, layout, ("ramp, even-zero", layout))
        even = (G.luma(ramp) % 2 == 0)[None].repeat(3, 0)
        assert np.array_equal(half[even].view(np.uint32), ramp[even].view(np.uint32))


def test_entry_point_refusals_leave_the_outputs_alone():
    H, W = 70, 100
    hc, wc = G.grid(H, W)
    src, flt = _pictures(H, W)
    ks, vs, rs, ps, mask = U.strided(src, H, W, 8, 24, 12, DEV)
    kf, vf, _, _, _ = U.strided(flt, H, W, 8, 24, 12, DEV)
    ko, vo, _, _, _ = U.strided(None, H, W, 8, 24, 12, DEV)
    held, h0 = U.guarded(hc * wc, 0, np.uint16, SENT16, DEV)
    full = G.full_counts(H, W)
    held[h0:h0 + hc * wc] = torch.from_numpy(full.astype(np.uint16).reshape(-1).view(np.int16)).to(DEV)
    acc, a0 = U.guarded(G.WORDS, 0, np.uint64, SENT64, DEV)
    stab = torch.from_numpy(G.stabs()["rising"].view(np.int16)).to(DEV)
    m = dict(src=vs.data_ptr(), srs=rs, sps=ps, flt=vf.data_ptr(), frs=rs, fps=ps, H=H, W=W, held=held.data_ptr() + 2 * h0,
             acc=acc.data_ptr() + 8 * a0)
    order = ("src", "srs", "sps", "flt", "frs", "fps", "H", "W", "held", "acc")
    bad = [{k: None} for k in ("src", "flt", "held", "acc")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("srs", "frs")] + [{k: (H - 1) * rs + W - 1} for k in ("sps", "fps")] + \
          [{k: m[k] + 2} for k in ("src", "flt")] + [{"held": m["held"] + 1}, {"acc": m["acc"] + 4}]
    for b in bad:
        v = dict(m, **b)
        assert lib.hip().dcvc_grain_measure(*[v[k] for k in order], U.stream(DEV)) == -1, b
    a = dict(inp=vs.data_ptr(), irs=rs, ips=ps, out=vo.data_ptr(), ors=rs, ops=ps, H=H, W=W, t=3, kh=7, kv=3, stab=stab.data_ptr())
    aorder = ("inp", "irs", "ips", "out", "ors", "ops", "H", "W", "t", "kh", "kv", "stab")
    span = 4 * (2 * ps + (H - 1) * rs + W)
    bad = [{k: None} for k in ("inp", "out", "stab")] + [{"H": 0}, {"W": 0}, {"H": 32769}, {"W": 32769}] + \
          [{k: W - 1} for k in ("irs", "ors")] + [{k: (H - 1) * rs + W - 1} for k in ("ips", "ops")] + \
          [{k: a[k] + 2} for k in ("inp", "out")] + [{"stab": a["stab"] + 1}, {"kh": 25}, {"kh": -25}, {"kv": 25}, {"kv": -25}, {"t": -1}] + \
          [{"out": a["inp"]}, {"out": a["inp"] + span - 4}, {"out": a["inp"] - span + 4}, {"inp": a["out"] + 4 * ps}]
    for b in bad:
        v = dict(a, **b)
        assert lib.hip().dcvc_grain_apply(*[v[k] for k in aorder], U.stream(DEV)) == -1, b
    torch.cuda.synchronize(DEV)
    assert (U.words(acc) == SENT64).all() and np.isnan(ko.cpu().numpy()).all()
    acc[a0:a0 + G.WORDS] = 0  # (and the arguments were good ones)
    assert lib.hip().dcvc_grain_measure(*[m[k] for k in order], U.stream(DEV)) == 0
    assert np.array_equal(acc.cpu().numpy()[a0:a0 + G.WORDS], G.measure(src, flt, full)) and U.guards_intact(acc, a0, G.WORDS, SENT64)
    assert lib.hip().dcvc_grain_apply(*[a[k] for k in aorder], U.stream(DEV)) == 0
    want = G.apply(src, 3, 7, 3, G.stabs()["rising"])
    assert np.array_equal(ko.cpu().numpy()[mask].view(np.uint32), want.reshape(-1).view(np.uint32))


def _padded(pic, Hp, Wp):
    out = np.zeros((1, 3, Hp, Wp), F32)
    out[0, :, :pic.shape[1], :pic.shape[2]] = pic
    return out


def test_meter_and_synth_follow_the_gops():
    from vcm_ts_amd.scenecut import GopPlan

    H, W, Hp, Wp = 70, 100, 128, 128
    pics, intra = list(R.clip(H, W)[0]), {0, 4}
    gops, run = G.record(pics, SETTING, intra, 256)
    f, meter = N.TnrFilter(N.TNR(*SETTING), (H, W), DEV, totals=False), GR.GrainMeter((H, W), DEV)
    with pytest.raises(ValueError, match="first picture of a stream is an I picture"):
        meter.step(torch.zeros((1, 3, Hp, Wp), device=DEV), f, 0, False)
    for t, pic in enumerate(pics):
        x = torch.from_numpy(_padded(pic, Hp, Wp)).to(DEV)
        f.step(x, t in intra)
        meter.step(x, f, t, t in intra)
    # an I picture launches nothing; the first GOP's sums left in one copy when the second began, and nobody has waited for them
    assert meter.launches == len(pics) - 2 and len(meter._log.done) == 1 and meter._log.keys == [4]
    sums = meter.sums()
    assert sorted(sums) == [0, 4] and not meter._log.done
    assert {g: GR.params(acc, 256) for g, acc in sums.items()} == gops and max(gops[0]["points"]) > 0 and max(gops[4]["points"]) > 0
    with pytest.raises(ValueError, match="no CPU fallback"):
        meter.step(torch.zeros((1, 3, Hp, Wp)), f, 9, False)
    # the synthesis: I pictures and an all-zero GOP are returned themselves, nothing launched; P pictures are grained copies
    plan = GopPlan(len(pics), sorted(intra))
    record = GR.record_of(GR.Grain(256), N.TNR(*SETTING), {**gops, 4: dict(gops[4], points=[0] * 8)})
    synth = GR.GrainSynth(record, plan, (H, W), DEV, 100)
    shown = G.grained([r[0] for r in run], gops, intra)
    launches = []
    for t in range(len(pics)):
        x = torch.from_numpy(_padded(run[t][0], Hp, Wp)).to(DEV)
        y = synth.shown(t, x)
        launches.append(synth.launches)
        assert (y is x) == (t == 0 or t >= 4), t
        if y is not x:
            assert np.array_equal(y.cpu().numpy().view(np.uint32), _padded(shown[t], Hp, Wp).view(np.uint32)), t
            assert not np.array_equal(shown[t], run[t][0])
    assert launches == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    both = GR.GrainSynth(GR.record_of(GR.Grain(256), N.TNR(*SETTING), gops), plan, (H, W), DEV, 200)  # across the boundary
    tab = G.table(gops[4]["points"], gops[4]["kh"], gops[4]["kv"], 200)
    for t in (3, 4, 5):
        x = torch.from_numpy(_padded(run[t][0], Hp, Wp)).to(DEV)
        want = run[t][0] if t == 4 else G.apply(run[t][0], t, gops[t // 4 * 4]["kh"], gops[t // 4 * 4]["kv"],
                                                G.table(gops[t // 4 * 4]["points"], gops[t // 4 * 4]["kh"], gops[t // 4 * 4]["kv"], 200))
        assert np.array_equal(both.shown(t, x).cpu().numpy().view(np.uint32), _padded(want, Hp, Wp).view(np.uint32)), t
    assert tab.any()
    with pytest.raises(ValueError, match="plan"):
        GR.GrainSynth(record, GopPlan.fixed(len(pics), 3), (H, W), DEV)
    with pytest.raises(ValueError, match="percent"):
        GR.GrainSynth(record, plan, (H, W), DEV, 0)


# -------------------------------------------------------------------------------------------------------- file loops
GOP, N_FRAMES, FH, FW = 4, 8, 128, 192
TNR = N.TNR(*SETTING)
INTRA = {0, 4}


@contextlib.contextmanager
def _shown():
    """{frame number: the float32 picture the output stage was handed} of the decodes run inside."""
    from vcm_ts_amd import run_codec as RC

    seen = {}
    png_put, video_put = RC._PngStage.put, RC._VideoStage.put

    def spy(put):
        def wrapped(self, k, g, frame):
            seen[g] = frame.cpu().numpy()
            return put(self, k, g, frame)
        return wrapped

    RC._PngStage.put, RC._VideoStage.put = spy(png_put), spy(video_put)
    try:
        yield seen
    finally:
        RC._PngStage.put, RC._VideoStage.put = png_put, video_put


def _files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def _grained_equals(plain, grained, gops, h, w, percent=100):
    """The grained decode's pictures are the restatement applied to the plain decode's; I pictures are identical."""
    want = G.grained([plain[t][0, :, :h, :w] for t in range(N_FRAMES)], gops, INTRA, percent)
    for t in range(N_FRAMES):
        got = grained[t][0, :, :h, :w]
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want[t]).view(np.uint32)), t
        assert np.array_equal(got, plain[t][0, :, :h, :w]) == (t in INTRA), t


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, file_nets):
    """the noisy clip as PNGs, coded with the prefilter: without the measurement and with it"""
    from vcm_ts_amd import run_codec as RC

    tmp = tmp_path_factory.mktemp("grain_e2e")
    u8 = np.rint(R.clip(FH, FW)[0][:N_FRAMES] * 255).astype(np.uint8)
    U.write_pngs(tmp / "png", u8.transpose(0, 2, 3, 1))
    pics = [a.astype(F32) / F32(255.0) for a in u8]
    RC.encode_folder(str(tmp / "png"), str(tmp / "tnr"), str(tmp / "tnr_rec"), gop=GOP, nets=file_nets, picture_hash=True, tnr=TNR)
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "grain"), str(tmp / "grain_rec"), gop=GOP, nets=file_nets,
                                  picture_hash=True, tnr=TNR, grain=GR.Grain())
    assert size == (FH, FW) and len(bits) == N_FRAMES
    gops, _ = G.record(pics, SETTING, INTRA, 1024)
    return dict(tmp=tmp, pics=pics, gops=gops)


def test_encode_writes_the_restatements_record_and_nothing_else_changes(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, gops = e2e["tmp"], e2e["gops"]
    want = {"version": 1, "min_samples": 1024, "tnr": TNR.to_json(), "gops": {str(g): gops[g] for g in sorted(gops)}}
    assert json.loads((tmp / "grain" / "grain.json").read_text()) == want
    assert all(max(rec["points"]) > 0 for rec in gops.values())  # (the clip's GOPs have something to say)
    with_, without = _files(tmp / "grain"), _files(tmp / "tnr")
    assert sorted(set(with_) - set(without)) == ["grain.json"] and all(with_[n] == without[n] for n in without)
    assert "hashes.json" in without and _files(tmp / "grain_rec") == _files(tmp / "tnr_rec")
    RC.encode_folder(str(tmp / "png"), str(tmp / "grain2"), gop=GOP, nets=file_nets, gop_streams=2, picture_hash=True, tnr=TNR,
                     grain=GR.Grain())
    assert _files(tmp / "grain2") == with_  # two GOP streams: the same record, the same bytes
    RC.encode_folder(str(tmp / "png"), str(tmp / "grain2"), gop=GOP, nets=file_nets, picture_hash=True, tnr=TNR)
    assert _files(tmp / "grain2") == without  # (a stale grain.json is removed)


def test_decode_grains_the_p_pictures_it_writes(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, gops = e2e["tmp"], e2e["gops"]
    with _shown() as plain:
        assert RC.decode_folder(str(tmp / "grain"), str(tmp / "dec"), FH, FW, gop=GOP) == N_FRAMES
    U.same_pngs(tmp / "dec", tmp / "tnr_rec", N_FRAMES)  # without the option: the bytes of before, grain.json is not followed
    with _shown() as grained:
        assert RC.decode_folder(str(tmp / "grain"), str(tmp / "dec_g"), FH, FW, gop=GOP, grain=100, verify="strict") == N_FRAMES
    _grained_equals(plain, grained, gops, FH, FW)
    for t in range(N_FRAMES):  # (the PNGs: I pictures are the files of before, P pictures are not)
        name = f"im{t + 1:05d}.png"
        assert ((tmp / "dec_g" / name).read_bytes() == (tmp / "dec" / name).read_bytes()) == (t in INTRA), t
    with _shown() as half:
        RC.decode_folder(str(tmp / "grain"), str(tmp / "dec_h"), FH, FW, gop=GOP, grain=50)
    _grained_equals(plain, half, gops, FH, FW, 50)
    from vcm_ts_amd import picturehash as PH

    assert PH.verify_pngs(str(tmp / "grain"), str(tmp / "dec")) is None
    assert PH.verify_pngs(str(tmp / "grain"), str(tmp / "dec_g")) is not None  # deliberately: the digests are of the ungrained picture
    with pytest.raises(ValueError, match=r"no grain\.json"):
        RC.decode_folder(str(tmp / "tnr"), str(tmp / "never"), FH, FW, gop=GOP, grain=100)
    assert not (tmp / "never").exists()


def test_base_layer_is_grained_at_display_size(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.encode_folder(str(tmp / "png"), str(tmp / "half"), gop=GOP, nets=file_nets, base_scale="1/2", tnr=TNR, grain=GR.Grain())
    assert json.loads((tmp / "half" / "grain.json").read_text()) == json.loads((tmp / "grain" / "grain.json").read_text())
    with _shown() as plain:
        RC.decode_folder(str(tmp / "half"), str(tmp / "half_dec"), FH, FW, gop=GOP)
    with _shown() as grained:
        RC.decode_folder(str(tmp / "half"), str(tmp / "half_g"), FH, FW, gop=GOP, grain=100)
    assert grained[1].shape[2] >= FH and grained[1].shape[3] >= FW
    _grained_equals(plain, grained, e2e["gops"], FH, FW)
    with pytest.raises(ValueError, match="takes no grain="):
        RC.decode_folder(str(tmp / "half"), str(tmp / "never"), FH, FW, gop=GOP, grain=100, base_scale=None)


def test_y4m_round_trip(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y

    tmp = e2e["tmp"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(pic, dtype=np.float64)) for pic in e2e["pics"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, FW, FH, fps="30:1")
    with Y.open_video(str(tmp / "src.y4m")) as reader:
        src = [x.cpu().numpy()[0, :, :FH, :FW] for x, _ in RC._video_pictures(reader, range(N_FRAMES), reader.spec(), False, DEV)]
    gops, _ = G.record(src, SETTING, INTRA, 512)
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vtnr"), gop=GOP, nets=file_nets, tnr=TNR)
    RC.encode_video(str(tmp / "src.y4m"), str(tmp / "vbins"), gop=GOP, nets=file_nets, gop_streams=2, tnr=TNR, grain=GR.Grain(512))
    record = json.loads((tmp / "vbins" / "grain.json").read_text())
    assert record["gops"] == {str(g): gops[g] for g in sorted(gops)} and record["min_samples"] == 512
    with_, without = _files(tmp / "vbins"), _files(tmp / "vtnr")
    assert sorted(set(with_) - set(without)) == ["grain.json"] and all(with_[n] == without[n] for n in without)
    with _shown() as plain:
        assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec.y4m")) == N_FRAMES
    with _shown() as grained:
        assert RC.decode_video(str(tmp / "vbins"), str(tmp / "dec_g.y4m"), grain=100) == N_FRAMES
    _grained_equals(plain, grained, gops, FH, FW)
    assert (tmp / "dec.y4m").stat().st_size == (tmp / "dec_g.y4m").stat().st_size
    assert (tmp / "dec.y4m").read_bytes() != (tmp / "dec_g.y4m").read_bytes()


def test_command_line(e2e, capsys):
    from vcm_ts_amd import run_codec as RC

    tmp = e2e["tmp"]
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli"), "--gop", str(GOP), "--tnr", "12", "--grain",
             "--picture-hash"])
    assert _files(tmp / "cli") == _files(tmp / "grain")
    RC.main(["encode", "--frames", str(tmp / "png"), "--bins", str(tmp / "cli2"), "--gop", str(GOP), "--tnr", "12", "--grain",
             "--grain-min-samples", "100000"])
    record = json.loads((tmp / "cli2" / "grain.json").read_text())
    assert record["min_samples"] == 100000 and all(not any(rec["points"]) for rec in record["gops"].values())
    common = ["--height", str(FH), "--width", str(FW), "--gop", str(GOP)]
    for percent in (100, 50):  # (the API's pictures of the same folder)
        RC.decode_folder(str(tmp / "grain"), str(tmp / f"api_{percent}"), FH, FW, gop=GOP, grain=percent)
    RC.decode_folder(str(tmp / "grain"), str(tmp / "api_plain"), FH, FW, gop=GOP)
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_g"), "--grain", "--verify", "strict"] + common)
    U.same_pngs(tmp / "cli_g", tmp / "api_100", N_FRAMES)
    RC.main(["decode", "--bins", str(tmp / "cli"), "--recon", str(tmp / "cli_h"), "--grain", "50"] + common)
    U.same_pngs(tmp / "cli_h", tmp / "api_50", N_FRAMES)
    assert (tmp / "cli_h" / "im00002.png").read_bytes() != (tmp / "cli_g" / "im00002.png").read_bytes()
    RC.main(["decode", "--bins", str(tmp / "cli2"), "--recon", str(tmp / "cli_0"), "--grain"] + common)  # all-zero GOPs: nothing added
    U.same_pngs(tmp / "cli_0", tmp / "api_plain", N_FRAMES)
