"""The base layer's resampler on the device (csrc/scale.hip) against tests/scale_ref.py bit for bit, the two layers chained
without the codec, and the file loops with a base scale.

Shapes are the smallest at which the kernel can go wrong: odd sides and sides that are no multiple of 4 (scalar loads and
stores), every tap count (12, 9, 9 again at 3/4, 24, and 6 upwards), 130x260 -> 65x130 for more than one tile in both
directions (a tile is 16 rows x 64 columns), contiguous pictures and offset, strided views of NaN-filled buffers.

The end-to-end tests run 16 pictures, GOP 8, at full sizes 128x128 (1/2) and 96x96 (2/3): both give the 64x64 base the
suite already codes.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import gpu_util as U
from tests import roi_ref as XR
from tests import scale_ref as R
from tests.gpu_util import file_nets, no_garbage_left_behind  # noqa: F401 (fixtures)
from tests.test_scale_host import _HostScale
from vcm_ts_amd import picturehash as PH
from vcm_ts_amd import roi as X
from vcm_ts_amd import scale as SC
from vcm_ts_amd import synthetic

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("no_garbage_left_behind")]
DEV = torch.device("cuda:0")
NAN = float("nan")

# (full size, ratio)
CASES = [((40, 52), (1, 2)), ((96, 160), (2, 3)), ((75, 107), (3, 4)), ((100, 132), (1, 4)), ((130, 260), (1, 2))]
_IDS = [f"{h}x{w}at{n}of{d}" for (h, w), (n, d) in CASES]


def _data(seed, shape):
    """random values, a fifth of them outside [0, 1], a few NaN inside"""
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    a = np.where(rng.random(shape) < 0.2, a * 3.0 - 1.0, a).astype(np.float32)
    flat = a.reshape(-1)
    flat[rng.integers(0, flat.size, 5)] = np.nan
    return a


def _view(shape, off=3, pad_w=5, pad_h=2):
    """a (1, 3, H, W) view at an odd element offset inside a larger NaN-filled buffer, rows longer than W, slack between
    the planes; (buffer, view, mask of the buffer's elements that belong to the view)"""
    _, C_, H, W = shape
    rs = W + pad_w
    ps = (H + pad_h) * rs + 1
    buf = torch.full((off + C_ * ps + 7,), NAN, dtype=torch.float32, device=DEV)
    v = buf.as_strided((1, C_, H, W), (C_ * ps, ps, rs, 1), off)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside.as_strided((1, C_, H, W), (C_ * ps, ps, rs, 1), off).fill_(True)
    return buf, v, inside


@pytest.fixture(scope="module")
def refs():
    """per case: the source, its down-scaled picture and that one scaled up again, by the restatement (computed once)"""
    out = {}
    for (h, w), (n, d) in CASES:
        src = _data(h * 1000 + w, (1, 3, h, w))
        base = R.down(src, n, d)
        # the way up starts from data of its own: base-size values outside [0, 1] and NaN too
        low = _data(h * 1000 + w + 1, base.shape)
        out[(h, w)] = dict(src=src, down=base, low=low, up=R.up(low, (h, w)))
    return out


@pytest.mark.parametrize("layout", ["contiguous", "views"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_kernel_equals_the_restatement_bit_for_bit(case, layout, refs):
    (h, w), (n, d) = case
    ref = refs[(h, w)]
    s = SC.Scale((h, w), (n, d), DEV)
    assert s.base == R.base_size(h, w, n, d) == ref["down"].shape[-2:]
    for which, fn, src, want in (("down", s.down, ref["src"], ref["down"]), ("up", s.up, ref["low"], ref["up"])):
        assert np.isnan(src).any() and (src[np.isfinite(src)] > 1).any() and (src[np.isfinite(src)] < 0).any()
        if layout == "contiguous":
            got = fn(torch.from_numpy(src).to(DEV))
            assert got.is_contiguous() and tuple(got.shape) == want.shape
        else:
            _, x, _ = _view(src.shape)
            x.copy_(torch.from_numpy(src))
            buf, got, inside = _view(want.shape, off=5, pad_w=3, pad_h=1)
            assert x.data_ptr() % 16 and got.data_ptr() % 16
            assert fn(x, out=got) is got
            assert torch.isnan(buf[~inside]).all() and not torch.isnan(buf[inside]).any()  # the surroundings are intact
        np.testing.assert_array_equal(U.f32_bits(got.cpu().numpy()), U.f32_bits(want), err_msg=which)
        assert not np.isnan(want).any() and want.min() >= 0 and want.max() <= 1 and (want == 0).any()  # (clamped; NaN -> 0)
        assert which == "down" or (want == 1).any()


def test_aligned_padded_interior_and_batches(refs):
    """What the codec does: the down-scaled picture written into the interior of a zeroed 64-padded picture (16-byte
    aligned rows: the vector path), the crop of a padded reconstruction read in place; and several pictures in one call."""
    (h, w), (n, d) = CASES[1]
    ref = refs[(h, w)]
    s = SC.Scale((h, w), (n, d), DEV)
    hb, wb = s.base
    padded = torch.zeros((1, 3, 128, 128), device=DEV)
    s.down(torch.from_numpy(ref["src"]).to(DEV), out=padded[..., :hb, :wb])
    np.testing.assert_array_equal(U.f32_bits(padded[..., :hb, :wb].cpu().numpy()), U.f32_bits(ref["down"]))
    assert float(padded[..., hb:, :].abs().sum()) == 0 and float(padded[..., :, wb:].abs().sum()) == 0
    padded[..., :hb, :wb] = torch.from_numpy(ref["low"]).to(DEV)
    padded[..., hb:, :] = NAN
    padded[..., :, wb:] = NAN
    np.testing.assert_array_equal(U.f32_bits(s.up(padded[..., :hb, :wb]).cpu().numpy()), U.f32_bits(ref["up"]))
    both = torch.from_numpy(np.stack([ref["src"][0], ref["src"][0, ::-1].copy()])).to(DEV)  # (2, 3, H, W)
    got = s.down(both).cpu().numpy()
    np.testing.assert_array_equal(U.f32_bits(got[0]), U.f32_bits(ref["down"][0]))
    np.testing.assert_array_equal(U.f32_bits(got[1]), U.f32_bits(ref["down"][0, ::-1]))
    np.testing.assert_array_equal(U.f32_bits(s.down(both[0]).cpu().numpy()), U.f32_bits(ref["down"][0]))  # (3, H, W) too


def test_wrong_inputs_are_value_errors():
    s = SC.Scale((40, 52), "1/2", DEV)
    good = torch.zeros((1, 3, 40, 52), device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        s.down(good.cpu())
    with pytest.raises(ValueError, match="float32"):
        s.down(good.double())
    with pytest.raises(ValueError, match="float32"):
        s.down(torch.zeros((1, 4, 40, 52), device=DEV))
    with pytest.raises(ValueError, match=r"expected a \(..., 3, 40, 52\)"):
        s.down(torch.zeros((1, 3, 20, 26), device=DEV))
    with pytest.raises(ValueError, match=r"expected a \(..., 3, 20, 26\)"):
        s.up(good)
    with pytest.raises(ValueError, match="out="):
        s.down(good, out=torch.zeros((1, 3, 20, 27), device=DEV))
    with pytest.raises(ValueError, match="out="):
        s.down(good, out=torch.zeros((1, 3, 26, 20), device=DEV).transpose(2, 3))


# ------------------------------------------------------------------------------------ the two layers, without the codec
@pytest.mark.parametrize("case,worst", [(((128, 192), (1, 2)), 23), (((96, 160), (2, 3)), 14), (((75, 107), (3, 4)), 11)],
                         ids=["128x192at1of2", "96x160at2of3", "75x107at3of4"])
def test_down_up_residual_fuse_returns_the_source_inside_the_boxes(case, worst):
    """A base layer at reduced size plus the residual inside the boxes is the source there, at EVERY pixel -- which holds
    only while |code(src) - code(up)| <= 127 (the residual's range): the figure is asserted, so a clipped residual cannot
    hide a scaler that is merely close."""
    ((h, w), (n, d)) = case
    fr = synthetic.frames(3, 2, h, w)
    s = SC.Scale((h, w), (n, d), DEV)
    boxes = np.array([[3, 2, w // 2 + 1, h // 2, 0], [w // 3, h // 3, w - 1, h, 0], [0, h - 9, 7, h, 0]], np.int32)
    mask = XR.binary_mask(boxes, h, w)
    assert mask.any() and not mask.all()
    largest = 0
    for t in range(2):
        src = torch.from_numpy(fr[t:t + 1]).to(DEV)
        up = s.up(s.down(src))
        np.testing.assert_array_equal(U.f32_bits(up.cpu().numpy()), U.f32_bits(R.up(R.down(fr[t:t + 1], n, d), (h, w))))
        diff = np.abs(R.code(fr[t]) - R.code(up.cpu().numpy()[0]))
        largest = max(largest, int(diff.max()))
        res = X.residual_layer(src, up, boxes)
        fused = X.fuse(up, res, boxes, (X.RoiClass(0),)).cpu().numpy()[0]
        assert np.array_equal(R.code(fused)[:, mask], R.code(fr[t])[:, mask])
        assert np.array_equal(R.code(fused)[:, ~mask], R.code(up.cpu().numpy()[0])[:, ~mask])
        assert (R.code(fused)[:, ~mask] != R.code(fr[t])[:, ~mask]).any()  # (the base layer alone is not the source)
    print(f"{case}: largest |code(src) - code(up)| = {largest}")
    assert largest == worst <= 127


# ------------------------------------------------------------------------------------------------------- end to end
GOP, N = 8, 16


E2E = {"128at1of2": ((128, 128), (1, 2)), "96at2of3": ((96, 96), (2, 3))}


def _hwc(a):
    """the (H, W, 3) uint8 picture save_torch_image writes of a (3, H, W) float picture"""
    return R.code(a).transpose(1, 2, 0).astype(np.uint8)


@pytest.fixture(scope="module", params=sorted(E2E))
def e2e(request, tmp_path_factory, file_nets):
    """One clip per full size, as PNGs.  `direct`: the down() pictures coded through the API that exists without the option
    (an _EncodeRun fed by a generator), with every base reconstruction kept; `want`: those scaled up by the restatement --
    the reference all tests share.  `scaled`: the encode with base_scale, one stream, everything switched on."""
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd.pipeline import pad_frame
    from vcm_ts_amd.scenecut import GopPlan

    (h, w), ratio = E2E[request.param]
    tmp = tmp_path_factory.mktemp("scale_" + request.param)
    clip = np.rint(synthetic.frames(5, N, h, w).transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)
    U.write_pngs(tmp / "png", clip)
    s = SC.Scale((h, w), ratio, DEV)
    hb, wb = s.base
    assert (hb, wb) == (64, 64)
    run = RC._EncodeRun(str(tmp / "direct"), GopPlan.fixed(N, GOP), (hb, wb), GOP, DEV, None, None, None, "host", file_nets, 1, None)
    kept = {}

    def frames(k):
        for g in run.order(k):
            yield pad_frame(s.down(RC.u8_to_unit_float(torch.from_numpy(clip[g]).to(DEV))))

    run.encode(frames, (1.0, 1.0, 1.0), lambda k, g, ref: kept.__setitem__(g, ref[0, :, :hb, :wb].cpu().numpy().copy()))
    direct_bits, _ = run.results(None)
    want = [R.up(kept[g][None], (h, w))[0] for g in range(N)]
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "scaled"), str(tmp / "scaled_rec"), gop=GOP, nets=file_nets,
                                  picture_hash=True, base_scale=ratio)
    return dict(tmp=tmp, h=h, w=w, ratio=ratio, clip=clip, base=kept, want=want, direct_bits=direct_bits, bits=bits, size=size,
                scale=s)


def test_bins_are_those_of_the_down_scaled_pictures_and_recon_is_the_up_scaled_one(e2e, file_nets):
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    assert U.bins(tmp / "scaled") == U.bins(tmp / "direct") and len(U.bins(tmp / "direct")) == N
    assert U.others(tmp / "direct") == [] and U.others(tmp / "scaled") == ["hashes.json", "scale.json"]
    assert e2e["size"] == (h, w) and e2e["bits"] == e2e["direct_bits"]
    info = json.loads((tmp / "scaled" / "scale.json").read_text())
    assert info == _HostScale((h, w), e2e["ratio"]).to_json() and info["base"] == [64, 64] and info["full"] == [h, w]
    for t in range(N):
        assert np.array_equal(U.png(tmp / "scaled_rec" / f"im{t + 1:05d}.png"), _hwc(e2e["want"][t])), t
    # two GOP streams: the same bytes and the same records
    RC.encode_folder(str(tmp / "png"), str(tmp / "two"), gop=GOP, nets=file_nets, gop_streams=2, picture_hash=True, base_scale=e2e["ratio"])
    assert U.bins(tmp / "two") == U.bins(tmp / "direct")
    for name in ("hashes.json", "scale.json"):
        assert (tmp / "two" / name).read_text() == (tmp / "scaled" / name).read_text()


def test_report_speaks_of_the_full_size(tmp_path, file_nets):
    """At 192x192 coded at 1/2 (a 96x96 base layer, padded to 128x128), 4 pictures: --report measures MS-SSIM, which refuses
    sides of 160 or less, so the report cannot be asked for at the 128x128 and 96x96 full sizes of the other tests.  What is
    asserted is the same: every bpp key divides by the FULL-size pixels, PSNR and the ROI figures compare the full-size
    source with the up-scaled picture (the restatement applied to the base reconstructions the encoder held)."""
    import math

    from tests import test_gpu_roi as G
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import stream as S

    h = w = 192
    n, gop = 4, 4
    clip = np.rint(synthetic.frames(7, n, h, w).transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)
    U.write_pngs(tmp_path / "png", clip)
    roi = X.Roi(G._e2e_boxes(h, w), tuple(X.RoiClass(b) for b in G.E2E_BORDERS), ("liplates", "faces"))
    seen, shown = {}, RC._BaseLayer.shown

    def spy(self, k, g, ref_frame):
        seen[g] = ref_frame[0, :, :96, :96].cpu().numpy().copy()
        return shown(self, k, g, ref_frame)

    from vcm_ts_amd import ratectl

    budgets, target_bits_of = [], ratectl.target_bits_of
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(RC._BaseLayer, "shown", spy)
        mp.setattr(ratectl, "target_bits_of", lambda bpp, hh, ww: budgets.append((bpp, hh, ww)) or target_bits_of(bpp, hh, ww))
        bits, size, rd = RC.encode_folder(str(tmp_path / "png"), str(tmp_path / "bins"), gop=gop, nets=file_nets, roi=roi, report=True,
                                          residual_bins=str(tmp_path / "bins"), target_bpp=2.0, base_scale="1/2")
    assert size == (h, w) and S.decode_i(str(tmp_path / "bins" / "im00001.bin"))[:2] == (96, 96)
    assert rd["frame_pixel_num"] == h * w
    assert rd["frame_bpp"] == [b / (h * w) for b in bits]
    assert rd["ave_all_frame_bpp"] == pytest.approx(sum(bits) / n / (h * w), rel=1e-12)
    assert rd["frame_bpp_enh"] == [b / (h * w) for b in rd["frame_bits_enh"]] and min(rd["frame_bits_enh"]) > 64
    assert rd["ave_all_frame_bpp_total"] == pytest.approx(rd["ave_all_frame_bpp"] + sum(rd["frame_bits_enh"]) / n / (h * w), rel=1e-12)
    # --target-bpp counts full-size pixels: 2.0 * 192 * 192 bits per picture
    assert budgets == [(2.0, h, w)] and len(rd["frame_bits_target"]) == n and rd["frame_bits_target"][3] is not None
    for t in range(n):
        src, up = XR.T[clip[t].transpose(2, 0, 1)], R.up(seen[t][None], (h, w))[0]
        sse = float(((up.astype(np.float64) - src.astype(np.float64)) ** 2).sum())
        assert rd["frame_psnr"][t] == pytest.approx(10.0 * math.log10(3 * h * w / sse), abs=1e-3), t
        assert np.isfinite(rd["frame_msssim"][t])
        sums = XR.sse(up, src, roi.boxes(t).array, G.E2E_BORDERS)
        assert rd["frame_roi_pixels"][t] == sums[2] > 0
        assert rd["frame_psnr_roi"][t] == pytest.approx(XR.psnr(sums, h, w, "samples")[2], rel=1e-12)
        assert rd["frame_psnr_bg"][t] == pytest.approx(XR.psnr(sums, h, w, "samples")[1], rel=1e-12)


def test_decode_follows_scale_json_and_base_only_ignores_it(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    assert RC.decode_folder(str(tmp / "scaled"), str(tmp / "dec"), h, w, gop=GOP, verify="strict") == N
    for t in range(N):
        name = f"im{t + 1:05d}.png"
        assert (tmp / "dec" / name).read_bytes() == (tmp / "scaled_rec" / name).read_bytes(), t
        assert np.array_equal(U.png(tmp / "dec" / name), _hwc(e2e["want"][t])), t
    # run_codec verify checks the folder decode --recon writes
    assert PH.verify_pngs(str(tmp / "scaled"), str(tmp / "dec")) is None
    RC.main(["verify", "--bins", str(tmp / "scaled"), "--recon", str(tmp / "dec")])
    # --base-only: today's decode of those bins (state is still checked, pixels is not)
    assert RC.decode_folder(str(tmp / "direct"), str(tmp / "direct_dec"), 64, 64, gop=GOP) == N
    assert RC.decode_folder(str(tmp / "scaled"), str(tmp / "base_only"), h, w, gop=GOP, base_scale=None, verify="strict") == N
    for t in range(N):
        name = f"im{t + 1:05d}.png"
        assert (tmp / "base_only" / name).read_bytes() == (tmp / "direct_dec" / name).read_bytes(), t
        assert np.array_equal(U.png(tmp / "base_only" / name), _hwc(e2e["base"][t])), t
    RC.main(["decode", "--bins", str(tmp / "scaled"), "--recon", str(tmp / "cli_base"), "--height", str(h), "--width", str(w),
             "--gop", str(GOP), "--base-only"])
    assert U.png(tmp / "cli_base" / "im00003.png").shape == (64, 64, 3)
    # a drifting scaler is caught: 8 units of 16384 moved from one tap of the decoder's up table to the next (rows still sum)
    with pytest.MonkeyPatch.context() as mp:
        real = SC._tables

        def drifted(full, base):
            tables = real(full, base)
            start, k = tables["up_x"]
            k = k.copy()
            k[:, 0] += 8
            k[:, 1] -= 8
            return dict(tables, up_x=(start, k))

        mp.setattr(SC, "parse_scale", lambda info, where=None: {"full": (h, w), "base": (64, 64), "ratio": SC.as_ratio(tuple(info["ratio"]))})
        mp.setattr(SC, "_tables", drifted)
        with pytest.raises(PH.PictureHashMismatch) as ex:
            RC.decode_folder(str(tmp / "scaled"), str(tmp / "drift"), h, w, gop=GOP)
        assert ex.value.which == "pixels" and ex.value.picture < GOP


def test_a_scale_json_that_does_not_fit_is_refused_before_any_launch(e2e):
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    other = (2, 3) if e2e["ratio"] == (1, 2) else (1, 2)

    def folder(name, info):
        dst = tmp / name
        os.makedirs(dst)
        for n, data in U.bins(tmp / "scaled").items():
            (dst / n).write_bytes(data)
        (dst / "hashes.json").write_text((tmp / "scaled" / "hashes.json").read_text())
        (dst / "scale.json").write_text(json.dumps(info))
        return dst

    good = json.loads((tmp / "scaled" / "scale.json").read_text())
    d = good["tables"]["down_y"]
    cases = [(folder("ratio", _HostScale((h, w), other).to_json()), (h, w), "the .bin files hold 64x64"),
             (folder("edited", dict(good, ratio=list(other))), (h, w), "gives a base of"),
             (folder("digest", dict(good, tables=dict(good["tables"], down_y=("0" if d[0] != "0" else "1") + d[1:]))), (h, w),
              "down_y table built on this host"),
             (tmp / "scaled", (h, w + 2), f"a base layer of {w}x{h} pictures, decoding {w + 2}x{h}")]
    with pytest.MonkeyPatch.context() as mp:
        def launched(*a, **k):
            raise AssertionError("a launch")

        mp.setattr(SC, "scale_planes", launched)
        mp.setattr(RC, "_nets", launched)
        mp.setattr(PH, "_launch", launched)
        for path, (hh, ww), match in cases:
            with pytest.raises(ValueError, match=match):
                RC.decode_folder(str(path), str(tmp / "never"), hh, ww, gop=GOP, verify="off")
        with pytest.raises(ValueError, match="base_scale: expected"):
            RC.decode_folder(str(tmp / "scaled"), str(tmp / "never"), h, w, gop=GOP, base_scale="1/2")
    assert not (tmp / "never").exists()


def test_residual_bins_at_step_one_return_the_source_in_the_boxes(e2e, file_nets):
    from tests import test_gpu_roi as G
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    roi = X.Roi(G._e2e_boxes(h, w), tuple(X.RoiClass(b) for b in G.E2E_BORDERS), ("liplates", "faces"))
    bits, size = RC.encode_folder(str(tmp / "png"), str(tmp / "roi"), gop=GOP, nets=file_nets, gop_streams=2, roi=roi,
                                  residuals=str(tmp / "res.gbrp"), residual_bins=str(tmp / "roi"), base_scale=e2e["ratio"])
    assert U.bins(tmp / "roi") == U.bins(tmp / "direct") and size == (h, w)
    raw = np.frombuffer((tmp / "res.gbrp").read_bytes(), np.uint8).reshape(N, 3, h, w)
    assert RC.decode_folder(str(tmp / "roi"), str(tmp / "fused"), h, w, gop=GOP, roi=roi, residual_bins=str(tmp / "roi")) == N
    changed = 0
    for t in range(N):
        src, up, boxes = XR.T[e2e["clip"][t].transpose(2, 0, 1)], e2e["want"][t], roi.boxes(t).array
        res = XR.residual(src, up, boxes)  # (against the up-scaled picture, boxes in full-size coordinates)
        assert np.array_equal(raw[t][[2, 0, 1]], res), t
        got = U.png(tmp / "fused" / f"im{t + 1:05d}.png")
        assert np.array_equal(got, _hwc(XR.fuse(up, res, boxes, G.E2E_BORDERS))), t
        changed += int((got != _hwc(up)).sum())
        # (the name-seeded weights of the suite reconstruct poorly: |code(src) - code(up)| reaches 254 here, the residual
        # clips, and the source does not come back exactly as it does in the two-layer test above)
    assert changed > 1000  # the enhancement layer did something
    with pytest.raises(ValueError, match="base-only decode"):
        RC.decode_folder(str(tmp / "roi"), str(tmp / "never"), h, w, gop=GOP, roi=roi, residual_bins=str(tmp / "roi"), base_scale=None)


def test_y4m_round_trip(e2e, file_nets):
    from tests import yuv_ref as YR
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    planes = [tuple(p.astype(np.uint8) for p in YR.from_rgb(a.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0), dtype=np.float64))
              for a in e2e["clip"]]
    YR.write_y4m(str(tmp / "src.y4m"), planes, w, h, fps="30:1")
    seen, shown = {}, RC._BaseLayer.shown

    def spy(self, k, g, ref_frame):
        seen[g] = ref_frame[0, :, :64, :64].cpu().numpy().copy()
        return shown(self, k, g, ref_frame)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(RC._BaseLayer, "shown", spy)
        bits, size = RC.encode_video(str(tmp / "src.y4m"), str(tmp / "v"), str(tmp / "v_enc.y4m"), gop=GOP, nets=file_nets, gop_streams=2,
                                     picture_hash=True, base_scale=e2e["ratio"])
    assert size == (h, w) and sorted(seen) == list(range(N))
    assert U.others(tmp / "v") == ["hashes.json", "scale.json", "sequence.json"]
    info = json.loads((tmp / "v" / "sequence.json").read_text())
    assert (info["height"], info["width"]) == (h, w)
    assert RC.decode_video(str(tmp / "v"), str(tmp / "v_dec.y4m"), verify="strict") == N
    assert (tmp / "v_dec.y4m").read_bytes() == (tmp / "v_enc.y4m").read_bytes()
    assert RC.decode_folder(str(tmp / "v"), str(tmp / "v_png"), h, w, gop=GOP) == N
    for t in range(N):
        assert np.array_equal(U.png(tmp / "v_png" / f"im{t + 1:05d}.png"), _hwc(R.up(seen[t][None], (h, w))[0])), t
    assert RC.decode_video(str(tmp / "v"), str(tmp / "v_base.y4m"), base_scale=None) == N
    assert os.path.getsize(tmp / "v_base.y4m") < os.path.getsize(tmp / "v_dec.y4m") * (64 * 64) / (h * w) + 4096


def test_refused_combinations_and_the_option_left_out(e2e, file_nets):
    from tests import test_gpu_roi as G
    from vcm_ts_amd import run_codec as RC

    tmp, h, w = e2e["tmp"], e2e["h"], e2e["w"]
    roi = X.Roi(G._e2e_boxes(h, w), tuple(X.RoiClass(b) for b in G.E2E_BORDERS))
    kw = dict(gop=GOP, nets=file_nets, base_scale=e2e["ratio"])
    with pytest.raises(NotImplementedError, match="roi_q="):
        RC.encode_folder(str(tmp / "png"), str(tmp / "no"), roi=roi, roi_q=X.RoiQ(100, (60, 60)), **kw)
    with pytest.raises(NotImplementedError, match="bit_map= and roi="):
        RC.encode_folder(str(tmp / "png"), str(tmp / "no"), roi=roi, bit_map=True, report=True, **kw)  # (before any metric)
    with pytest.raises(NotImplementedError, match="bit_map= and roi="):
        RC.encode_folder(str(tmp / "png"), str(tmp / "no"), roi=roi, bit_map=str(tmp / "maps"), **kw)
    with pytest.raises(ValueError, match="1/4 <= n/d < 1"):
        RC.encode_folder(str(tmp / "png"), str(tmp / "no"), gop=GOP, nets=file_nets, base_scale="1/8")
    assert not (tmp / "no").exists()
    # bit_map without roi is unchanged: the cells of the base grid
    RC.encode_folder(str(tmp / "png"), str(tmp / "maps_bins"), bit_map=str(tmp / "maps"), **kw)
    assert np.load(tmp / "maps" / "im00001.npy").shape == (1, 4, 4) and U.bins(tmp / "maps_bins") == U.bins(tmp / "direct")
    # without the option: no launch, no file (a stale one is removed), and the bytes are those of the layers below the file
    # loops, which the option does not reach (pipeline.ConcurrentGopEncoder and the stream.py containers, fed by hand)
    stale = tmp / "stale"
    os.makedirs(stale)
    (stale / "scale.json").write_text((tmp / "scaled" / "scale.json").read_text())
    launches = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(SC, "scale_planes", lambda *a, **k: launches.append(a))
        RC.encode_folder(str(tmp / "scaled_rec"), str(stale), gop=GOP, nets=file_nets)
        RC.encode_folder(str(tmp / "scaled_rec"), str(tmp / "plain"), gop=GOP, nets=file_nets)
        assert RC.decode_folder(str(stale), str(tmp / "stale_dec"), h, w, gop=GOP) == N
    assert launches == [] and U.others(stale) == [] and U.others(tmp / "plain") == [] and U.bins(stale) == U.bins(tmp / "plain")
    from vcm_ts_amd import stream as S
    from vcm_ts_amd.pipeline import ConcurrentGopEncoder, pad_frame

    os.makedirs(tmp / "by_hand")

    def sink(kind, qidx, payload, t):
        path = str(tmp / "by_hand" / f"im{t + 1:05d}.bin")
        if kind == "I":
            S.encode_i(h, w, qidx[0], payload, path)
        else:
            S.encode_p(payload, qidx[0], qidx[1], path)

    pictures = (pad_frame(RC.u8_to_unit_float(torch.from_numpy(U.png(tmp / "scaled_rec" / f"im{t + 1:05d}.png").copy()).to(DEV)))
                for t in range(N))
    with torch.no_grad():
        ConcurrentGopEncoder(lambda: file_nets[0], gop_size=GOP, streams=1).encode_gops([pictures], 1.0, 1.0, 1.0, sinks=[sink])
    assert U.bins(tmp / "by_hand") == U.bins(tmp / "plain") and len(U.bins(tmp / "plain")) == N
