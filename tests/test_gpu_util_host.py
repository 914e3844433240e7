"""tests/gpu_util.py on CPU tensors: a strided view, a guard or a byte comparison that is subtly wrong is a GPU test that
cannot fail, so the scaffolding is held against what it says it builds."""
import numpy as np
import pytest
import torch

from tests import gpu_util as U

CPU = torch.device("cpu")


@pytest.mark.parametrize("with_picture", [False, True])
def test_strided_is_the_view_it_describes(with_picture):
    H, W, row_pad, plane_pad, offset = 3, 5, 3, 7, 5
    pic = np.arange(3 * H * W, dtype=np.float32).reshape(3, H, W) if with_picture else None
    buf, view, rs, ps, mask = U.strided(pic, H, W, row_pad, plane_pad, offset, CPU)
    assert (rs, ps) == (W + row_pad, H * (W + row_pad) + plane_pad) == (8, 31)
    assert view.shape == (3, H, W) and view.stride() == (ps, rs, 1) and view.storage_offset() == offset
    assert view.data_ptr() == buf.data_ptr() + 4 * offset and buf.dtype == torch.float32
    assert buf.numel() == offset + 3 * ps + U.GUARD and mask.shape == (buf.numel(),) and mask.dtype == bool
    # the mask marks exactly the view's words: writing through the view changes those and no others
    assert int(mask.sum()) == 3 * H * W and not mask[:offset].any() and not mask[offset + 2 * ps + (H - 1) * rs + W:].any()
    before = buf.numpy().copy()
    if with_picture:
        assert np.array_equal(view.numpy(), pic) and np.array_equal(before[mask], pic.reshape(-1))
    else:
        assert np.isnan(before).all()
    assert np.isnan(before[~mask]).all()
    view.fill_(-1.0)
    after = buf.numpy()
    assert (after[mask] == -1.0).all() and np.isnan(after[~mask]).all()
    assert U.strided(None, H, W, row_pad, plane_pad, offset, CPU, guard=3)[0].numel() == offset + 3 * ps + 3


@pytest.mark.parametrize("dtype,sentinel", [(np.uint16, 0xABCD), (np.uint32, 0xABCD1234)], ids=["uint16", "uint32"])
@pytest.mark.parametrize("shift", [0, 3])
def test_guards_see_one_word_on_either_side(dtype, sentinel, shift):
    n = 10
    buf, first = U.guarded(n, shift, dtype, sentinel, CPU)
    assert first == U.GUARD + shift and buf.numel() == 2 * U.GUARD + shift + n
    assert buf.dtype == {np.uint16: torch.int16, np.uint32: torch.int32}[dtype]
    assert (U.words(buf) == sentinel).all() and U.guards_intact(buf, first, n, sentinel)  # fresh
    buf[first:first + n] = 0
    assert U.guards_intact(buf, first, n, sentinel) and (U.words(buf)[first:first + n] == 0).all()  # all n words written
    for at in (first - 1, first + n, 0, buf.numel() - 1):
        hit = buf.clone()
        hit[at] += 1
        assert not U.guards_intact(hit, first, n, sentinel), at
    for at in (first, first + n - 1):  # (the inside words are the caller's)
        hit = buf.clone()
        hit[at] += 1
        assert U.guards_intact(hit, first, n, sentinel), at


def test_folder_helpers_and_the_png_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    pics = rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    U.write_pngs(tmp_path / "a", pics)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["im00001.png", "im00002.png"]
    for t in range(2):
        assert np.array_equal(U.png(tmp_path / "a" / f"im{t + 1:05d}.png"), pics[t])
        planar = U.png(tmp_path / "a" / f"im{t + 1:05d}.png", planar=True)
        assert planar.shape == (3, 8, 8) and np.array_equal(planar, pics[t].transpose(2, 0, 1))
    # float (3, H, W) pictures of exact 8-bit samples are the same files; anything else is refused
    exact = pics.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    U.write_pngs(tmp_path / "b", exact)
    U.same_pngs(tmp_path / "a", tmp_path / "b", 2)
    with pytest.raises(AssertionError):
        U.write_pngs(tmp_path / "c", exact + np.float32(1e-4))
    with pytest.raises(FileExistsError):
        U.write_pngs(tmp_path / "a", pics)
    # same_pngs: one byte
    data = bytearray((tmp_path / "b" / "im00002.png").read_bytes())
    data[-1] ^= 1
    (tmp_path / "b" / "im00002.png").write_bytes(bytes(data))
    U.same_pngs(tmp_path / "a", tmp_path / "b", 1)
    with pytest.raises(AssertionError):
        U.same_pngs(tmp_path / "a", tmp_path / "b", 2)
    # bins / others
    (tmp_path / "a" / "im00002.bin").write_bytes(b"two")
    (tmp_path / "a" / "im00001.bin").write_bytes(b"")
    (tmp_path / "a" / "sequence.json").write_text("{}")
    assert U.bins(tmp_path / "a") == {"im00001.bin": b"", "im00002.bin": b"two"}
    assert list(U.bins(tmp_path / "a")) == ["im00001.bin", "im00002.bin"]
    assert U.others(tmp_path / "a") == ["im00001.png", "im00002.png", "sequence.json"]


def test_f32_bits_and_the_small_ones():
    a = np.array([[0.0, -0.0, 1.0], [np.nan, np.inf, 0.1]], dtype=np.float32)
    got = U.f32_bits(a)
    assert got.dtype == np.uint32 and got.shape == a.shape and np.array_equal(got, U.f32_bits(torch.from_numpy(a)))
    assert got[0, 0] == 0 and got[0, 1] == 0x80000000 and got[0, 2] == 0x3F800000
    assert np.array_equal(U.f32_bits(torch.from_numpy(a).t()), got.T)  # (a view that is not contiguous)
    t = U.to_dev(a[:, ::2], CPU)
    assert t.is_contiguous() and np.array_equal(U.f32_bits(t), got[:, ::2])
    assert U.intra_dpb(t) == {"ref_frame": t, "ref_feature": None, "ref_y": None, "ref_mv_y": None}


def test_picture_in_a_crop_is_the_picture_with_foreign_values_around_it():
    a = np.random.default_rng(2).random((3, 5, 7), dtype=np.float32)
    whole, crop = U.picture(a, False, CPU), U.picture(a, True, CPU)
    assert whole.shape == crop.shape == (1, 3, 5, 7) and whole.is_contiguous() and not crop.is_contiguous()
    assert np.array_equal(whole.numpy()[0], a) and np.array_equal(crop.numpy()[0], a)
    assert crop.stride() == (3 * 64 * 192, 64 * 192, 192, 1) and crop.storage_offset() == 192 + 1
    crop.fill_(0.77)
    assert bool((crop._base == 0.77).all())  # everything around the view was 0.77
