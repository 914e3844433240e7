"""Reconstruction PNGs made on the device at 1920x1080 (the record in profiles/pngdev_1080p.txt).

    python3 tools/pngdev_time.py kernels [launches=50] [rounds=5]   dcvc_png_encode (both launches) on the 1080x1920 crop of a
                                                                    padded picture, alternated in one process with
                                                                    dcvc_hash_pixels on the same pictures -- that kernel reads
                                                                    the same 24.9 MB and forms the same codes, so it is the
                                                                    yardstick -- on one picture (cache-resident) and rotating
                                                                    over 16 (HBM); then the files' sizes against PIL's default
                                                                    for the same pixels
    python3 tools/pngdev_time.py files [n_frames=34] [repeats=3] [io_workers=8]
                                                                    encode_folder and decode_folder frames/s into a PNG folder
                                                                    with and without png_device=, alternating in one process

The file setting: synthetic.frames as a PNG folder, GOP 32, two GOP streams, fp16x3, one pair of codecs per stream shared by
every run, a warm-up pass of both variants first.  The pixels of the two folders must agree (checked, picture for picture,
through PIL), and the .bin totals too.  The yardstick is the run without the option in the same process; set the difference
beside the spread of the repeats.  Frames/s from a host clock around work that ends with the last file written.
"""
import io
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import picturehash as PH  # noqa: E402
from vcm_ts_amd import pngdev as P  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
GOP, STREAMS, POOL = 32, 2, 16
DEV = torch.device("cuda:0")


def _pil_size(u8):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(u8).save(b, format="PNG")
    return len(b.getvalue())


def kernels(launches, rounds):
    from PIL import Image

    from vcm_ts_amd.synthetic import frames

    ground = torch.from_numpy(frames(0, 1, H, W, noise=0)).to(DEV)
    pool = timing.noisy_pool(ground, (H, W), POOL)
    dev = P.PngDevice((H, W), DEV)
    out, scratch = torch.zeros(1, dtype=torch.uint32, device=DEV), PH.new_scratch(DEV)
    buf, staging = dev.files[0], dev.staging[0]

    def png(x):
        P.devargs.launch("dcvc_png_encode", DEV, x.data_ptr(), WP, HP * WP, H, W, dev.rows, dev.words.ctypes.data, dev.tables.data_ptr(),
                         dev.words.shape[0], staging.data_ptr(), buf.data_ptr() + 16, P.C.c_int64(dev.capacity), buf.data_ptr())

    variants = {}
    for where, pick in ((", one picture (cache-resident)", lambda i: pool[0:1]), (f", rotating over {POOL} pictures (HBM)", lambda i: pool[i % POOL:i % POOL + 1])):
        variants["png_encode" + where] = lambda i, pick=pick: png(pick(i))
        variants["hash_pixels" + where] = lambda i, pick=pick: PH.crc32_pixels(pick(i), (H, W), out=out, scratch=scratch)
    print(f"# {H}x{W} crops of padded {HP}x{WP} pictures, {launches} calls each in {rounds} alternating rounds; a call is two launches; "
          f"bands of {dev.rows} rows ({-(-H // dev.rows)} workgroups), {dev.words.shape[0]} presets; us per call: median (min .. max), "
          f"and the 24.9 MB of fp32 a call reads at the median")
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    med = timing.kernel_table(times, lambda name: 12 * H * W, 52)
    for where in ("cache-resident", "HBM"):
        a, b = (next(v for k, v in med.items() if k.startswith(n) and where in k) for n in ("png_encode", "hash_pixels"))
        print(f"# png_encode / hash_pixels = x{a / b:.2f} ({where})")
    # the files: what PIL reads back, and their sizes against PIL's default (zlib level 6) for the same pixels
    print("# file sizes: bytes on the device, bytes with PIL's default, their ratio")
    pictures = {"synthetic.frames, noise-free": ground, "synthetic.frames under +-4 codes of uniform noise": pool[1:2, :, :H, :W],
                "synthetic.frames under Gaussian noise, sigma 1.5 codes": ground + 1.5 / 255 * torch.randn(ground.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1)),
                "flat 77": torch.full((1, 3, H, W), 77 / 255, device=DEV)}
    for name, x in pictures.items():
        full = torch.zeros((1, 3, HP, WP), device=DEV)
        full[..., :H, :W] = x
        h = dev.put(0, full)
        data = bytes(h.data())
        h.release()
        u8 = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        want = torch.round(255.0 * full[0, :, :H, :W].clamp(0, 1)).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(u8, want), name  # (PIL is the judge)
        pil = _pil_size(u8)
        print(f"  {name:56s} {len(data):9d} {pil:9d}   x{len(data) / pil:.2f}")


def _folder_bytes(folder):
    return sum(os.path.getsize(os.path.join(folder, n)) for n in os.listdir(folder) if n.endswith(".png"))


def files(n, repeats, io_workers):
    from PIL import Image

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd.synthetic import frames

    with timing.workdir("dcvc_pngdev_time_") as tmp:
        src = os.path.join(tmp, "src")
        os.makedirs(src)
        for t, a in enumerate(frames(0, n, H, W)):
            Image.fromarray(np.rint(a.transpose(1, 2, 0) * 255).astype(np.uint8)).save(os.path.join(src, f"im{t + 1:05d}.png"), compress_level=1)
        nets = timing.codec_pairs(DEV, "fp16x3", STREAMS)
        bins, totals, sizes = os.path.join(tmp, "bins"), set(), {}

        def encode(on_device, max_frames=None):
            out = os.path.join(tmp, "rec_dev" if on_device else "rec_host")
            shutil.rmtree(out, ignore_errors=True)
            rate = timing.fps(lambda: totals.add(sum(RC.encode_folder(src, bins, out, max_frames=max_frames, gop=GOP, gop_streams=STREAMS,
                                                                      nets=nets, io_workers=io_workers, png_device=on_device)[0])), n, DEV)
            if max_frames is None:
                assert len(totals) == 1, totals  # the option changes no .bin byte
                sizes[on_device] = _folder_bytes(out)
            return rate

        def decode(on_device):
            out = os.path.join(tmp, "dec_dev" if on_device else "dec_host")
            shutil.rmtree(out, ignore_errors=True)
            with timing.shared_nets(nets[0]):
                return timing.fps(lambda: RC.decode_folder(bins, out, H, W, gop=GOP, precision="fp16x3", io_workers=io_workers,
                                                           png_device=on_device), n, DEV)

        variants = {"without png_device": False, "png_device=True": True}
        for v in variants.values():  # warm-up: both code paths once
            encode(v, max_frames=min(n, GOP + 2))
        totals.clear()
        enc = timing.alternating(variants, repeats, encode)
        dec = timing.alternating(variants, repeats, decode)
        for t in range(n):  # the same pixels, picture for picture, from all four folders
            name = f"im{t + 1:05d}.png"
            a = np.asarray(Image.open(os.path.join(tmp, "rec_host", name)))
            for other in ("rec_dev", "dec_host", "dec_dev"):
                assert np.array_equal(a, np.asarray(Image.open(os.path.join(tmp, other, name)).convert("RGB"))), (other, t)
        print(f"# {n} pictures {W}x{H} from a PNG folder, GOP {GOP}, {STREAMS} GOP streams, fp16x3, io_workers {io_workers}; .bin total of "
              f"every run {totals.pop()} bits; the four folders hold the same pixels")
        print(f"# folder sizes: {sizes[True]} bytes from the device, {sizes[False]} from PIL: x{sizes[True] / sizes[False]:.2f}")
        print(f"# encode_folder into a PNG folder, frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(enc, baseline="without", width=24)
        print(f"# decode_folder into a PNG folder, frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(dec, baseline="without", width=24)


if __name__ == "__main__":
    timing.main(__doc__, "pngdev_time.py", {"kernels": (kernels, (50, 5)), "files": (files, (34, 3, 8))}, default="kernels")
