"""Files to files at 1080p: run_codec.encode_folder on a PNG folder beside run_codec.encode_video on a Y4M file of the
same pictures (the record in profiles/yuv_io_1080p.txt).

    python3 tools/yuv_io_time.py files [n_frames=64] [repeats=3]     frames/s of both paths, alternating
    python3 tools/yuv_io_time.py kernels [launches=20] [plain|full]  the two colour kernels alone at 1088x1920, for
                                                                     `rocprofv3 --kernel-trace --stats -- python3 ...`

`files`: synthetic.frames content -> 4:2:0 samples (the tested rgb_to_yuv420 kernel) -> a Y4M file; the pictures
encode_video(quantize8=True) makes of it, as 8-bit RGB PNGs, are the folder, so both paths code identical inputs and
their .bin totals must agree (checked).  GOP 32, two GOP streams, fp16x3, one pair of codecs per stream built once and
shared by every run; a warm-up pass of every variant first; then the variants alternate, `repeats` times each.
Frames/s from a host clock around work that ends in a device synchronise.
"""
import os
import shutil
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import run_codec as RC  # noqa: E402
from vcm_ts_amd import yuv as Y  # noqa: E402

H, W = timing.SIZE
GOP, STREAMS = 32, 2
DEV = torch.device("cuda:0")


def make_inputs(tmp, n):
    from PIL import Image

    spec, png = Y.ColorSpec(), os.path.join(tmp, "png")
    os.makedirs(png)
    y4m = timing.y4m_clip(tmp, n, (H, W))
    with Y.open_video(y4m, None, 8, None) as reader, ThreadPoolExecutor(8) as pool:
        samples, jobs = np.empty(reader.frame_bytes, np.uint8), []
        for t in range(n):  # the folder holds what encode_video(quantize8=True) makes of the file's samples
            reader.read_into(t, samples)
            x = Y.yuv420_to_rgb(torch.from_numpy(samples).to(DEV), H, W, spec, pad=False, quantize8=True)
            u8 = torch.round(x[0] * 255.0).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
            jobs.append(pool.submit(lambda a, p: Image.fromarray(a).save(p), u8, os.path.join(png, f"im{t + 1:05d}.png")))
        for j in jobs:
            j.result()
    return y4m, png


def files(n, repeats):
    with timing.workdir("dcvc_yuv_io_") as tmp:
        t0 = time.time()
        y4m, png = make_inputs(tmp, n)
        print(f"# inputs: {n} pictures {W}x{H}; src.y4m {os.path.getsize(y4m) / 1e6:.1f} MB, PNG folder "
              f"{sum(os.path.getsize(os.path.join(png, f)) for f in os.listdir(png)) / 1e6:.1f} MB ({time.time() - t0:.0f} s to make)")
        common = dict(gop=GOP, gop_streams=STREAMS, nets=timing.codec_pairs(DEV, "fp16x3", STREAMS))
        totals = set()

        def run(path, recon, workers, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            if path == "png":
                code = lambda: RC.encode_folder(png, os.path.join(out, "bin"), os.path.join(out, "rec") if recon else None,
                                                io_workers=workers, max_frames=max_frames, **common)
            else:
                code = lambda: RC.encode_video(y4m, os.path.join(out, "bin"), os.path.join(out, "rec.y4m") if recon else None,
                                               quantize8=True, io_workers=workers, max_frames=max_frames, **common)
            rate = timing.fps(lambda: totals.add(sum(code()[0])), n, DEV)
            assert max_frames is not None or len(totals) == 1, totals  # identical inputs, identical .bin totals
            return rate

        what = {"png": "encode_folder, PNG folder, 8 I/O threads", "y4m": "encode_video,  Y4M file,  no helper threads"}
        variants = {f"{what[p]:44s} {'+ reconstruction output' if r else '  bins only            '}": (p, r)
                    for r in (False, True) for p in ("png", "y4m")}
        for p, r in variants.values():  # warm-up: every shape and every code path once
            run(p, r, 8, max_frames=GOP + 2)
        totals.clear()
        rates = timing.alternating(variants, repeats, lambda v: run(v[0], v[1], 8))
        total = next(iter(totals))
        print(f"# .bin total of every run: {total} bits ({total / (n * H * W):.4f} bpp)")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, width=69)
        print("# io_workers=0 (reading, decoding and writing inline on the encoding thread), one run each")
        for p, r in variants.values():
            print(f"  {'encode_folder' if p == 'png' else 'encode_video '} io_workers=0 {'+ reconstruction output' if r else '  bins only            '}  "
                  f"{run(p, r, 0):6.2f}")


def kernels(launches, variant):
    """variant "plain": yuv420_to_rgb and rgb_to_yuv420 as the default path uses them; "full": with quantize8 and with
    the source planes and integer sums (the kernels keep their names, so each variant is traced in a run of its own)."""
    spec, full = Y.ColorSpec(), variant == "full"
    g = torch.Generator().manual_seed(1)
    src = torch.randint(16, 236, (H * W * 3 // 2,), generator=g, dtype=torch.uint8).to(DEV)
    for _ in range(launches):
        rgb = Y.yuv420_to_rgb(src, H, W, spec, quantize8=full)
    for _ in range(launches):
        Y.rgb_to_yuv420(rgb, H, W, spec, source=src if full else None)
    torch.cuda.synchronize(DEV)
    to_rgb = H * W * 3 // 2 + 3 * timing.padded((H, W))[0] * W * 4
    from_rgb = H * W * 3 // 2 + 3 * H * W * 4 + (H * W * 3 // 2 if full else 0)
    print(f"# variant {variant}: {launches} launches each; bytes per launch from the shapes: yuv420_to_rgb {to_rgb / 1e6:.2f} MB "
          f"(1.5 read + 12 written per pixel, 8 padding rows included), rgb_to_yuv420 {from_rgb / 1e6:.2f} MB")


if __name__ == "__main__":
    timing.main(__doc__, "yuv_io_time.py", {"files": (files, (64, 3)), "kernels": (kernels, (20, "plain"))}, default="files")
