"""The noise estimate at 1920x1080 (the record in profiles/noise_1080p.txt).

    python3 tools/noise_time.py kernels [launches=200] [rounds=5]
                                        dcvc_noise_cells beside dcvc_motion_step (the yardstick: the streaming kernel with the
                                        same tiling on the same three fp32 planes) on the same pictures, alternating in one
                                        process: on one set of pictures (cache-resident) and rotating over 16 sets (HBM); and
                                        dcvc_noise_hist over one picture's cell words and over 64 pictures', with the words
                                        spread out over the bins, as the noisy pictures above give them, and ALL IN ONE BIN (the
                                        contended case its LDS histogram exists for).  HIP events around `launches`
                                        back-to-back launches, `rounds` times each
    python3 tools/noise_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr T against --tnr-auto resolving to
                                        the same T (one more pass over the source, two more kernels a picture in it),
                                        alternating in one process

Bytes per launch come from the shapes: dcvc_noise_cells reads 12 bytes a pixel of picture and 1 of the previous luma and
writes 1; the yardstick reads 12 bytes a pixel of picture and reads and writes 2 of model.  dcvc_noise_hist reads 4 bytes a
word, and every workgroup zeroes and scans its 32 KB of LDS whatever it counts, so it is reported in words per microsecond.
Frames/s from a host clock around work that ends in a device synchronise.
"""
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
POOL = 16
BATCH = 64  # NoiseScan's default: the pictures whose cells one dcvc_noise_hist launch counts
BYTES = {"noise_cells": (12 + 1 + 1) * H * W, "motion_step": (12 + 4) * H * W}


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)
    cur = timing.noisy_pool(ground, (H, W), POOL)  # a static scene under +-4 codes of noise
    hc, wc = grid_of(H, W)
    n, ys = hc * wc, -(-W // 4) * 4
    planes = torch.zeros((POOL + 1, H, ys), dtype=torch.uint8, device=dev)  # picture k's luma at k + 1, its predecessor's at k
    words = torch.empty((POOL, n), dtype=torch.int32, device=dev)
    bg = torch.empty((POOL, H, W), dtype=torch.uint16, device=dev)
    counts = torch.empty(n, dtype=torch.uint16, device=dev)
    hist = torch.zeros(16 * 512, dtype=torch.int32, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def cells(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_noise_cells(cur[k].data_ptr(), WP, HP * WP, H, W, planes[k].data_ptr(), planes[k + 1].data_ptr(), ys,
                                       words[k].data_ptr(), st), "noise_cells")

    def motion(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_motion_step(cur[k].data_ptr(), WP, HP * WP, H, W, bg[k].data_ptr(), 0, 24, 4, 8, counts.data_ptr(), st),
                  "motion_step")

    for k in range(POOL):  # every luma plane and every model is a picture's before the clock starts
        lib.check(hip.dcvc_noise_cells(cur[k].data_ptr(), WP, HP * WP, H, W, None, planes[k + 1].data_ptr(), ys, words[k].data_ptr(), st),
                  "noise_cells")
        lib.check(hip.dcvc_motion_step(cur[(k + 1) % POOL].data_ptr(), WP, HP * WP, H, W, bg[k].data_ptr(), 1, 24, 4, 8, counts.data_ptr(), st),
                  "init")
    planes[0].copy_(planes[POOL])
    for k in range(POOL):
        cells(k, True)
    torch.cuda.synchronize(dev)
    measured = words.cpu().numpy().view(np.uint32)
    counted = measured[measured != 0xFFFFFFFF]
    bins = len(np.unique((counted >> 16) * 512 + np.minimum((counted & 0xFFFF) >> 4, 511)))

    # the histogram's inputs: the pool's own words repeated to 64 pictures, words spread over 14 x 256 bins, one bin
    g = np.random.default_rng(0)
    spread = ((g.integers(1, 15, BATCH * n) << 16) | g.integers(0, 4096, BATCH * n)).astype(np.uint32)
    inputs = {"the noisy pictures' own words": np.tile(measured.reshape(-1), BATCH // POOL),
              "words spread over 3584 bins": spread, "ALL WORDS IN ONE BIN": np.full(BATCH * n, (8 << 16) | 300, dtype=np.uint32)}
    inputs = {name: torch.from_numpy(w.view(np.int32)).to(dev) for name, w in inputs.items()}

    def count(i, w, pictures):
        lib.check(hip.dcvc_noise_hist(w.data_ptr(), pictures * n, hist.data_ptr(), st), "noise_hist")

    variants = {"noise_cells, one set of pictures (cache-resident)": lambda i: cells(i, False),
                "motion_step, one set of pictures (cache-resident)": lambda i: motion(i, False),
                "noise_cells, rotating over 16 sets (HBM)": lambda i: cells(i, True),
                "motion_step, rotating over 16 sets (HBM)": lambda i: motion(i, True)}
    for pictures in (1, BATCH):
        for name, w in inputs.items():
            variants[f"noise_hist, {pictures:2d} picture{'s' if pictures > 1 else ' '}, {name}"] = (lambda i, w=w, p=pictures: count(i, w, p))
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, a static scene under +-4 codes of noise ({bins} bins hold its {len(counted)} "
          f"counted cell words); {rounds} alternating rounds of {launches} launches between two HIP events, us per launch: median "
          f"(min .. max), bytes/s at the median")
    print(f"# bytes per launch: noise_cells {BYTES['noise_cells']} = 14 a pixel, motion_step {BYTES['motion_step']} = 16 a pixel: "
          f"x{BYTES['noise_cells'] / BYTES['motion_step']:.3f}")
    streaming = {name: t for name, t in times.items() if not name.startswith("noise_hist")}
    med = timing.kernel_table(streaming, lambda name: BYTES[name.split(",")[0]], width=52)
    for where in ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)"):
        print(f"# {where}: noise_cells / motion_step = x{med['noise_cells, ' + where] / med['motion_step, ' + where]:.2f} in time")
    print(f"# dcvc_noise_hist over {n} words a picture ({hc} x {wc} cells), us per launch: median (min .. max), words per us at the median")
    for name, t in times.items():
        if name.startswith("noise_hist"):
            t, pictures = np.array(t), int(name.split(",")[1].split()[0])
            print(f"  {name:60s} {np.median(t):7.2f}  ({t.min():.2f} .. {t.max():.2f})   {pictures * n / np.median(t):9.1f} words/us")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_noise_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        auto = N.AutoTNR()
        bits = {"--tnr-auto": sum(run(auto))}  # warm-up, and the threshold the source resolves to
        with open(os.path.join(tmp, "bins", RC.NOISE_JSON)) as f:
            noise = json.load(f)
        T = noise["threshold"]
        variants = {f"encode_video --tnr {T}": N.TNR(T), "encode_video --tnr-auto": auto}
        bits[f"--tnr {T}"] = sum(run(N.TNR(T)))  # warm-up
        assert len(set(bits.values())) == 1, bits  # (the same bytes: the option resolves to that setting)
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file (sensor noise of 2 codes a channel; measured mad32 {noise['mad32']}, "
              f"sigma {noise['sigma_milli'] / 1000:.3f} codes of luma, {noise['cells']} cells counted), GOP 32, one GOP stream, seeded "
              f"synthetic weights (the bits mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: "
              f"mean (min .. max)")
        timing.rate_table(rates, width=28, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "noise_time.py", {"kernels": (kernels, (200, 5)), "encode": (encode, (32, 3))})
