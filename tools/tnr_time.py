"""The temporal noise prefilter at 1920x1080 (the record in profiles/tnr_1080p.txt).

    python3 tools/tnr_time.py kernels [launches=200] [rounds=5]
                                        dcvc_tnr_step beside dcvc_motion_step (the yardstick: the streaming kernel with the
                                        same tiling on the same three fp32 planes) on the same picture, alternating in one
                                        process: on one set of pictures (cache-resident) and rotating over 16 sets (HBM).
                                        HIP events around `launches` back-to-back launches, `rounds` times each
    python3 tools/tnr_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file without the option and with --tnr 8,
                                        alternating in one process

Bytes per launch come from the shapes: the step reads 24 bytes a pixel of cur and ref, 20 * 260 / (16 * 256) times over
for the 2-pixel halo of its 16 x 256 strips, and writes 12; the yardstick reads 12 bytes a pixel of picture and reads and
writes 2 of model.  Frames/s from a host clock around work that ends in a device synchronise.
"""
import ctypes as C
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
HALO = (16 + 4) * (256 + 4) / (16 * 256)  # how often the strip's halo makes a pixel of cur and ref be read
BYTES = {"tnr_step": (24 * HALO + 12) * H * W, "motion_step": (12 + 4) * H * W}
NOMINAL = (24 + 12) * H * W  # without the halo


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    # a static scene under +-4 codes of noise, and a band of rows 30 codes away (passed through)
    cur, ref = (timing.noisy_pool(ground, (H, W), POOL) for _ in range(2))
    out = torch.zeros((POOL, 3, HP, WP), device=dev)
    cur[:, :, 400:656, :W] += 30.0 / 255.0
    hc, wc = grid_of(H, W)
    tnr = N.TNR(8)
    wtab = torch.from_numpy(tnr.table().view(np.int16)).to(dev)
    sad = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    held = torch.empty(hc * wc, dtype=torch.int16, device=dev)
    bg = torch.empty((POOL, H, W), dtype=torch.uint16, device=dev)
    counts = torch.empty(hc * wc, dtype=torch.uint16, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def step(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_tnr_step(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP,
                                    H, W, wtab.data_ptr(), tnr.pixel, sad.data_ptr(), held.data_ptr(), st), "tnr_step")

    def motion(i, rotate, init=0):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_motion_step(cur[k].data_ptr(), WP, HP * WP, H, W, bg[k].data_ptr(), init, 24, 4, 8, counts.data_ptr(), st),
                  "motion_step")

    for k in range(POOL):
        lib.check(hip.dcvc_motion_step(ref[k].data_ptr(), WP, HP * WP, H, W, bg[k].data_ptr(), 1, 24, 4, 8, counts.data_ptr(), st), "init")
    step(0, False)
    torch.cuda.synchronize(dev)
    share = int(held.to(torch.int64).sum()) / (H * W)
    variants = {"tnr_step, one set of pictures (cache-resident)": lambda i: step(i, False),
                "motion_step, one set of pictures (cache-resident)": lambda i: motion(i, False),
                "tnr_step, rotating over 16 sets (HBM)": lambda i: step(i, True),
                "motion_step, rotating over 16 sets (HBM)": lambda i: motion(i, True)}
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, T = 8, {share:.3f} of the pixels blended; {rounds} alternating rounds of "
          f"{launches} launches between two HIP events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: tnr_step {BYTES['tnr_step']:.0f} = {BYTES['tnr_step'] / (H * W):.2f} a pixel (36 without the halo: "
          f"{NOMINAL}), motion_step {BYTES['motion_step']}: x{BYTES['tnr_step'] / BYTES['motion_step']:.2f} "
          f"(x{NOMINAL / BYTES['motion_step']:.2f} without the halo)")
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=52)
    for where in ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)"):
        print(f"# {where}: tnr_step / motion_step = x{med['tnr_step, ' + where] / med['motion_step, ' + where]:.2f} in time")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_tnr_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video": None, "encode_video --tnr 8": N.TNR(8)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=24, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "tnr_time.py", {"kernels": (kernels, (200, 5)), "encode": (encode, (32, 3))})
