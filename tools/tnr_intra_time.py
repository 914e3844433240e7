"""The look-ahead filter of I pictures at 1920x1080 (the record in profiles/tnr_intra_1080p.txt).

    python3 tools/tnr_intra_time.py kernels [launches=200] [rounds=5]
                                        dcvc_tnr_fuse at n = 1, 2 and 4 references beside dcvc_tnr_step (the yardstick: the
                                        same strips, the same window, one reference) on the same pictures, alternating in
                                        one process: on one set of pictures (cache-resident) and rotating over 16 sets
                                        (HBM).  HIP events around `launches` back-to-back launches, `rounds` times each
    python3 tools/tnr_intra_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr 8 --tnr-search 16 and with the
                                        same plus --tnr-intra 2, one GOP stream, alternating in one process

Bytes per launch come from the shapes: without the halo the fusion reads 12 bytes a pixel of cur and of each of its n
references and writes 12, (12 (n + 1) + 12) / 36 = x1.00, x1.33 and x2.00 of the step's 36; with the 2-pixel halo of the
16 x 256 strips everything read is read 20 * 260 / (16 * 256) times over.  The second look at every reference in the blend
is not counted: it is expected to hit in L2.  Frames/s from a host clock around work that ends in a device synchronise.
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
REFS = (1, 2, 4)
HALO = (16 + 4) * (256 + 4) / (16 * 256)  # how often the strip's halo makes a pixel of cur and of a reference be read
BYTES = {"tnr_step": (24 * HALO + 12) * H * W, **{f"tnr_fuse n={n}": (12 * (n + 1) * HALO + 12) * H * W for n in REFS}}
NOMINAL = {"tnr_step": 36 * H * W, **{f"tnr_fuse n={n}": (12 * (n + 1) + 12) * H * W for n in REFS}}  # without the halo


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
    cur = timing.noisy_pool(ground, (H, W), POOL)
    refs = [timing.noisy_pool(ground, (H, W), POOL) for _ in range(max(REFS))]
    out = torch.zeros((POOL, 3, HP, WP), device=dev)
    cur[:, :, 400:656, :W] += 30.0 / 255.0
    hc, wc = grid_of(H, W)
    tnr = N.TNR(8, intra=max(REFS))
    wtab = torch.from_numpy(tnr.table().view(np.int16)).to(dev)
    rtab = torch.from_numpy(tnr.rcp_table()).to(dev)
    sad = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    held = torch.empty(hc * wc, dtype=torch.int16, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def step(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_tnr_step(cur[k].data_ptr(), WP, HP * WP, refs[0][k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP,
                                    H, W, wtab.data_ptr(), tnr.pixel, sad.data_ptr(), held.data_ptr(), st), "tnr_step")

    def fuse(n):
        def launch(i, rotate):
            k = i % POOL if rotate else 0
            ptrs = [refs[j][k].data_ptr() if j < n else None for j in range(4)]
            lib.check(hip.dcvc_tnr_fuse(cur[k].data_ptr(), WP, HP * WP, *ptrs, WP, HP * WP, n, out[k].data_ptr(), WP, HP * WP, H, W,
                                        wtab.data_ptr(), rtab.data_ptr(), tnr.pixel, sad.data_ptr(), held.data_ptr(), st), "tnr_fuse")
        return launch

    shares = {}
    for n in REFS:
        fuse(n)(0, False)
        torch.cuda.synchronize(dev)
        shares[n] = int(held.to(torch.int64).sum()) / (H * W)
    sets = ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)")
    variants = {}
    for where, rotate in zip(sets, (False, True)):
        for name, fn in [("tnr_step", step)] + [(f"tnr_fuse n={n}", fuse(n)) for n in REFS]:
            variants[f"{name}, {where}"] = (lambda fn, rotate: lambda i: fn(i, rotate))(fn, rotate)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, T = 8, " +
          ", ".join(f"{shares[n]:.3f} of the pixels blended at n = {n}" for n in REFS) + f"; {rounds} alternating rounds of "
          f"{launches} launches between two HIP events, us per launch: median (min .. max), bytes/s at the median")
    print("# bytes per launch with the halo (without): " +
          ", ".join(f"{name} {BYTES[name]:.0f} ({NOMINAL[name]}, x{NOMINAL[name] / NOMINAL['tnr_step']:.2f} of tnr_step)" for name in BYTES))
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=56)
    for where in sets:
        for n in REFS:
            print(f"# {where}: tnr_fuse n={n} / tnr_step = x{med[f'tnr_fuse n={n}, {where}'] / med['tnr_step, ' + where]:.2f} in time, "
                  f"x{NOMINAL[f'tnr_fuse n={n}'] / NOMINAL['tnr_step']:.2f} in bytes")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_tnr_intra_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --tnr 8 --tnr-search 16": N.TNR(8, search=16),
                    "encode_video --tnr 8 --tnr-search 16 --tnr-intra 2": N.TNR(8, search=16, intra=2)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=52, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "tnr_intra_time.py", {"kernels": (kernels, (200, 5)), "encode": (encode, (32, 3))})
