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
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, HP, WP, POOL = 1080, 1920, 1088, 1920, 16
HALO = (16 + 4) * (256 + 4) / (16 * 256)  # how often the strip's halo makes a pixel of cur and ref be read
BYTES = {"tnr_step": (24 * HALO + 12) * H * W, "motion_step": (12 + 4) * H * W}
NOMINAL = (24 + 12) * H * W  # without the halo


def _event_us(torch, fn, launches):
    for i in range(5):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    def noisy():  # a static scene under +-4 codes of noise, and a band of rows 30 codes away (passed through)
        x = torch.zeros((POOL, 3, HP, WP), device=dev)
        x[:, :, :H, :W] = ground + (torch.randint(-4, 5, (POOL, 3, H, W), device=dev).float() / 255.0)
        return x

    cur, ref, out = noisy(), noisy(), torch.zeros((POOL, 3, HP, WP), device=dev)
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
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():  # alternating
            times[name].append(_event_us(torch, fn, launches))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, T = 8, {share:.3f} of the pixels blended; {rounds} alternating rounds of "
          f"{launches} launches between two HIP events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: tnr_step {BYTES['tnr_step']:.0f} = {BYTES['tnr_step'] / (H * W):.2f} a pixel (36 without the halo: "
          f"{NOMINAL}), motion_step {BYTES['motion_step']}: x{BYTES['tnr_step'] / BYTES['motion_step']:.2f} "
          f"(x{NOMINAL / BYTES['motion_step']:.2f} without the halo)")
    med = {}
    for name, t in times.items():
        t = np.array(t)
        med[name] = np.median(t)
        print(f"  {name:52s} {np.median(t):7.2f}  ({t.min():.2f} .. {t.max():.2f})   {BYTES[name.split(',')[0]] / np.median(t) / 1e6:6.2f} TB/s")
    for where in ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)"):
        print(f"# {where}: tnr_step / motion_step = x{med['tnr_step, ' + where] / med['motion_step, ' + where]:.2f} in time")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd import yuv as Y
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="dcvc_tnr_time_")
    try:
        spec, y4m = Y.ColorSpec(), os.path.join(tmp, "src.y4m")
        ground = frames(0, 1, H, W, noise=0)[0]
        g = np.random.default_rng(1)
        with Y.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:  # a static camera, sensor noise and one moving rectangle
            for t in range(n):
                pic = np.clip(ground + np.float32(2 / 255) * g.standard_normal(ground.shape).astype(np.float32), 0, 1)
                x = 64 + (16 * t) % (W - 512)
                pic[:, 400:656, x:x + 384] = 1.0 if ground[:, 400:656, x:x + 384].mean() < 0.5 else 0.0
                wr.write(t, Y.rgb_to_yuv420(torch.from_numpy(pic[None]).to(dev), H, W, spec).cpu().numpy())
        nets = RC._nets(dev, None)
        variants = {"encode_video": None, "encode_video --tnr 8": N.TNR(8)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = {name: [] for name in variants}
        for _ in range(repeats):
            for name, tnr in variants.items():  # alternating
                torch.cuda.synchronize(dev)
                t0 = time.time()
                run(tnr)
                torch.cuda.synchronize(dev)
                rates[name].append(n / (time.time() - t0))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        for name, r in rates.items():
            a = np.array(r)
            print(f"  {name:24s} {a.mean():7.2f}  ({a.min():.2f} .. {a.max():.2f})   " + " ".join(f"{x:.2f}" for x in a))
        a, b = np.array(rates["encode_video"]), np.array(rates["encode_video --tnr 8"])
        print(f"# with / without = x{b.mean() / a.mean():.3f} in frames/s; the spread of the repeats without the option is "
              f"x{a.min() / a.mean():.3f} .. x{a.max() / a.mean():.3f} of their mean")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode not in ("kernels", "encode"):
        sys.exit(__doc__)
    import torch

    if not torch.cuda.is_available():
        sys.exit("tnr_time.py measures on the GPU; none is visible")
    if mode == "kernels":
        kernels(arg(2, 200), arg(3, 5))
    else:
        encode(arg(2, 32), arg(3, 3))
