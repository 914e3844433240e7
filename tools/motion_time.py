"""Motion ROI boxes at 1920x1080 (the record in profiles/motion_1080p.txt).

    python3 tools/motion_time.py kernels [launches=200] [rounds=5]
                                        dcvc_motion_step beside dcvc_aq_activity (the yardstick: the streaming kernel that
                                        reads the same three fp32 planes) on the same picture, alternating in one process:
                                        on one picture (cache-resident) and rotating over 16 pictures and 16 models (HBM).
                                        HIP events around `launches` back-to-back launches, `rounds` times each
    python3 tools/motion_time.py boxes [n_frames=64] [repeats=3]
                                        frames/s of the whole `boxes` pass (scan, box rule, files) from a Y4M file

Bytes per launch come from the shapes: the step reads 12 bytes a pixel of picture and reads and writes 2 bytes a pixel of
model (1080 rows); the yardstick reads 12 bytes a pixel of the padded picture (1088 rows).  Frames/s from a host clock
around work that ends in a device synchronise.
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
BYTES = {"motion_step": (12 + 4) * H * W, "aq_activity": 12 * HP * WP}


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
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    base = torch.zeros((POOL, 3, HP, WP), device=dev)
    base[:, :, :H, :W] = torch.from_numpy(frames(0, 1, H, W)).to(dev)
    base += torch.rand((POOL, 1, 1, 1), device=dev) * 0.2  # (a few luma codes to well past the threshold: both branches)
    hc, wc = grid_of(H, W)
    bg = torch.empty((POOL, H, W), dtype=torch.uint16, device=dev)
    counts = torch.empty(hc * wc, dtype=torch.uint16, device=dev)
    L = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def motion(i, rotate, init=0, shift=0):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_motion_step(base[(k + shift) % POOL].data_ptr(), WP, HP * WP, H, W, bg[k].data_ptr(), init, 24, 4, 8,
                                       counts.data_ptr(), st), "motion_step")

    def activity(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_aq_activity(base[k].data_ptr(), WP, HP * WP, HP, WP, L.data_ptr(), total.data_ptr(), st), "aq_activity")

    for k in range(POOL):  # model k starts as picture k + 1: every timed step sees another picture than the model's own
        motion(k, True, init=1, shift=1)
    variants = {"motion_step, one picture (cache-resident)": lambda i: motion(i, False),
                "aq_activity, one picture (cache-resident)": lambda i: activity(i, False),
                "motion_step, rotating over 16 pictures (HBM)": lambda i: motion(i, True),
                "aq_activity, rotating over 16 pictures (HBM)": lambda i: activity(i, True)}
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():  # alternating
            times[name].append(_event_us(torch, fn, launches))
    print(f"# {W}x{H} crop of a {WP}x{HP} padded picture; {rounds} alternating rounds of {launches} launches between two HIP "
          f"events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: motion_step {BYTES['motion_step']} (picture read, model read and written), aq_activity "
          f"{BYTES['aq_activity']}: x{BYTES['motion_step'] / BYTES['aq_activity']:.2f}")
    med = {}
    for name, t in times.items():
        t = np.array(t)
        med[name] = np.median(t)
        print(f"  {name:46s} {np.median(t):7.2f}  ({t.min():.2f} .. {t.max():.2f})   {BYTES[name.split(',')[0]] / np.median(t) / 1e6:6.2f} TB/s")
    for where in ("one picture (cache-resident)", "rotating over 16 pictures (HBM)"):
        print(f"# {where}: motion_step / aq_activity = x{med['motion_step, ' + where] / med['aq_activity, ' + where]:.2f} in time")


def boxes(n, repeats):
    import torch

    from vcm_ts_amd import motionroi as M
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="dcvc_motion_time_")
    try:
        spec, y4m = Y.ColorSpec(), os.path.join(tmp, "src.y4m")
        ground = frames(0, 1, H, W, noise=0)[0]
        g = np.random.default_rng(1)
        with Y.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:  # a static camera and one moving rectangle
            for t in range(n):
                pic = np.clip(ground + np.float32(1 / 255) * g.standard_normal(ground.shape).astype(np.float32), 0, 1)
                x = 64 + (16 * t) % (W - 512)
                pic[:, 400:656, x:x + 384] = 1.0 if ground[:, 400:656, x:x + 384].mean() < 0.5 else 0.0
                wr.write(t, Y.rgb_to_yuv420(torch.from_numpy(pic[None]).to(dev), H, W, spec).cpu().numpy())
        params = M.MotionParams(24)

        def run():
            out = os.path.join(tmp, "root")
            shutil.rmtree(out, ignore_errors=True)
            return RC.motion_boxes_video(y4m, out, params, dev)

        found = run()  # warm-up
        rates = []
        for _ in range(repeats):
            torch.cuda.synchronize(dev)
            t0 = time.time()
            run()
            torch.cuda.synchronize(dev)
            rates.append(n / (time.time() - t0))
        a = np.array(rates)
        print(f"# run_codec boxes --video: {n} pictures {W}x{H} from a Y4M file, threshold 24, default parameters; "
              f"{sum(len(b) for b in found)} boxes in {sum(1 for b in found if len(b))} pictures")
        print(f"# frames/s, {repeats} repeats after one warm-up: mean (min .. max)")
        print(f"  boxes pass (read, convert, scan, box rule, write)  {a.mean():7.2f}  ({a.min():.2f} .. {a.max():.2f})   "
              + " ".join(f"{x:.2f}" for x in a))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode not in ("kernels", "boxes"):
        sys.exit(__doc__)
    import torch

    if not torch.cuda.is_available():
        sys.exit("motion_time.py measures on the GPU; none is visible")
    if mode == "kernels":
        kernels(arg(2, 200), arg(3, 5))
    else:
        boxes(arg(2, 64), arg(3, 3))
