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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
POOL = 16
BYTES = {"motion_step": (12 + 4) * H * W, "aq_activity": 12 * HP * WP}


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
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crop of a {WP}x{HP} padded picture; {rounds} alternating rounds of {launches} launches between two HIP "
          f"events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: motion_step {BYTES['motion_step']} (picture read, model read and written), aq_activity "
          f"{BYTES['aq_activity']}: x{BYTES['motion_step'] / BYTES['aq_activity']:.2f}")
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=46)
    for where in ("one picture (cache-resident)", "rotating over 16 pictures (HBM)"):
        print(f"# {where}: motion_step / aq_activity = x{med['motion_step, ' + where] / med['aq_activity, ' + where]:.2f} in time")


def boxes(n, repeats):
    import torch

    from vcm_ts_amd import motionroi as M
    from vcm_ts_amd import run_codec as RC

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_motion_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=1)  # a static camera and one moving rectangle
        params = M.MotionParams(24)

        def run():
            out = os.path.join(tmp, "found")
            shutil.rmtree(out, ignore_errors=True)
            return RC.motion_boxes_video(y4m, out, params, dev)

        found = run()  # warm-up
        rates = timing.alternating({"boxes pass (read, convert, scan, box rule, write)": run}, repeats, lambda fn: timing.fps(fn, n, dev))
        print(f"# run_codec boxes --video: {n} pictures {W}x{H} from a Y4M file, threshold 24, default parameters; "
              f"{sum(len(b) for b in found)} boxes in {sum(1 for b in found if len(b))} pictures")
        print(f"# frames/s, {repeats} repeats after one warm-up: mean (min .. max)")
        timing.rate_table(rates, width=50, fmt="7.2f")


if __name__ == "__main__":
    timing.main(__doc__, "motion_time.py", {"kernels": (kernels, (200, 5)), "boxes": (boxes, (64, 3))})
