"""Scene-cut detection at 1920x1080 (the record in profiles/scenecut_1080p.txt).

    python3 tools/scenecut_time.py kernels [rounds=30]        dcvc_scene_hist beside dcvc_roi_sse (the yardstick: an existing
                                                              streaming kernel of the same shape that reads TWO such
                                                              pictures) on a random and on a constant picture, alternating
                                                              in one process.  Prints device-event times of batches; for
                                                              per-dispatch kernel times run it under
                                                              `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 ...`
                                                              and give the trace to `trace`
    python3 tools/scenecut_time.py trace KERNEL_TRACE.csv     per-variant kernel times from that trace (the launch order of
                                                              `kernels` is fixed, so dispatch i belongs to variant i mod 4)
    python3 tools/scenecut_time.py scan [n_frames=64] [repeats=3]
                                                              frames/s of the scan pass alone (Y4M file; PNG folder with 8
                                                              readers) and of encode with --scenecut against plain encode,
                                                              alternating in one process

Bytes per launch come from the shapes: the histogram reads 12 bytes a pixel (three fp32 planes), the yardstick 24.
Frames/s from a host clock around work that ends in a device synchronise.
"""
import csv
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
GOP, STREAMS, BATCH = 32, 2, 20
VARIANTS = ("scene_hist random", "roi_sse random", "scene_hist constant", "roi_sse constant")
BYTES = {"scene_hist": 12 * H * W, "roi_sse": 24 * H * W}


def kernels(rounds):
    import torch

    from vcm_ts_amd import roi as X
    from vcm_ts_amd import scenecut as SC

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    rand = [torch.rand((1, 3, H, W), generator=g).to(dev) for _ in range(2)]
    flat = [torch.full((1, 3, H, W), v, device=dev) for v in (0.4, 0.4)]
    scan = SC.SceneScan(dev, H, W, 1)
    none, classes = X.FrameBoxes(), (X.RoiClass(0),)
    sums = torch.zeros(3, dtype=torch.int64, device=dev)
    steps = (lambda: scan.add(rand[0], row=0), lambda: X.region_sse(rand[0], rand[1], none, classes, sums=sums),
             lambda: scan.add(flat[0], row=0), lambda: X.region_sse(flat[0], flat[1], none, classes, sums=sums))
    for step in steps:  # warm-up: code objects, allocations
        for _ in range(3):
            step()
    torch.cuda.synchronize(dev)
    # each variant BATCH launches back to back between two events
    times = timing.alternating(dict(zip(VARIANTS, steps)), rounds, lambda step: timing.event_us(lambda i: step(), BATCH, warmup=0, sync="event"))
    print(f"# {W}x{H}, {rounds} alternating rounds of {BATCH} launches per variant; device events around a batch, us per launch "
          f"(includes whatever gap the host leaves between launches): median (min .. max), bytes/s at the median")
    timing.kernel_table(times, lambda name: BYTES[name.split()[0]], width=22)
    print(f"# launch order for `trace`: {', '.join(VARIANTS)}; {3 * len(steps)} warm-up dispatches first")


def trace(path):
    rows = list(csv.DictReader(open(path)))
    picked = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows
                    if "scene_hist_kernel" in r["Kernel_Name"] or "roi_kernel" in r["Kernel_Name"])
    picked = picked[12:]  # the warm-up: 3 dispatches of each of the 4 variants
    assert len(picked) % (4 * BATCH) == 0 and picked, len(picked)
    times = {v: [] for v in VARIANTS}
    for i, (t0, t1, name) in enumerate(picked):
        k = (i // BATCH) % 4
        assert ("scene_hist" in name) == (k % 2 == 0), (i, name)
        times[VARIANTS[k]].append((t1 - t0) / 1e3)
    print(f"# kernel times from a rocprofv3 kernel trace, {W}x{H}, {len(times[VARIANTS[0]])} dispatches per variant, us: "
          f"median (min .. max), bytes/s at the median")
    med = list(timing.kernel_table(times, lambda name: BYTES[name.split()[0]], width=22).values())
    for k, what in ((0, "random"), (2, "constant")):
        print(f"# {what}: scene_hist / roi_sse = {med[k] / med[k + 1]:.2f}  ({'within' if med[k] <= med[k + 1] else 'ABOVE'} the yardstick)")


def scan(n, repeats):
    import torch
    from PIL import Image

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import scenecut as SC
    from vcm_ts_amd import yuv as Y
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_scenecut_time_") as tmp:
        spec, png = Y.ColorSpec(), os.path.join(tmp, "png")
        os.makedirs(png)
        # two scenes, the second from frame n // 2 + 3 on: one cut in the middle of a GOP
        cut = n // 2 + 3
        rgb = np.concatenate([0.5 + 0.5 * frames(0, cut, H, W), 0.35 * frames(1, n - cut, H, W)]).astype(np.float32)
        y4m = timing.y4m_clip(tmp, n, (H, W), frames=rgb)
        for t in range(n):
            Image.fromarray(np.rint(rgb[t].transpose(1, 2, 0) * 255).astype(np.uint8)).save(os.path.join(png, f"im{t + 1:05d}.png"))
        nets = timing.codec_pairs(dev, "fp16x3", STREAMS)
        common = dict(gop=GOP, gop_streams=STREAMS, nets=nets)

        def scan_y4m():
            with Y.open_video(y4m, None, 8, None) as reader:
                ring, s = RC._PinnedRing(dev, reader.frame_bytes), SC.SceneScan(dev, H, W, n)
                for g in range(n):
                    reader.read_into(g, ring.host())
                    s.add(Y.yuv420_to_rgb(ring.upload().view(torch.uint8), H, W, spec, pad=True))
                return SC.plan(s.distances(), GOP, 0.5, 1)

        def scan_png():
            reader, ring, s = RC.PNGReader(png), RC._PinnedRing(dev, (H, W, 3)), SC.SceneScan(dev, H, W, n)
            for u8 in reader.prefetching(workers=8, depth=16, raw=True):
                ring.host()[...] = u8
                s.add(RC.pad_frame(RC.u8_to_unit_float(ring.upload())))
            return SC.plan(s.distances(), GOP, 0.5, 1)

        def encode(scenecut, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            bits, _ = RC.encode_video(y4m, out, max_frames=max_frames, scenecut=scenecut, **common)
            return len(bits)

        variants = {"scan pass alone, Y4M file": scan_y4m, "scan pass alone, PNG folder, 8 readers": scan_png,
                    "encode (Y4M), plain": lambda: encode(None), "encode (Y4M), --scenecut 0.5": lambda: encode(0.5)}
        encode(None, GOP + 2), encode(0.5, GOP + 2), scan_y4m(), scan_png()  # warm-up: every shape and code path once
        plans = set()

        def noted(fn):
            r = fn()
            if isinstance(r, list):
                plans.add(tuple(r))

        rates = timing.alternating(variants, repeats, lambda fn: timing.fps(lambda: noted(fn), n, dev))
        print(f"# {n} pictures {W}x{H}, a scene change at frame {cut}, GOP {GOP}, {STREAMS} GOP streams, fp16x3, bins only; "
              f"plans found by the scans: {sorted(plans)}")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, width=42, fmt="7.2f")
        base, cutr = np.mean(rates["encode (Y4M), plain"]), np.mean(rates["encode (Y4M), --scenecut 0.5"])
        print(f"# encode with --scenecut against plain: {100 * (cutr / base - 1):+.1f} % frames/s (the scan pass, plus one more I picture)")


if __name__ == "__main__":
    if sys.argv[1:2] == ["trace"] and len(sys.argv) > 2:  # (a path, and no GPU)
        sys.exit(trace(sys.argv[2]))
    timing.main(__doc__, "scenecut_time.py", {"kernels": (kernels, (30,)), "scan": (scan, (64, 3))})
