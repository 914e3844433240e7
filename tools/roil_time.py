"""The coded ROI residual layer at 1920x1080 (the record in profiles/roil_1080p.txt).

    python3 tools/roil_time.py kernels [launches=20] [boxes=8] [step=1]   encode (two launches) and decode (two launches) alone,
                                                                          for `rocprofv3 --kernel-trace --stats -- python3 ...`
                                                                          (one run per box count: the kernels keep their names)
    python3 tools/roil_time.py files [n_frames=64] [repeats=3]            encode_video frames/s with residual_bins=, with
                                                                          residuals=x.gbrp and with neither, alternating in one
                                                                          process, for 0, 8 and 64 boxes a picture

Boxes, pictures and the file setting are tools/roi_time.py's (seeded plate- and face-sized boxes; synthetic.frames as a Y4M
file, GOP 32, two GOP streams, fp16x3, one pair of codecs per stream shared by every run, a warm-up pass of every variant
first; the .bin totals of all variants must agree, checked).  `files` also prints the records' sizes beside the 6.2 MB of a
raw frame.  The yardsticks are the .gbrp path in the same process and the run with neither; set the differences beside the
pool's +-3 % box spread.  Frames/s from a host clock around work that ends in a device synchronise.
"""
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from tools.roi_time import BOX_COUNTS, CLASSES, DEV, GOP, STREAMS, H, W, make_boxes, pictures  # noqa: E402
from vcm_ts_amd import roi as X  # noqa: E402
from vcm_ts_amd import roilayer as Y  # noqa: E402


def kernels(launches, n, step):
    src, rec = pictures()
    boxes = make_boxes(n)
    cells, counts = Y.active_cells(boxes, H, W)
    pending = [Y.encode_layer(src, rec, boxes, step) for _ in range(launches)]
    record = pending[-1].bytes()
    for _ in range(launches):
        Y.decode_layer(record, boxes, H, W, layout="planar", order="gbr")
    torch.cuda.synchronize(DEV)
    print(f"# {n} boxes, step {step}, {launches} encodes and decodes; {len(cells)} active cells, {int(counts.sum())} pixels inside, "
          f"record {len(record)} bytes ({8 * len(record) / max(int(counts.sum()) * 3, 1):.2f} bits per sample; a raw frame has "
          f"{3 * H * W} bytes), device-to-host copy per encode {Y.HEADER + Y.CELL_MAX * len(cells) + 4} bytes")


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_roil_time_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        common = dict(gop=GOP, gop_streams=STREAMS, nets=timing.codec_pairs(DEV, "fp16x3", STREAMS))
        sizes, totals = {}, set()

        def run(n_boxes, how, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            extra = {}
            if how != "neither":
                lists = [make_boxes(n_boxes, seed=t) for t in range(n)]
                extra = dict(roi=X.Roi(lambda t: lists[t], CLASSES))
                extra.update(dict(residuals=os.path.join(out, "res.gbrp")) if how == "gbrp" else dict(residual_bins=os.path.join(out, "rl")))
            rate = timing.fps(lambda: totals.add(sum(RC.encode_video(y4m, os.path.join(out, "bin"), max_frames=max_frames, **extra, **common)[0])),
                              n, DEV)
            if max_frames is None:
                assert len(totals) == 1, totals  # the enhancement layer changes no .bin byte
                if how == "records":
                    sizes[n_boxes] = [os.path.getsize(os.path.join(out, "rl", f)) for f in sorted(os.listdir(os.path.join(out, "rl")))]
            return rate

        variants = {"without roi": (None, "neither")}
        for b in BOX_COUNTS:
            variants[f"{b:2d} boxes a picture, residuals to .gbrp"] = (b, "gbrp")
            variants[f"{b:2d} boxes a picture, residual_bins (.rl)"] = (b, "records")
        for v in variants.values():  # warm-up: every shape and every code path once
            run(*v, max_frames=GOP + 2)
        totals.clear()
        rates = timing.alternating(variants, repeats, lambda v: run(*v))
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams; .bin total of every run {totals.pop()} bits")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, baseline="without", width=44)
        for b, s in sizes.items():
            print(f"# {b:2d} boxes: records of {np.mean(s):.0f} bytes a picture ({min(s)} .. {max(s)}) at step 1; a raw frame has {3 * H * W}")


if __name__ == "__main__":
    timing.main(__doc__, "roil_time.py", {"kernels": (kernels, (20, 8, 1)), "files": (files, (64, 3))}, default="files")
