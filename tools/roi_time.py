"""The ROI enhancement layer at 1920x1080 (the record in profiles/roi_1080p.txt).

    python3 tools/roi_time.py kernels [launches=20] [boxes=8]   the three kernels alone, for
                                                                `rocprofv3 --kernel-trace --stats -- python3 ...` (one run per
                                                                box count: the kernels keep their names)
    python3 tools/roi_time.py host [repeats=5]                  the same three steps the reference's way: numpy on host arrays,
                                                                the device -> host copies of the pictures included
    python3 tools/roi_time.py files [n_frames=64] [repeats=3]   encode_video frames/s with and without roi + residuals,
                                                                alternating in one process

Boxes: seeded, half plate-sized (about 120 x 40, border 10), half face-sized (about 80 x 80, border 25), anywhere in the
picture.  `files`: synthetic.frames content as a Y4M file, GOP 32, two GOP streams, fp16x3, one pair of codecs per
stream shared by every run, a warm-up pass of both variants first; the .bin totals of both variants must agree
(checked).  Frames/s and host times from a host clock around work that ends in a device synchronise.
"""
import os
import shutil
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import roi as X  # noqa: E402

H, W = timing.SIZE
GOP, STREAMS = 32, 2
DEV = torch.device("cuda:0")
CLASSES = (X.RoiClass(10), X.RoiClass(25))
BOX_COUNTS = (0, 8, 64)


def make_boxes(n, seed=0):
    rng = np.random.default_rng(seed + n)
    rows = []
    for i in range(n):
        cls = i % 2
        w, h = (int(rng.integers(90, 150)), int(rng.integers(30, 50))) if cls == 0 else (int(rng.integers(60, 100)), int(rng.integers(60, 100)))
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        rows.append([x, y, x + w, y + h, cls])
    return X.FrameBoxes(np.array(rows, np.int32).reshape(-1, 5))


def pictures():
    from vcm_ts_amd.synthetic import frames

    fr = torch.from_numpy(frames(0, 2, H, W)).to(DEV)
    src = torch.round(fr[0:1] * 255.0) / 255.0
    rec = (fr[0:1] * 0.97 + fr[1:2] * 0.03).clamp(0.0, 1.0).contiguous()
    return src.contiguous(), rec


def kernels(launches, n):
    src, rec = pictures()
    boxes = make_boxes(n)
    for _ in range(launches):
        res = X.residual_layer(src, rec, boxes, layout="planar", order="gbr")
    for _ in range(launches):
        X.fuse(rec, res, boxes, CLASSES, order="gbr")
    for _ in range(launches):
        sums = X.region_sse(rec, src, boxes, CLASSES)
    torch.cuda.synchronize(DEV)
    px = H * W
    print(f"# {n} boxes, {launches} launches each; bytes per launch from the shapes: residual {px * 27 / 1e6:.2f} MB "
          f"(24 read + 3 written per pixel), fuse {px * 27 / 1e6:.2f} MB (12 + 3 read, 12 written), sse {px * 24 / 1e6:.2f} MB; "
          f"pixels inside {int(sums[2])}")


def host(repeats):
    """compute_residuals, fuse_layers and calc_visual_metrics as the reference computes them (numpy, float32 HWC
    arrays), starting from pictures on the device: what a caller of the codec had to do without the kernels."""
    src, rec = pictures()
    to_u8 = lambda t: np.clip(np.rint(t[0].permute(1, 2, 0).cpu().numpy() * 255), 0, 255).astype(np.uint8)

    def gradient(w, h, border):
        if border == 0:
            return np.ones((h, w, 1), np.float32)
        mask = np.zeros((h, w, 1), np.float32)
        for i, x in enumerate(np.linspace(0.9, 0.0, border)):
            mask[i:h - i, i:w - i, :] = 1 - x
        return mask

    print(f"# host way, {W}x{H}, ms per picture: mean (min .. max) over {repeats} repeats; d2h = two pictures to uint8 HWC arrays")
    for n in BOX_COUNTS:
        boxes = make_boxes(n).array
        times = {k: [] for k in ("d2h", "residual", "fuse", "metrics")}
        for _ in range(repeats):
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            s8, r8 = to_u8(src), to_u8(rec)
            t1 = time.perf_counter()
            residual = np.clip(s8.astype(np.float32) - r8.astype(np.float32) + 128, 0.0, 255.0)
            mask = np.zeros((H, W, 1), np.float32)
            for x1, y1, x2, y2, _ in boxes:
                mask[y1:y2, x1:x2] = 1.0
            res8 = (residual * mask).astype(np.uint8)
            t2 = time.perf_counter()
            mask = np.zeros((H, W, 1), np.float32)
            for x1, y1, x2, y2, c in boxes:
                mask[y1:y2, x1:x2] = gradient(x2 - x1, y2 - y1, CLASSES[c].border)
            fused = np.clip(r8.astype(np.float32) + mask * (res8.astype(np.float32) - 128), 0, 255).astype(np.uint8)
            t3 = time.perf_counter()
            mask = np.zeros((H, W, 1), np.float32)
            for x1, y1, x2, y2, c in boxes:
                p = CLASSES[c].shrink
                mask[y1 + p:y2 - p, x1 + p:x2 - p] = 1.0
            nz = np.count_nonzero(mask)
            mse = (s8.astype(np.float32) / 255.0 - fused.astype(np.float32) / 255.0) ** 2
            _ = (np.mean(mse), np.sum(mse * (1.0 - mask)) / (s8.size - nz), np.sum(mse * mask) / max(nz, 1))
            t4 = time.perf_counter()
            for k, v in zip(times, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                times[k].append(v * 1e3)
        print(f"  {n:3d} boxes  " + "  ".join(f"{k} {np.mean(v):7.2f} ({min(v):.2f} .. {max(v):.2f})" for k, v in times.items()) +
              f"  sum {sum(np.mean(v) for v in times.values()):7.2f}")


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_roi_time_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        common = dict(gop=GOP, gop_streams=STREAMS, nets=timing.codec_pairs(DEV, "fp16x3", STREAMS))
        totals = set()

        def run(n_boxes, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            extra = {}
            if n_boxes is not None:
                lists = [make_boxes(n_boxes, seed=t) for t in range(n)]
                extra = dict(roi=X.Roi(lambda t: lists[t], CLASSES), residuals=os.path.join(out, "res.gbrp"))
            rate = timing.fps(lambda: totals.add(sum(RC.encode_video(y4m, os.path.join(out, "bin"), max_frames=max_frames, **extra, **common)[0])),
                              n, DEV)
            if max_frames is None:
                assert len(totals) == 1, totals  # the enhancement layer changes no .bin byte
            return rate

        variants = {"without roi": None, **{f"roi, {v:2d} boxes a picture, residuals to .gbrp": v for v in (8, 64)}}
        for v in variants.values():  # warm-up: every shape and every code path once
            run(v, max_frames=GOP + 2)
        totals.clear()
        rates = timing.alternating(variants, repeats, run)
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, bins only; .bin total of every "
              f"run {totals.pop()} bits")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, baseline="without", width=44)


if __name__ == "__main__":
    timing.main(__doc__, "roi_time.py", {"kernels": (kernels, (20, 8)), "host": (host, (5,)), "files": (files, (64, 3))}, default="files")
