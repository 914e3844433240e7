"""Rate control at 1080p on the synthetic clip (the record in profiles/ratectl_1080p.txt).

    python3 tools/ratectl_time.py model [n_frames=32]            how well T_s predicts picture t, and where a controlled
                                                                 GOP lands against its target (GOP 32, fp16x3)
    python3 tools/ratectl_time.py files [n_frames=64] [repeats=3]   frames/s of encode_video with and without target_bpp,
                                                                 alternating in one process (two GOP streams, warm codecs)
    python3 tools/ratectl_time.py clip FILE.y4m [n_frames=64]    write the clip, for timing `run_codec encode --video` itself

Random (name-seeded) weights: the figures say how the controller behaves on this code, nothing about rate or quality.
"""
import os
import shutil
import sys
from fractions import Fraction

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import ratectl  # noqa: E402
from vcm_ts_amd import run_codec as RC  # noqa: E402
from vcm_ts_amd.pipeline import GopEncoder, pad_frame  # noqa: E402
from vcm_ts_amd.synthetic import frames  # noqa: E402

H, W = timing.SIZE
GOP, STREAMS = 32, 2
DEV = torch.device("cuda:0")


def write_clip(path, n):
    with timing.workdir("dcvc_ratectl_") as tmp:
        shutil.move(timing.y4m_clip(tmp, n, (H, W)), path)


def model(n):
    nets = RC._nets(DEV, "fp16x3")
    rgb = frames(0, n, H, W)
    xs = [pad_frame(torch.from_numpy(rgb[t:t + 1]).to(DEV)) for t in range(n)]
    enc = GopEncoder(*nets, gop_size=GOP)
    with torch.no_grad():
        coded, total, _ = enc.encode_gop(xs, 1.0, 1.0, 1.0)
    free = [(len(p) + (14 if k == "I" else 8)) * 8 for k, _, p in coded]
    print(f"# {n} pictures {W}x{H}, GOP {GOP}, q 1 1 1, fp16x3; free run: {total} bits, {total / (n * H * W):.4f} bpp, "
          f"I picture {free[0]} bits, P pictures {min(free[1:])} .. {max(free[1:])} bits")
    for frac in (Fraction(1, 2), Fraction(3, 4), Fraction(3, 2)):
        target = frac * Fraction(total, n)
        res = {}
        with torch.no_grad():
            _, bits, _ = enc.encode_gop(xs, 1.0, 1.0, 1.0, rate=ratectl.factory(target, GOP), res=res)
        print(f"# target {float(frac):.2f} x the free run's average = {float(target):.0f} bits per picture "
              f"({float(target) / (H * W):.4f} bpp): coded {bits} bits, {bits / (n * H * W):.4f} bpp, "
              f"{bits / float(target * n):.3f} of the target; P pictures from the third on "
              f"{sum(e[1] for e in res['rate_log'][3:GOP]) / float(sum(e[2] for e in res['rate_log'][3:GOP])):.3f} of their budgets")
        log = res["rate_log"][:GOP]
        rc = ratectl.RateControl(target, GOP)
        ratios = []
        print("#   picture  q_y   actual bits   budget      predicted from t-2   predicted / actual")
        for j, (q, a, b, est) in enumerate(log):
            rc.record(j, q, a, est)  # (a replay of the log: the decisions are the run's)
            if j >= 3:
                pred = float(rc.predict(j - 2, q))
                ratios.append(pred / a)
                print(f"    {j:4d}   {q / 100:6.2f}  {a:10d}  {float(b):10.0f}  {pred:12.0f}  {pred / a:14.3f}")
        r = np.array(ratios)
        print(f"#   predicted / actual over {len(r)} pictures: mean {r.mean():.3f}, min {r.min():.3f}, max {r.max():.3f}")


def files(n, repeats):
    with timing.workdir("dcvc_ratectl_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        common = dict(gop=GOP, gop_streams=STREAMS, nets=timing.codec_pairs(DEV, "fp16x3", STREAMS))
        totals = []

        def run(target):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            return timing.fps(lambda: totals.append(sum(RC.encode_video(y4m, out, target_bpp=target, **common)[0])), n, DEV)

        run(None)
        target = 0.75 * totals[0] / (n * H * W)
        run(target)  # (warm-up of both variants done)
        rates = timing.alternating({"without target_bpp": None, f"target_bpp={target:.4f}": target}, repeats, run)
        print(f"# {n} pictures {W}x{H}, GOP {GOP}, {STREAMS} GOP streams, fp16x3, Y4M file -> .bin folder; frames/s, {repeats} "
              f"alternating repeats: mean (min .. max)")
        timing.rate_table(rates, width=24)


if __name__ == "__main__":
    timing.main(__doc__, "ratectl_time.py", {"model": (model, (32,)), "files": (files, (64, 3)), "clip": (write_clip, (str, 64))})
