"""Backward-adaptive quantisation at 1920x1080 (the record in profiles/aq_1080p.txt).

    python3 tools/aq_time.py kernels [launches=200]            the two kernels alone on padded 1088x1920 pictures, from HIP
                                                               events: per launch, beside the time that reading 3 Hp Wp 4
                                                               bytes takes at the warp kernel's 4.5 TB/s
    python3 tools/aq_time.py files [n_frames=64] [repeats=3]   encode_video frames/s with and without aq=AQ(100),
                                                               alternating in one process
    python3 tools/aq_time.py decode [n_frames=32] [repeats=2]  decode_video frames/s of those two encodes, alternating

`kernels` times the activity kernel twice: on ONE picture launch after launch (25 MB: it stays in the 256 MiB Infinity Cache,
which is also where a reference picture the codec has just written is likely to be), and rotating over 16 pictures (401 MB:
every launch reads from HBM).  The yardstick applies to the second.  `files` and `decode` are tools/roil_time.py's setting:
synthetic.frames as a Y4M file, GOP 32, two GOP streams (decode: one), fp16x3, one pair of codecs per stream shared by every
run, a warm-up pass of every variant first.  Set the differences beside the pool's +-3 % box spread (README.md).  Frames/s
from a host clock around work that ends in a device synchronise.
"""
import ctypes as C
import os
import shutil
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import aq as A  # noqa: E402
from vcm_ts_amd import lib  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
GOP, STREAMS = 32, 2
DEV = torch.device("cuda:0")
YARDSTICK_TBS = 4.5  # the warp kernel's measured rate
SETTING = A.AQ(100)


def kernels(launches):
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.synthetic import frames

    maps = A.AqMaps(SETTING, DEV)
    base = torch.zeros((16, 3, HP, WP), device=DEV)
    base[:, :, :H, :W] = torch.from_numpy(frames(0, 1, H, W)).to(DEV)
    base += torch.rand((16, 1, 1, 1), device=DEV) * 0.01
    hc, wc = HP // 16, WP // 16
    L = torch.empty(hc * wc, dtype=torch.int32, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty(hc * wc, dtype=torch.float32, device=DEV)
    st = C.c_void_p(_raw_stream(DEV.index))
    hip = lib.hip()

    def activity(i, rotate):
        p = base[i % 16 if rotate else 0]
        lib.check(hip.dcvc_aq_activity(p.data_ptr(), WP, HP * WP, HP, WP, L.data_ptr(), total.data_ptr(), st), "aq_activity")

    def to_map(i):
        lib.check(hip.dcvc_aq_map(L.data_ptr(), total.data_ptr(), hc, wc, maps.ktab.data_ptr(), maps.ftab.data_ptr(), None,
                                  out.data_ptr(), st), "aq_map")

    us = lambda fn: timing.event_us(fn, launches, warmup=min(launches, 32), sync="device")
    nbytes = 3 * HP * WP * 4
    floor_us = nbytes / (YARDSTICK_TBS * 1e12) * 1e6
    one = us(lambda i: activity(i, False))
    many = us(lambda i: activity(i, True))
    total.zero_()
    activity(0, False)
    mapped = us(to_map)
    whole = us(lambda i: maps.map(base[i % 16:i % 16 + 1]))
    print(f"# {WP}x{HP} padded picture, {nbytes} bytes read per launch, {hc * wc} cells; {launches} launches between two HIP events")
    print(f"# yardstick: {nbytes} bytes at {YARDSTICK_TBS} TB/s = {floor_us:.2f} us")
    print(f"  dcvc_aq_activity, one picture (cache-resident)     {one:7.2f} us   {nbytes / one / 1e6:6.2f} TB/s   x{one / floor_us:.2f} of the yardstick")
    print(f"  dcvc_aq_activity, rotating over 16 pictures (HBM)  {many:7.2f} us   {nbytes / many / 1e6:6.2f} TB/s   x{many / floor_us:.2f} of the yardstick")
    print(f"  dcvc_aq_map                                        {mapped:7.2f} us")
    print(f"  AqMaps.map (memset + both launches, from Python)   {whole:7.2f} us   (host-bound: launches issued back to back)")


def files(n, repeats, decode=False):
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_aq_time_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        nets = timing.codec_pairs(DEV, "fp16x3", STREAMS)
        common = dict(gop=GOP, gop_streams=STREAMS, nets=nets)
        setting = {"without": None, f"aq=AQ({SETTING.strength})": SETTING}
        totals = {}

        def encode(v, where, max_frames=None):
            shutil.rmtree(where, ignore_errors=True)

            def run():
                totals[v] = sum(RC.encode_video(y4m, where, max_frames=max_frames, aq=setting[v], **common)[0])
            return timing.fps(run, n, DEV)

        if not decode:
            for v in setting:  # warm-up: every shape and every code path once
                encode(v, os.path.join(tmp, "out"), max_frames=GOP + 2)
            rates = timing.alternating({v: v for v in setting}, repeats, lambda v: encode(v, os.path.join(tmp, "out")))
            print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3; .bin totals "
                  f"{totals} bits (name-seeded weights: no rate is claimed)")
        else:
            bins = {v: os.path.join(tmp, f"bins{k}") for k, v in enumerate(setting)}
            for v in setting:
                encode(v, bins[v])
            with timing.shared_nets(nets[0]):
                def run(where):
                    return timing.fps(lambda: RC.decode_video(where, os.path.join(tmp, "dec.y4m"), precision="fp16x3"), n, DEV)

                for where in bins.values():
                    run(where)
                rates = timing.alternating(bins, repeats, run)
            print(f"# decode_video, {n} pictures {W}x{H} to a Y4M file, GOP {GOP}, one stream, fp16x3")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, baseline="without", width=28)


if __name__ == "__main__":
    timing.main(__doc__, "aq_time.py", {"kernels": (kernels, (200,)), "files": (files, (64, 3)),
                                        "decode": (lambda n, repeats: files(n, repeats, decode=True), (32, 2))}, default="files")
