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
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vcm_ts_amd import aq as A  # noqa: E402
from vcm_ts_amd import lib  # noqa: E402

H, W, GOP, STREAMS = 1080, 1920, 32, 2
HP, WP = 1088, 1920
DEV = torch.device("cuda:0")
YARDSTICK_TBS = 4.5  # the warp kernel's measured rate
SETTING = A.AQ(100)


def _event_us(fn, launches):
    """microseconds per call of fn(i), i = 0 .. launches - 1, between two HIP events (after a warm-up of every call)"""
    for i in range(min(launches, 32)):
        fn(i)
    torch.cuda.synchronize(DEV)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(launches):
        fn(i)
    t1.record()
    torch.cuda.synchronize(DEV)
    return 1000.0 * t0.elapsed_time(t1) / launches


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

    nbytes = 3 * HP * WP * 4
    floor_us = nbytes / (YARDSTICK_TBS * 1e12) * 1e6
    one = _event_us(lambda i: activity(i, False), launches)
    many = _event_us(lambda i: activity(i, True), launches)
    total.zero_()
    activity(0, False)
    mapped = _event_us(to_map, launches)
    whole = _event_us(lambda i: maps.map(base[i % 16:i % 16 + 1]), launches)
    print(f"# {WP}x{HP} padded picture, {nbytes} bytes read per launch, {hc * wc} cells; {launches} launches between two HIP events")
    print(f"# yardstick: {nbytes} bytes at {YARDSTICK_TBS} TB/s = {floor_us:.2f} us")
    print(f"  dcvc_aq_activity, one picture (cache-resident)     {one:7.2f} us   {nbytes / one / 1e6:6.2f} TB/s   x{one / floor_us:.2f} of the yardstick")
    print(f"  dcvc_aq_activity, rotating over 16 pictures (HBM)  {many:7.2f} us   {nbytes / many / 1e6:6.2f} TB/s   x{many / floor_us:.2f} of the yardstick")
    print(f"  dcvc_aq_map                                        {mapped:7.2f} us")
    print(f"  AqMaps.map (memset + both launches, from Python)   {whole:7.2f} us   (host-bound: launches issued back to back)")


def _source(tmp, n):
    from vcm_ts_amd import yuv as V
    from vcm_ts_amd.synthetic import frames

    spec, y4m = V.ColorSpec(), os.path.join(tmp, "src.y4m")
    rgb = frames(0, n, H, W)
    with V.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:
        for t in range(n):
            wr.write(t, V.rgb_to_yuv420(torch.from_numpy(rgb[t:t + 1]).to(DEV), H, W, spec).cpu().numpy())
    return y4m


def _report(title, variants, rates, repeats):
    print(title)
    print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
    base = np.mean(rates[variants[0]])
    for v in variants:
        a = np.array(rates[v])
        print(f"  {v:28s} {a.mean():6.2f}  ({a.min():.2f} .. {a.max():.2f})   " + " ".join(f"{x:.2f}" for x in a) +
              ("" if v == variants[0] else f"   {100 * (a.mean() / base - 1):+.1f} % against {variants[0]}"))


def files(n, repeats, decode=False):
    from vcm_ts_amd import run_codec as RC

    tmp = tempfile.mkdtemp(prefix="dcvc_aq_time_")
    try:
        y4m = _source(tmp, n)
        nets = [RC._nets(DEV, "fp16x3") for _ in range(STREAMS)]
        common = dict(gop=GOP, gop_streams=STREAMS, nets=nets)
        variants = ["without", f"aq=AQ({SETTING.strength})"]
        setting = {variants[0]: None, variants[1]: SETTING}
        totals = {}

        def encode(v, where, max_frames=None):
            shutil.rmtree(where, ignore_errors=True)
            torch.cuda.synchronize(DEV)
            t0 = time.time()
            bits, _ = RC.encode_video(y4m, where, max_frames=max_frames, aq=setting[v], **common)
            torch.cuda.synchronize(DEV)
            totals[v] = sum(bits)
            return len(bits) / (time.time() - t0)

        if not decode:
            for v in variants:  # warm-up: every shape and every code path once
                encode(v, os.path.join(tmp, "out"), max_frames=GOP + 2)
            rates = {v: [] for v in variants}
            for _ in range(repeats):
                for v in variants:  # alternating
                    rates[v].append(encode(v, os.path.join(tmp, "out")))
            _report(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3; .bin totals "
                    f"{totals} bits (name-seeded weights: no rate is claimed)", variants, rates, repeats)
            return
        for k, v in enumerate(variants):
            encode(v, os.path.join(tmp, f"bins{k}"))
        made = RC._nets
        RC._nets = lambda *a, **kw: nets[0]  # (decode_video builds its codecs itself: hand it the pair every run shares)
        try:
            def run(k):
                torch.cuda.synchronize(DEV)
                t0 = time.time()
                count = RC.decode_video(os.path.join(tmp, f"bins{k}"), os.path.join(tmp, "dec.y4m"), precision="fp16x3")
                torch.cuda.synchronize(DEV)
                return count / (time.time() - t0)

            for k in range(2):
                run(k)
            rates = {v: [] for v in variants}
            for _ in range(repeats):
                for k, v in enumerate(variants):
                    rates[v].append(run(k))
        finally:
            RC._nets = made
        _report(f"# decode_video, {n} pictures {W}x{H} to a Y4M file, GOP {GOP}, one stream, fp16x3", variants, rates, repeats)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "files"
    if not torch.cuda.is_available():
        sys.exit("aq_time.py measures on the GPU; none is visible")
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode == "kernels":
        kernels(arg(2, 200))
    elif mode == "files":
        files(arg(2, 64), arg(3, 3))
    elif mode == "decode":
        files(arg(2, 32), arg(3, 2), decode=True)
    else:
        sys.exit(__doc__)
