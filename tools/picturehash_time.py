"""Decoded-picture hashes at 1920x1080 (the record in profiles/picturehash_1080p.txt).

    python3 tools/picturehash_time.py kernels [launches=200]        both digests alone on a padded 1088x1920 picture: the
                                                                    `pixels` digest of its 1080x1920 crop and the `state`
                                                                    digest of all of it (two launches each), timed with
                                                                    device events around `launches` calls; also the shape for
                                                                    `rocprofv3 --kernel-trace --stats -- python3 ...`
    python3 tools/picturehash_time.py files [n_frames=64] [repeats=3]   encode_video frames/s with and without picture_hash=,
                                                                    alternating in one process

The file setting is tools/roil_time.py's: synthetic.frames as a Y4M file, GOP 32, two GOP streams, fp16x3, one pair of codecs
per stream shared by every run, a warm-up pass of both variants first; the .bin totals must agree (checked), and the digests
of the repeats must be the same (checked).  The yardstick is the run without the option in the same process; set the
difference beside the pool's +-3 % box spread.  Frames/s from a host clock around work that ends in a device synchronise.
"""
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vcm_ts_amd import picturehash as PH  # noqa: E402

H, W, HP, WP, GOP, STREAMS = 1080, 1920, 1088, 1920, 32, 2
DEV = torch.device("cuda:0")


def kernels(launches):
    from vcm_ts_amd.synthetic import frames

    x = torch.zeros((1, 3, HP, WP), device=DEV)
    x[..., :H, :W] = torch.from_numpy(frames(0, 1, H, W)).to(DEV)
    out, scratch = torch.zeros(2, dtype=torch.uint32, device=DEV), PH.new_scratch(DEV)
    calls = {"pixels, the 1080x1920 crop (6.2 MB of codes from 24.9 MB of fp32)": lambda: PH.crc32_pixels(x, (H, W), out=out[0:1], scratch=scratch),
             "state, all of 3x1088x1920 fp32 (25.1 MB)": lambda: PH.crc32_f32(x, out=out[1:2], scratch=scratch)}
    host = x.cpu().numpy()[0]
    code = np.rint(np.float32(255.0) * np.clip(host[:, :H, :W], np.float32(0.0), np.float32(1.0))).astype(np.uint8)
    want = [zlib.crc32(code.transpose(1, 2, 0).tobytes()), zlib.crc32(host.tobytes())]
    print(f"# one padded {HP}x{WP} picture, {launches} calls each (a call is two launches: the blocks, then the fold); "
          f"{PH.lib.hash_constant('dcvc_hash_block_bytes')} bytes per workgroup")
    for n, (what, call) in enumerate(calls.items()):
        for _ in range(5):
            call()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            call()
        stop.record()
        stop.synchronize()
        assert int(out.cpu().numpy()[n]) == want[n], what  # (zlib on the host is the judge here too)
        print(f"  {what:72s} {1000 * start.elapsed_time(stop) / launches:8.1f} us per call")


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as V
    from vcm_ts_amd.synthetic import frames

    tmp = tempfile.mkdtemp(prefix="dcvc_picturehash_time_")
    try:
        spec, y4m = V.ColorSpec(), os.path.join(tmp, "src.y4m")
        rgb = frames(0, n, H, W)
        with V.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:
            for t in range(n):
                wr.write(t, V.rgb_to_yuv420(torch.from_numpy(rgb[t:t + 1]).to(DEV), H, W, spec).cpu().numpy())
        nets = [RC._nets(DEV, "fp16x3") for _ in range(STREAMS)]
        records = []

        def run(hashed, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            torch.cuda.synchronize(DEV)
            t0 = time.time()
            bits, _ = RC.encode_video(y4m, out, max_frames=max_frames, gop=GOP, gop_streams=STREAMS, nets=nets, picture_hash=hashed)
            torch.cuda.synchronize(DEV)
            dt = time.time() - t0
            assert os.path.exists(os.path.join(out, PH.HASHES_JSON)) == hashed
            if hashed and max_frames is None:
                records.append(json.load(open(os.path.join(out, PH.HASHES_JSON))))
            return len(bits) / dt, sum(bits)

        for v in (False, True):  # warm-up: both code paths once
            run(v, max_frames=GOP + 2)
        rates, total = {False: [], True: []}, None
        for _ in range(repeats):
            for v in (False, True):  # alternating
                fps, bits = run(v)
                rates[v].append(fps)
                total = bits if total is None else total
                assert bits == total, (bits, total)  # the option changes no .bin byte
        assert all(r == records[0] for r in records)  # the same digests every time
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3; .bin total of every run "
              f"{total} bits; {len(records)} identical hashes.json, pixels[0] {records[0]['pixels'][0]} state[0] {records[0]['state'][0]}")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        base = np.mean(rates[False])
        for v in (False, True):
            a = np.array(rates[v])
            print(f"  {'picture_hash=True' if v else 'without picture_hash':24s} {a.mean():6.2f}  ({a.min():.2f} .. {a.max():.2f})   " +
                  " ".join(f"{x:.2f}" for x in a) + (f"   {100 * (a.mean() / base - 1):+.1f} % against without" if v else ""))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "files"
    if not torch.cuda.is_available():
        sys.exit("picturehash_time.py measures on the GPU; none is visible")
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode == "kernels":
        kernels(arg(2, 200))
    elif mode == "files":
        files(arg(2, 64), arg(3, 3))
    else:
        sys.exit(__doc__)
