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
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import picturehash as PH  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
GOP, STREAMS = 32, 2
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
        us = timing.event_us(lambda i: call(), launches, warmup=5, sync="event")
        assert int(out.cpu().numpy()[n]) == want[n], what  # (zlib on the host is the judge here too)
        print(f"  {what:72s} {us:8.1f} us per call")


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_picturehash_time_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        nets = timing.codec_pairs(DEV, "fp16x3", STREAMS)
        records, totals = [], set()

        def run(hashed, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            rate = timing.fps(lambda: totals.add(sum(RC.encode_video(y4m, out, max_frames=max_frames, gop=GOP, gop_streams=STREAMS, nets=nets,
                                                                     picture_hash=hashed)[0])), n, DEV)
            assert os.path.exists(os.path.join(out, PH.HASHES_JSON)) == hashed
            if max_frames is None:
                assert len(totals) == 1, totals  # the option changes no .bin byte
                if hashed:
                    records.append(json.load(open(os.path.join(out, PH.HASHES_JSON))))
            return rate

        variants = {"without picture_hash": False, "picture_hash=True": True}
        for v in variants.values():  # warm-up: both code paths once
            run(v, max_frames=GOP + 2)
        totals.clear()
        rates = timing.alternating(variants, repeats, run)
        assert all(r == records[0] for r in records)  # the same digests every time
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3; .bin total of every run "
              f"{totals.pop()} bits; {len(records)} identical hashes.json, pixels[0] {records[0]['pixels'][0]} state[0] {records[0]['state'][0]}")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, baseline="without", width=24)


if __name__ == "__main__":
    timing.main(__doc__, "picturehash_time.py", {"kernels": (kernels, (200,)), "files": (files, (64, 3))}, default="files")
