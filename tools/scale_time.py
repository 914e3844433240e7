"""The base layer's resampler at 1080p and 2160p (the record belongs in profiles/scale_1080p.txt).

    python3 tools/scale_time.py kernels [launches=200]      dcvc_scale_planes alone: 2160p -> 1080p, 1080p -> 540p and
                                                            540p -> 1080p on one picture (3 planes), each result checked
                                                            against tests/scale_ref.py bit for bit on a 64-row band, timed
                                                            with device events around `launches` calls; also the shape for
                                                            `rocprofv3 --kernel-trace --stats -- python3 ...` in a run of
                                                            its own
    python3 tools/scale_time.py files [n_frames=64] [repeats=3]    encode_video frames/s at 1080p with and without
                                                            base_scale="1/2", alternating in one process
    python3 tools/scale_time.py workspace                   reserved device memory of one GOP stream coding a 2160p source
                                                            at 1/2 (8 pictures), to be set beside the 33 GB of a native
                                                            1080p stream

The file setting is tools/picturehash_time.py's: synthetic.frames as a Y4M file, GOP 32, two GOP streams, fp16x3, one pair of
codecs per stream shared by every run, a warm-up pass of both variants first.  With the option the codec codes a quarter of
the pixels, so the two rates are NOT expected to agree: the yardstick says what the option costs or saves as a whole; set it
beside the pool's +-3 % box spread.  Frames/s from a host clock around work that ends in a device synchronise.
"""
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402
from vcm_ts_amd import scale as SC  # noqa: E402

H, W = timing.SIZE
GOP, STREAMS = 32, 2
DEV = torch.device("cuda:0")


def kernels(launches):
    from tests import scale_ref as R
    from vcm_ts_amd.synthetic import frames

    print(f"# one picture (3 planes), {launches} calls each, one launch per call")
    for (h, w), which in (((2160, 3840), "down"), ((1080, 1920), "down"), ((1080, 1920), "up")):
        s = SC.Scale((h, w), "1/2", DEV)
        src_size, dst_size = (s.full, s.base) if which == "down" else (s.base, s.full)
        x = torch.from_numpy(frames(0, 1, *src_size)).to(DEV)
        out = torch.empty((1, 3) + dst_size, device=DEV)
        call = (lambda: s.down(x, out=out)) if which == "down" else (lambda: s.up(x, out=out))
        us = timing.event_us(lambda i: call(), launches, warmup=5, sync="event")
        # the judge: the numpy restatement, compared on a band of 64 output rows of one plane
        want = R.resize(x.cpu().numpy()[0, 1], dst_size)[100:164]
        assert np.array_equal(out.cpu().numpy()[0, 1, 100:164].view(np.uint32), want.view(np.uint32)), (h, w, which)
        mb = 12 * (src_size[0] * src_size[1] + dst_size[0] * dst_size[1]) / 1e6
        print(f"  {src_size[1]}x{src_size[0]} -> {dst_size[1]}x{dst_size[0]} ({mb:6.1f} MB read + written) {us:8.1f} us per call")


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_scale_time_") as tmp:
        y4m = timing.y4m_clip(tmp, n, (H, W))
        nets = timing.codec_pairs(DEV, "fp16x3", STREAMS)
        totals = {}

        def run(ratio, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)

            def code():
                bits, size = RC.encode_video(y4m, out, max_frames=max_frames, gop=GOP, gop_streams=STREAMS, nets=nets, base_scale=ratio)
                assert size == (H, W)
                if max_frames is None:
                    assert totals.setdefault(ratio, sum(bits)) == sum(bits)  # every repeat codes the same bytes

            rate = timing.fps(code, n, DEV)
            assert os.path.exists(os.path.join(out, SC.SCALE_JSON)) == (ratio is not None)
            return rate

        variants = {"without base_scale": None, "base_scale=1/2": "1/2"}
        for v in variants.values():  # warm-up: both code paths once
            run(v, max_frames=GOP + 2)
        rates = timing.alternating(variants, repeats, run)
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3, no output but the "
              f".bin files (one down() launch per picture, no up()); .bin totals {totals[None]} bits without, {totals['1/2']} with")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        timing.rate_table(rates, baseline="without", width=24)


def workspace():
    from vcm_ts_amd import run_codec as RC

    with timing.workdir("dcvc_scale_time_") as tmp:
        y4m = timing.y4m_clip(tmp, 8, (2160, 3840))
        torch.cuda.synchronize(DEV)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
        bits, size = RC.encode_video(y4m, os.path.join(tmp, "out"), gop=8, gop_streams=1, precision="fp16x3", base_scale="1/2")
        torch.cuda.synchronize(DEV)
        print(f"# one GOP stream, 8 pictures 3840x2160 coded at 1/2 (a 1920x1080 base layer), fp16x3: {sum(bits)} bits")
        print(f"  peak reserved {torch.cuda.max_memory_reserved(DEV) / 2 ** 30:6.2f} GiB, peak allocated "
              f"{torch.cuda.max_memory_allocated(DEV) / 2 ** 30:6.2f} GiB (torch's caching allocator; a native 1080p stream: ~33 GB)")


if __name__ == "__main__":
    timing.main(__doc__, "scale_time.py", {"kernels": (kernels, (200,)), "files": (files, (64, 3)), "workspace": (workspace, ())},
                default="files")
