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
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vcm_ts_amd import scale as SC  # noqa: E402

H, W, GOP, STREAMS = 1080, 1920, 32, 2
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
        for _ in range(5):
            call()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            call()
        stop.record()
        stop.synchronize()
        # the judge: the numpy restatement, compared on a band of 64 output rows of one plane
        want = R.resize(x.cpu().numpy()[0, 1], dst_size)[100:164]
        assert np.array_equal(out.cpu().numpy()[0, 1, 100:164].view(np.uint32), want.view(np.uint32)), (h, w, which)
        mb = 12 * (src_size[0] * src_size[1] + dst_size[0] * dst_size[1]) / 1e6
        us = 1000 * start.elapsed_time(stop) / launches
        print(f"  {src_size[1]}x{src_size[0]} -> {dst_size[1]}x{dst_size[0]} ({mb:6.1f} MB read + written) {us:8.1f} us per call")


def _y4m(path, n, h, w):
    from vcm_ts_amd import yuv as V
    from vcm_ts_amd.synthetic import frames

    spec = V.ColorSpec()
    rgb = frames(0, n, h, w)
    with V.Y4MWriter(path, w, h, spec, fps=(30, 1)) as wr:
        for t in range(n):
            wr.write(t, V.rgb_to_yuv420(torch.from_numpy(rgb[t:t + 1]).to(DEV), h, w, spec).cpu().numpy())


def files(n, repeats):
    from vcm_ts_amd import run_codec as RC

    tmp = tempfile.mkdtemp(prefix="dcvc_scale_time_")
    try:
        y4m = os.path.join(tmp, "src.y4m")
        _y4m(y4m, n, H, W)
        nets = [RC._nets(DEV, "fp16x3") for _ in range(STREAMS)]

        def run(ratio, max_frames=None):
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            torch.cuda.synchronize(DEV)
            t0 = time.time()
            bits, size = RC.encode_video(y4m, out, max_frames=max_frames, gop=GOP, gop_streams=STREAMS, nets=nets, base_scale=ratio)
            torch.cuda.synchronize(DEV)
            dt = time.time() - t0
            assert size == (H, W) and os.path.exists(os.path.join(out, SC.SCALE_JSON)) == (ratio is not None)
            return len(bits) / dt, sum(bits)

        for v in (None, "1/2"):  # warm-up: both code paths once
            run(v, max_frames=GOP + 2)
        rates, totals = {None: [], "1/2": []}, {}
        for _ in range(repeats):
            for v in (None, "1/2"):  # alternating
                fps, bits = run(v)
                rates[v].append(fps)
                assert totals.setdefault(v, bits) == bits  # every repeat codes the same bytes
        print(f"# encode_video, {n} pictures {W}x{H} from a Y4M file, GOP {GOP}, {STREAMS} GOP streams, fp16x3, no output but the "
              f".bin files (one down() launch per picture, no up()); .bin totals {totals[None]} bits without, {totals['1/2']} with")
        print(f"# frames/s, {repeats} alternating repeats: mean (min .. max)")
        base = np.mean(rates[None])
        for v in (None, "1/2"):
            a = np.array(rates[v])
            print(f"  {'base_scale=1/2' if v else 'without base_scale':24s} {a.mean():6.2f}  ({a.min():.2f} .. {a.max():.2f})   " +
                  " ".join(f"{x:.2f}" for x in a) + (f"   {100 * (a.mean() / base - 1):+.1f} % against without" if v else ""))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def workspace():
    from vcm_ts_amd import run_codec as RC

    tmp = tempfile.mkdtemp(prefix="dcvc_scale_time_")
    try:
        y4m = os.path.join(tmp, "uhd.y4m")
        _y4m(y4m, 8, 2160, 3840)
        torch.cuda.synchronize(DEV)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
        bits, size = RC.encode_video(y4m, os.path.join(tmp, "out"), gop=8, gop_streams=1, precision="fp16x3", base_scale="1/2")
        torch.cuda.synchronize(DEV)
        print(f"# one GOP stream, 8 pictures 3840x2160 coded at 1/2 (a 1920x1080 base layer), fp16x3: {sum(bits)} bits")
        print(f"  peak reserved {torch.cuda.max_memory_reserved(DEV) / 2 ** 30:6.2f} GiB, peak allocated "
              f"{torch.cuda.max_memory_allocated(DEV) / 2 ** 30:6.2f} GiB (torch's caching allocator; a native 1080p stream: ~33 GB)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "files"
    if not torch.cuda.is_available():
        sys.exit("scale_time.py measures on the GPU; none is visible")
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode == "kernels":
        kernels(arg(2, 200))
    elif mode == "files":
        files(arg(2, 64), arg(3, 3))
    elif mode == "workspace":
        workspace()
    else:
        sys.exit(__doc__)
