"""The deinterlacer at 1920x1080 (the record in profiles/deint_1080p.txt).

    python3 tools/deint_time.py kernels [launches=200] [rounds=5]
                                        dcvc_deinterlace420 beside dcvc_yuv420_to_rgb (the yardstick: the launch that follows it in
                                        the file loop, on the same frames) in one process, alternating: on one set of frames
                                        (cache-resident) and rotating over 16 sets (HBM), at 8 and at 10 bits, for the earlier
                                        and for the later field.  HIP events around `launches` back-to-back launches, `rounds`
                                        times each
    python3 tools/deint_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file whose header says It with --deinterlace frame,
                                        against the same bytes relabelled Ip without the option, alternating in one process

Bytes per launch come from the shapes and are the MINIMUM the work needs, not what the lanes issue: the deinterlacer reads
cur once, one neighbour frame in full and the other by half, and writes one frame -- 3.75 + 1.5 samples a pixel; the
conversion reads 1.5 samples a pixel and writes 12 bytes for each pixel of the padded picture.  Frames/s from a host clock
around work that ends in a device synchronise.
"""
import ctypes as C
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
POOL = 16


def nbytes(name):
    sb = 2 if "10 bits" in name else 1
    return 5.25 * sb * H * W if name.startswith("deinterlace") else 1.5 * sb * H * W + 12 * HP * WP


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import yuv as Y
    from vcm_ts_amd.engine import _raw_stream

    dev = torch.device("cuda:0")
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()
    n, bands = Y.frame_samples(H, W), -(-H // 8)
    rgb = torch.zeros((POOL, 3, HP, WP), device=dev)
    moved = torch.empty(bands, dtype=torch.int32, device=dev)
    variants = {}
    for depth in (8, 10):
        dtype = torch.uint8 if depth == 8 else torch.int16
        frames = torch.randint(0, 1 << depth, (POOL + 2, n), device=dev).to(dtype)  # frame k's neighbours are k - 1 and k + 1
        out = torch.empty((POOL, n), dtype=dtype, device=dev)
        cc = Y.ColorSpec(bit_depth=depth).coeffs()

        def planes(t):  # (made once: between two events only the calls themselves are on the host's clock)
            return [p.data_ptr() for p in Y.split_planes(t, H, W)] + [W, W // 2]

        src, dst = [planes(f) for f in frames], [planes(f) for f in out]
        pics, cref, words = [rgb[k].data_ptr() for k in range(POOL)], C.byref(cc), moved.data_ptr()

        def deint(i, rotate, second, src=src, dst=dst, depth=depth):
            k = 1 + (i % POOL if rotate else 0)
            lib.check(hip.dcvc_deinterlace420(*src[k - 1], *src[k], *src[k + 1], H, W, depth, second, second, *dst[k - 1], words, bands, st),
                      "deinterlace420")

        def to_rgb(i, rotate, dst=dst, cref=cref, pics=pics):
            k = i % POOL if rotate else 0
            lib.check(hip.dcvc_yuv420_to_rgb(*dst[k][:3], H, W, W, W // 2, cref, pics[k], HP, WP, WP, HP * WP, 0, st), "yuv420_to_rgb")

        for where, rotate in (("one set of frames (cache-resident)", False), ("rotating over 16 sets (HBM)", True)):
            for second in (0, 1):
                variants[f"deinterlace420, {depth} bits, {'later' if second else 'earlier'} field, {where}"] = \
                    (lambda i, r=rotate, s=second, f=deint: f(i, r, s))
            variants[f"yuv420_to_rgb, {depth} bits, {where}"] = (lambda i, r=rotate, f=to_rgb: f(i, r))
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} I420 frames of random samples, top field first; {rounds} alternating rounds of {launches} launches between two HIP "
          f"events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch at 8 bits (the minimum, see the tool's head): deinterlace420 {nbytes('deinterlace'):.0f} = 5.25 a pixel, "
          f"yuv420_to_rgb {nbytes('yuv'):.0f}; twice the samples' share at 10 bits")
    timing.kernel_table(times, nbytes, width=76)


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_deint_time_") as tmp:
        ip = timing.y4m_clip(tmp, n, (H, W))
        it = os.path.join(tmp, "src_it.y4m")
        data = open(ip, "rb").read()
        end = data.index(b"\n")
        assert data[:end].count(b" Ip") == 1
        with open(it, "wb") as f:  # the same bytes, the header relabelled
            f.write(data[:end].replace(b" Ip", b" It") + data[end:])
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video, the file labelled Ip": (ip, None), "encode_video --deinterlace frame, labelled It": (it, "frame")}

        def run(v):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(v[0], out, gop=32, nets=nets, deinterlace=v[1])[0]

        bits = {name: sum(run(v)) for name, v in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda v: timing.fps(lambda: run(v), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file (synthetic PROGRESSIVE pictures: deinterlacing them changes the "
              f"samples where they move, so the two rows code different pictures), GOP 32, one GOP stream, seeded synthetic weights "
              f"(the bits mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=50, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "deint_time.py", {"kernels": (kernels, (200, 5)), "encode": (encode, (32, 3))})
