"""The motion search and compensation in front of the temporal noise prefilter at 1920x1080 (the record in
profiles/me_1080p.txt).

    python3 tools/me_time.py kernels [launches=50] [rounds=5]
                                        dcvc_me_search at R = 8, 16, 32 and dcvc_me_compensate beside dcvc_tnr_step (the
                                        yardstick: the streaming kernel they stand in front of) on the same pictures,
                                        alternating in one process: on one set of pictures (cache-resident) and rotating
                                        over 16 sets (HBM).  HIP events around `launches` back-to-back launches, `rounds`
                                        times each
    python3 tools/me_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr 8 and with --tnr 8 --tnr-search 16,
                                        alternating in one process

Two yardsticks, neither a time fixed in advance: dcvc_tnr_step in the same process, and for the search the count of byte
differences a launch makes, (2R + 1)^2 H W.  Bytes per launch come from the shapes: the search reads 12 bytes a pixel of cur
and 12 of ref (16 + 2R) (16 + 4 ceil((2R + 1) / 4)) / 256 times over for the window of every cell; the compensation reads 12
and writes 12; the step reads 24, 20 * 260 / (16 * 256) times over, and writes 12.  Frames/s from a host clock around work
that ends in a device synchronise.
"""
import ctypes as C
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
POOL = 16
RADII = (8, 16, 32)
HALO = (16 + 4) * (256 + 4) / (16 * 256)


def window(R):
    """How often the windows of the cells make a pixel of ref be read."""
    return (16 + 2 * R) * (16 + 4 * ((2 * R + 1 + 3) // 4)) / 256


def differences(R):
    return (2 * R + 1) ** 2 * H * W


BYTES = dict({f"me_search R={R}": (12 + 12 * window(R)) * H * W for R in RADII},
             **{"me_compensate": 24 * H * W, "tnr_step": (24 * HALO + 12) * H * W})


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    # a static scene under +-4 codes of noise; in cur a band of rows stands 6 columns further right than in ref
    cur, ref = (timing.noisy_pool(ground, (H, W), POOL) for _ in range(2))
    out = torch.zeros((POOL, 3, HP, WP), device=dev)
    y0, y1, _ = timing.BOX
    cur[:, :, y0:y1, 6:W] = ref[:, :, y0:y1, :W - 6]
    hc, wc = grid_of(H, W)
    tnr = N.TNR(8)
    wtab = torch.from_numpy(tnr.table().view(np.int16)).to(dev)
    sad = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    held = torch.empty(hc * wc, dtype=torch.int16, device=dev)
    mv = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)
    found = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)  # what compensate moves by: the vectors of R = 16
    cost = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    zero = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def search(i, rotate, R, into=mv):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_search(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, R, N.PENALTY,
                                     into.data_ptr(), cost.data_ptr(), zero.data_ptr(), st), "me_search")

    def compensate(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_compensate(ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, found.data_ptr(), st),
                  "me_compensate")

    def step(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_tnr_step(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP,
                                    H, W, wtab.data_ptr(), tnr.pixel, sad.data_ptr(), held.data_ptr(), st), "tnr_step")

    search(0, False, 16, found)
    torch.cuda.synchronize(dev)
    moved = int((found.view(-1, 2) != 0).any(dim=1).sum()) / (-(-H // 16) * -(-W // 16))
    where = (", one set of pictures (cache-resident)", False), (", rotating over 16 sets (HBM)", True)
    variants = {}
    for label, rotate in where:
        for R in RADII:
            variants[f"me_search R={R}{label}"] = lambda i, R=R, rotate=rotate: search(i, rotate, R)
        variants["me_compensate" + label] = lambda i, rotate=rotate: compensate(i, rotate)
        variants["tnr_step" + label] = lambda i, rotate=rotate: step(i, rotate)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, lambda = {N.PENALTY}, {moved:.3f} of the cells moved at R = 16; {rounds} "
          f"alternating rounds of {launches} launches between two HIP events, us per launch: median (min .. max), bytes/s at the median")
    print("# bytes per launch: " + ", ".join(f"{name} {BYTES[name]:.0f} = {BYTES[name] / (H * W):.2f} a pixel" for name in BYTES))
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=56)
    for label, _ in where:
        for R in RADII:
            t = med[f"me_search R={R}{label}"]
            print(f"# me_search R={R}{label}: {differences(R) / 1e9:.2f} G byte differences a launch, {differences(R) / t / 1e6:.2f} T/s; "
                  f"me_search / tnr_step = x{t / med['tnr_step' + label]:.2f} in time")
        print(f"# me_compensate{label}: me_compensate / tnr_step = x{med['me_compensate' + label] / med['tnr_step' + label]:.2f} in time")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_me_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --tnr 8": N.TNR(8), "encode_video --tnr 8 --tnr-search 16": N.TNR(8, search=16)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=40, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "me_time.py", {"kernels": (kernels, (50, 5)), "encode": (encode, (32, 3))})
