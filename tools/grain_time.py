"""Film-grain synthesis at 1920x1080 (the record in profiles/grain_1080p.txt).

    python3 tools/grain_time.py kernels [launches=200] [rounds=5]
                                        dcvc_grain_measure and dcvc_grain_apply beside dcvc_tnr_step (the yardstick: the
                                        streaming kernel with the same strips on the same fp32 planes) on the same pictures,
                                        alternating in one process: on one set of pictures (cache-resident) and rotating
                                        over 16 sets (HBM).  HIP events around `launches` back-to-back launches, `rounds`
                                        times each
    python3 tools/grain_time.py decode [n_frames=32] [repeats=3]
                                        frames/s of decode_video to a Y4M file without the option and with --grain,
                                        alternating in one process, of a folder coded with --tnr 8 --grain

Bytes per launch come from the shapes: the measurement reads 24 bytes a pixel (source and filtered picture) where the cell
was blended throughout and nothing elsewhere, the synthesis reads 12 and writes 12; the yardstick moves 36 without its halo.
Frames/s from a host clock around work that ends in a device synchronise.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

H, W = timing.SIZE
HP, WP = timing.padded((H, W))
POOL = 16
HALO = (16 + 4) * (256 + 4) / (16 * 256)  # how often the strip's halo makes the yardstick read a pixel of cur and ref
BYTES = {"grain_measure": 24 * H * W, "grain_apply": 24 * H * W, "tnr_step": (24 * HALO + 12) * H * W}
NOMINAL = 36 * H * W  # the yardstick without the halo


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import grain as GR
    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)
    # a static scene under +-4 codes of noise, and a band of rows 30 codes away (passed through: its cells stay out)
    cur, ref = (timing.noisy_pool(ground, (H, W), POOL) for _ in range(2))
    out = torch.zeros((POOL, 3, HP, WP), device=dev)
    shown = torch.zeros((POOL, 3, HP, WP), device=dev)
    cur[:, :, 400:656, :W] += 30.0 / 255.0
    hc, wc = grid_of(H, W)
    tnr = N.TNR(8)
    wtab = torch.from_numpy(tnr.table().view(np.int16)).to(dev)
    sad = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    held = torch.empty((POOL, hc * wc), dtype=torch.int16, device=dev)
    acc = torch.zeros(GR.WORDS, dtype=torch.int64, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def step(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_tnr_step(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP,
                                    H, W, wtab.data_ptr(), tnr.pixel, sad.data_ptr(), held[k].data_ptr(), st), "tnr_step")

    def measure(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_grain_measure(cur[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, held[k].data_ptr(),
                                         acc.data_ptr(), st), "grain_measure")

    for k in range(POOL):  # every set's filtered picture and held cells
        step(k, True)
    acc.zero_()
    measure(0, False)
    torch.cuda.synchronize(dev)
    sums = acc.tolist()
    rec = GR.params(sums, 1024)
    stab = torch.from_numpy(GR.table(rec["points"], rec["kh"], rec["kv"]).view(np.int16)).to(dev)
    share = sum(sums[0::4]) / (H * W)
    BYTES["grain_measure"] = 24 * H * W * share

    def apply(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_grain_apply(out[k].data_ptr(), WP, HP * WP, shown[k].data_ptr(), WP, HP * WP, H, W, i, rec["kh"], rec["kv"],
                                       stab.data_ptr(), st), "grain_apply")

    sets = ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)")
    variants = {}
    for where, rotate in zip(sets, (False, True)):
        for name, fn in (("grain_measure", measure), ("grain_apply", apply), ("tnr_step", step)):
            variants[f"{name}, {where}"] = (lambda fn, rotate: lambda i: fn(i, rotate))(fn, rotate)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, T = 8, {share:.3f} of the pixels in cells blended throughout; record "
          f"{rec['points']} kh {rec['kh']} kv {rec['kv']}; {rounds} alternating rounds of {launches} launches between two HIP "
          f"events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: grain_measure {BYTES['grain_measure']:.0f} (24 a pixel of the cells that take part), grain_apply "
          f"{BYTES['grain_apply']} (24 a pixel), tnr_step {BYTES['tnr_step']:.0f} ({NOMINAL} without the halo): x"
          f"{BYTES['grain_apply'] / NOMINAL:.2f} of tnr_step's without the halo")
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=52)
    for where in sets:
        for name in ("grain_measure", "grain_apply"):
            print(f"# {where}: {name} / tnr_step = x{med[f'{name}, {where}'] / med['tnr_step, ' + where]:.2f} in time")


def decode(n, repeats):
    import torch

    from vcm_ts_amd import grain as GR
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_grain_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        bins = os.path.join(tmp, "bins")
        RC.encode_video(y4m, bins, gop=32, nets=nets, tnr=N.TNR(8), grain=GR.Grain())
        record = RC.S.read_sidecar(bins, GR.GRAIN_JSON)[1]
        variants = {"decode_video": None, "decode_video --grain": 100}

        def run(grain):
            return RC.decode_video(bins, os.path.join(tmp, "dec.y4m"), grain=grain)

        with timing.shared_nets(nets):
            for grain in variants.values():  # warm-up
                assert run(grain) == n
            rates = timing.alternating(variants, repeats, lambda grain: timing.fps(lambda: run(grain), n, dev))
        print(f"# decode_video: {n} pictures {W}x{H} to a Y4M file, GOP 32, coded with --tnr 8 --grain, seeded synthetic weights; "
              f"the first GOP's record {record['gops']['0']['points']} kh {record['gops']['0']['kh']} kv {record['gops']['0']['kv']}; "
              f"frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=24, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "grain_time.py", {"kernels": (kernels, (200, 5)), "decode": (decode, (32, 3))})
