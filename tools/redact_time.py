"""ROI redaction at 1920x1080 (the record in profiles/redact_1080p.txt).

    python3 tools/redact_time.py kernels [launches=200] [rounds=5]
                                        dcvc_redact beside dcvc_tnr_step (the yardstick: the streaming kernel on the same three
                                        fp32 planes, which reads two pictures and writes one) on the same pictures, alternating in
                                        one process: on one set of pictures (cache-resident) and rotating over 16 sets (HBM), for
                                        three lists -- one empty box (no block touched: the kernel's copy path; the file loops
                                        launch nothing for such a picture), 10 boxes, one box over the whole picture -- as a
                                        mosaic of 8 x 8 tiles, and the whole picture also with 64 x 64 tiles and as a solid fill.
                                        HIP events around `launches` back-to-back launches, `rounds` times each
    python3 tools/redact_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file without the option and with a moving box
                                        redacted in every picture, alternating in one process

Bytes per launch come from the shapes: the kernel reads 12 bytes a pixel and writes 12 (the box list and the counts are
noise beside them); the yardstick reads 24 and writes 12, plus its halo.  Frames/s from a host clock around work that ends
in a device synchronise.
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
HALO = (16 + 4) * (256 + 4) / (16 * 256)
BYTES = {"redact": 24 * H * W, "tnr_step": (24 * HALO + 12) * H * W}


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    cur, ref = (timing.noisy_pool(ground, (H, W), POOL).clamp_(0, 1) for _ in range(2))
    out = torch.zeros((POOL, 3, HP, WP), device=dev)
    hc, wc = grid_of(H, W)
    tnr = N.TNR(8)
    wtab = torch.from_numpy(tnr.table().view(np.int16)).to(dev)
    sad = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    held = torch.empty(hc * wc, dtype=torch.int16, device=dev)
    count = torch.empty(hc * wc, dtype=torch.int16, device=dev)
    g = np.random.default_rng(2)
    x1, y1 = g.integers(0, W - 200, 10), g.integers(0, H - 120, 10)
    lists = {"no block touched": np.array([[5, 5, 5, 9, 0]], np.int32),
             "10 boxes": np.stack([x1, y1, x1 + g.integers(40, 200, 10), y1 + g.integers(30, 120, 10), np.zeros(10, np.int64)], 1).astype(np.int32),
             "the whole picture": np.array([[0, 0, W, H, 0]], np.int32)}
    on_dev = {k: torch.from_numpy(v.reshape(-1).copy()).to(dev) for k, v in lists.items()}
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def redact(i, rotate, which, tile, fill):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_redact(cur[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, lists[which].ctypes.data,
                                  on_dev[which].data_ptr(), len(lists[which]), 1, 4, tile, fill, count.data_ptr(), st), "redact")

    def step(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_tnr_step(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP,
                                    H, W, wtab.data_ptr(), tnr.pixel, sad.data_ptr(), held.data_ptr(), st), "tnr_step")

    shares = {}
    for which in lists:
        redact(0, False, which, 8, -1)
        torch.cuda.synchronize(dev)
        shares[which] = int(count.to(torch.int64).sum()) / (H * W)
    cases = [(w, 8, -1, f"{w}, tile 8") for w in lists] + [("the whole picture", 64, -1, "the whole picture, tile 64"),
                                                         ("the whole picture", 0, 128, "the whole picture, fill")]
    variants = {}
    for where, rotate in (("one set of pictures (cache-resident)", False), ("rotating over 16 sets (HBM)", True)):
        for which, tile, fill, label in cases:
            variants[f"redact, {label}, {where}"] = (lambda i, r=rotate, w=which, t=tile, f=fill: redact(i, r, w, t, f))
        variants[f"tnr_step, {where}"] = (lambda i, r=rotate: step(i, r))
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, grow 4; the share of the picture in R: "
          + ", ".join(f"{k} {v:.4f}" for k, v in shares.items()) + f"; {rounds} alternating rounds of {launches} launches between two "
          f"HIP events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: redact {BYTES['redact']} = 24 a pixel, tnr_step {BYTES['tnr_step']:.0f} = {BYTES['tnr_step'] / (H * W):.2f} a pixel")
    timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=78)


def encode(n, repeats):
    import torch

    from vcm_ts_amd import redact as D
    from vcm_ts_amd import roi as X
    from vcm_ts_amd import run_codec as RC

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_redact_time_") as tmp:
        y4m, root = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise, one moving rectangle with its box
        boxes = X.PickleBoxes(root)
        roi = X.Roi(boxes, boxes.classes)
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --roi-root": None, "encode_video --roi-root --redact motion --redact-tile 16": D.Redact(("motion",), tile=16)}

        def run(redact):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, roi=roi, redact=redact)[0]

        bits = {name: sum(run(r)) for name, r in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda r: timing.fps(lambda: run(r), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, one 384 x 256 box a picture, seeded "
              f"synthetic weights (the bits mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: "
              f"mean (min .. max)")
        timing.rate_table(rates, width=58, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "redact_time.py", {"kernels": (kernels, (200, 5)), "encode": (encode, (32, 3))})
