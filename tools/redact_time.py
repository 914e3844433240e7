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
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, HP, WP, POOL = 1080, 1920, 1088, 1920, 16
HALO = (16 + 4) * (256 + 4) / (16 * 256)
BYTES = {"redact": 24 * H * W, "tnr_step": (24 * HALO + 12) * H * W}


def _event_us(torch, fn, launches):
    for i in range(5):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    def noisy():
        x = torch.zeros((POOL, 3, HP, WP), device=dev)
        x[:, :, :H, :W] = (ground + (torch.randint(-4, 5, (POOL, 3, H, W), device=dev).float() / 255.0)).clamp_(0, 1)
        return x

    cur, ref, out = noisy(), noisy(), torch.zeros((POOL, 3, HP, WP), device=dev)
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
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():  # alternating
            times[name].append(_event_us(torch, fn, launches))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, grow 4; the share of the picture in R: "
          + ", ".join(f"{k} {v:.4f}" for k, v in shares.items()) + f"; {rounds} alternating rounds of {launches} launches between two "
          f"HIP events, us per launch: median (min .. max), bytes/s at the median")
    print(f"# bytes per launch: redact {BYTES['redact']} = 24 a pixel, tnr_step {BYTES['tnr_step']:.0f} = {BYTES['tnr_step'] / (H * W):.2f} a pixel")
    for name, t in times.items():
        t = np.array(t)
        print(f"  {name:78s} {np.median(t):7.2f}  ({t.min():.2f} .. {t.max():.2f})   {BYTES[name.split(',')[0]] / np.median(t) / 1e6:6.2f} TB/s")


def encode(n, repeats):
    import pickle

    import torch

    from vcm_ts_amd import redact as D
    from vcm_ts_amd import roi as X
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import yuv as Y
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="dcvc_redact_time_")
    try:
        spec, y4m = Y.ColorSpec(), os.path.join(tmp, "src.y4m")
        ground = frames(0, 1, H, W, noise=0)[0]
        g = np.random.default_rng(1)
        os.makedirs(os.path.join(tmp, "root", "motion_coords"))
        with Y.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:  # a static camera, sensor noise and one moving rectangle with its box
            for t in range(n):
                pic = np.clip(ground + np.float32(2 / 255) * g.standard_normal(ground.shape).astype(np.float32), 0, 1)
                x = 64 + (16 * t) % (W - 512)
                pic[:, 400:656, x:x + 384] = 1.0 if ground[:, 400:656, x:x + 384].mean() < 0.5 else 0.0
                wr.write(t, Y.rgb_to_yuv420(torch.from_numpy(pic[None]).to(dev), H, W, spec).cpu().numpy())
                with open(os.path.join(tmp, "root", "motion_coords", "%05d" % (t + 1)), "wb") as f:
                    pickle.dump(np.array([[x, 400, x + 384, 656]], np.uint16), f)
        boxes = X.PickleBoxes(os.path.join(tmp, "root"))
        roi = X.Roi(boxes, boxes.classes)
        nets = RC._nets(dev, None)
        variants = {"encode_video --roi-root": None, "encode_video --roi-root --redact motion --redact-tile 16": D.Redact(("motion",), tile=16)}

        def run(redact):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, roi=roi, redact=redact)[0]

        bits = {name: sum(run(r)) for name, r in variants.items()}  # warm-up
        rates = {name: [] for name in variants}
        for _ in range(repeats):
            for name, r in variants.items():  # alternating
                torch.cuda.synchronize(dev)
                t0 = time.time()
                run(r)
                torch.cuda.synchronize(dev)
                rates[name].append(n / (time.time() - t0))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, one 384 x 256 box a picture, seeded "
              f"synthetic weights (the bits mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: "
              f"mean (min .. max)")
        for name, r in rates.items():
            a = np.array(r)
            print(f"  {name:58s} {a.mean():7.2f}  ({a.min():.2f} .. {a.max():.2f})   " + " ".join(f"{x:.2f}" for x in a))
        a, b = (np.array(r) for r in rates.values())
        print(f"# with / without = x{b.mean() / a.mean():.3f} in frames/s; the spread of the repeats without the option is "
              f"x{a.min() / a.mean():.3f} .. x{a.max() / a.mean():.3f} of their mean")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    if mode not in ("kernels", "encode"):
        sys.exit(__doc__)
    import torch

    if not torch.cuda.is_available():
        sys.exit("redact_time.py measures on the GPU; none is visible")
    if mode == "kernels":
        kernels(arg(2, 200), arg(3, 5))
    else:
        encode(arg(2, 32), arg(3, 3))
