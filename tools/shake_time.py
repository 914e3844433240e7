"""The camera-shake registration at 1920x1080 (the record in profiles/shake_1080p.txt).

    python3 tools/shake_time.py kernels [launches=200] [rounds=5]
                                        dcvc_shake_plane, dcvc_shake_tiles at R = 8 and R = 16, dcvc_shake_vote and
                                        dcvc_me_compensate with the uniform field, beside dcvc_noise_cells (the streaming
                                        yardstick) and dcvc_me_search at R = 8 (the full search the tile search is a sparse
                                        sample of), on the same pictures, alternating in one process: on one set of pictures
                                        (cache-resident) and rotating over 16 sets (HBM).  HIP events around `launches`
                                        back-to-back launches, `rounds` times each
    python3 tools/shake_time.py boxes [n_frames=512] [repeats=3]
                                        frames/s of the `boxes` pass without and with --shake 8 (three more launches a picture
                                        and the border mask on the host), alternating in one process, from two Y4M files of the
                                        same scene: a STILL camera, where the option finds (0, 0) in every picture and only
                                        costs, and a camera that SHAKES by up to 6 pixels per axis, where it also changes what
                                        the host's box rule is handed

Bytes per launch come from the shapes: dcvc_shake_plane reads 12 bytes a pixel and writes 1; dcvc_shake_tiles reads 12 bytes
a pixel of every fourth row inside the tiles and per tile the (61 + 2R) x (64 + 4 NG) bytes of its window; dcvc_shake_vote
moves a few kilobytes (20 bytes a tile read twice, 4 a cell written) and is given no rate; dcvc_me_compensate reads and
writes 12 bytes a pixel; dcvc_noise_cells 14 a pixel; dcvc_me_search is given as the 24 bytes a pixel of its two pictures
(its windows overlap; it is bound by its SADs).
Frames/s from a host clock around work that ends in a device synchronise.
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
TILES = (H // 64) * (W // 64)


def _window(R):
    return (61 + 2 * R) * (64 + 4 * ((R + 2) // 2))


BYTES = {"shake_plane": 13 * H * W, "shake_tiles R = 8": 3 * 64 * 64 * TILES + _window(8) * TILES,
         "shake_tiles R = 16": 3 * 64 * 64 * TILES + _window(16) * TILES,
         "me_compensate": 24 * H * W, "noise_cells": 14 * H * W, "me_search R = 8": 24 * H * W}


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)
    cur = timing.noisy_pool(ground, (H, W), POOL)  # a static scene under +-4 codes of noise
    hc, wc = grid_of(H, W)
    n, ys = hc * wc, -(-W // 4) * 4
    planes = torch.zeros((POOL + 1, H, ys), dtype=torch.uint8, device=dev)  # picture k's luma at k + 1, its predecessor's at k
    tiles = torch.zeros((POOL, TILES, 5), dtype=torch.int32, device=dev)  # what R = 8 found before the clock: the vote's input
    timed = torch.zeros((POOL, TILES, 5), dtype=torch.int32, device=dev)  # what the timed searches write
    record = torch.zeros((POOL, 8), dtype=torch.int32, device=dev)
    mv = torch.zeros((POOL, n, 2), dtype=torch.int16, device=dev)
    out = torch.empty((POOL, 3, H, W), dtype=torch.float32, device=dev)
    words = torch.empty((POOL, n), dtype=torch.int32, device=dev)
    cost, zero = torch.empty((POOL, n), dtype=torch.int32, device=dev), torch.empty((POOL, n), dtype=torch.int32, device=dev)
    smv = torch.empty((POOL, n, 2), dtype=torch.int16, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def pick(i, rotate):
        return i % POOL if rotate else 0

    def plane(i, rotate):
        k = pick(i, rotate)
        lib.check(hip.dcvc_shake_plane(cur[k].data_ptr(), WP, HP * WP, H, W, planes[k + 1].data_ptr(), ys, st), "shake_plane")

    def search(i, rotate, R, into=timed):
        k = pick(i, rotate)
        lib.check(hip.dcvc_shake_tiles(cur[k].data_ptr(), WP, HP * WP, H, W, planes[k].data_ptr(), ys, R, into[k].data_ptr(), st), "shake_tiles")

    def vote(i, rotate):
        k = pick(i, rotate)
        lib.check(hip.dcvc_shake_vote(tiles[k].data_ptr(), TILES, 8, 8, H, W, record[k].data_ptr(), mv[k].data_ptr(), st), "shake_vote")

    def compensate(i, rotate):
        k = pick(i, rotate)
        lib.check(hip.dcvc_me_compensate(cur[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), W, H * W, H, W, mv[k].data_ptr(), st), "me_compensate")

    def cells(i, rotate):
        k = pick(i, rotate)
        lib.check(hip.dcvc_noise_cells(cur[k].data_ptr(), WP, HP * WP, H, W, planes[k].data_ptr(), planes[k + 1].data_ptr(), ys,
                                       words[k].data_ptr(), st), "noise_cells")

    def full(i, rotate):
        k = pick(i, rotate)
        lib.check(hip.dcvc_me_search(cur[k].data_ptr(), WP, HP * WP, cur[(k + 1) % POOL].data_ptr(), WP, HP * WP, H, W, 8, 4,
                                     smv[k].data_ptr(), cost[k].data_ptr(), zero[k].data_ptr(), st), "me_search")

    for k in range(POOL):  # every plane, tile record and vector field is a picture's before the clock starts
        plane(k, True)
    planes[0].copy_(planes[POOL])
    for k in range(POOL):
        search(k, True, 8, tiles)
        vote(k, True)
    torch.cuda.synchronize(dev)
    found = record.cpu().numpy()

    variants = {}
    for where, rotate in (("one set of pictures (cache-resident)", False), ("rotating over 16 sets (HBM)", True)):
        variants[f"shake_plane, {where}"] = lambda i, r=rotate: plane(i, r)
        variants[f"shake_tiles R = 8, {where}"] = lambda i, r=rotate: search(i, r, 8)
        variants[f"shake_tiles R = 16, {where}"] = lambda i, r=rotate: search(i, r, 16)
        variants[f"shake_vote, {where}"] = lambda i, r=rotate: vote(i, r)
        variants[f"me_compensate, {where}"] = lambda i, r=rotate: compensate(i, r)
        variants[f"noise_cells, {where}"] = lambda i, r=rotate: cells(i, r)
        variants[f"me_search R = 8, {where}"] = lambda i, r=rotate: full(i, r)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, a static scene under +-4 codes of noise: {TILES} tiles, of which "
          f"{int(found[:, 2].min())} .. {int(found[:, 2].max())} vote, every vector ({int(found[:, 0].min())} .. {int(found[:, 0].max())}, "
          f"{int(found[:, 1].min())} .. {int(found[:, 1].max())}); {rounds} alternating rounds of {launches} launches between two HIP "
          f"events, us per launch: median (min .. max), bytes/s at the median")
    med = {}
    for name, t in times.items():  # (the vote moves a few kilobytes: a launch, not a stream -- no rate is given for it)
        if name.startswith("shake_vote"):
            t = np.array(t)
            med[name] = np.median(t)
            print(f"  {name:56s} {med[name]:7.2f}  ({t.min():.2f} .. {t.max():.2f})")
        else:
            med.update(timing.kernel_table({name: t}, lambda name: BYTES[name.split(",")[0]], width=56))
    for where in ("one set of pictures (cache-resident)", "rotating over 16 sets (HBM)"):
        per = sum(med[f"{k}, {where}"] for k in ("shake_tiles R = 8", "shake_vote", "me_compensate"))
        print(f"# {where}: shake_tiles R = 8 / me_search R = 8 = x{med['shake_tiles R = 8, ' + where] / med['me_search R = 8, ' + where]:.3f}, "
              f"shake_tiles R = 16 / R = 8 = x{med['shake_tiles R = 16, ' + where] / med['shake_tiles R = 8, ' + where]:.2f}, "
              f"a registered picture (tiles R = 8 + vote + compensate) {per:.2f} us = x{per / med['noise_cells, ' + where]:.2f} of noise_cells")


def shaken_clip(tmp, n, radius=6, noise=2.0, name="src.y4m"):
    """tmp/name: a camera that shakes by up to `radius` whole pixels per axis (0: a still camera) over synthetic.frames' static
    ground, under sensor noise of `noise` codes; written picture by picture.  Returns (the path, the shifts)."""
    import torch

    from vcm_ts_amd import synthetic
    from vcm_ts_amd import yuv as V

    dev, spec, y4m = torch.device("cuda:0"), V.ColorSpec(), os.path.join(tmp, name)
    m = 16
    world = torch.from_numpy(synthetic.frames(0, 1, H + 2 * m, W + 2 * m, noise=0)[0]).to(dev)
    g = np.random.default_rng(3)
    moves = [(0, 0)] + [tuple(int(v) for v in g.integers(-radius, radius + 1, 2)) for _ in range(n - 1)]
    gen = torch.Generator(device=dev).manual_seed(5)
    with V.Y4MWriter(y4m, W, H, spec, fps=(30, 1)) as wr:
        for t, (sy, sx) in enumerate(moves):
            pic = world[:, m + sy:m + sy + H, m + sx:m + sx + W] + (noise / 255.0) * torch.randn((3, H, W), device=dev, generator=gen)
            wr.write(t, V.rgb_to_yuv420(pic.clamp(0.0, 1.0)[None].contiguous(), H, W, spec).cpu().numpy())
    return y4m, moves


def boxes(n, repeats):
    import json

    import torch

    from vcm_ts_amd import motionroi as M
    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import shake as SH

    dev = torch.device("cuda:0")
    params, shake = M.MotionParams(24), SH.ShakeParams(8)
    with timing.workdir("dcvc_shake_time_") as tmp:
        for camera, radius in (("still", 0), ("shaking", 6)):
            y4m, moves = shaken_clip(tmp, n, radius, name=f"{camera}.y4m")

            def run(option):
                out = os.path.join(tmp, "found")
                shutil.rmtree(out, ignore_errors=True)
                return RC.motion_boxes_video(y4m, out, params, dev, shake=option)

            plain = run(None)  # warm-up
            steady = run(shake)  # warm-up, and what the registration found
            with open(os.path.join(tmp, "found", RC.SHAKE_JSON)) as f:
                doc = json.load(f)
            exact = sum(tuple(r[:2]) == mv for r, mv in zip(doc["records"], moves))
            rates = timing.alternating({f"{camera} camera, boxes pass": None, f"{camera} camera, boxes pass --shake 8": shake}, repeats,
                                       lambda o: timing.fps(lambda: run(o), n, dev))
            print(f"# run_codec boxes --video: {n} pictures {W}x{H} from a Y4M file of a {camera} camera (shifts within +-{radius} pixels "
                  f"per axis, sensor noise of 2 codes, nothing else moves), threshold 24, default parameters; the registration found "
                  f"{exact} of {n} vectors exactly, {doc['summary']['lost']} pictures lost, smallest agreement "
                  f"{doc['summary']['min_agree'][0]} of {doc['summary']['min_agree'][1]} voting tiles; box area a picture "
                  f"{_area(plain) / n:.0f} pixels without, {_area(steady) / n:.0f} with")
            print(f"# frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
            timing.rate_table(rates, width=40, fmt="7.2f", ratio=True)


def _area(found):
    return sum(int((b[:, 2] - b[:, 0]).astype(np.int64) @ (b[:, 3] - b[:, 1]).astype(np.int64)) for b in found if len(b))


if __name__ == "__main__":
    timing.main(__doc__, "shake_time.py", {"kernels": (kernels, (200, 5)), "boxes": (boxes, (512, 3))})
