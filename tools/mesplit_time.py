"""Vectors per 8 x 8 sub-cell in front of the temporal noise prefilter at 1920x1080 (the record in
profiles/mesplit_1080p.txt).

    python3 tools/mesplit_time.py kernels [launches=50] [rounds=5]
                                        dcvc_me_split beside dcvc_me_refine and dcvc_me_compensate_split beside
                                        dcvc_me_compensate_sub on the same pictures, alternating in one process -- once with
                                        the vectors the search and the refinement find on the synthetic clip, where almost
                                        every cell sees nine equal whole candidates, and once with random quarter-pel
                                        vectors, where every cell has nine distinct candidates and every sub-cell a vector of
                                        its own: on one set of pictures (cache-resident) and rotating over 16 sets (HBM).  HIP
                                        events around `launches` back-to-back launches, `rounds` times each
    python3 tools/mesplit_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr 8 --tnr-search 16 --tnr-subpel
                                        and with --tnr-split on top, alternating in one process

No time is fixed in advance: the yardsticks are the refinement and the cell compensation in the same process, and the
multiply-adds a launch makes when every candidate pixel is counted with its two 8-tap passes: the refinement 49 candidates x
256 pixels x 16 taps per cell, the re-selection 9 x 256 x 16 per cell with nine distinct candidates and none where nine equal
whole candidates leave one unfiltered SAD.  Bytes per launch come from the shapes: the re-selection reads 12 bytes a pixel of
cur and 12 of ref (23 x 23 / 256 times over per staged candidate, counted here for ONE), either compensation reads 12 and
writes 12.  Frames/s from a host clock around work that ends in a device synchronise.
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
R = 8
CELLS = -(-H // 16) * -(-W // 16)
MACS = {"me_refine": 49 * 256 * 16 * CELLS, "me_split random": 9 * 256 * 16 * CELLS}
KERNELS = ("me_refine", "me_split", "me_split random", "me_compensate_sub", "me_compensate_split", "me_compensate_sub random",
           "me_compensate_split random")
BYTES = {"me_refine": (12 + 12 * 24 * 24 / 256) * H * W, "me_split": 24 * H * W, "me_split random": (12 + 12 * 23 * 23 / 256) * H * W,
         "me_compensate_sub": 24 * H * W, "me_compensate_split": 24 * H * W, "me_compensate_sub random": 24 * H * W,
         "me_compensate_split random": 24 * H * W}


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
    g = torch.Generator(device="cpu").manual_seed(19)
    lim = 4 * N.MAX_R + 3
    mv = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)     # the search's vectors at R = 8 on set 0
    mvq = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)    # their refinement
    mv8 = torch.zeros(8 * hc * wc, dtype=torch.int16, device=dev)    # their re-selection
    rand = torch.randint(-lim, lim + 1, (2 * hc * wc,), generator=g, dtype=torch.int16).to(dev)   # a random vector per cell
    rand8 = torch.randint(-lim, lim + 1, (8 * hc * wc,), generator=g, dtype=torch.int16).to(dev)  # ... per sub-cell
    spare = torch.zeros(8 * hc * wc, dtype=torch.int16, device=dev)  # what the timed refinements and re-selections write
    cost = torch.empty(4 * hc * wc, dtype=torch.int32, device=dev)
    zero = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def refine(i, rotate, into=spare):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_refine(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, N.PENALTY, mv.data_ptr(),
                                     into.data_ptr(), cost.data_ptr(), st), "me_refine")

    def split(i, rotate, vectors, into=spare):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_split(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, N.PENALTY, 4, vectors.data_ptr(),
                                    into.data_ptr(), cost.data_ptr(), st), "me_split")

    def compensate_sub(i, rotate, vectors):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_compensate_sub(ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, vectors.data_ptr(), st),
                  "me_compensate_sub")

    def compensate_split(i, rotate, vectors):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_compensate_split(ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, vectors.data_ptr(), st),
                  "me_compensate_split")

    lib.check(hip.dcvc_me_search(cur[0].data_ptr(), WP, HP * WP, ref[0].data_ptr(), WP, HP * WP, H, W, R, N.PENALTY, mv.data_ptr(),
                                 cost.data_ptr(), zero.data_ptr(), st), "me_search")
    refine(0, False, mvq)
    split(0, False, mvq, mv8)
    torch.cuda.synchronize(dev)
    moved = int((mvq.view(-1, 2) != 0).any(dim=1).sum()) / CELLS
    left = (mv8.view(hc, 2, wc, 2, 2) != mvq.view(hc, 1, wc, 1, 2)).any(dim=4).view(2 * hc, 2 * wc)[:-(-H // 8), :-(-W // 8)]
    where = (", one set of pictures (cache-resident)", False), (", rotating over 16 sets (HBM)", True)
    variants = {}
    for label, rotate in where:
        variants["me_refine" + label] = lambda i, rotate=rotate: refine(i, rotate)
        variants["me_split" + label] = lambda i, rotate=rotate: split(i, rotate, mvq)
        variants["me_split random" + label] = lambda i, rotate=rotate: split(i, rotate, rand)
        variants["me_compensate_sub" + label] = lambda i, rotate=rotate: compensate_sub(i, rotate, mvq)
        variants["me_compensate_split" + label] = lambda i, rotate=rotate: compensate_split(i, rotate, mv8)
        variants["me_compensate_sub random" + label] = lambda i, rotate=rotate: compensate_sub(i, rotate, rand)
        variants["me_compensate_split random" + label] = lambda i, rotate=rotate: compensate_split(i, rotate, rand8)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, lambda = {N.PENALTY}, R = {R}: {moved:.3f} of the cells moved, "
          f"{int(left.sum()) / left.numel():.4f} of the sub-cells left their cell's vector; `random`: a random quarter-pel vector per cell "
          f"(per sub-cell for me_compensate_split); {rounds} alternating rounds of {launches} launches between two HIP events, us per "
          f"launch: median (min .. max), bytes/s at the median")
    print("# bytes per launch: " + ", ".join(f"{name} {BYTES[name]:.0f} = {BYTES[name] / (H * W):.2f} a pixel" for name in KERNELS))
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=60)
    for label, _ in where:
        r, s, sr = med["me_refine" + label], med["me_split" + label], med["me_split random" + label]
        print(f"# me_split{label}: me_split / me_refine = x{s / r:.2f} in time on the clip (no multiply-add where nine candidates agree) and "
              f"x{sr / r:.2f} with random vectors: {MACS['me_split random'] / 1e9:.2f} G multiply-adds a launch (9 candidates x 256 pixels x 16 "
              f"taps per cell), {MACS['me_split random'] / sr / 1e6:.2f} T/s, against the refinement's {MACS['me_refine'] / 1e9:.2f} G, "
              f"{MACS['me_refine'] / r / 1e6:.2f} T/s")
        c, cs = med["me_compensate_sub" + label], med["me_compensate_split" + label]
        cr, csr = med["me_compensate_sub random" + label], med["me_compensate_split random" + label]
        print(f"# me_compensate_split{label}: me_compensate_split / me_compensate_sub = x{cs / c:.2f} in time on the clip ({cs:.2f} us "
              f"against {c:.2f} us) and x{csr / cr:.2f} with random vectors ({csr:.2f} us against {cr:.2f} us)")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_mesplit_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --tnr 8 --tnr-search 16 --tnr-subpel": N.TNR(8, search=16, subpel=True),
                    "encode_video --tnr 8 --tnr-search 16 --tnr-subpel --tnr-split": N.TNR(8, search=16, subpel=True, split=True)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=64, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "mesplit_time.py", {"kernels": (kernels, (50, 5)), "encode": (encode, (32, 3))})
