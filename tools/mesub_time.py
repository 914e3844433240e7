"""Quarter-pel motion in front of the temporal noise prefilter at 1920x1080 (the record in profiles/mesub_1080p.txt).

    python3 tools/mesub_time.py kernels [launches=50] [rounds=5]
                                        dcvc_me_refine beside dcvc_me_search at R = 8, and dcvc_me_compensate_sub (with the
                                        refined vectors, and with whole vectors only) beside dcvc_me_compensate, on the same
                                        pictures, alternating in one process: on one set of pictures (cache-resident) and
                                        rotating over 16 sets (HBM).  HIP events around `launches` back-to-back launches,
                                        `rounds` times each
    python3 tools/mesub_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr 8 --tnr-search 16 and with
                                        --tnr-subpel on top, alternating in one process

No time is fixed in advance: the yardsticks are the two whole-pel kernels in the same process, and for the refinement the
multiply-adds a launch makes when every candidate pixel is counted with its two 8-tap passes: 49 candidates x 256 pixels x 16
taps per cell.  (The kernel makes the horizontal pass once per position, not per candidate, so it makes fewer.)  Bytes per
launch come from the shapes: the refinement reads 12 bytes a pixel of cur and 12 of ref, 24 x 24 / 256 times over for the window
of every cell; either compensation reads 12 and writes 12, the interpolating one 23 x 23 / 256 times over in a fractional
cell.  Frames/s from a host clock around work that ends in a device synchronise.
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
MACS = 49 * 256 * 16 * CELLS
BYTES = {"me_search R=8": (12 + 12 * (16 + 2 * R) * (16 + 4 * ((2 * R + 1 + 3) // 4)) / 256) * H * W,
         "me_refine": (12 + 12 * 24 * 24 / 256) * H * W, "me_compensate": 24 * H * W, "me_compensate_sub": 24 * H * W,
         "me_compensate_sub whole": 24 * H * W}


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
    mv = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)     # the search's vectors at R = 8 on set 0
    mvq = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)    # their refinement
    whole = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)  # 4 mv: the same motion without a fraction
    spare = torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev)  # what the timed searches and refinements write
    cost = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    zero = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def search(i, rotate, into=spare):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_search(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, R, N.PENALTY,
                                     into.data_ptr(), cost.data_ptr(), zero.data_ptr(), st), "me_search")

    def refine(i, rotate, into=spare):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_refine(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, N.PENALTY, mv.data_ptr(),
                                     into.data_ptr(), cost.data_ptr(), st), "me_refine")

    def compensate(i, rotate):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_compensate(ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, mv.data_ptr(), st),
                  "me_compensate")

    def compensate_sub(i, rotate, vectors):
        k = i % POOL if rotate else 0
        lib.check(hip.dcvc_me_compensate_sub(ref[k].data_ptr(), WP, HP * WP, out[k].data_ptr(), WP, HP * WP, H, W, vectors.data_ptr(), st),
                  "me_compensate_sub")

    search(0, False, mv)
    refine(0, False, mvq)
    whole.copy_(4 * mv)
    torch.cuda.synchronize(dev)
    moved = int((mvq.view(-1, 2) != 0).any(dim=1).sum()) / CELLS
    frac = int((mvq.view(-1, 2) & 3 != 0).any(dim=1).sum()) / CELLS
    where = (", one set of pictures (cache-resident)", False), (", rotating over 16 sets (HBM)", True)
    variants = {}
    for label, rotate in where:
        variants["me_search R=8" + label] = lambda i, rotate=rotate: search(i, rotate)
        variants["me_refine" + label] = lambda i, rotate=rotate: refine(i, rotate)
        variants["me_compensate" + label] = lambda i, rotate=rotate: compensate(i, rotate)
        variants["me_compensate_sub" + label] = lambda i, rotate=rotate: compensate_sub(i, rotate, mvq)
        variants["me_compensate_sub whole" + label] = lambda i, rotate=rotate: compensate_sub(i, rotate, whole)
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, lambda = {N.PENALTY}, R = {R}: {moved:.3f} of the cells moved, {frac:.3f} by a "
          f"fraction; {rounds} alternating rounds of {launches} launches between two HIP events, us per launch: median (min .. max), "
          f"bytes/s at the median")
    print("# bytes per launch: " + ", ".join(f"{name} {BYTES[name]:.0f} = {BYTES[name] / (H * W):.2f} a pixel" for name in BYTES))
    med = timing.kernel_table(times, lambda name: BYTES[name.split(",")[0]], width=60)
    for label, _ in where:
        t = med["me_refine" + label]
        print(f"# me_refine{label}: {MACS / 1e9:.2f} G multiply-adds a launch (49 candidates x 256 pixels x 16 taps per cell), "
              f"{MACS / t / 1e6:.2f} T/s; me_refine / me_search R=8 = x{t / med['me_search R=8' + label]:.2f} in time")
        print(f"# me_compensate_sub{label}: {med['me_compensate_sub' + label]:.2f} us against {med['me_compensate' + label]:.2f} us of me_compensate; "
              f"me_compensate_sub / me_compensate = x{med['me_compensate_sub' + label] / med['me_compensate' + label]:.2f} "
              f"in time, with whole vectors only x{med['me_compensate_sub whole' + label] / med['me_compensate' + label]:.2f}")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_mesub_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --tnr 8 --tnr-search 16": N.TNR(8, search=16),
                    "encode_video --tnr 8 --tnr-search 16 --tnr-subpel": N.TNR(8, search=16, subpel=True)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=52, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "mesub_time.py", {"kernels": (kernels, (50, 5)), "encode": (encode, (32, 3))})
