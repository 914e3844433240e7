"""The hierarchical motion search in front of the temporal noise prefilter at 1920x1080 (the record in
profiles/mepyr_1080p.txt).

    python3 tools/mepyr_time.py kernels [launches=50] [rounds=5]
                                        dcvc_me_pyramid, then dcvc_me_coarse and dcvc_me_descend at (levels, R) = (2, 32),
                                        (1, 64) and (2, 128), the chain's total (two pyramids, the coarse search and the
                                        descents, as TnrFilter launches them in place of one dcvc_me_search) and
                                        dcvc_me_search at R = 32 (the yardstick) on the same pictures, alternating in one
                                        process, rotating over 16 sets of pictures (HBM).  HIP events around `launches`
                                        back-to-back launches, `rounds` times each
    python3 tools/mepyr_time.py encode [n_frames=32] [repeats=3]
                                        frames/s of encode_video from a Y4M file with --tnr 8 --tnr-search 32 and with
                                        --tnr 8 --tnr-search 32 --tnr-levels 2, alternating in one process

Two yardsticks, neither a time fixed in advance: dcvc_me_search at R = 32 in the same process and rounds, and the count of
byte differences a chain makes: (2 R_L + 1)^2 H W / 4 for the coarse search (64 samples a cell at either level: at level 1
the cell's own, at level 2 an 8 x 8 block around its 4 x 4) and 26 H W + 10 H W / 4 for the descents, against (2 R + 1)^2 H W
for the full search.  Bytes per launch come from the shapes: the pyramid reads 12 bytes a pixel and writes 1 + 1/4 + 1/16.
Frames/s from a host clock around work that ends in a device synchronise.
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
CASES = ((2, 32), (1, 64), (2, 128))  # (levels, R)
FULL = 32  # the full search's radius beside them


def differences(levels, R):
    """The byte differences of a chain: the coarse search's (2 R_L + 1)^2 candidates of 64 samples a cell, 26 candidates of
    256 in the descent to level 0 and, with two levels, 10 of 64 in the descent to level 1."""
    RL = -(-R // (1 << levels))
    return ((2 * RL + 1) ** 2 * 64 + 26 * 256 + (levels - 1) * 10 * 64) * (-(-H // 16) * -(-W // 16))


def nbytes(name):
    """What a call reads and writes, from the shapes: the pyramid 12 bytes a pixel in and 1 + 1/4 + 1/16 out; per cell the
    coarse search its 64 samples and their window, a descent its block of cur, of ref at (0, 0) and the candidates' window."""
    cells, pyr = -(-H // 16) * -(-W // 16), (12 + 1 + 1 / 4 + 1 / 16) * H * W
    if name.startswith("me_pyramid"):
        return pyr
    if name.startswith("me_search"):
        return 24.0 * H * W
    levels, R = (int(part[2:]) for part in name.split(" ")[1:])
    RL = -(-R // (1 << levels))
    coarse = cells * (64 + (8 + 2 * RL) * (8 + 4 * ((2 * RL + 1 + 3) // 4)))
    descents = cells * (256 + (20 + 16) * 24 + 4 + (levels - 1) * (64 + (10 + 8) * 16 + 4))
    return {"me_coarse": coarse, "me_descend": descents, "chain": 2 * pyr + coarse + descents}[name.split(" ")[0]]


def kernels(launches, rounds):
    import torch

    from vcm_ts_amd import lib
    from vcm_ts_amd import tnr as N
    from vcm_ts_amd.engine import _raw_stream
    from vcm_ts_amd.roi import grid_of
    from vcm_ts_amd.synthetic import frames

    dev = torch.device("cuda:0")
    ground = torch.from_numpy(frames(0, 1, H, W)).to(dev)

    # a static scene under +-4 codes of noise; in cur a band of rows stands 40 columns further right than in ref
    cur, ref = (timing.noisy_pool(ground, (H, W), POOL) for _ in range(2))
    y0, y1, _ = timing.BOX
    cur[:, :, y0:y1, 40:W] = ref[:, :, y0:y1, :W - 40]
    hc, wc = grid_of(H, W)

    def planes():  # the byte planes of one picture: levels 0, 1, 2, rows padded to 4 bytes
        sides, out = (H, W), []
        for _ in range(3):
            out.append(torch.empty((sides[0], -(-sides[1] // 4) * 4), dtype=torch.uint8, device=dev))
            sides = (-(-sides[0] // 2), -(-sides[1] // 2))
        return out

    yc, yr = [planes() for _ in range(POOL)], [planes() for _ in range(POOL)]
    vec = [torch.zeros(2 * hc * wc, dtype=torch.int16, device=dev) for _ in range(3)]
    cost = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    zero = torch.empty(hc * wc, dtype=torch.int32, device=dev)
    st, hip = C.c_void_p(_raw_stream(dev.index)), lib.hip()

    def pyramid(i, levels=2, which=None):
        k = i % POOL
        for pic, y in ((cur, yc), (ref, yr)) if which is None else (which,):
            lib.check(hip.dcvc_me_pyramid(pic[k].data_ptr(), WP, HP * WP, H, W, levels, y[k][0].data_ptr(), y[k][0].shape[1], y[k][1].data_ptr(),
                                          y[k][1].shape[1], y[k][2].data_ptr(), y[k][2].shape[1], st), "me_pyramid")

    def coarse(i, levels, R):
        k = i % POOL
        lib.check(hip.dcvc_me_coarse(yc[k][levels].data_ptr(), yc[k][levels].shape[1], yr[k][levels].data_ptr(), yr[k][levels].shape[1], H, W, R,
                                     levels, N.PENALTY, vec[levels].data_ptr(), st), "me_coarse")

    def descend(i, levels, R):
        k = i % POOL
        for level in range(levels - 1, -1, -1):
            lib.check(hip.dcvc_me_descend(yc[k][level].data_ptr(), yc[k][level].shape[1], yr[k][level].data_ptr(), yr[k][level].shape[1], H, W, R,
                                          levels, level, N.PENALTY, vec[level + 1].data_ptr(), vec[level].data_ptr(), cost.data_ptr(),
                                          zero.data_ptr(), st), "me_descend")

    def chain(i, levels, R):
        pyramid(i, levels)
        coarse(i, levels, R)
        descend(i, levels, R)

    def search(i):
        k = i % POOL
        lib.check(hip.dcvc_me_search(cur[k].data_ptr(), WP, HP * WP, ref[k].data_ptr(), WP, HP * WP, H, W, FULL, N.PENALTY, vec[0].data_ptr(),
                                     cost.data_ptr(), zero.data_ptr(), st), "me_search")

    for i in range(POOL):  # every set's planes, and vectors of every level for the descents timed on their own
        chain(i, 2, 128)
    torch.cuda.synchronize(dev)
    found = int((vec[0].view(-1, 2) != 0).any(dim=1).sum()) / (-(-H // 16) * -(-W // 16))
    variants = {"me_pyramid (one picture)": lambda i: pyramid(i, 2, (cur, yc))}
    for levels, R in CASES:
        tag = f" L={levels} R={R}"
        variants["me_coarse" + tag] = lambda i, a=(levels, R): coarse(i, *a)
        variants["me_descend" + tag] = lambda i, a=(levels, R): descend(i, *a)
        variants["chain" + tag] = lambda i, a=(levels, R): chain(i, *a)
    variants[f"me_search R={FULL}"] = search
    times = timing.alternating(variants, rounds, lambda fn: timing.event_us(fn, launches, warmup=5, sync="event"))
    print(f"# {W}x{H} crops of {WP}x{HP} padded pictures, lambda = {N.PENALTY}, {found:.3f} of the cells moved at L = 2, R = 128, rotating over "
          f"{POOL} sets of pictures (HBM); {rounds} alternating rounds of {launches} calls between two HIP events, us per call: median "
          f"(min .. max), bytes/s at the median.  me_descend is both descents where L = 2; chain is pyramid(cur), pyramid(ref), coarse, descents")
    med = timing.kernel_table(times, nbytes, width=40)
    full = med[f"me_search R={FULL}"]
    for levels, R in CASES:
        tag = f" L={levels} R={R}"
        d = differences(levels, R)
        print(f"# chain{tag}: {d / 1e9:.3f} G byte differences in the coarse search and the descents ({(2 * FULL + 1) ** 2 * H * W / d:.1f} times fewer than "
              f"me_search R={FULL}'s), {med['me_coarse' + tag]:.2f} + {med['me_descend' + tag]:.2f} us behind the pyramids; "
              f"chain / me_search R={FULL} = x{med['chain' + tag] / full:.2f} in time")


def encode(n, repeats):
    import torch

    from vcm_ts_amd import run_codec as RC
    from vcm_ts_amd import tnr as N

    dev = torch.device("cuda:0")
    with timing.workdir("dcvc_mepyr_time_") as tmp:
        y4m, _ = timing.moving_box_clip(tmp, n, (H, W), noise=2)  # a static camera, sensor noise and one moving rectangle
        nets = timing.codec_pairs(dev, None, 1)[0]
        variants = {"encode_video --tnr 8 --tnr-search 32": N.TNR(8, search=32),
                    "encode_video --tnr 8 --tnr-search 32 --tnr-levels 2": N.TNR(8, search=32, levels=2)}

        def run(tnr):
            out = os.path.join(tmp, "bins")
            shutil.rmtree(out, ignore_errors=True)
            return RC.encode_video(y4m, out, gop=32, nets=nets, tnr=tnr)[0]

        bits = {name: sum(run(tnr)) for name, tnr in variants.items()}  # warm-up
        rates = timing.alternating(variants, repeats, lambda tnr: timing.fps(lambda: run(tnr), n, dev))
        print(f"# encode_video: {n} pictures {W}x{H} from a Y4M file, GOP 32, one GOP stream, seeded synthetic weights (the bits "
              f"mean nothing: {bits}); frames/s, {repeats} alternating repeats after one warm-up each: mean (min .. max)")
        timing.rate_table(rates, width=56, fmt="7.2f", ratio=True)


if __name__ == "__main__":
    timing.main(__doc__, "mepyr_time.py", {"kernels": (kernels, (50, 5)), "encode": (encode, (32, 3))})
