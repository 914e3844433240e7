"""The measuring loop of the tools/*_time.py tools, written once: the clocks, the alternating order, the two report tables,
the clips they code, the shared codecs and the command line.  A new timing tool takes these from here and keeps only its own
docstring, constants, variants and kernel closures.

    SIZE, padded(size)                         the picture every tool measures (1080 x 1920) and its padding to 64
    event_us(fn, launches, warmup, sync)       microseconds per call between two HIP events
    fps(fn, n, device)                         n / seconds of fn() on a host clock between two device synchronises
    alternating(variants, rounds, measure)     {name: [measure(variant) per round]}, every round in dict order
    kernel_table(times, nbytes_of, width)      median (min .. max)  TB/s
    rate_table(rates, baseline, width, fmt)    mean (min .. max), each repeat, % against the first row
    y4m_clip, moving_box_clip, noisy_pool      the sources
    workdir, codec_pairs, shared_nets          a scratch folder, warm codecs, decode_video on those codecs
    main(doc, name, modes, default)            the command line

torch is imported inside the functions that need it, so a tool's usage text prints without it.
"""
import contextlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np

SIZE = (1080, 1920)  # (a module attribute so that a test can measure a smaller picture; not an option of any tool)
MIN_SIZE = (720, 1024)  # the moving box lies in rows 400..656 and travels over W - 512 columns; the fixed boxes need as much
BOX = (400, 656, 384)  # the moving rectangle: first row, last row + 1, width


def _checked(size):
    h, w = size
    if h < MIN_SIZE[0] or w < MIN_SIZE[1]:
        raise ValueError(f"timing.SIZE must be at least {MIN_SIZE[0]} x {MIN_SIZE[1]} (the moving-box clip and the fixed boxes "
                         f"need that much), got {h} x {w}")
    return h, w


def padded(size):
    """(Hp, Wp): `size` padded to multiples of 64 on the bottom and right, as stream.get_padding_size pads a picture."""
    h, w = _checked(size)
    return -(-h // 64) * 64, -(-w // 64) * 64


# -------------------------------------------------------------------------------------------------------------- clocks
def event_us(fn, launches, warmup, sync="device"):
    """Microseconds per call of fn(i), i = 0 .. launches - 1, between two HIP events, after fn(0) .. fn(warmup - 1).

    sync="device" synchronises the device after the warm-up and after the second event; sync="event" waits for the second
    event only, so the warm-up's launches are still in flight when the first event is recorded.  Which tool uses which
    (the records under profiles/ were made by these rules, and they are not the same rule):

        aq_time kernels                           warmup=min(launches, 32)  sync="device"
        motion_time, tnr_time, redact_time,       warmup=5                  sync="event"
        grain_time kernels
        picturehash_time, scale_time kernels      warmup=5                  sync="event"
        scenecut_time kernels                     warmup=0                  sync="event", launches=BATCH (20); the tool warms every
                                                                            variant up 3 times and synchronises before round 1
    """
    import torch

    assert sync in ("device", "event"), sync
    for i in range(warmup):
        fn(i)
    if sync == "device":
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    if sync == "device":
        torch.cuda.synchronize()
    else:
        b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def fps(fn, n, device):
    """n / seconds of fn() on a host clock, between two synchronises of `device`."""
    import torch

    torch.cuda.synchronize(device)
    t0 = time.time()
    fn()
    torch.cuda.synchronize(device)
    return n / (time.time() - t0)


def alternating(variants, rounds, measure):
    """{name: [measure(variants[name]) for every round]}: the variants in dict order inside every round."""
    values = {name: [] for name in variants}
    for _ in range(rounds):
        for name, v in variants.items():
            values[name].append(measure(v))
    return values


# -------------------------------------------------------------------------------------------------------------- tables
def kernel_table(times, nbytes_of, width):
    """One row per kernel variant: us per launch as median (min .. max), and nbytes_of(name) bytes at the median as
    TB/s.  Returns {name: median}."""
    med = {}
    for name, t in times.items():
        t = np.array(t)
        med[name] = np.median(t)
        print(f"  {name:{width}s} {med[name]:7.2f}  ({t.min():.2f} .. {t.max():.2f})   {nbytes_of(name) / med[name] / 1e6:6.2f} TB/s")
    return med


def rate_table(rates, baseline=None, width=28, fmt="6.2f", ratio=False):
    """One row per variant: mean (min .. max) and every repeat.  With `baseline`, the word for the first row, every
    later row ends in its mean against the first row's in per cent; with `ratio`, a closing line sets the second row
    against the first and beside the first row's own spread."""
    means = []
    for name, r in rates.items():
        a = np.array(r)
        means.append(a.mean())
        print(f"  {name:{width}s} {a.mean():{fmt}}  ({a.min():.2f} .. {a.max():.2f})   " + " ".join(f"{x:.2f}" for x in a) +
              (f"   {100 * (a.mean() / means[0] - 1):+.1f} % against {baseline}" if baseline and len(means) > 1 else ""))
    if ratio:
        a = np.array(next(iter(rates.values())))
        print(f"# with / without = x{means[1] / means[0]:.3f} in frames/s; the spread of the repeats without the option is "
              f"x{a.min() / a.mean():.3f} .. x{a.max() / a.mean():.3f} of their mean")


# ------------------------------------------------------------------------------------------------------------- sources
def y4m_clip(tmp, n, size, frames=None):
    """Write `n` pictures as tmp/src.y4m (4:2:0, through the rgb_to_yuv420 kernel) and return the path: synthetic.frames
    of seed 0, or `frames`, an (n, 3, H, W) float32 array."""
    import torch

    from vcm_ts_amd import yuv as V
    from vcm_ts_amd import synthetic

    h, w = size
    dev, spec, y4m = torch.device("cuda:0"), V.ColorSpec(), os.path.join(tmp, "src.y4m")
    rgb = synthetic.frames(0, n, h, w) if frames is None else frames
    with V.Y4MWriter(y4m, w, h, spec, fps=(30, 1)) as wr:
        for t in range(n):
            wr.write(t, V.rgb_to_yuv420(torch.from_numpy(rgb[t:t + 1]).to(dev), h, w, spec).cpu().numpy())
    return y4m


def moving_box_clip(tmp, n, size, noise):
    """A static camera under sensor noise of `noise` codes (sigma) and one 384 x 256 rectangle that moves 16 columns a
    picture, as tmp/src.y4m, with the rectangle's box per picture as pickles under tmp/root/motion_coords.  Returns
    (the Y4M path, the root)."""
    import pickle

    from vcm_ts_amd import synthetic

    h, w = _checked(size)
    y0, y1, bw = BOX
    ground = synthetic.frames(0, 1, h, w, noise=0)[0]
    g = np.random.default_rng(1)
    root = os.path.join(tmp, "root")
    os.makedirs(os.path.join(root, "motion_coords"))
    pics = np.empty((n,) + ground.shape, np.float32)
    for t in range(n):
        pics[t] = np.clip(ground + np.float32(noise / 255) * g.standard_normal(ground.shape).astype(np.float32), 0, 1)
        x = 64 + (16 * t) % (w - 512)
        pics[t, :, y0:y1, x:x + bw] = 1.0 if ground[:, y0:y1, x:x + bw].mean() < 0.5 else 0.0
        with open(os.path.join(root, "motion_coords", "%05d" % (t + 1)), "wb") as f:
            pickle.dump(np.array([[x, y0, x + bw, y1]], np.uint16), f)
    return y4m_clip(tmp, n, size, frames=pics), root


def noisy_pool(ground, size, pool=16):
    """`pool` padded pictures on ground's device: `ground` (1, 3, H, W) under +-4 codes of uniform noise, zero padding."""
    import torch

    h, w = _checked(size)
    hp, wp = padded(size)
    x = torch.zeros((pool, 3, hp, wp), device=ground.device)
    x[:, :, :h, :w] = ground + (torch.randint(-4, 5, (pool, 3, h, w), device=ground.device).float() / 255.0)
    return x


# ------------------------------------------------------------------------------------------------------ files and codecs
@contextlib.contextmanager
def workdir(prefix):
    """A scratch folder that is removed on the way out."""
    tmp = tempfile.mkdtemp(prefix=prefix)
    try:
        yield tmp
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def codec_pairs(dev, precision, streams):
    """One (I codec, P codec) pair per GOP stream, built once so that every run of a tool codes on warm codecs."""
    from vcm_ts_amd import run_codec as RC

    return [RC._nets(dev, precision) for _ in range(streams)]


@contextlib.contextmanager
def shared_nets(pair):
    """decode_video builds its codecs itself: inside this block it is handed `pair` every time."""
    from vcm_ts_amd import run_codec as RC

    made = RC._nets
    RC._nets = lambda *a, **kw: pair
    try:
        yield
    finally:
        RC._nets = made


# -------------------------------------------------------------------------------------------------------- command line
def main(doc, name, modes, default=None):
    """Run modes[mode] = (function, defaults) on the command line `mode [argument ...]`: an argument is converted to the
    type of its default (an int, or a str), and a default that is a type marks an argument that must be given.  An unknown
    mode, or none where there is no `default`, prints `doc`."""
    argv = sys.argv[1:]
    mode = argv[0] if argv else default
    if mode not in modes:
        sys.exit(doc)
    fn, defaults = modes[mode]
    given = argv[1:len(defaults) + 1]
    if any(isinstance(d, type) for d in defaults[len(given):]):
        sys.exit(doc)
    import torch

    if not torch.cuda.is_available():
        sys.exit(f"{name} measures on the GPU; none is visible")
    return fn(*[(d if isinstance(d, type) else type(d))(a) for a, d in zip(given, defaults)], *defaults[len(given):])
