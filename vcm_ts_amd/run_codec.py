"""Folder-level encode / decode: the base-layer loop of the reference's
``video_coder.run_dcvc`` (/root/reference/video_coder.py:80-155) and its PNG conventions
(DCVC_HEM/src/utils/png_reader.py:10-46, stream_helper.py:148-153) on the MI355X path.

    python -m vcm_ts_amd.run_codec encode --frames DIR --bins DIR [--recon DIR] [--gop 32] [--q 1.0 1.0 1.0] [--report JSON]
    python -m vcm_ts_amd.run_codec decode --bins DIR --recon DIR --height H --width W
    python -m vcm_ts_amd.run_codec encode --video FILE.y4m --bins DIR [--recon-video FILE.y4m] [--report JSON]
    python -m vcm_ts_amd.run_codec encode --video FILE.yuv --size 1920x1080 [--bit-depth 10] [--fps 50] --bins DIR
    python -m vcm_ts_amd.run_codec decode --bins DIR --recon-video FILE.y4m
    python -m vcm_ts_amd.run_codec encode ... --roi-root DIR [--plate-border N] [--face-border N] [--residuals FILE.gbrp | DIR]
    python -m vcm_ts_amd.run_codec decode ... --roi-root DIR --residuals FILE.gbrp | DIR
    python -m vcm_ts_amd.run_codec encode ... --roi-root DIR --residual-bins DIR [--residual-step S]
    python -m vcm_ts_amd.run_codec decode ... --roi-root DIR --residual-bins DIR
    python -m vcm_ts_amd.run_codec encode ... --scenecut T [--min-gop N]
    python -m vcm_ts_amd.run_codec encode ... --roi-root DIR [--plate-q F] [--face-q F] [--background-q F] [--roi-q-grow N]
    python -m vcm_ts_amd.run_codec encode ... --report JSON --bit-map [DIR]
    python -m vcm_ts_amd.run_codec encode ... --picture-hash
    python -m vcm_ts_amd.run_codec decode ... [--verify strict|pixels|warn|off]
    python -m vcm_ts_amd.run_codec verify --bins DIR --recon DIR
    python -m vcm_ts_amd.run_codec encode ... --base-scale N/D
    python -m vcm_ts_amd.run_codec decode ... [--base-only]
    python -m vcm_ts_amd.run_codec encode ... --aq-strength A [--aq-clamp LO HI]
    python -m vcm_ts_amd.run_codec boxes (--frames DIR | --video FILE [--size WxH]) --out ROOT --threshold T [--learn KB KF]
                                         [--min-pixels P] [--grow G] [--min-cells C] [--max-boxes N]
    python -m vcm_ts_amd.run_codec encode ... --roi-root ROOT [--motion-border N] [--motion-q F]
    python -m vcm_ts_amd.run_codec encode ... --tnr T [--tnr-floor W] [--tnr-pixel P] [--tnr-search R [--tnr-penalty L] [--tnr-subpel] [--tnr-split] [--tnr-levels L]]
    python -m vcm_ts_amd.run_codec encode ... --tnr T --tnr-intra K
    python -m vcm_ts_amd.run_codec encode ... --tnr-auto [K] [--tnr-auto-min-cells N] [every --tnr-* option]
    python -m vcm_ts_amd.run_codec noise (--frames DIR | --video FILE) [--out FILE] [--max-frames N] [--min-cells N] [--scale K]
    python -m vcm_ts_amd.run_codec shake (--frames DIR | --video FILE) --radius R [--min-votes N] [--out FILE] [--max-frames N]
    python -m vcm_ts_amd.run_codec encode ... --tnr T --grain [--grain-min-samples N]
    python -m vcm_ts_amd.run_codec decode ... --grain [PERCENT]
    python -m vcm_ts_amd.run_codec encode ... --roi-root ROOT --redact NAME [NAME ...] (--redact-tile N | --redact-fill K)
                                              [--redact-grow G] [--redact-hold N] [--redact-restorable]

Video files are Y4M or raw I420 at 8 or 10 bits (vcm_ts_amd/yuv.py): no PNG detour, the colour conversion runs on the
GPU (include/dcvc_hip_color.h), and `encode --video` leaves a `sequence.json` beside the `.bin` files from which
`decode --recon-video` takes size, frame rate and colour description.

With a ROI (vcm_ts_amd/roi.py: the reference's box files under --roi-root) `encode` also writes the residual layer of
``video_coder.compute_residuals`` -- raw gbrp planes for an external encoder, or PNGs -- and `decode` fuses a decoded
residual layer into its output as ``fuse_layers`` does; the .bin files are the same with or without.

With --residual-bins DIR the residual layer is also CODED on the GPU (vcm_ts_amd/roilayer.py: a box-local coder, lossless at
--residual-step 1, within S // 2 of every sample at step S; not HEVC): one im%05d.rl per picture, which `decode
--residual-bins DIR` decodes and fuses in place of a --residuals file.  --report then states the layer's and the total bpp.

With --scenecut T an I picture also opens a new GOP wherever consecutive pictures differ by more than T
(vcm_ts_amd/scenecut.py: a scan pass over the source first, then the coding pass); --gop becomes the longest GOP, and the
I pictures are listed in a `gops.json` beside the `.bin` files, which `decode` follows when it is there.  There is no
default T.

With --plate-q / --face-q / --background-q F (and a ROI) the base layer itself quantises its latent y with a step that
varies per 16x16-pixel cell: F times the picture's step in the cells a plate / face box touches, the background's factor
elsewhere (vcm_ts_amd/roi.py RoiQ, q_map).  The .bin format is unchanged; the factors go to a `roiq.json` beside the .bin
files, and `decode` then needs the same boxes (--roi-root) to rebuild the maps.  There are no defaults other than 1.00.

With --bit-map the report also says where the bits of every picture went (vcm_ts_amd/bitmap.py: the code lengths of the
coder's own symbols, summed per 16x16-pixel cell on the GPU): per component, and with a ROI inside and outside the
boxes; with a DIR the per-cell maps are written there as im%05d.npy.  The .bin files are the same with or without.

With --picture-hash `encode` leaves a `hashes.json` beside the `.bin` files: two CRC-32 digests per coded picture, taken on
the GPU from the encoder's own reconstruction (vcm_ts_amd/picturehash.py) -- `pixels`, of the 8-bit picture a viewer sees,
and `state`, of the fp32 reference picture the next one is predicted from.  `decode` follows the file when it is there and
stops at the first picture it rebuilds differently (--verify); `verify` holds a folder of decoded PNGs against it on the host
alone.  The .bin files are the same with or without.

With --base-scale N/D (1/4 <= N/D < 1) the base layer is coded at reduced size: every picture is scaled down on the GPU before
the codec sees it and the reconstruction is scaled up again for everything that looks at it (vcm_ts_amd/scale.py: a separable
Lanczos-3 with integer taps whose arithmetic is part of the interface, so that encoder and decoder rebuild the same full-size
picture bit for bit and the residual layer stays lossless).  The .bin files are an ordinary sequence of base-size pictures; a
`scale.json` beside them says how they are scaled up, which `decode` follows (`decode --base-only` ignores it and writes the
base-size pictures).  Reports, residuals, boxes, --target-bpp, --height / --width and sequence.json all speak of the full size.

With --aq-strength A (hundredths of a QP per doubling of a cell's variance, 1 .. 400) every P picture is coded under a q-scale
map made on the GPU from its own reference picture (vcm_ts_amd/aq.py: backward-adaptive quantisation, an integer function of the
picture's 8-bit codes): cells flatter than the reference's mean get a finer step of the latent y, busier ones a coarser one.  The
decoder holds the same reference picture and rebuilds the map: the .bin format is unchanged and nothing is stored per picture; an
`aq.json` beside the .bin files carries the setting, which `decode` follows without any option.  I pictures are not adapted.
There is no tuned value.

`boxes` makes a --roi-root from the source alone (vcm_ts_amd/motionroi.py: a background model of the luma on the GPU, a
scan pass of its own like --scenecut's, boxes around the 16x16 cells that differ from the model): ROOT/motion_coords/%05d
in the reference's coordinate format and ROOT/motion.json.  A root that holds motion_coords has a third box class, "motion",
with --motion-border and --motion-q beside the plates' and faces' options; without the folder nothing changes.  There is no
default T, the other parameters are untuned placeholders, and nothing is claimed about detection quality.

With --tnr T (1 .. 64 luma codes) the codec is handed a temporally filtered picture in place of every P picture
(vcm_ts_amd/tnr.py: a motion-adaptive noise prefilter for fixed-camera content, one kernel per picture on the GPU): the source
blended with the previous filtered picture wherever their luma differs by fewer than T codes on average over a 5x5 window, the
source itself wherever something moves.  The filter restarts at every I picture.  It is encoder side only: the .bin format is
unchanged, no file is written and `decode` needs nothing; --report keeps measuring against the unfiltered source and gains
`tnr`, `frame_tnr_held` and `frame_tnr_mad`.  There is no default T (--tnr-auto measures one, below), --tnr-floor and
--tnr-pixel are untuned placeholders, and nothing is claimed about rate or quality.  Motion compensation is opt-in: with --tnr-search R (1 .. 32 pixels) every 16x16 cell
of a P picture is searched for in the previous filtered picture (whole-pixel full search on luma SAD plus --tnr-penalty codes
per pixel of vector length, default 4, untuned), that picture is moved cell by cell and the blend runs against the moved
picture: three kernels per P picture.  --report then also gains `frame_tnr_moved` and `frame_tnr_mad_zero`.
With --tnr-subpel (opt-in, belongs to --tnr-search) every vector is refined to quarter pixels and the previous filtered
picture is moved through a 7/8-tap interpolation filter (vcm_ts_amd/tnr.py): four kernels per P picture, and
--report gains `frame_tnr_subpel`, the cells whose vector has a fractional component.
With --tnr-split (opt-in, belongs to --tnr-search, with or without --tnr-subpel) every 8 x 8 quarter of a cell chooses again
among its own cell's vector and the eight neighbours' and the previous filtered picture is moved sub-cell by sub-cell
(vcm_ts_amd/tnr.py): one more kernel per P picture, and --report gains `frame_tnr_split`, the sub-cells whose
vector differs from their cell's.
With --tnr-levels L (1 or 2; opt-in, belongs to --tnr-search) the search is hierarchical and R may be 2 .. 64 (L = 1) or
4 .. 128 (L = 2): the luma of both pictures is reduced to L coarser levels of 2 x 2 means, the coarsest is searched
exhaustively and every level below chooses among the few vectors around twice the level above's and (0, 0)
(vcm_ts_amd/tnr.py): 3 + L more kernels per P picture, and --report gains `frame_tnr_far`, the cells whose
vector has a component beyond 32.  Fine texture defeats it (the means alias it), nothing is tuned, and --tnr-subpel and
--tnr-split stop at R = 32 until their kernels are widened.
With --tnr-intra K (1 .. 4; opt-in, no default, untuned) the I picture is filtered too: it is blended in one pass (one
dcvc_tnr_fuse launch) with up to K pictures that FOLLOW it in its own GOP -- never a picture of another GOP, so GOP streams,
shards and scene cuts keep the bytes of sequential coding -- each searched for and moved onto it first with --tnr-search, and
the recursive filter starts from the filtered I picture.  A GOP of one picture is left as it is.  --report's figures are then
nonzero for such I pictures (against the picture that follows) and it gains `frame_tnr_refs`.  With --grain the I picture is
measured too and `decode --grain` grains I pictures exactly when grain.json's `tnr` entry says `intra`.  Nothing is claimed
about rate or quality.

With --tnr-auto [K] in place of --tnr T the threshold is MEASURED (vcm_ts_amd/noise.py): a scan pass over the
whole source before anything is coded -- the --scenecut scan's own pass where that is given too -- takes per 16x16 cell the mean
absolute luma difference of consecutive pictures (two kernels on the GPU), the lower quartile of the cells is the noise level,
and T = ceil(K x that level) clamped to 1 .. 64 (K within 0.50 .. 16.00, default 3.0; K and --tnr-auto-min-cells, the counted
cells an estimate needs, default 1024, are untuned placeholders).  Every --tnr-* option and --grain belong to either.  The
.bin files are those of --tnr T; noise.json beside them and --report's `noise` hold the estimate and the chosen T.  Fixed
camera only: a pan is measured as noise and nothing warns of it (but see --shake below).  A source without an estimate is refused: pass --tnr T.
`run_codec noise` is the scan alone and prints the same JSON.

With --shake R (boxes, noise, encode --tnr-auto; vcm_ts_amd/shake.py) a camera that is fixed but SHAKES by up to R
whole pixels is steadied ahead of those scans: picture 0 is the anchor, every later picture is searched for in its luma (a
2-D search on a sparse sample of every 64x64 tile, a median vote over the tiles: two kernels) and moved onto it by the one
vector found (dcvc_me_compensate) before the scan sees it.  shake.json holds a record per picture; a picture with too few
votes (--shake-min-votes, default 8, an untuned placeholder) or a vector at +-R is LOST and passed on unmoved, and a source
with more than a quarter of its pictures lost is refused by the noise scan: the camera moves, pass --tnr T.  The coding pass
is not touched (--tnr-search finds the shake cell by cell), the scene-cut scan keeps the unregistered pictures.  Whole pixels,
translation only, no re-anchoring.  `run_codec shake` is the registration alone and prints the JSON.  Without the option
nothing changes.
With --tnr T --grain the encoder also measures what the filter took out of every P picture (vcm_ts_amd/grain.py: one more
kernel per P picture, right behind the filter's) and leaves grain.json beside the .bin files: per GOP eight strengths by
intensity, two taps and the sample counts.  Every other output is that of an encode without the option.  `decode --grain
[PERCENT]` (1 .. 200, default 100) re-synthesises noise of that strength and shape on every P picture it writes: opt-in, never
followed silently, display side only.  --verify keeps checking the ungrained picture; a grained folder deliberately does not
pass `verify`, whose digests are of the ungrained picture.  P pictures only, achromatic, a 3-tap separable shape, per-GOP
parameters; --grain-min-samples is an untuned placeholder and nothing is claimed about rate, quality or detection.

With --redact NAME ... (and a ROI) the codec is handed every picture with the boxes of the named classes made unreadable
(vcm_ts_amd/redact.py: one kernel per picture that has such a box): a mosaic of N x N tiles on a picture-aligned grid
(--redact-tile N), or a solid fill (--redact-fill K); neither has a default.  It is encoder side only: the .bin format is
unchanged and `decode` needs nothing; a `redact.json` beside the .bin files tells a receiver; --report keeps measuring against
the unredacted source and gains `redact` and `frame_redacted`.  --residuals / --residual-bins would hold what was removed and
are refused beside it unless --redact-restorable says that this is wanted.  A mosaic is not a security guarantee, boxes are
taken as given (--redact-hold narrows, not closes, the gap a detector leaves), and nothing is claimed about rate or quality.

Frames are ``im1.png`` / ``im00001.png`` ...; coded pictures are ``im00001.bin`` ... in the
reference's `.bin` format (an I picture every `gop` frames).  Unlike run_dcvc the encoder does not
run the decoder: its own reconstruction is bit-identical to what `decode` produces.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import stream as S
from .goplog import GopLog
from .scenecut import GopPlan
from .pipeline import ConcurrentGopEncoder, decode_picture, pad_frame


class PNGReader:
    """im1.png or im00001.png naming, RGB float32 in [0, 1], (3, H, W)."""

    def __init__(self, folder):
        names = os.listdir(folder)
        if "im1.png" in names:
            self.width = 1
        elif "im00001.png" in names:
            self.width = 5
        else:
            raise ValueError("unknown image naming convention; expected im1.png or im00001.png")
        self.folder, self.index = folder, 1

    def path_of(self, index):
        return os.path.join(self.folder, f"im{str(index).zfill(self.width)}.png")

    @staticmethod
    def load_u8(path):
        """(H, W, 3) uint8"""
        from PIL import Image  # (here, not at the top: the video path never touches PNGs)

        return np.asarray(Image.open(path).convert("RGB"))

    @staticmethod
    def load(path):
        return PNGReader.load_u8(path).astype("float32").transpose(2, 0, 1) / 255.0

    def read_one_frame(self):
        path = self.path_of(self.index)
        if not os.path.exists(path):
            return None
        self.index += 1
        return self.load(path)

    def sequential(self):
        while (f := self.read_one_frame()) is not None:
            yield f

    def prefetching(self, workers=6, depth=12, raw=False):
        """Iterate over the remaining frames with `workers` threads decoding up to `depth` PNGs ahead (PIL and numpy
        release the GIL while they decode / convert; a 1920x1080 PNG costs 40-140 ms on one host thread, more than the
        GPU needs to code the picture).  Same arrays in the same order as read_one_frame(); raw=True: the (H, W, 3)
        uint8 pixels instead (u8_to_unit_float turns them into the same floats on the device)."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=workers) as pool:
            pending = deque()
            while True:
                while len(pending) < depth:
                    path = self.path_of(self.index)
                    if not os.path.exists(path):
                        break
                    self.index += 1
                    pending.append(pool.submit(self.load_u8 if raw else self.load, path))
                if not pending:
                    return
                yield pending.popleft().result()


_LUT = {}


def u8_to_unit_float(u8: torch.Tensor):
    """(H, W, 3) uint8 on a device -> (1, 3, H, W) float32 with exactly the reference's values (png_reader.py: uint8 ->
    float32, / 255.0 on the host): a 256-entry table of those host-computed quotients, so that no device division
    (which torch may turn into a multiplication by a reciprocal) is involved.  4x fewer bytes cross PCIe."""
    lut = _LUT.get(u8.device)
    if lut is None:
        lut = _LUT[u8.device] = torch.from_numpy(np.arange(256).astype("float32") / 255.0).to(u8.device)
    return lut[u8.to(torch.int64)].permute(2, 0, 1)[None].contiguous()


def _save_array(a, path):
    from PIL import Image

    Image.fromarray(np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)).save(path)


def _save_u8(a, path):
    from PIL import Image

    Image.fromarray(a).save(path)


class PNGWriters:
    """A bounded pool of PNG-encoding threads: at most 2 x workers pictures (25 MB of float32 each at 1080p) wait in
    host memory, and a failed write (disk full, bad path) surfaces in the caller -- at the next save or at close() --
    instead of being dropped with its future.  workers == 0: write inline, as the reference does."""

    def __init__(self, workers):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        self.pool = ThreadPoolExecutor(max_workers=workers) if workers > 0 else None
        self.pending, self.limit = deque(), 2 * max(workers, 1)

    def submit(self, a, path, save=_save_array):
        if self.pool is None:
            return save(a, path)
        while len(self.pending) >= self.limit:
            self.pending.popleft().result()  # re-raises a writer's exception
        self.pending.append(self.pool.submit(save, a, path))

    def close(self):
        try:
            while self.pending:
                self.pending.popleft().result()
        finally:
            if self.pool is not None:
                self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.close()
        elif self.pool is not None:  # already failing: do not mask the first error with a writer's
            self.pool.shutdown(wait=True, cancel_futures=True)


def save_torch_image(img: torch.Tensor, path, writers: PNGWriters = None):
    """stream_helper.py:148-153.  writers: a PNGWriters pool that takes the PNG encoding (the device -> host copy still
    happens here, while the tensor is valid)."""
    a = img.squeeze(0).permute(1, 2, 0).detach().cpu().numpy()
    if writers is None:
        _save_array(a, path)
    else:
        writers.submit(a, path)


def _nets(device, precision, i_ckpt=None, p_ckpt=None):
    from .dmc import DMC
    from .intra import IntraNoAR

    i_net, p_net = IntraNoAR(precision=precision), DMC(precision=precision)
    if i_ckpt:
        i_net.load_state_dict(S.get_state_dict(i_ckpt), strict=False)
    if p_ckpt:
        p_net.load_state_dict(S.get_state_dict(p_ckpt), strict=False)
    return i_net.to(device).eval(), p_net.to(device).eval()


def interpolate_log(min_val, max_val, num, decending=True):
    """DCVC_HEM/src/utils/common.py:23-31: `num` values spaced evenly in log(q) between the two anchors."""
    import numpy as np

    assert max_val > min_val > 0
    lo, hi = np.log(min_val), np.log(max_val)
    return np.exp(np.linspace(hi, lo, num) if decending else np.linspace(lo, hi, num))


def rate_point_q_scales(i_q_scales, y_q_scales, mv_y_q_scales, rate_count, quality):
    """video_coder.py:181-197: the (I, mv_y, y) q-scales of rate point `quality` out of `rate_count` points interpolated
    in log space between the first (coarsest) and the last (finest) anchor a model was trained with.  The arguments
    are the flattened q_scale tensors of the checkpoints (IntraNoAR.get_q_scales_from_ckpt / DMC.get_q_scales_from_ckpt)
    or of the live modules.  Returns (q_i, q_mv_y, q_y) in the order encode_folder takes them."""
    if not 0 <= quality < rate_count:
        raise ValueError(f"quality must be in [0, {rate_count})")
    pick = lambda qs: float(interpolate_log(float(qs[-1]), float(qs[0]), rate_count)[quality])
    return pick(i_q_scales), pick(mv_y_q_scales), pick(y_q_scales)


def rd_report(frame_types, bits, psnrs, msssims, frame_pixel_num):
    """The per-sequence RD log of the reference's test harness (DCVC_HEM/src/utils/common.py:63-112, same keys): per
    picture bpp / PSNR / MS-SSIM and their averages over the I pictures (type 0), the P pictures (type 1) and all."""
    out = {"frame_pixel_num": frame_pixel_num}
    kinds = {"i": [n for n, k in enumerate(frame_types) if k == 0], "p": [n for n, k in enumerate(frame_types) if k != 0],
             "all": list(range(len(frame_types)))}
    out["i_frame_num"], out["p_frame_num"] = len(kinds["i"]), len(kinds["p"])
    for name, idx in kinds.items():
        mean = lambda v: (sum(v[n] for n in idx) / len(idx)) if idx else 0
        out[f"ave_{name}_frame_bpp"] = mean(bits) / frame_pixel_num
        out[f"ave_{name}_frame_psnr"] = mean(psnrs)
        out[f"ave_{name}_frame_msssim"] = mean(msssims)
    out["frame_bpp"] = [b / frame_pixel_num for b in bits]
    out["frame_psnr"], out["frame_msssim"], out["frame_type"] = list(psnrs), list(msssims), list(frame_types)
    return out


class _QualityLog:
    """PSNR and MS-SSIM of every coded picture of one GOP stream, taken on the device (vcm_ts_amd/metrics.py: one launch
    sequence per picture on the stream that coded it) from the reconstruction clamped to [0, 1] against the source,
    both cropped to the unpadded size (DCVC_HEM/test_video.py:156-163).  The values of a GOP go to pinned host memory in
    ONE asynchronous copy behind its last picture and are looked at when the folder is done: the host never waits for a
    picture's metric."""

    def __init__(self, plan):
        self.plan, self.log = plan, GopLog()

    def add(self, g, recon, source, size):
        self._add(g, recon, source, size)

    def _add(self, g, recon, source, size, *more):
        from . import metrics

        h, w = size
        ms, _, sse = metrics.measure(recon[..., :h, :w], source[..., :h, :w], 1.0, clamp01=True)
        self.log.add(g, torch.cat([ms, sse, *more]))
        if self.plan.is_gop_end(g):
            self.flush()

    def flush(self):
        self.log.flush()

    def collect(self, elements):
        """{frame number: (psnr dB, ms-ssim)}"""
        import math

        out = {}
        for idx, (host,) in self.log.collect():
            for g, (ms, sse), more in zip(idx, host[:, :2].double().tolist(), self._more(host)):
                out[g] = (10.0 * math.log10(elements / sse) if sse > 0 else float("inf"), ms, *more)
        return out

    def _more(self, host):
        """What a row holds behind its two metrics, per picture: nothing."""
        return [()] * host.shape[0]


def _bitmap_args(bit_map, report):
    """bit_map= of an encode loop (None | True | a folder for im%05d.npy) -> the folder or None, refused by name before any
    GPU work."""
    if bit_map is None or bit_map is False:
        return None
    if bit_map is True:
        if not report:
            raise ValueError("bit_map=True needs report= (where the regional bit counts go), or give a folder for the maps")
        return None
    if not isinstance(bit_map, (str, os.PathLike)):
        raise ValueError(f"bit_map: expected None, True or a folder, got {type(bit_map).__name__}")
    return os.fspath(bit_map)


def _rate_args(target_bpp, q_range, height, width, gop):
    """target_bpp= / q_range= of an encode loop -> the `rate` factory of GopEncoder.encode_gop (one ratectl.RateControl
    per GOP, target_bpp * height * width bits per picture of the UNPADDED size) or None, refused by name before any GPU
    work: a target that is not above 0, a q_range without a target, lowest > highest, q-scales outside [0.01, 655]."""
    if target_bpp is None:
        if q_range is not None:
            raise ValueError("q_range= belongs to target_bpp= (the range the rate control may move q_y in)")
        return None
    from . import ratectl

    return ratectl.factory(ratectl.target_bits_of(target_bpp, height, width), int(gop), ratectl.q_index_range(q_range))


BIT_KEYS = ("frame_bits_mv_z", "frame_bits_mv_y", "frame_bits_z", "frame_bits_y")  # (bitmap.COMPONENTS' order)


class _BitLog:
    """The bit maps (vcm_ts_amd/bitmap.py) of every coded picture of one GOP stream.  The region sums of a picture are
    enqueued on the stream that coded it, behind its map kernels (labels 0 / 1 from labels_of(g), or one label without a
    ROI); the rows of a GOP -- and, with a folder, its per-cell maps -- go to pinned host memory in ONE asynchronous copy
    behind its last picture and are looked at when the sequence is done, like the _QualityLog's values."""

    def __init__(self, plan, labels_of, keep_cells):
        self.plan, self.labels_of, self.keep_cells = plan, labels_of, keep_cells
        self.K = 2 if labels_of else 1
        self.log, self.cells, self._one = GopLog(), [], None

    def add(self, g, bits):
        if self.labels_of:
            labels = self.labels_of(g)
        else:
            if self._one is None or tuple(self._one.shape[1:]) != (bits.hc, bits.wc):
                self._one = torch.zeros((1, bits.hc, bits.wc), dtype=torch.uint8, device=bits.status.device)
            labels = self._one
        row = bits.regions_enqueue(labels, self.K)
        self.log.add(g, torch.cat([row, labels.sum(dtype=torch.int64).reshape(1)]))
        if self.keep_cells:
            self.cells.append(bits.cells_device())
        if self.plan.is_gop_end(g):
            self.flush()

    def flush(self):
        if self.log.keys:
            self.log.flush(torch.stack(self.log.rows), torch.stack(self.cells) if self.cells else None)
            self.cells = []

    def collect(self):
        """{frame number: ((K, 4) int64 sums in 2^-20 bit, cells of label 1, the (1, hc, wc) float64 cell map or None)}"""
        from .bitmap import BitMap

        out = {}
        for idx, (rows, cells) in self.log.collect():
            for n, g in enumerate(idx):
                row = rows[n].numpy()
                out[g] = (BitMap.decode(row[:-1], 1, self.K)[0], int(row[-1]), None if cells is None else cells[n].numpy())
        return out


class _PinnedRing:
    """Pictures go to the device through a ring of pinned buffers on a copy stream of their own: a pageable
    `.to(device)` would be a synchronous copy queued BEHIND the previous picture's kernels, i.e. the host could
    never run ahead of the GPU (measured: 26 ms of every picture's 66 spent blocked in that call)."""

    def __init__(self, dev, shape, slots=3):
        self.dev, self.n, self.copy_stream = dev, 0, torch.cuda.Stream(dev)
        self.ring = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.done = [None] * slots

    def host(self):
        """The next buffer to fill, as a numpy array."""
        j = self.n % len(self.ring)
        if self.done[j] is not None:
            self.done[j].synchronize()  # the copy that last read this pinned buffer (three pictures ago)
        return self.ring[j].numpy()

    def upload(self):
        """The buffer host() handed out, as a device tensor the current stream may read."""
        j = self.n % len(self.ring)
        self.n += 1
        with torch.cuda.stream(self.copy_stream):
            d = self.ring[j].to(self.dev, non_blocking=True)
            self.done[j] = torch.cuda.Event()
            self.done[j].record(self.copy_stream)
        cur = torch.cuda.current_stream(self.dev)  # (this GOP stream's: ConcurrentGopEncoder pulls frames inside it)
        cur.wait_event(self.done[j])
        d.record_stream(cur)
        return d


class _EncodeRun:
    """What encoding a sequence of `n_frames` pictures of `size` = (height, width) into `bin_dir` is, whatever the
    pictures come from: the GOP streams and their codecs, which frame numbers each stream codes, the .bin sink and
    the bits / quality report.  _encode_sequence supplies the pictures and takes the reconstructions."""

    def __init__(self, bin_dir, plan, size, gop, device, precision, i_ckpt, p_ckpt, coder, nets, gop_streams, log_cls,
                 bit_log=None, rate=None, picture_hash=False, base=None):
        """plan: the GopPlan of the sequence (`gop` is its longest GOP).  nets, gop_streams: see encode_folder.
        base: None, or the _BaseLayer of encode_folder's base_scale= -- `size` is then the BASE size (what the .bin files
        hold); the report, hashes.json and the returned size speak of base.full, and `pixels` is of base.shown().
        log_cls: the _QualityLog to keep per stream, or None for no report.
        bit_log: None, or (labels_of or None, folder or None) -- keep a _BitLog per stream (encode_folder's bit_map=).
        rate: None, or the factory of _rate_args (encode_folder's target_bpp=).
        picture_hash: keep a picturehash.HashLog per stream and write hashes.json (encode_folder's picture_hash=)."""
        from . import picturehash as PH

        os.makedirs(bin_dir, exist_ok=True)
        PH.remove_hashes(bin_dir)  # (a stale record must not describe these .bin files; ours is written by results())
        self.rate, self.rate_log = rate, {}
        self.bin_dir, self.plan, self.n_frames, self.size, self.gop = bin_dir, plan, plan.n_frames, size, gop
        self.base, self.full = base, (base.full if base else size)
        self.dev = torch.device(device)
        self.n_gops = plan.n_gops
        self.K = K = max(1, min(int(gop_streams), self.n_gops))
        pairs = [nets] if (nets is not None and not isinstance(nets, list)) else list(nets or [])
        made = iter(pairs[:K] + [None] * K)
        self.cenc = ConcurrentGopEncoder(lambda: next(made) or _nets(self.dev, precision, i_ckpt, p_ckpt), gop_size=gop,
                                         streams=K, coder=coder)
        self.bits = {}
        self.quality = [log_cls(plan) for _ in range(K)] if log_cls else None
        self.bit_dir = bit_log[1] if bit_log else None
        self.bit_logs = [_BitLog(plan, bit_log[0], self.bit_dir is not None) for _ in range(K)] if bit_log else None
        if self.bit_dir:
            os.makedirs(self.bit_dir, exist_ok=True)
        self.orders = [plan.order(k, K) for k in range(K)]
        self.hash_logs = [PH.HashLog(plan) for _ in range(K)] if picture_hash else None

    def global_index(self, k, t):  # picture t of stream k's sequence -> 0-based frame number in the sequence
        return self.orders[k][t]

    def order(self, k):
        """The frame numbers stream k codes, in its coding order: GOPs k, k + K, ... of the plan."""
        return self.orders[k]

    def intra(self, k):
        """The picture numbers of stream k's sequence that are coded as I pictures."""
        return {t for t, g in enumerate(self.orders[k]) if self.plan.is_intra(g)}

    def _sink(self, k):
        def sink(kind, qidx, payload, t):
            g = self.global_index(k, t)
            path = os.path.join(self.bin_dir, f"im{str(g + 1).zfill(5)}.bin")
            if kind == "I":
                S.encode_i(self.size[0], self.size[1], qidx[0], payload, path)
            else:
                S.encode_p(payload, qidx[0], qidx[1], path)
            self.bits[g] = S.filesize(path) * 8

        return sink

    def encode(self, frames, q, on_recon=None, q_map=None, aq=None):
        """frames(k): generator of stream k's padded pictures, those of order(k).  on_recon(k, g, ref_frame): sees the
        reconstruction of frame g while it is valid (and before stream k's next picture is pulled from frames(k)).
        q_map(g): the q-scale map frame g is coded with, made on the stream that codes it (None: no maps, no launch).
        aq: the aq.AQ of backward-adaptive quantisation (encode_folder's aq=), None for none."""
        maps_of = lambda k: (lambda t: q_map(self.global_index(k, t))) if q_map else None
        def recon_of(k):
            if self.hash_logs is None:
                return (lambda t, ref_frame: on_recon(k, self.global_index(k, t), ref_frame)) if on_recon else None

            def hashed(t, ref_frame):  # (on the stream that coded the picture: two launches each, nothing waited for)
                g = self.global_index(k, t)
                if self.base:
                    self.hash_logs[k].add(g, ref_frame, self.full, display=self.base.shown(k, g, ref_frame))
                else:
                    self.hash_logs[k].add(g, ref_frame, self.size)
                if on_recon:
                    on_recon(k, g, ref_frame)

            return hashed

        bits_of = lambda k: (lambda t, bits: self.bit_logs[k].add(self.global_index(k, t), bits))
        # (GopEncoder reads the split-fp16 range guard once per GOP and raises lib.KernelError: no .bin of a clamped GOP
        # is reported as a success)
        with torch.no_grad():
            self.cenc.encode_gops([frames(k) for k in range(self.K)], q[0], q[1], q[2], sinks=[self._sink(k) for k in range(self.K)],
                                  on_recons=[recon_of(k) for k in range(self.K)], intra=[self.intra(k) for k in range(self.K)],
                                  q_maps=[maps_of(k) for k in range(self.K)] if q_map else None,
                                  bit_maps=[bits_of(k) for k in range(self.K)] if self.bit_logs else None, rate=self.rate,
                                  aq=aq)
        if self.rate is not None:
            for k, log in enumerate(self.cenc.rate_logs):
                self.rate_log.update({self.global_index(k, t): entry for t, entry in enumerate(log)})

    def _bit_results(self, order):
        """Collects the bit logs: writes im%05d.npy when a folder was given, returns the report's keys."""
        values = {}
        for k, log in enumerate(self.bit_logs):
            with torch.cuda.stream(self.cenc.streams[k]):
                log.flush()  # a trailing partial GOP
            values.update(log.collect())
        if self.bit_dir:
            for g in order:
                np.save(os.path.join(self.bit_dir, f"im{str(g + 1).zfill(5)}.npy"), values[g][2])
        from .bitmap import REGION_UNIT

        keys = {name: [float(values[g][0][:, c].sum()) / REGION_UNIT for g in order] for c, name in enumerate(BIT_KEYS)}
        if self.bit_logs[0].K == 2:
            keys["frame_bits_roi"] = [float(values[g][0][1].sum()) / REGION_UNIT for g in order]
            keys["frame_bits_bg"] = [float(values[g][0][0].sum()) / REGION_UNIT for g in order]
            keys["frame_roi_cells"] = [values[g][1] for g in order]
        return keys

    def _write_hashes(self):
        """hashes.json: once, when everything has been coded."""
        from . import picturehash as PH

        digests = {}
        for k, log in enumerate(self.hash_logs):
            with torch.cuda.stream(self.cenc.streams[k]):
                log.flush()  # a trailing partial GOP
            digests.update(log.collect())
        h, w = self.full  # (with a base scale: the display size `pixels` is of; `state` is of the base reference picture)
        l, r, t, b = S.get_padding_size(h, w)
        PH.write_hashes(self.bin_dir, digests, h, w, (h + t + b, w + l + r), self.cenc.encoders[0].p_net.engine().precision)

    def results(self, report, extras=None):
        """(bits per frame list, size) -- with a report also the rd_report() dictionary, which every keys(rd, frame types,
        [the logs' value per frame]) of the list `extras` extends, in order, before the bit and rate keys are added and it is
        written to `report` (if that is a path)."""
        order = sorted(self.bits)
        bit_list = [self.bits[g] for g in order]
        if self.hash_logs:
            self._write_hashes()
        bit_keys = self._bit_results(order) if self.bit_logs else None
        if self.quality is None:
            return bit_list, self.full
        h, w = self.full
        values = {}
        for k, log in enumerate(self.quality):
            with torch.cuda.stream(self.cenc.streams[k]):
                log.flush()  # a trailing partial GOP
            values.update(log.collect(3 * h * w))
        types = [0 if self.plan.is_intra(g) else 1 for g in order]
        rd = rd_report(types, bit_list, [values[g][0] for g in order], [values[g][1] for g in order], h * w)
        for keys in extras or ():
            keys(rd, types, [values[g] for g in order])
        if bit_keys:
            rd.update(bit_keys)
        if self.rate is not None:  # (the q-scale each picture's y was coded with -- an I picture's is q_i -- and the budget
            rd["frame_q_y"] = [self.rate_log[g][0] / 100 for g in order]  # its controller gave it; null where none was)
            rd["frame_bits_target"] = [None if self.rate_log[g][2] is None else float(self.rate_log[g][2]) for g in order]
        if isinstance(report, (str, os.PathLike)):
            import json

            with open(report, "w") as f:
                json.dump(rd, f, indent=2)
        return bit_list, self.full, rd


GOPS_JSON = "gops.json"


def _scan_pass(source, gop, scenecut, min_gop, auto=None, steady=None):
    """(the GopPlan of an encode loop, the noise estimate of its source or None).  Without `scenecut` the fixed plan, and
    the source is not read.  With it the scan pass: every picture of the source once, in order, as the coding pass will see
    it (same reader, same conversion); each is summarised on the device (scenecut.SceneScan: one kernel per picture,
    nothing synchronised) and the distances are read back in one copy at the end.

    auto: a tnr.AutoTNR -- the pictures of the SAME pass also go through a noise.NoiseScan (one more kernel per picture,
    nothing synchronised) and the second value is the noise.NoiseEstimate of the whole source: with scenecut the source is
    still read once before it is coded, and without scenecut this is the one pass that reads it.

    steady: a shake.Registrar for the source (_registrar), with auto -- every picture goes through it first and the noise scan
    is handed the picture registered onto picture 0 (three more launches per picture, nothing synchronised); the scene scan keeps the
    UNREGISTERED picture, whose histograms do not care about a shift of a few pixels and whose plan must not change.  The
    border is not masked here: dcvc_noise_hist reads the cells on the device, and the band a registered picture replicates
    from its edge only ever inflates a border cell's difference, which the lower quartile does not see.  The caller reads the
    registrar's log afterwards (_shake_document)."""
    from . import scenecut as SC

    n_frames = source.n_frames
    SC.check_options(gop, scenecut, min_gop)
    if scenecut is None and auto is None:
        return GopPlan.fixed(n_frames, gop), None
    scan = SC.SceneScan(source.dev, source.size[0], source.size[1], n_frames) if scenecut is not None else None
    if auto is not None:
        from . import noise as NS

        meter = NS.NoiseScan(source.dev, source.size[0], source.size[1])
    seen = 0
    with torch.no_grad():
        for x, _ in source.pictures(range(n_frames)):
            if scan is not None:
                scan.add(x)
            if auto is not None:
                meter.add(x if steady is None else steady.add(x))
            seen += 1
    if seen != n_frames:
        raise ValueError(f"the scan pass saw {seen} pictures of {n_frames}")
    plan = GopPlan.fixed(n_frames, gop) if scan is None else GopPlan(n_frames, SC.plan(scan.distances(), gop, scenecut, min_gop))
    return plan, (None if auto is None else NS.estimate(meter.histogram(), auto.min_cells, meter.pairs))


def _registrar(source, shake):
    """The shake.Registrar of an opened source for the shake.ShakeParams `shake`; None without."""
    if shake is None:
        return None
    from . import shake as SH

    return SH.Registrar(source.dev, source.size[0], source.size[1], source.n_frames, shake)


def _shake_document(steady, source):
    """What shake.json says after the scan pass (None without a registrar).  A source with more than max_lost percent of its
    pictures lost is a ValueError by name, before any estimate is made of it."""
    if steady is None:
        return None
    from . import shake as SH

    moved = SH.document(steady.log(), steady.params, *source.size)
    SH.check_lost(moved["summary"], steady.params)
    return moved


def write_gop_plan(bin_dir, plan, gop, scenecut, min_gop):
    """gops.json beside the .bin files -- only for a plan that came from a scan: a fixed plan needs none (and a stale
    file of an earlier encode into the same folder must not describe these .bin files)."""
    S.write_sidecar(bin_dir, GOPS_JSON, None if scenecut is None else
                    dict(plan.to_json(), gop=int(gop), min_gop=int(min_gop), scenecut=float(scenecut)))


ROIQ_JSON = "roiq.json"


def _roiq_args(roi, roi_q):
    """roi_q= of an encode loop against its roi=, refused by name before any GPU work."""
    if roi_q is None:
        return
    from . import roi as X

    if roi is None:
        raise ValueError("roi_q= needs roi= (the boxes the q-scale maps are made from)")
    if not isinstance(roi_q, X.RoiQ):
        raise ValueError(f"roi_q: expected a roi.RoiQ, got {type(roi_q).__name__}")
    names = X.as_roi(roi).names
    if len(roi_q.classes) != len(names):
        raise ValueError(f"roi_q: {len(roi_q.classes)} class factors for the roi's classes {list(names)}")


def write_roiq(bin_dir, roi_q, names=()):
    """roiq.json beside the .bin files -- only for an encode with q-scale maps: without them none is needed (and a stale
    file of an earlier encode into the same folder must not describe these .bin files)."""
    S.write_sidecar(bin_dir, ROIQ_JSON, None if roi_q is None else roi_q.to_json(names))


def _aq_args(aq):
    """aq= of an encode loop, refused by name before any GPU work."""
    from . import aq as A

    if aq is not None and not isinstance(aq, A.AQ):
        raise ValueError(f"aq: expected an aq.AQ, got {type(aq).__name__}")
    return aq


def read_roiq(bin_dir, roi=None):
    """The roi.RoiQ the .bin files of `bin_dir` were coded with, or None without a roiq.json.  Refused by name: the file
    without `roi` (the maps are rebuilt from the boxes), class names that are not the roi's, values out of range."""
    from . import roi as X

    found = S.read_sidecar(bin_dir, ROIQ_JSON)
    if found is None:
        return None
    path, info = found
    if roi is None:
        raise ValueError(f"{path}: these pictures were coded with q-scale maps made from ROI boxes; decoding them needs the "
                         f"same boxes (roi=, --roi-root)")
    try:
        return X.RoiQ.from_json(info, X.as_roi(roi).names)
    except ValueError as ex:
        raise ValueError(f"{path}: {ex}") from None


def _count_bins(bin_dir):
    n = 0
    while os.path.exists(os.path.join(bin_dir, f"im{str(n + 1).zfill(5)}.bin")):
        n += 1
    return n


def read_gop_plan(bin_dir, gop=None):
    """(GopPlan of the .bin files in `bin_dir`, its longest GOP): from gops.json when encode left one, else an I picture
    every `gop` (default 32) pictures.  Refused by name: a plan whose frame count is not the number of .bin files, and an
    explicit `gop` that is not the plan's."""
    n, found = _count_bins(bin_dir), S.read_sidecar(bin_dir, GOPS_JSON)
    if found is None:
        return GopPlan.fixed(n, gop or 32), gop or 32
    path, info = found
    try:
        plan = GopPlan.from_json(info)
    except ValueError as ex:
        raise ValueError(f"{path}: {ex}") from None
    if plan.n_frames != n:
        raise ValueError(f"{path}: a plan of {plan.n_frames} frames beside {n} .bin files")
    if gop is not None and info.get("gop") is not None and int(gop) != int(info["gop"]):
        raise ValueError(f"{path}: the plan was made with gop {info['gop']}, not {gop}")
    longest = max((len(plan.gop_range(j)) for j in range(plan.n_gops)), default=1)
    return plan, int(info.get("gop") or longest)


class _BaseLayer:
    """The reduced-resolution base layer of a file loop (base_scale=, vcm_ts_amd/scale.py): full-size pictures go down to
    the codec's size on the stream that codes them, reconstructions come up again for whatever looks at them.  The DPB
    keeps the base picture: up() is display side only."""

    def __init__(self, scale):
        self.scale, self.full, self.size, self.cur = scale, scale.full, scale.base, {}
        l, r, t, b = S.get_padding_size(*self.size)
        self.padded = (self.size[0] + t + b, self.size[1] + l + r)

    def down(self, x):
        """The zeroed, 64-padded base picture the codec takes of a (padded) full-size picture: one launch into its interior."""
        (h, w), (hb, wb) = self.full, self.size
        out = torch.zeros((1, 3) + self.padded, dtype=torch.float32, device=x.device)
        self.scale.down(x[..., :h, :w], out=out[..., :hb, :wb])
        return out

    def shown(self, k, g, ref_frame):
        """The full-size picture of frame g's base reconstruction, made once per picture on stream k's current stream."""
        if self.cur.get(k, (None, None))[0] != g:
            self.cur[k] = (g, self.scale.up(ref_frame[..., :self.size[0], :self.size[1]]))
        return self.cur[k][1]


def _base_args(base_scale, roi, roi_q, bit_map, size, dev):
    """base_scale= of an encode loop -> its _BaseLayer (None without), refused by name before any other GPU work."""
    if base_scale is None:
        return None
    from . import scale as SC

    ratio = SC.as_ratio(base_scale)
    if roi_q is not None:
        raise NotImplementedError("base_scale= with roi_q= (--plate-q / --face-q / --background-q): q-scale maps of boxes on "
                                  "the base grid are not implemented")
    if bit_map and roi is not None:
        raise NotImplementedError("base_scale= with bit_map= and roi= (--bit-map with --roi-root): regional bit counts of "
                                  "boxes on the base grid are not implemented")
    return _BaseLayer(SC.Scale(size, ratio, dev))


def _decode_scale(bin_dir, height, width, base_scale, roi, residuals, residual_bins):
    """base_scale= of a decode loop ("file": follow the folder's scale.json; None: ignore it, --base-only) ->
    (scale.read_scale's record of the scaler to build, or None when nothing is scaled up; the (height, width) of the coded
    pictures).  height, width: the display size.  Host work only (_decode_sequence builds the tables on the device, once every
    refusal has had its turn).  Refused by name: a scale.json of another display size or whose base is not what the .bin
    files hold, a base-only decode with a ROI, anything but "file" and None.  A base-only decode does not read the file:
    the first .bin file's header says what size the pictures are."""
    from . import scale as SC

    if base_scale not in ("file", None):
        raise ValueError(f"base_scale: expected 'file' (follow {SC.SCALE_JSON}) or None (base only), got {base_scale!r}")
    where, first = os.path.join(bin_dir, SC.SCALE_JSON), os.path.join(bin_dir, "im00001.bin")
    if base_scale is None:
        if not (os.path.exists(where) and os.path.exists(first)):
            return None, (height, width)
        if roi is not None or residuals is not None or residual_bins is not None:
            raise ValueError("a base-only decode (base_scale=None, --base-only) takes no roi=, residuals= or residual_bins=: "
                             "boxes and the residual layer live at full size")
        return None, tuple(S.decode_i(first)[:2])
    info = SC.read_scale(bin_dir)
    if info is None:
        return None, (height, width)
    if info["full"] != (int(height), int(width)):
        raise ValueError(f"{where}: a base layer of {info['full'][1]}x{info['full'][0]} pictures, decoding {width}x{height}")
    if os.path.exists(first) and tuple(S.decode_i(first)[:2]) != info["base"]:
        coded = S.decode_i(first)[:2]
        raise ValueError(f"{where}: a base layer of {info['base'][1]}x{info['base'][0]} pictures (ratio {info['ratio']}), the "
                         f".bin files hold {coded[1]}x{coded[0]}")
    return info, info["base"]


def _png_pictures(reader, order, size, dev, pool, io_workers, sharers):
    """The pictures of a PNG folder that `order` names, on the device, as the padded float32 pictures the codec takes: what
    the coding pass, the scene-cut scan and the motion scan all read.  The (H, W, 3) uint8 arrays are decoded up to `depth`
    ahead by the shared `pool` (which `sharers` such generators draw on together; None: inline)."""
    from collections import deque

    h, w = size

    def raw_frames():
        if pool is None:
            for g in order:
                yield reader.load_u8(reader.path_of(g + 1))
            return
        depth, pending, nxt = max(2, 2 * io_workers // sharers), deque(), 0
        while nxt < len(order) or pending:
            while nxt < len(order) and len(pending) < depth:
                pending.append(pool.submit(reader.load_u8, reader.path_of(order[nxt] + 1)))
                nxt += 1
            yield pending.popleft().result()

    ring = _PinnedRing(dev, (h, w, 3))
    for rgb in raw_frames():
        assert tuple(rgb.shape) == (h, w, 3), "all frames must have one size"
        ring.host()[...] = rgb
        yield pad_frame(u8_to_unit_float(ring.upload()))


def _video_pictures(reader, order, spec, quantize8, dev, deinterlace=None, moved=None):
    """(the padded RGB picture the codec takes, the file's samples on the device) of every frame of a yuv reader that
    `order` names: the one path from the file to the codec (a ring of pinned buffers, one asynchronous copy, the colour
    conversion on the device) of the coding pass, the scene-cut scan and the motion scan.
    deinterlace: a deint.Deinterlace -- `order` then names OUTPUT PICTURES; the up to three file frames a picture needs
    go up through the same ring (what the previous picture uploaded is kept: a sequential order uploads every frame once),
    one dcvc_deinterlace420 launch makes the progressive I420 buffer, and that buffer is the `samples` of the pair and what
    the unchanged colour conversion reads.  moved: a dictionary that then takes {picture: the sum of its `moved` words, on
    the device}."""
    from . import yuv as Y

    sample_dtype = torch.uint8 if spec.bit_depth == 8 else torch.int16
    ring = _PinnedRing(dev, reader.frame_bytes)

    def upload(n):
        reader.read_into(n, ring.host())
        return ring.upload().view(sample_dtype)

    held = {}  # file frame -> its samples on the device, of the picture before
    for g in order:
        if deinterlace is None:
            samples = upload(g)
        else:
            frames, second = deinterlace.needs(g, reader.n_frames)
            held = {n: held[n] if n in held else upload(n) for n in sorted(set(frames))}
            samples, words = deinterlace.step(*(held[n] for n in frames), reader.height, reader.width, spec.bit_depth, second)
            if moved is not None:
                moved[g] = words.sum(dtype=torch.int64)
        yield Y.yuv420_to_rgb(samples, reader.height, reader.width, spec, pad=True, quantize8=quantize8), samples


class _PngSource:
    """A PNG folder as the source of a file loop.  open() reads the folder: the reader, `size` = (height, width),
    `n_frames` and the shared pool of PNG-decoding threads.  Refused by name there: a folder that has neither im1.png nor
    im00001.png."""

    def __init__(self, frames_dir, device, io_workers=8, max_frames=None):
        self.frames_dir, self.dev, self.io_workers, self.max_frames = frames_dir, torch.device(device), io_workers, max_frames
        self.pool = None

    def open(self):
        from concurrent.futures import ThreadPoolExecutor

        from PIL import Image

        self.reader, self.n_frames = PNGReader(self.frames_dir), 0
        while os.path.exists(self.reader.path_of(self.n_frames + 1)) and (self.max_frames is None or self.n_frames < self.max_frames):
            self.n_frames += 1
        with Image.open(self.reader.path_of(1)) as first:  # (the header only)
            self.size = first.size[::-1]
        self.pool = ThreadPoolExecutor(max_workers=self.io_workers) if self.io_workers > 0 else None

    def pictures(self, order, sharers=1):
        """(the padded picture the codec takes, None) of every frame `order` names; `sharers` such generators draw on
        the pool together."""
        for x in _png_pictures(self.reader, order, self.size, self.dev, self.pool, self.io_workers, sharers):
            yield x, None

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)


class _VideoSource:
    """A `.y4m` / raw `.yuv` file (or an open yuv reader, which then stays the caller's to close) as the source of a file
    loop.  open() opens the file: the reader, the colour description, `size` and `n_frames`.  Every refusal about the file
    happens there, before any GPU work: what yuv.open_video refuses, a bit depth that is not the description's, a file
    without frames.
    deinterlace: None, a deint.Deinterlace, or a mode ("frame" / "field") whose field order the file's header gives -- the
    file is then opened as interlaced material, `n_frames` is the number of OUTPUT PICTURES (which max_frames counts) and
    pictures() numbers pictures; refused in open() as well: a height that is no multiple of 4, a missing field order.
    keep_moved: keep every picture's `moved` total on the device for the report (deint_moved())."""

    def __init__(self, video, device, size=None, spec=None, quantize8=False, bit_depth=8, fps=None, max_frames=None, deinterlace=None,
                 keep_moved=False):
        self.video, self.dev, self.args, self.spec, self.quantize8 = video, torch.device(device), (size, bit_depth, fps), spec, quantize8
        self.max_frames, self.reader, self.deinterlace = max_frames, None, deinterlace
        self.moved = {} if keep_moved and deinterlace is not None else None

    def open(self):
        from . import yuv as Y

        if isinstance(self.video, (str, os.PathLike)):
            more = {} if self.deinterlace is None else {"interlaced": True, "field_order": getattr(self.deinterlace, "order", None)}
            self.reader = Y.open_video(self.video, *self.args, **more)
        else:
            self.reader = self.video
        reader = self.reader
        self.spec = self.spec or reader.spec()
        if self.spec.bit_depth != reader.bit_depth:
            raise ValueError(f"the file holds {reader.bit_depth}-bit samples, the colour description says {self.spec.bit_depth}")
        self.size = (reader.height, reader.width)
        n = reader.n_frames
        if self.deinterlace is not None:
            from . import deint as DI

            if not isinstance(self.deinterlace, DI.Deinterlace):
                if reader.field_order is None:
                    raise ValueError(f"{getattr(reader, 'path', self.video)}: deinterlacing needs a field order and the file names none "
                                     f"(--field-order tff|bff)")
                self.deinterlace = DI.Deinterlace(self.deinterlace, reader.field_order)
            DI.check_height(reader.height)
            n = self.deinterlace.pictures_of(n)
        self.n_frames = n if self.max_frames is None else min(n, int(self.max_frames))
        if self.n_frames < 1:
            raise ValueError(f"{getattr(reader, 'path', self.video)}: no frames")

    def pictures(self, order, sharers=1):
        """(the padded picture the codec takes, the file's samples on the device) of every frame `order` names -- with
        deinterlace, of every output picture it names and the progressive samples made for it."""
        return _video_pictures(self.reader, order, self.spec, self.quantize8, self.dev, self.deinterlace, self.moved)

    def deint_moved(self):
        """[the `moved` total of every output picture], one copy to the host after the device has finished."""
        torch.cuda.synchronize(self.dev)
        return torch.stack([self.moved[g] for g in range(self.n_frames)]).tolist()

    def close(self):
        if self.reader is not None and self.reader is not self.video:
            self.reader.close()


class _PngStage:
    """Output stage "PNG folder" of a file loop -- or, without a folder, nothing: put() writes the unpadded picture as
    im%05d.png through a pool of PNG-encoding threads.  png_device: the device the files are made on instead
    (vcm_ts_amd/pngdev.py: two launches and one asynchronous copy per picture on the stream that made it; the threads
    then only wait for the copy and write) -- None: the pictures are copied to the host and encoded there."""
    sums = 0  # (integer sums measure() adds to a picture's report row)

    def __init__(self, path, io_workers, png_device=None):
        if png_device is not None and not path:
            raise ValueError("png_device belongs to recon_dir (the folder the PNGs are written to)")
        self.path, self.io_workers, self.savers, self.png_device, self.dev = path, io_workers, None, png_device, None

    def open(self, size, streams=1, source=None):
        self.size = size
        if self.path:
            if self.png_device is not None:  # (refuses by name, before any launch or file, what the kernels cannot take)
                from . import pngdev

                self.dev = pngdev.PngDevice(size, self.png_device, streams)
            os.makedirs(self.path, exist_ok=True)
            self.savers = PNGWriters(self.io_workers)

    def put(self, k, g, frame):
        if self.path:
            h, w = self.size
            path = os.path.join(self.path, f"im{str(g + 1).zfill(5)}.png")
            if self.dev is not None:
                from .pngdev import save_handle

                self.savers.submit(self.dev.put(k, frame), path, save_handle)
            else:
                save_torch_image(frame[..., :h, :w], path, self.savers)

    def flush(self):
        if self.savers:
            self.savers.close()  # (re-raises a writer's exception)

    def close(self, failed):
        if self.savers and failed:  # (already failing: do not mask the first error with a writer's)
            self.savers.__exit__(RuntimeError, None, None)

    def report_keys(self):
        return None

    def finish(self, bin_dir, n_frames, gop, roi, residual_step):
        pass


class _VideoStage:
    """Output stage "video file" of a file loop -- or, without a path, no file: put() converts the picture to 4:2:0 on the
    stream that made it and hands it to that stream's _VideoOut.  For an encode it also owns what only a video source has:
    the sample-domain sums and keys of the report, and sequence.json."""
    sums = 3

    def __init__(self, path, spec=None, fps=None, **extras):
        """spec, fps, extras (chroma, interlace, aspect): of the file to write; an encode takes them from its source."""
        self.path, self.spec, self.fps, self.container, self.extras = path, spec, fps, None, extras
        self.writer, self.outs, self.cur, self.deinterlace = None, None, {}, None

    def open(self, size, streams=1, source=None):
        from . import yuv as Y

        self.Y, self.size = Y, size
        if source is not None:  # (an encode: the output file and sequence.json describe the source)
            reader = source.reader
            self.spec, self.fps, self.container = source.spec, reader.fps, "y4m" if isinstance(reader, Y.Y4MReader) else "yuv"
            self.extras = {name: getattr(reader, name, None) for name in ("chroma", "interlace", "aspect")}
            self.deinterlace = source.deinterlace
            if self.deinterlace is not None:  # (what was coded is progressive: a picture per field doubles the rate)
                self.extras["interlace"] = "p"
                if self.fps and self.deinterlace.mode == "field":
                    self.fps = (2 * self.fps[0], self.fps[1])
        if self.path:
            self.writer = Y.create_video(self.path, size[1], size[0], self.spec, self.fps, **self.extras)
            self.outs = [_VideoOut(self.writer) for _ in range(streams)]

    def measure(self, k, frame, samples):
        """The three integer sums of the picture's samples against the file's: the ONE conversion of a reported picture,
        whose samples put() then writes."""
        self.cur[k], sums = self.Y.rgb_to_yuv420(frame, self.size[0], self.size[1], self.spec, source=samples)
        return sums

    def put(self, k, g, frame):
        """frame: padded or not -- rgb_to_yuv420 reads its top-left corner in place."""
        out = self.cur.pop(k, None)
        if self.outs:
            self.outs[k].put(g, self.Y.rgb_to_yuv420(frame, self.size[0], self.size[1], self.spec) if out is None else out)

    def flush(self):
        for o in self.outs or []:
            o.close()

    def close(self, failed):
        if self.writer:
            self.writer.close()

    def report_keys(self):
        (h, w), Y, depth = self.size, self.Y, self.spec.bit_depth

        def keys(rd, types, values):
            per = [Y.psnr_yuv(v[2][:3], h, w, depth) for v in values]
            for n, name in enumerate(("y", "u", "v", "yuv")):
                rd[f"frame_psnr_{name}"] = [p[n] for p in per]
            for name, keep in (("i", lambda k: k == 0), ("p", lambda k: k != 0), ("all", lambda k: True)):
                sel = [p[3] for p, k in zip(per, types) if keep(k)]
                rd[f"ave_{name}_frame_psnr_yuv"] = sum(sel) / len(sel) if sel else 0

        return keys

    def finish(self, bin_dir, n_frames, gop, roi, residual_step):
        write_sequence_info(bin_dir, self.size[1], self.size[0], n_frames, gop, self.fps, self.spec, self.container, **self.extras,
                            roi=roi, residual_step=residual_step, deinterlace=self.deinterlace)


def _encode_sequence(source, out, bin_dir, gop=32, q=(1.0, 1.0, 1.0), device="cuda:0", precision=None, i_ckpt=None, p_ckpt=None,
                     coder="host", io_workers=8, nets=None, gop_streams=1, report=None, roi=None, residuals=None, scenecut=None,
                     min_gop=1, roi_q=None, bit_map=None, target_bpp=None, q_range=None, residual_bins=None, residual_step=1,
                     picture_hash=False, base_scale=None, aq=None, tnr=None, redact=None, grain=None, shake=None):
    """The one encode loop: the pictures of `source` (a _PngSource or a _VideoSource, opened here and closed on every exit)
    through tnr, redact and the base layer's scaling into an _EncodeRun, and every reconstruction through the base layer's
    up-scaling to the residual outputs, the report and `out` (a _PngStage or a _VideoStage).  The options are
    encode_folder's.  Refusals in this order, all before any launch or file: the residual layer's arguments, roi_q, aq, tnr,
    grain, redact, bit_map; then what the source refuses about its files; the rate control's, base_scale, the scene cut's options,
    the boxes of every frame, the redaction's merged lists."""
    from . import aq as A
    from . import scale as SC

    _roi_args(roi, residuals, residual_bins, residual_step)
    _roiq_args(roi, roi_q)
    _aq_args(aq)
    _tnr_args(tnr)
    _shake_args(shake, tnr)
    _grain_args(grain, tnr)
    _redact_args(redact, roi, residuals, residual_bins)
    bit_dir = _bitmap_args(bit_map, report)
    try:
        source.open()
        h, w = source.size
        rate = _rate_args(target_bpp, q_range, h, w, gop)
        dev = torch.device(device)
        base = _base_args(base_scale, roi, roi_q, bit_map, (h, w), dev)
        steady = _registrar(source, shake)
        plan, estimate = _scan_pass(source, gop, scenecut, min_gop, _tnr_auto(tnr), steady)
        moved = _shake_document(steady, source)
        tnr, measured = _resolve_tnr(tnr, estimate, moved)  # (from here on a plain tnr.TNR: nothing below knows the difference)
        layer = _RoiLayer(roi, plan, (h, w), dev) if roi is not None else None
        held = _redact_frames(redact, layer)
        run = _EncodeRun(bin_dir, plan, base.size if base else (h, w), gop, device, precision, i_ckpt, p_ckpt, coder, nets,
                         gop_streams, (_VideoQualityLog if layer or out.sums else _QualityLog) if report else None,
                         _bit_log(bit_map, bit_dir, layer, roi_q), rate, picture_hash, base)
        write_gop_plan(bin_dir, plan, gop, scenecut, min_gop)
        write_roiq(bin_dir, roi_q, layer.roi.names if layer else ())
        SC.write_scale(bin_dir, base.scale if base else None)
        A.write_aq(bin_dir, aq)
        S.write_sidecar(bin_dir, NOISE_JSON, measured)
        S.write_sidecar(bin_dir, SHAKE_JSON, moved)
        res_out = _ResidualOut(residuals, (h, w), run.K, io_workers) if residuals is not None else None
        rec_out = _RecordOut(residual_bins, residual_step, run.K) if residual_bins is not None else None
        filters = _tnr_filters(tnr, run, (h, w), report)
        meters = _grain_meters(grain, bin_dir, run, (h, w))
        _write_redact(bin_dir, redact)
        redaction = _Redaction(redact, layer, held, run, report) if redact is not None else None
        out.open((h, w), run.K, source)
        compared = bool(report or res_out or rec_out)  # (something will look at the source beside the reconstruction)
        current = {}

        def frames(k):
            intra = run.intra(k) if filters or redaction else ()
            pictures = source.pictures(run.order(k), run.K)
            look = None
            if filters and tnr.intra is not None:  # (an I picture sees up to tnr.intra pictures of its own GOP ahead of it)
                pictures = look = _LookAhead(pictures, intra, tnr.intra, len(run.order(k)), _held_ahead)
            for t, (x, aux) in enumerate(pictures):
                if compared:  # (the picture being yielded, never one pulled ahead)
                    current[k] = (x, aux)  # (what on_recon's reconstruction belongs to: encode_steps codes it before pulling the next)
                if filters:  # (the codec sees the filtered picture; current[k] stays the unfiltered one)
                    src = x
                    x = filters[k].step(x, t in intra, [a[0] for a in look.ahead]) if look else filters[k].step(x, t in intra)
                    if meters:  # (what the filter took out of this picture, right behind it on the same stream)
                        meters[k].step(src, filters[k], run.global_index(k, t), t in intra)
                if redaction:  # (after the filter, whose own state stays unredacted; current[k] stays the unredacted one)
                    x = redaction.step(k, run.global_index(k, t), x, t in intra)
                yield base.down(x) if base else x

        def on_recon(k, g, ref_frame):
            x, aux = current.get(k, (None, None))
            if base:  # (everything below looks at the full-size picture; the DPB keeps the base one)
                ref_frame = base.shown(k, g, ref_frame)
            if res_out:
                res_out.put(k, g, x[..., :h, :w], ref_frame[..., :h, :w], layer.boxes(g))
            if rec_out:
                rec_out.put(k, g, x[..., :h, :w], ref_frame[..., :h, :w], layer.boxes(g))
            if report:
                sums = [out.measure(k, ref_frame, aux)] if out.sums else []
                if layer:
                    sums.append(layer.X.region_sse(ref_frame[..., :h, :w], x[..., :h, :w], layer.boxes(g), layer.classes))
                if sums:
                    run.quality[k].add_yuv(g, ref_frame, x, (h, w), torch.cat(sums) if len(sums) > 1 else sums[0])
                else:
                    run.quality[k].add(g, ref_frame, x, (h, w))
            out.put(k, g, ref_frame)

        failed = True
        try:
            run.encode(frames, q, on_recon if (out.path or compared) else None,
                       (lambda g: layer.q_map(g, roi_q)) if roi_q is not None else None, aq)
            out.flush()
            if meters:
                _write_grain(bin_dir, grain, tnr, meters)
            failed = False
        finally:
            out.close(failed)
            if res_out:
                res_out.close(failed)
            if rec_out:
                rec_out.close(failed)
    finally:
        source.close()
    out.finish(bin_dir, plan.n_frames, gop, layer.roi if layer else None, residual_step if rec_out else None)
    keys = [_roi_report_keys(h, w) if layer else None, out.report_keys(), _deint_report_keys(source) if report else None,
            _enh_report_keys(rec_out, h, w) if rec_out else None,
            _tnr_report_keys(tnr, filters, run, h, w) if filters else None,
            _noise_report_keys(measured) if measured and report else None,
            _redact_report_keys(redact, redaction, run, h, w) if redaction else None]
    return run.results(report, [k for k in keys if k])


def encode_folder(frames_dir, bin_dir, recon_dir=None, gop=32, q=(1.0, 1.0, 1.0), device="cuda:0", precision=None,
                  i_ckpt=None, p_ckpt=None, max_frames=None, coder="host", io_workers=8, nets=None, gop_streams=1,
                  report=None, roi=None, residuals=None, scenecut=None, min_gop=1, roi_q=None, bit_map=None, target_bpp=None,
                  q_range=None, residual_bins=None, residual_step=1, picture_hash=False, base_scale=None, aq=None, tnr=None,
                  redact=None, png_device=False, grain=None, shake=None):
    """Returns (bits per frame list, (height, width)) -- and, with `report` (True, or the path of a JSON file to write),
    as a third value the rd_report() dictionary: PSNR and MS-SSIM of every picture measured on the device, one host read
    per GOP; without it no metric kernel is launched.  coder="device": payloads in the opt-in GPU
    format (include/dcvc_hip_rans.h) inside the same .bin containers; decode_folder reads both.
    io_workers: host threads decoding PNGs ahead of the encoder (0: read in the encode loop as run_dcvc does).
    nets: (i_frame_net, p_frame_net) already on the device -- or a list of such pairs, one per GOP stream -- instead
    of building them here.
    gop_streams (round 4): GOPs of the folder in flight together on the GPU (pipeline.ConcurrentGopEncoder: own codec
    instances, DPB and HIP stream each; stream k codes GOPs k, k + K, k + 2K, ...), fed by ONE pool of PNG-decoding
    threads.  GOPs are independent (every GOP starts from an I picture, video_coder.py:122-130), so the .bin files are
    byte-identical to the one-stream loop's (tests/test_gpu_codec.py); each stream holds its own workspace (~33 GB at
    1088x1920).
    roi: a roi.Roi, or (box source, classes) -- roi.PickleBoxes or any callable frame_index -> roi.FrameBoxes.
    residuals (with roi): where the residual layer of video_coder.compute_residuals goes, taken on the stream that coded
    the picture from the source and the reconstruction there: a `.gbrp` path (raw G, B, R planes, what
    `ffmpeg -f rawvideo -pix_fmt gbrp` reads) or a folder for im%05d.png.  With report and roi every picture gains
    frame_psnr_roi / frame_psnr_bg (base layer, per sample inside and outside the boxes shrunk by their class's shrink)
    and frame_roi_pixels.  The .bin files are the same with or without.
    scenecut: a threshold in (0, 1] on the distance of consecutive pictures (vcm_ts_amd/scenecut.py; no default value
    exists).  A scan pass then reads every picture once, through the same pool and upload path as the coding pass, before
    anything is coded; an I picture opens a new GOP wherever the distance exceeds the threshold and the GOP is at least
    min_gop pictures old, `gop` becomes the longest GOP, and the plan is written to gops.json beside the .bin files
    (decode_folder follows it).  Without scenecut nothing changes and no such file is written.
    roi_q (with roi): a roi.RoiQ -- ROI-weighted quantisation.  The map of picture g is made from the roi's boxes of g on
    the stream that codes it (one small launch per picture) and multiplies the quantisation step of the latent y cell by
    cell; the factors are written to roiq.json beside the .bin files, and decode_folder / decode_video then need the same
    roi.  The .bin format is unchanged.  Without roi_q nothing changes, no kernel is launched and no such file is written
    (a stale one is removed).
    bit_map: True (needs report), or a folder -- where the bits of every picture went (vcm_ts_amd/bitmap.py: the code lengths
    of the coder's own symbols, summed per 16x16 cell on the stream that coded the picture).  The report gains
    frame_bits_mv_z / _mv_y / _z / _y (floats in bits; the mv entries of an I picture are 0) and, with roi,
    frame_bits_roi / frame_bits_bg / frame_roi_cells: the bits and the number of the cells a box touches -- boxes grown by
    roi_q.grow when roi_q is on, by 0 otherwise.  A folder also receives im%05d.npy, the (1, hc, wc) float64 bits per cell of
    each picture.  One more host read per GOP; the .bin files are the same with or without.  None: nothing changes.
    target_bpp: rate control (vcm_ts_amd/ratectl.py) -- a target in bits per pixel of the unpadded picture.
    `q` is then the starting point: q[0] and q[1] stay the I and mv_y settings of every picture, and q[2] is what the first
    two P pictures of each GOP are coded with; from the third on the GOP's controller moves q_y inside q_range (a
    (lowest, highest) pair of q-scales, default the wire range [0.01, 655]).  The I picture is not controlled.  Every .bin
    header carries its own q indexes, so decoding needs nothing new.  With report the dictionary gains frame_q_y and
    frame_bits_target (null where nothing was decided).  None: no launch, file, key or byte changes.
    residual_bins (with roi): a folder -- it may be bin_dir -- for the CODED residual layer, im%05d.rl per picture
    (vcm_ts_amd/roilayer.py, include/dcvc_hip_roil.h): the residual inside the boxes, quantised with the integer
    residual_step (1 .. 64; 1 is lossless, S keeps every sample within S // 2), coded cell by cell on the stream that coded the
    picture; decode_folder / decode_video take the same folder in place of residuals=.  It may be given together with
    residuals=.  With report the dictionary gains frame_bits_enh (8 x the record's size), frame_bpp_enh,
    ave_all_frame_bpp_enh and ave_all_frame_bpp_total (base + enhancement).  None: no launch, file, key or byte changes.
    picture_hash: write hashes.json beside the .bin files (vcm_ts_amd/picturehash.py): per coded picture the CRC-32 of the
    8-bit codes of the unpadded reconstruction (`pixels`: the bytes of its PNG) and of the fp32 bits of the padded
    reference picture (`state`), taken on the stream that coded the picture -- two small launches each, one host read per
    GOP -- and the engine's precision.  Written once, after everything was coded; decode_folder / decode_video follow it.
    The .bin files are the same with or without.  False: no launch, key or byte changes and no file (a stale one is
    removed).
    base_scale: a ratio n/d with 1/4 <= n/d < 1 (a Fraction, an (n, d) pair or "n/d") -- code the base layer at reduced size
    (vcm_ts_amd/scale.py).  Each side becomes (2 side n + d) // (2 d); every picture is scaled down on the stream
    that codes it (one launch) and then padded as usual, so the .bin files are an ordinary sequence of base-size pictures,
    and scale.json beside them says how decode_folder / decode_video scale them up.  Everything that looks at a
    reconstruction sees it scaled up to the full size, on the same stream, only when something does: recon_dir, report
    (PSNR, MS-SSIM and the ROI figures against the full-size source; every bpp per full-size pixel), residuals and
    residual_bins (taken against the up-scaled picture, boxes in full-size coordinates) and picture_hash (`pixels` is of the
    up-scaled picture, `state` of the base reference picture).  target_bpp counts full-size pixels; the scene-cut scan sees
    the full-size source; bit_map without roi maps the base grid.  With roi_q, or bit_map with roi: NotImplementedError.
    None: no launch, file, key or byte changes (a stale scale.json is removed).
    aq: an aq.AQ -- backward-adaptive quantisation (vcm_ts_amd/aq.py).  Every P picture is coded with a
    q-scale map made on the stream that codes it from its own reference picture (a memset and two launches per picture):
    cells flatter than the reference's mean activity get a finer step of the latent y, busier ones a coarser one.  The
    decoder holds the same reference picture and rebuilds the map, so the .bin format is unchanged and no map is stored;
    aq.json beside the .bin files records the setting and the digests of its two tables, and decode_folder / decode_video
    follow it.  I pictures are not adapted.  With roi_q the two factors multiply; with base_scale the map is taken from the
    base-size reference; target_bpp prices every picture under its map.  None: no launch, file or byte changes (a stale
    aq.json is removed).
    tnr: a tnr.TNR -- the motion-adaptive temporal noise prefilter (vcm_ts_amd/tnr.py).  Every P picture
    the codec is handed is the source blended with the previous filtered picture where the luma of the two stays close
    over a 5 x 5 window, and the source itself where something moves (one launch per P picture on the stream that codes
    it, before base_scale's scaling); the filter restarts at every I picture of the plan, so gop_streams and scenecut keep
    giving the bytes of sequential coding.  Encoder side only: no file is written and decode_folder / decode_video need
    nothing.  The report's PSNR / MS-SSIM / ROI figures, residuals / residual_bins, the scene-cut scan and `boxes` keep
    looking at the UNFILTERED source; aq, target_bpp, roi_q, bit_map, picture_hash and base_scale simply code the filtered
    picture.  With report the dictionary gains tnr (the setting), frame_tnr_held (the fraction of the picture's pixels that
    were blended) and frame_tnr_mad (the mean absolute luma difference to the previous filtered picture, in codes), both 0.0
    for an I picture.  With tnr.search (motion compensation, opt-in) that previous picture is moved cell by cell by the
    vectors of a block search first, and the report also gains frame_tnr_moved (the cells with a nonzero vector among the
    cells that hold a pixel) and frame_tnr_mad_zero (frame_tnr_mad against the picture as it stood), 0.0 for an I picture.
    With tnr.subpel (opt-in, with tnr.search) the vectors are refined to quarter pixels and that picture is interpolated;
    the report gains frame_tnr_subpel (the cells whose vector has a fractional component among the cells that hold a pixel).
    With tnr.split (opt-in, with tnr.search) every 8 x 8 sub-cell chooses again among its cell's vector and the neighbours'
    and that picture is moved sub-cell by sub-cell; the report gains frame_tnr_split (the sub-cells whose vector differs from
    their cell's among the sub-cells that hold a pixel).
    With tnr.levels = L (opt-in, with tnr.search, which may then reach 64 L pixels) the search is hierarchical over L coarser
    levels of 2 x 2 luma means; the report gains frame_tnr_far (the cells whose vector has a component beyond 32 pixels among
    the cells that hold a pixel).
    With tnr.intra = K (look-ahead, opt-in) every I picture is blended in one dcvc_tnr_fuse launch with up to K pictures that
    follow it in its own GOP (pulled ahead from the source by a _LookAhead, never past the next I picture), the P pictures
    start from the filtered I picture, the figures above are those of reference 0 for such an I picture, and the report
    gains frame_tnr_refs (n, 1 for a P picture, 0 for an I picture left as it was).
    A tnr.AutoTNR in place of the TNR: the threshold is measured.  Before anything is coded a scan pass --
    the scene-cut scan's own pass where scenecut is given too, so the source is read once before it is coded either way --
    hands every picture to a noise.NoiseScan, the whole source's estimate resolves the setting to a plain TNR, and everything
    above holds for that TNR; one estimate for every GOP, so gop_streams keeps the bytes of sequential coding.  noise.json
    beside the .bin files (informational: no decoder reads it) and the report's `noise` key hold the estimate, the scale and
    the resolved threshold and pixel.  A source without an estimate is a ValueError that says to pass a TNR.
    None: no launch, allocation, key or byte changes (a stale noise.json is removed).
    redact (with roi): a redact.Redact -- ROI redaction (vcm_ts_amd/redact.py).  Inside the boxes of the named
    classes (grown by redact.grow; with redact.hold also the boxes of that many pictures before and after) the picture the
    codec is handed is a mosaic of the source on a picture-aligned grid, or a solid fill: one launch per picture that has
    such a box on the stream that codes it, after tnr and before base_scale's scaling; a picture without one launches
    nothing.  I and P pictures alike.  Encoder side only: the .bin format is unchanged and decode_folder / decode_video need
    nothing; redact.json beside the .bin files records the setting for whoever receives them.  The report's PSNR / MS-SSIM /
    ROI figures, the scene-cut scan and `boxes` keep looking at the UNREDACTED source; with report the dictionary gains
    redact (the setting) and frame_redacted (the fraction of the picture's pixels that were replaced).  residuals /
    residual_bins are taken from the unredacted source too, so those files would hold what was removed inside the boxes
    themselves: that combination is a ValueError unless redact.restorable is set.  A mosaic is not a security guarantee.
    None: no launch, allocation, file, key or byte changes (a stale redact.json is removed).
    png_device: the PNGs of recon_dir are made on the device (vcm_ts_amd/pngdev.py; include/dcvc_hip_png.h): the same pixels
    in other, usually somewhat larger, files, and no picture crosses to the host as float32.  A ValueError without recon_dir
    and for a picture wider than 8191.  False: no launch, file or byte changes.
    grain: a grain.Grain, with tnr= -- film-grain synthesis (vcm_ts_amd/grain.py): right behind the filter's
    launch, one dcvc_grain_measure per P picture adds up what the filter took out of the cells it blended throughout, and
    grain.json beside the .bin files keeps, per GOP, eight strengths by intensity, two taps and the sample counts -- the
    same file with one or two GOP streams.  decode_folder(grain=) synthesises from it; nothing else reads it.  The .bin
    files, recon_dir, the report and hashes.json are those of an encode without it.  Without tnr= a ValueError.  None: no
    launch, allocation, key or byte changes (a stale grain.json is removed).
    shake: a shake.ShakeParams, with a tnr.AutoTNR -- the camera's shake is taken out ahead of the noise scan
    (vcm_ts_amd/shake.py): every picture of the scan pass is registered onto picture 0 by one whole-pixel
    vector before the noise scan sees it; the scene-cut scan and the coding pass keep the pictures as they are.  noise.json and
    the report's `noise` gain a "shake" summary and shake.json beside the .bin files holds the per-picture records.  A
    source with more than shake.max_lost percent of its pictures lost is a ValueError: the camera moves, pass a tnr.TNR.
    Without a tnr.AutoTNR a ValueError.  None: no launch, allocation, file, key or byte changes (a stale shake.json is
    removed)."""
    options = locals()
    frames_dir, recon_dir, max_frames, png_device = (options.pop(name) for name in ("frames_dir", "recon_dir", "max_frames", "png_device"))
    return _encode_sequence(_PngSource(frames_dir, device, io_workers, max_frames),
                            _PngStage(recon_dir, io_workers, device if png_device else None), **options)


def _decode_bins(nets, bin_dir, height, width, plan, emit, q_map=None, aq=None):
    """Decode im00001.bin ... of `bin_dir` (I pictures where `plan`, read_gop_plan's, has them) in order, handing every
    reconstruction to emit(t, ref_frame) while it is valid.  q_map(t): the q-scale map picture t was coded with (None: no
    maps).  aq: the aq.AqMaps of the folder's aq.json (None: none).  Returns the picture count."""
    i_net, p_net = nets
    i_net.update()
    p_net.update()
    dpb = None

    def range_guard():  # once per GOP: raises lib.KernelError if a split-fp16 kernel clamped an activation
        i_net.engine().check_status()
        p_net.engine().check_status()

    with torch.no_grad():
        for t in range(plan.n_frames):
            path = os.path.join(bin_dir, f"im{str(t + 1).zfill(5)}.bin")
            if plan.is_intra(t):
                if t:
                    range_guard()
                h, w, qi, payload = S.decode_i(path)
                assert (h, w) == (height, width)
                kind, q = "I", (qi,)
            else:
                qmv, qy, payload = S.decode_p(path)
                kind, q = "P", (qmv, qy)
            dpb = decode_picture(i_net, p_net, kind, q, payload, dpb, height, width, q_map=q_map(t) if q_map else None,
                                 aq=aq)
            emit(t, dpb["ref_frame"])
        if plan.n_frames:
            range_guard()
    return plan.n_frames


def _verify_args(verify, bin_dir, plan, height, width):
    """verify= of a decode loop -> (the folder's hashes.json record or None, the mode), refused by name before any GPU
    work (picturehash.verify_mode, check_record).  Mode "off" reads no file."""
    from . import picturehash as PH

    if verify == "off":
        return None, "off"
    record = PH.read_hashes(bin_dir)
    mode = PH.verify_mode(verify, record, bin_dir)
    if mode != "off":
        l, r, t, b = S.get_padding_size(height, width)
        PH.check_record(record, plan, height, width, (height + t + b, width + l + r), os.path.join(bin_dir, PH.HASHES_JSON))
    return record, mode


def _decode_grain(grain, bin_dir, plan, residuals, residual_bins, base_scale):
    """grain= of a decode loop (None, or the per cent of the measured strength) -> None, or (the folder's checked grain.json
    record, per cent); refused by name before any GPU work."""
    if grain is None:
        return None
    from . import grain as GR
    from .devargs import whole

    percent = whole("grain", grain, 1, GR.MAX_PERCENT, "per cent of the measured strength")
    if residuals is not None or residual_bins is not None:
        raise NotImplementedError("grain= with residuals= / residual_bins= (--grain with --residuals / --residual-bins): inside "
                                  "lossless boxes the source's own noise is already there, and sparing boxes is not implemented")
    if base_scale is None:
        raise ValueError("a base-only decode (base_scale=None, --base-only) takes no grain= (--grain): the grain was measured "
                         "at display size")
    return GR.read_grain(bin_dir, plan), percent


def _grain_synth(grain, plan, shown, dev):
    """The grain.GrainSynth of a decode loop (None without grain=: nothing is allocated)."""
    if grain is None:
        return None
    from .grain import GrainSynth

    return GrainSynth(grain[0], plan, shown, dev, grain[1])


def _decode_sequence(bin_dir, size, out, gop=None, device="cuda:0", precision=None, i_ckpt=None, p_ckpt=None, roi=None,
                     residuals=None, residual_bins=None, verify=None, base_scale="file", check=None, grain=None):
    """The one decode loop: the .bin files of `bin_dir`, pictures of the display `size` = (height, width), through the
    verifier, the base layer's up-scaling, the grain synthesis and the ROI fusion into `out` (a _PngStage or a _VideoStage).  The options are
    decode_folder's.  check(shown, coded, scaled): the caller's own refusals once the size of what is written is known.
    Every refusal comes before any launch and before `out` is opened."""
    from . import aq as A
    from . import picturehash as PH
    from . import scale as SC

    height, width = size
    _roi_args(roi, residuals, residual_bins, decode=True)
    plan, _ = read_gop_plan(bin_dir, gop)
    roi_q = read_roiq(bin_dir, roi)
    aq = A.read_aq(bin_dir)  # (host work only: its refusals come here, the maps are made once every refusal has had its turn)
    record, verify = _verify_args(verify, bin_dir, plan, height, width)
    grain = _decode_grain(grain, bin_dir, plan, residuals, residual_bins, base_scale)
    dev = torch.device(device)
    scaled, coded = _decode_scale(bin_dir, height, width, base_scale, roi, residuals, residual_bins)
    shown = (height, width) if scaled else coded  # (the size of what is written)
    if check:
        check(shown, coded, scaled)
    base = _BaseLayer(SC.Scale(scaled["full"], scaled["ratio"], dev)) if scaled else None
    fuse_roi = _fuse_roi(roi, residuals, roi_q, residual_bins)
    picture, close = _fused_emit(fuse_roi, residuals, plan, shown, dev, residual_bins)
    try:
        maps = _decode_maps(roi, roi_q, plan, (height, width), dev)
        aq = A.AqMaps(aq, dev) if aq is not None else None
        nets = _nets(dev, precision, i_ckpt, p_ckpt)
        checker = PH.Verifier(record, verify, plan, shown, nets[1].engine().precision, shown == (height, width)) \
            if verify != "off" else None
        synth = _grain_synth(grain, plan, shown, dev)
        out.open(shown)

        def emit(t, ref_frame):
            full = base.shown(0, t, ref_frame) if base else None
            if checker:
                checker.add(t, ref_frame, display=full)
            if full is not None:
                ref_frame = full
            if synth:  # (display side only, after the verifier: the digests and the DPB are of the ungrained picture)
                ref_frame = synth.shown(t, ref_frame)
            # (without a ROI the padded reconstruction itself: the stage reads its top-left corner in place)
            out.put(0, t, ref_frame if fuse_roi is None else picture(t, ref_frame))

        failed = True
        try:
            n = _decode_bins(nets, bin_dir, coded[0], coded[1], plan, emit, maps, aq)
            if checker:
                checker.finish()
            out.flush()
            failed = False
        finally:
            out.close(failed)
        return n
    finally:
        close()


def decode_folder(bin_dir, recon_dir, height, width, gop=None, device="cuda:0", precision=None, i_ckpt=None, p_ckpt=None,
                  io_workers=8, roi=None, residuals=None, residual_bins=None, verify=None, base_scale="file", png_device=False,
                  grain=None):
    """roi, residuals: write video_coder.fuse_layers' picture instead of the reconstruction -- `residuals` is the decoded
    residual layer (a `.gbrp` file or a folder of im%05d.png, as encode_folder writes them) and `roi` the boxes and
    classes it was taken with.  Display side only: the decoder's reference pictures are not touched.
    gop: an I picture every `gop` pictures (default 32) -- unless encode left a gops.json beside the .bin files, which then
    says where the I pictures are; a `gop` given against it is refused (read_gop_plan).
    A roiq.json beside the .bin files (encode_folder's roi_q=) is followed: the q-scale maps are rebuilt from `roi`, which
    is then required -- with or without residuals.
    residual_bins: in place of residuals=, the folder of im%05d.rl records encode_folder's residual_bins= wrote: each is
    held against the frame's boxes by name before any GPU work, decoded on the device and fused.  Giving both is refused.
    verify: "strict", "pixels", "warn" or "off" -- what to do with a hashes.json beside the .bin files (encode_folder's
    picture_hash=), which is followed without any option: None means "pixels" with the file and "off" without.  Both
    digests of every decoded base-layer reconstruction (before ROI fusion) are taken on the device and compared GOP by GOP
    as their copies complete -- the pictures of the GOP in flight, and of the one being compared, may already have been
    written.  "pixels": picturehash.PictureHashMismatch at the first picture whose `pixels` digest differs, one warning at
    the first whose `state` alone differs; "strict": raises on either; "warn": never raises; "off": launches nothing.
    Refused by name before any launch: a mode other than "off" without the file, and a record of another frame count,
    picture size or padded size.
    base_scale: "file" -- a scale.json beside the .bin files (encode_folder's base_scale=) is followed: height and width stay
    the DISPLAY size, the .bin files hold the base-size pictures, and every reconstruction is scaled up on the device
    before it is fused and written (display side only: the DPB keeps the base picture); the `pixels` digest is of the
    up-scaled, unfused picture.  None: ignore the file and write the base-size pictures -- what a decoder that knows
    nothing of it gets anyway; `pixels` is then not checked, and a ROI is refused.  Also refused by name before any launch: a
    scale.json of another display size, of another base size than the .bin files', or whose tables this host builds
    differently (scale.read_scale).
    An aq.json beside the .bin files (encode_folder's aq=) is followed without any option: every P picture's q-scale map is
    rebuilt from the decoder's own reference picture (also in a base-only decode, from the base-size one).  Refused by
    name before any launch: an aq.json of an unknown version, with a value out of range, or whose tables this host builds
    differently (aq.read_aq).
    png_device: the PNGs are made on the device, as encode_folder's png_device= makes them.
    grain: None, or 1 .. 200 -- film-grain synthesis (vcm_ts_amd/grain.py) at that per cent of the strength the folder's
    grain.json (encode_folder's grain=) measured.  OPT-IN: the file is never followed silently.  Every P picture that is
    written is a grained copy (one dcvc_grain_apply launch, after the verifier and the base layer's up-scaling, so at display
    size); I pictures (unless the record's tnr entry says intra: encode_folder's tnr=TNR(..., intra=K)), the DPB and the digests
    are untouched, so verify= keeps checking the ungrained picture, while the
    PNGs of a grained folder deliberately do NOT pass `run_codec verify`.  Refused by name before any launch: no
    grain.json, one of an unknown version, with a value out of range or whose GOPs are not the folder's plan, and a base-only
    decode; with residuals= / residual_bins= a NotImplementedError."""
    return _decode_sequence(bin_dir, (height, width), _PngStage(recon_dir, io_workers, device if png_device else None), gop, device, precision, i_ckpt, p_ckpt, roi,
                            residuals, residual_bins, verify, base_scale, grain=grain)


# ------------------------------------------------------------------------------------------------- Y4M / raw YUV files
SEQUENCE_JSON = "sequence.json"


def write_sequence_info(bin_dir, width, height, frames, gop, fps, spec, container, chroma=None, interlace=None, aspect=None,
                        roi=None, residual_step=None, deinterlace=None):
    """What decode_video needs beside the .bin files (which stay what they are): size, frame count, GOP length, frame
    rate and colour description of the source, and the container it came in.  deinterlace: the deint.Deinterlace the
    pictures were made with, for information (frames, fps and interlace are then the coded pictures': progressive)."""
    info = {"width": int(width), "height": int(height), "frames": int(frames), "gop": int(gop),
            "fps": list(fps) if fps else None, "color": spec.to_json(), "container": container, "chroma": chroma,
            "interlace": interlace, "aspect": aspect}
    if roi is not None:  # class order and borders of the enhancement layer (the boxes themselves stay where they are)
        info["roi"] = roi.to_json()
    if residual_step is not None:  # the step of the coded residual layer (residual_bins=; every record carries it too)
        info["residual_step"] = int(residual_step)
    if deinterlace is not None:
        info["deinterlace"] = deinterlace.to_json()
    return S.write_sidecar(bin_dir, SEQUENCE_JSON, info)


def read_sequence_info(bin_dir):
    """The dictionary write_sequence_info stored (with "color" as a ColorSpec), or None without the file."""
    from .yuv import ColorSpec

    found = S.read_sidecar(bin_dir, SEQUENCE_JSON)
    if found is None:
        return None
    info = found[1]
    info["color"] = ColorSpec.from_json(info["color"])
    info["fps"] = tuple(info["fps"]) if info.get("fps") else None
    return info


class _VideoOut:
    """Output stage of one stream: a reconstruction becomes 4:2:0 samples on the stream that produced it
    (yuv.rgb_to_yuv420) and leaves the device as 1.5 bytes per pixel into a ring of pinned buffers; a buffer is written to
    the file, at the place its frame number gives it, when the ring comes round to it (or at close), so the host never
    waits for the picture it has just enqueued.  Several of these share one writer: frames land in display order
    whatever order the GOP streams finish in."""

    def __init__(self, writer, depth=4):
        from collections import deque

        self.writer, self.depth, self.free, self.busy = writer, depth, [], deque()

    def put(self, g, samples):
        if len(self.busy) >= self.depth:
            self._retire()
        host = self.free.pop() if self.free else torch.empty(self.writer.frame_bytes, dtype=torch.uint8).pin_memory()
        host.copy_(samples.view(torch.uint8), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(samples.device))
        self.busy.append((ev, host, g, samples))  # (samples: kept until its copy has run)

    def _retire(self):
        ev, host, g, _ = self.busy.popleft()
        ev.synchronize()
        self.writer.write(g, host.numpy())
        self.free.append(host)

    def close(self):
        while self.busy:
            self._retire()


class _VideoQualityLog(_QualityLog):
    """_QualityLog plus integer sums per picture: the three of rgb_to_yuv420(..., source=), the three of
    roi.region_sse, or the six of both.  They ride in the GOP's one asynchronous transfer as raw bits (an int64 seen as
    two float32 lanes of the row; nothing computes on them)."""

    def add_yuv(self, g, recon, source, size, sums):
        self._add(g, recon, source, size, sums.view(torch.float32))

    def _more(self, host):
        """collect() gives {frame number: (psnr dB, ms-ssim, the integer sums as a tuple)}"""
        return [(tuple(s),) for s in host[:, 2:].contiguous().view(torch.int64).tolist()]


class _RoiLayer:
    """The boxes of a file loop.  Every frame's list is read and validated when the loop starts (each refusal happens
    by name before any GPU work); the lists of one GOP go to the device in ONE pinned asynchronous copy, on the stream
    that codes the GOP, when its first picture asks."""

    def __init__(self, roi, plan, size, dev, frames=None):
        """frames: the lists to serve in place of the roi's own (the merged lists of a redaction)."""
        from . import roi as X

        if dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device())
        self.X, self.roi, self.plan, self.dev, self.size = X, X.as_roi(roi), plan, dev, size
        self.classes = self.roi.classes
        self.frames = [self.roi.frame(g, size[0], size[1]) for g in range(plan.n_frames)] if frames is None else list(frames)

    def q_map(self, g, roi_q):
        """The q-scale map of frame g on the current stream (roi.q_map: one launch, nothing synchronised)."""
        return self.X.q_map(self.boxes(g), self.size[0], self.size[1], roi_q, device=self.dev)

    def boxes(self, g):
        fb = self.frames[g]
        if len(fb) and not fb.attached(self.dev):
            frames = self.plan.gop_range(self.plan.gop_of(g))  # (never beyond the GOP: the next one may belong to another stream)
            group = [f for f in self.frames[frames.start:frames.stop] if len(f)]
            pin = torch.from_numpy(np.concatenate([f.array.reshape(-1) for f in group])).pin_memory()
            dev, at = pin.to(self.dev, non_blocking=True), 0
            for f in group:
                f.attach(pin, dev[at:at + 5 * len(f)])
                at += 5 * len(f)
        return fb


RESIDUAL_RAW_EXT = ".gbrp"


class _ResidualOut:
    """Where an encode loop's residual layer goes: a `.gbrp` file (raw G, B, R planes in display order whatever order
    the GOP streams finish in: roi.RawPlanarWriter behind one _VideoOut per stream) or a folder of im%05d.png."""

    def __init__(self, path, size, streams, io_workers):
        from . import roi as X

        self.X, self.path, (h, w) = X, path, size
        self.writer = self.savers = None
        if os.path.splitext(path)[1].lower() == RESIDUAL_RAW_EXT:
            self.writer = X.RawPlanarWriter(path, w, h)
            self.outs = [_VideoOut(self.writer) for _ in range(streams)]
        else:
            os.makedirs(path, exist_ok=True)
            self.savers = PNGWriters(io_workers)

    def put(self, k, g, source, recon, boxes):
        if self.writer:
            self.outs[k].put(g, self.X.residual_layer(source, recon, boxes, layout="planar", order="gbr").view(-1))
        else:
            a = self.X.residual_layer(source, recon, boxes, layout="hwc", order="rgb").cpu().numpy()
            self.savers.submit(a, os.path.join(self.path, f"im{str(g + 1).zfill(5)}.png"), _save_u8)

    def close(self, failed=False):
        try:
            if self.writer and not failed:
                for o in self.outs:
                    o.close()
        finally:
            if self.writer:
                self.writer.close()
            if self.savers:
                self.savers.__exit__(RuntimeError if failed else None, None, None)


class _ResidualIn:
    """A decoded residual layer, per frame on the device: a `.gbrp` file (roi.RawPlanarReader) or a folder of
    im%05d.png, through a ring of pinned buffers.  Everything about the files is checked when the loop starts."""

    def __init__(self, path, size, n_frames, dev):
        from . import roi as X

        (h, w), self.path, self.size = size, path, size
        self.reader = None
        if os.path.isdir(path):
            missing = [t + 1 for t in range(n_frames) if not os.path.exists(self.png(t))]
            if missing:
                raise ValueError(f"{path}: no residual picture im{str(missing[0]).zfill(5)}.png")
            self.layout, self.order, shape = "hwc", "rgb", (h, w, 3)
        else:
            self.reader = X.RawPlanarReader(path, w, h)
            if self.reader.n_frames < n_frames:
                self.reader.close()
                raise ValueError(f"{path}: {self.reader.n_frames} residual frames for {n_frames} pictures")
            self.layout, self.order, shape = "planar", "gbr", (3, h, w)
        self.ring = _PinnedRing(dev, shape)

    def png(self, t):
        return os.path.join(self.path, f"im{str(t + 1).zfill(5)}.png")

    def frame(self, t):
        host = self.ring.host()
        if self.reader:
            self.reader.read_into(t, host)
        else:
            a = PNGReader.load_u8(self.png(t))
            if a.shape != host.shape:
                raise ValueError(f"{self.png(t)}: a {a.shape[1]}x{a.shape[0]} picture, not {self.size[1]}x{self.size[0]}")
            host[...] = a
        return self.ring.upload()

    def close(self):
        if self.reader:
            self.reader.close()


class _RecordOut:
    """Where an encode loop's CODED residual layer goes: im%05d.rl in a folder (vcm_ts_amd/roilayer.py).  A picture's record
    is coded on the stream that coded the picture and leaves the device in one asynchronous copy to a pinned buffer; it is
    written to its file when its stream's ring comes round to it (or at close), as _VideoOut does, so the host never waits
    for the picture it has just enqueued, and every file carries its frame's number whatever order the GOP streams finish
    in.  sizes: {frame number: record bytes} of what has been written."""

    def __init__(self, folder, step, streams, depth=4):
        from collections import deque

        from . import roilayer as Y

        os.makedirs(folder, exist_ok=True)
        self.Y, self.folder, self.step, self.depth = Y, folder, step, depth
        self.busy, self.pool, self.sizes = [deque() for _ in range(streams)], [], {}

    def put(self, k, g, source, recon, boxes):
        if len(self.busy[k]) >= self.depth:
            self._retire(k)
        self.busy[k].append((g, self.Y.encode_layer(source, recon, boxes, self.step, pool=self.pool)))

    def _retire(self, k):
        g, pending = self.busy[k].popleft()
        data = pending.bytes()
        with open(os.path.join(self.folder, f"im{str(g + 1).zfill(5)}{self.Y.FILE_EXT}"), "wb") as f:
            f.write(data)
        self.sizes[g] = len(data)
        self.pool.append(pending.host)

    def close(self, failed=False):
        if not failed:
            for k in range(len(self.busy)):
                while self.busy[k]:
                    self._retire(k)


class _RecordIn:
    """A coded residual layer (im%05d.rl, _RecordOut's files), per frame decoded on the device into the planar picture
    roi.fuse reads.  Every file is read and held against the frame's boxes when the loop starts: a missing file or a record
    that disagrees with the boxes is named before any GPU work."""
    layout, order = "planar", "rgb"

    def __init__(self, folder, size, layer):
        from . import roilayer as Y

        self.Y, self.size, self.layer, self.records = Y, size, layer, []
        for t, boxes in enumerate(layer.frames):
            path = os.path.join(folder, f"im{str(t + 1).zfill(5)}{Y.FILE_EXT}")
            if not os.path.exists(path):
                raise ValueError(f"{folder}: no residual record im{str(t + 1).zfill(5)}{Y.FILE_EXT}")
            with open(path, "rb") as f:
                data = f.read()
            try:
                Y.check_record(data, Y.active_cells(boxes, size[0], size[1])[1])
            except Y.RoiLayerError as ex:
                raise Y.RoiLayerError(f"{path}: {ex}") from None
            self.records.append(data)

    def frame(self, t):
        return self.Y.decode_layer(self.records[t], self.layer.boxes(t), self.size[0], self.size[1], layout=self.layout,
                                   order=self.order, device=self.layer.dev)

    def close(self):
        pass


def _roi_args(roi, residuals, residual_bins=None, residual_step=1, decode=False):
    """The residual-layer arguments of a file loop against its roi=, refused by name before any GPU work."""
    if residuals is not None and roi is None:
        raise ValueError("residuals= needs roi= (the boxes the residual layer is taken in)")
    if residual_bins is not None and roi is None:
        raise ValueError("residual_bins= needs roi= (the boxes the residual layer is coded in)")
    if decode and residuals is not None and residual_bins is not None:
        raise ValueError("give one of residuals= (a decoded residual layer) and residual_bins= (a coded one), not both")
    if residual_bins is not None and not isinstance(residual_bins, (str, os.PathLike)):
        raise ValueError(f"residual_bins: expected a folder, got {type(residual_bins).__name__}")
    if not decode:
        from .roilayer import check_step

        if check_step(residual_step) != 1 and residual_bins is None:
            raise ValueError("residual_step= belongs to residual_bins= (the coded residual layer)")


def _enh_report_keys(rec_out, h, w):
    """--report's keys of the enhancement layer, video_coder.calc_bitrate_metrics' three figures: the record's bits and bpp
    per picture, their average, and base + enhancement."""
    def keys(rd, types, values):
        bits = [8 * rec_out.sizes[g] for g in sorted(rec_out.sizes)]
        rd["frame_bits_enh"] = bits
        rd["frame_bpp_enh"] = [b / (h * w) for b in bits]
        rd["ave_all_frame_bpp_enh"] = sum(rd["frame_bpp_enh"]) / len(bits) if bits else 0
        rd["ave_all_frame_bpp_total"] = rd["ave_all_frame_bpp"] + rd["ave_all_frame_bpp_enh"]

    return keys


class _LookAhead:
    """An iterator over `items` (the pictures of ONE GOP stream, in coding order) that yields every item exactly once and in
    order and, at an I picture, lets the caller see the items that follow it in its own GOP: after next() has returned
    item t, .ahead is the list of the next min(K, items before the stream's next I picture or its end) items when t is in
    `intra`, and [] otherwise.  Nothing is ever pulled past the next I picture or past item n - 1; between two I pictures the
    items pulled ahead are handed out before anything more is pulled.  hold(item) -> what is kept of an item pulled ahead
    (a source whose items are views of recycled memory copies them here).  K None (or 0): one item is pulled per item
    yielded, exactly as iter(items) would.  Plain Python: no GPU, no torch."""

    def __init__(self, items, intra, K, n, hold=None):
        from collections import deque

        self._items, self._intra, self._K, self._n, self._hold = iter(items), intra, K or 0, n, hold
        self._held, self._t, self.ahead = deque(), 0, []

    def __iter__(self):
        return self

    def __next__(self):
        item = self._held.popleft() if self._held else next(self._items)
        t, self._t = self._t, self._t + 1
        self.ahead = []
        if self._K and t in self._intra:
            while len(self._held) < self._K:
                nxt = t + 1 + len(self._held)
                if nxt >= self._n or nxt in self._intra:
                    break
                pulled = next(self._items)
                self._held.append(pulled if self._hold is None else self._hold(pulled))
            self.ahead = list(self._held)
        return item


def _held_ahead(item):
    """_LookAhead's hold= of a source's (picture, aux): the padded RGB picture is a fresh tensor of its own; the file's
    samples (a video source's aux) came up through the pinned ring on the copy stream, so a picture that waits is given a
    copy made on the stream that will read it."""
    x, aux = item
    return x, (aux.clone() if aux is not None else None)


def _tnr_filters(tnr, run, size, report):
    """tnr= of an encode loop -> one tnr.TnrFilter per GOP stream (None without: nothing is allocated).  Per-picture totals
    are kept only for a report."""
    if tnr is None:
        return None
    from .tnr import TnrFilter

    return [TnrFilter(tnr, size, run.dev, totals=bool(report)) for _ in range(run.K)]


def _grain_args(grain, tnr):
    """grain= of an encode loop against its tnr=, refused by name before any GPU work."""
    if grain is not None:
        from .grain import Grain

        if not isinstance(grain, Grain):
            raise ValueError(f"grain: expected a grain.Grain, got {type(grain).__name__}")
        if tnr is None:
            raise ValueError("grain= needs tnr= (--grain needs --tnr): what is measured is what the prefilter took out")


def _grain_meters(grain, bin_dir, run, size):
    """grain= of an encode loop -> one grain.GrainMeter per GOP stream (None without: nothing is allocated).  A grain.json
    of an earlier encode into the same folder must not describe these .bin files: ours is written when all is coded."""
    from . import grain as GR

    GR.write_grain(bin_dir, None)
    return [GR.GrainMeter(size, run.dev) for _ in range(run.K)] if grain is not None else None


def _write_grain(bin_dir, grain, tnr, meters):
    """grain.json: once, when everything has been coded -- every GOP's record from its own sums, whichever stream coded it."""
    from . import grain as GR

    sums = {}
    for m in meters:
        sums.update(m.sums())
    GR.write_grain(bin_dir, GR.record_of(grain, tnr, {g: GR.params(acc, grain.min_samples) for g, acc in sums.items()}))


def _tnr_args(tnr):
    """tnr= of an encode loop, refused by name before any GPU work."""
    if tnr is not None:
        from .tnr import TNR, AutoTNR

        if not isinstance(tnr, (TNR, AutoTNR)):
            raise ValueError(f"tnr: expected a tnr.TNR or a tnr.AutoTNR, got {type(tnr).__name__}")


NOISE_JSON, SHAKE_JSON = "noise.json", "shake.json"


def _shake_args(shake, tnr):
    """shake= of an encode loop, refused by name before any GPU work."""
    if shake is not None:
        from .shake import ShakeParams

        if not isinstance(shake, ShakeParams):
            raise ValueError(f"shake: expected a shake.ShakeParams, got {type(shake).__name__}")
        if _tnr_auto(tnr) is None:
            raise ValueError("shake belongs to a tnr.AutoTNR (--tnr-auto): it steadies the noise scan, and the coding pass is not touched")


def _tnr_auto(tnr):
    """tnr= of an encode loop where it is a tnr.AutoTNR (checked by _tnr_args), else None."""
    from .tnr import AutoTNR

    return tnr if isinstance(tnr, AutoTNR) else None


def _resolve_tnr(tnr, estimate, moved=None):
    """(the tnr.TNR of an encode loop's tnr=, what noise.json and --report's `noise` say -- with `moved`, what shake.json
    says, also its summary under "shake").  A TNR, or None, is itself and
    says nothing; a tnr.AutoTNR is resolved with the scan pass's estimate of the whole source -- one estimate for every GOP,
    GOP stream and shard -- or refuses by name where there is none."""
    auto = _tnr_auto(tnr)
    if auto is None:
        return tnr, None
    resolved = auto.resolve(estimate)
    return resolved, dict(estimate.to_json(), scale=auto.scale, threshold=resolved.threshold, pixel=resolved.pixel,
                          **({} if moved is None else {"shake": moved["summary"]}))


def _noise_report_keys(measured):
    """--report's `noise` key: what noise.json holds."""
    def keys(rd, types, values):
        rd["noise"] = dict(measured)

    return keys


def _stream_totals(steps, run):
    """{frame number: its totals} of the tnr.StreamFilters of the GOP streams.  The totals of each stream were copied to
    the host GOP by GOP; this waits for those copies only."""
    totals = {}
    for k, f in enumerate(steps):
        with torch.cuda.stream(run.cenc.streams[k]):
            per = f.totals()  # (flushes a trailing partial GOP)
        totals.update({run.global_index(k, t): v for t, v in enumerate(per)})
    return totals


def _tnr_report_keys(tnr, filters, run, h, w):
    """--report's keys of the temporal noise prefilter: the setting, and per picture the fraction of its pixels that were
    blended and the mean absolute luma difference to the previous filtered picture, both 0.0 for an I picture.  With
    tnr.search that picture is the motion-compensated one, and two more keys speak of the search: frame_tnr_moved, the
    cells with a nonzero vector among the cells that hold a pixel, and frame_tnr_mad_zero, what frame_tnr_mad would have
    been against the uncompensated picture; 0.0 for an I picture too.  With tnr.intra an I picture that had pictures ahead
    of it is filtered and has figures of its own (against reference 0, the picture that follows it), and frame_tnr_refs
    is the number of references of every picture: n for such an I picture, 1 for a P picture, 0 for an I picture left as
    it was.  With tnr.subpel the vectors are quarter pixels, and frame_tnr_subpel is the cells whose vector has a fractional
    component among the cells that hold a pixel, 0.0 where nothing was searched.  With tnr.split frame_tnr_split is the
    sub-cells whose vector differs from their cell's among the 8 x 8 sub-cells that hold a pixel, 0.0 where nothing was
    searched.  With tnr.levels frame_tnr_far is the cells whose vector has a component beyond 32 pixels among the cells that
    hold a pixel, 0.0 where nothing was searched."""
    def keys(rd, types, values):
        totals = _stream_totals(filters, run)
        order = sorted(totals)
        rd["tnr"] = tnr.to_json()
        rd["frame_tnr_held"] = [totals[g][0] / (h * w) for g in order]
        rd["frame_tnr_mad"] = [totals[g][1] / (h * w) for g in order]
        if tnr.search is not None:  # (the totals' rows are then (held, sad, moved, zero))
            cells = -(-h // 16) * -(-w // 16)  # the cells that hold a pixel
            rd["frame_tnr_moved"] = [totals[g][2] / cells for g in order]
            rd["frame_tnr_mad_zero"] = [totals[g][3] / (h * w) for g in order]
            if tnr.subpel:  # (the rows are then (held, sad, moved, zero, frac); moved counts quarter-pel vectors)
                rd["frame_tnr_subpel"] = [totals[g][4] / cells for g in order]
            if tnr.split:  # (the next column: the sub-cells that left their cell's vector)
                subs = -(-h // 8) * -(-w // 8)  # the sub-cells that hold a pixel
                rd["frame_tnr_split"] = [totals[g][5 if tnr.subpel else 4] / subs for g in order]
            if tnr.levels is not None:  # (the next column: the cells beyond the full search's reach)
                rd["frame_tnr_far"] = [totals[g][4 + tnr.subpel + tnr.split] / cells for g in order]
        if tnr.intra is not None:  # (every row then ends with the number of references of the step)
            rd["frame_tnr_refs"] = [totals[g][-1] for g in order]

    return keys


REDACT_JSON = "redact.json"


def _redact_args(redact, roi, residuals, residual_bins):
    """redact= of an encode loop against its roi= and residual outputs, refused by name before any GPU work."""
    if redact is None:
        return
    from . import roi as X
    from .redact import Redact

    if not isinstance(redact, Redact):
        raise ValueError(f"redact: expected a redact.Redact, got {type(redact).__name__}")
    if roi is None:
        raise ValueError("redact= needs roi= (the boxes to redact)")
    redact.mask(X.as_roi(roi).names)
    if (residuals is not None or residual_bins is not None) and not redact.restorable:
        raise ValueError("redact= with residuals= / residual_bins=: the residual layer is taken from the unredacted source, so "
                         "its files would hold what the redaction removes; say so with restorable=True (--redact-restorable) "
                         "and guard those files, or leave them out")


def _redact_frames(redact, layer):
    """The merged list of every picture (redact.held_boxes), or None without redact=: host work, before any launch."""
    if redact is None:
        return None
    from .redact import held_boxes

    mask = redact.mask(layer.roi.names)
    return [held_boxes(layer.frames, g, mask, redact.hold) for g in range(layer.plan.n_frames)]


def _write_redact(bin_dir, redact):
    """redact.json beside the .bin files of a redacted encode -- so that a receiver knows; decode ignores it.  Without
    redact= a stale file is removed."""
    S.write_sidecar(bin_dir, REDACT_JSON, None if redact is None else redact.to_json())


class _Redaction:
    """redact= of an encode loop: the merged lists (uploaded GOP by GOP like the roi's own) and one redact.Redactor per GOP
    stream.  Per-picture totals are kept only for a report."""

    def __init__(self, redact, layer, held, run, report):
        from .redact import Redactor

        self.layer = _RoiLayer(layer.roi, layer.plan, layer.size, layer.dev, held)
        self.steps = [Redactor(redact, layer.roi, layer.size, run.dev, totals=bool(report)) for _ in range(run.K)]

    def step(self, k, g, x, intra):
        if intra:
            self.steps[k].flush()  # (the GOP before this one: its totals, if any are kept, go to the host in one copy)
        return self.steps[k].step(x, self.layer.boxes(g))


def _redact_report_keys(redact, redaction, run, h, w):
    """--report's keys of the redaction: the setting, and per picture the fraction of its pixels that were replaced."""
    def keys(rd, types, values):
        totals = _stream_totals(redaction.steps, run)
        rd["redact"] = redact.to_json()
        rd["frame_redacted"] = [totals[g] / (h * w) for g in sorted(totals)]

    return keys


def _fuse_roi(roi, residuals, roi_q, residual_bins=None):
    """The roi a decode loop fuses a residual layer with: none when the roi is only there for the q-scale maps."""
    return None if (residuals is None and residual_bins is None and roi_q is not None) else roi


def _decode_maps(roi, roi_q, plan, size, dev):
    """q_map(t) of a decode loop that follows a roiq.json, or None without one."""
    if roi_q is None:
        return None
    layer = _RoiLayer(roi, plan, size, dev)
    return lambda t: layer.q_map(t, roi_q)


def _bit_log(bit_map, bit_dir, layer, roi_q):
    """_EncodeRun's bit_log of an encode loop: (labels of frame g or None without a ROI, the folder or None); None without
    bit_map."""
    if not bit_map:
        return None
    if layer is None:
        return None, bit_dir
    from .bitmap import labels_from_boxes

    grow = roi_q.grow if roi_q is not None else 0
    return (lambda g: labels_from_boxes(layer.boxes(g), layer.size[0], layer.size[1], grow, device=layer.dev)), bit_dir


def _deint_report_keys(source):
    """`deinterlace` (the setting) and `frame_deint_moved` (per picture, the missing luma samples that were not simply
    woven) of a source that deinterlaces; None for any other."""
    if getattr(source, "moved", None) is None:
        return None

    def keys(rd, types, values):
        rd["deinterlace"] = source.deinterlace.to_json()
        rd["frame_deint_moved"] = source.deint_moved()

    return keys


def _roi_report_keys(h, w):
    def keys(rd, types, values):
        from . import roi as X

        per = [X.region_psnr(v[2][-3:], h, w, "samples") for v in values]
        rd["frame_psnr_roi"], rd["frame_psnr_bg"] = [p[2] for p in per], [p[1] for p in per]
        rd["frame_roi_pixels"] = [int(v[2][-1]) for v in values]

    return keys


def _fused_emit(roi, residuals, plan, size, dev, residual_bins=None):
    """(picture(t, ref_frame) -> the fused unpadded picture, close()) of a decode loop; without a ROI the crop itself."""
    h, w = size
    if roi is None:
        return (lambda t, ref_frame: ref_frame[..., :h, :w]), (lambda: None)
    if residuals is None and residual_bins is None:
        raise ValueError("decoding with roi= needs residuals= (the decoded residual layer to fuse) or residual_bins= (the coded one)")
    layer = _RoiLayer(roi, plan, size, dev)
    source = _ResidualIn(residuals, size, plan.n_frames, dev) if residuals is not None else _RecordIn(residual_bins, size, layer)

    def picture(t, ref_frame):  # display side only: the DPB keeps the base-layer reconstruction
        return layer.X.fuse(ref_frame[..., :h, :w], source.frame(t), layer.boxes(t), layer.classes, layout=source.layout,
                            order=source.order)

    return picture, source.close


def encode_video(video, bin_dir, recon_video=None, size=None, spec=None, quantize8=False, gop=32, q=(1.0, 1.0, 1.0),
                 device="cuda:0", precision=None, i_ckpt=None, p_ckpt=None, max_frames=None, coder="host", io_workers=8,
                 nets=None, gop_streams=1, report=None, bit_depth=8, fps=None, roi=None, residuals=None, scenecut=None,
                 min_gop=1, roi_q=None, bit_map=None, target_bpp=None, q_range=None, residual_bins=None, residual_step=1,
                 picture_hash=False, base_scale=None, aq=None, tnr=None, redact=None, grain=None, deinterlace=None, shake=None):
    """encode_folder for a `.y4m` file, or a raw I420 `.yuv` file with size=(width, height) [bit_depth, fps]: same .bin
    files, same return values.  Per picture: file -> a ring of pinned buffers (the reader fills them in place) -> one
    asynchronous copy of 1.5 bytes per pixel on a copy stream -> yuv.yuv420_to_rgb on the GOP stream -> the encoder.
    spec: a yuv.ColorSpec overriding what the file says (default: its header, else bt709 / limited / left).
    quantize8: round the converted picture to 8-bit RGB first, i.e. code exactly what encode_folder would read from
    PNGs of those pixels; default off (no second quantisation of the source).
    recon_video: write the reconstructions as `.y4m` / `.yuv` with the source's parameters.
    report: as encode_folder (the existing keys measure against the RGB picture the codec was given), plus
    frame_psnr_y / _u / _v / _yuv and ave_{i,p,all}_frame_psnr_yuv in the sample domain of the source file.
    io_workers is accepted for symmetry with encode_folder: a 4:2:0 frame needs no decoding, so this path has no helper
    threads at any value.  Writes sequence.json beside the .bin files (read_sequence_info, decode_video).
    roi, residuals: as encode_folder (the residual is taken against the RGB picture the codec was given); sequence.json
    then also records the classes' names and borders.
    scenecut, min_gop: as encode_folder; the scan pass reads the file once through the same ring, copy and colour
    conversion (spec, quantize8) as the coding pass.  sequence.json is the same with or without.
    roi_q: as encode_folder (roiq.json beside the .bin files; sequence.json is the same with or without).
    bit_map, target_bpp, q_range: as encode_folder.
    residual_bins, residual_step: as encode_folder; sequence.json then also records residual_step.
    picture_hash: as encode_folder (the digests are of the RGB reconstruction, before any conversion back to YUV).
    base_scale: as encode_folder -- the scaling comes after the colour conversion (RGB only); sequence.json keeps the
    source's size, scale.json lies beside it.
    aq: as encode_folder (aq.json beside the .bin files; sequence.json is the same with or without).
    tnr: as encode_folder -- the filter comes after the colour conversion (RGB only); the YUV figures of the report stay
    against the file's own samples; sequence.json is the same with or without.
    redact: as encode_folder -- after the colour conversion and tnr (RGB only); redact.json lies beside sequence.json, which
    is the same with or without.
    grain: as encode_folder (grain.json beside the .bin files; sequence.json is the same with or without).
    shake: as encode_folder -- the pictures registered are the converted (and deinterlaced) ones; shake.json lies beside
    sequence.json, which is the same with or without.
    deinterlace: None, a deint.Deinterlace, or "frame" / "field" with the field order of the file's header -- the file is
    interlaced material (a Y4M It / Ib, any file with an explicit order) and what is coded are progressive pictures made
    from its fields on the device (vcm_ts_amd/deint.py), one per frame or one per field, in front of the colour
    conversion.  Everything above then speaks of those pictures: max_frames counts them, the report's YUV figures are
    against their samples, recon_video is progressive (the frame rate doubled in "field" mode), and sequence.json says
    so and records the setting.  The report gains `deinterlace` and `frame_deint_moved`.  An open reader must have been
    opened with interlaced=True.  Picture g depends on the file and g alone: not on GOPs, gop_streams or max_frames."""
    options = locals()
    video, recon_video = options.pop("video"), options.pop("recon_video")
    source = _VideoSource(video, device, **{name: options.pop(name) for name in ("size", "spec", "quantize8", "bit_depth", "fps",
                                                                                 "max_frames", "deinterlace")},
                          keep_moved=bool(report))
    return _encode_sequence(source, _VideoStage(recon_video), **options)


def decode_video(bin_dir, recon_video, height=None, width=None, gop=None, spec=None, fps=None, device="cuda:0",
                 precision=None, i_ckpt=None, p_ckpt=None, roi=None, residuals=None, residual_bins=None, verify=None,
                 base_scale="file", grain=None):
    """decode_folder's loop with the video output stage.  Size, GOP length, frame rate and colour description come from
    the sequence.json encode_video left in `bin_dir`; explicit arguments override it, and without the file height and
    width are required (gop then defaults to 32, the colour description to yuv.ColorSpec()).  Returns the picture count.
    roi, residuals, residual_bins: as decode_folder -- the fused picture is what is converted and written.  A roiq.json
    beside the .bin files is followed as decode_folder does.
    verify: as decode_folder (the digests are of the RGB reconstruction, before the conversion to YUV).
    base_scale: as decode_folder (None writes a video of the base size).
    An aq.json beside the .bin files is followed as decode_folder does.
    grain: as decode_folder (the grained RGB picture is what is converted and written)."""
    from . import yuv as Y

    info = read_sequence_info(bin_dir) or {}
    height, width = height or info.get("height"), width or info.get("width")
    if not height or not width:
        raise ValueError(f"no {SEQUENCE_JSON} in {bin_dir}: height and width are required")

    def check(shown, coded, scaled):
        Y.check_size(*shown)
        first = os.path.join(bin_dir, "im00001.bin")
        if not scaled and os.path.exists(first) and S.decode_i(first)[:2] != coded:  # (with a scale.json: _decode_scale's check)
            raise ValueError(f"the pictures in {bin_dir} are {S.decode_i(first)[:2]}, not {coded}")

    stage = _VideoStage(recon_video, spec or info.get("color") or Y.ColorSpec(), fps or info.get("fps"), chroma=info.get("chroma"),
                        interlace=info.get("interlace"), aspect=info.get("aspect"))
    # (gops.json, when encode left one, says where the I pictures are)
    return _decode_sequence(bin_dir, (height, width), stage, gop or info.get("gop"), device, precision, i_ckpt, p_ckpt, roi, residuals,
                            residual_bins, verify, base_scale, check, grain)


def _video_args(ap, a):
    """(size, fps) of the --video, --size and --fps options of encode and boxes, refused through ap.error."""
    from . import yuv as Y

    ext = os.path.splitext(a.video)[1].lower()
    if ext not in (".y4m", ".yuv"):
        ap.error("--video takes a .y4m or a .yuv file")
    if ext == ".yuv" and not a.size:
        ap.error("a raw .yuv file needs --size WxH")
    try:
        return (Y.parse_size(a.size) if a.size else None,
                tuple(int(v) for v in (a.fps.split(":") + ["1"])[:2]) if a.fps else None)
    except ValueError as ex:
        ap.error(str(ex))


def _deint_option(ap, a):
    """--deinterlace / --field-order of encode and boxes before the file is opened: (the keywords of yuv.open_video, the
    function that makes the deint.Deinterlace of the opened reader or refuses through ap.error)."""
    if a.field_order is not None and a.deinterlace is None:
        ap.error("--field-order belongs to --deinterlace")
    if a.deinterlace is not None and a.video is None:
        ap.error("--deinterlace belongs to --video: a PNG folder holds progressive pictures")
    if a.deinterlace is None:
        return {}, lambda reader: None

    def setting(reader):
        from . import deint as DI

        if reader.field_order is None:
            ap.error(f"--deinterlace: {a.video} names no field order (a .yuv file, or a Y4M header that says progressive): "
                     f"give --field-order tff|bff")
        try:
            DI.check_height(reader.height)
            return DI.Deinterlace(a.deinterlace, reader.field_order)
        except ValueError as ex:
            ap.error(f"--deinterlace: {ex}")

    return {"interlaced": True, "field_order": a.field_order}, setting


def _motion_boxes(source, root, params, shake=None):
    """The motion scan of motion_boxes_folder / motion_boxes_video over a source, which is closed on every exit.  shake: a
    shake.ShakeParams -- every picture goes through a shake.Registrar before the scan sees it, the counts of the cells that
    the band replicated from a registered picture's edge touches are zeroed on the host before the boxes are made,
    motion.json gains a "shake" entry and ROOT/shake.json holds the records."""
    from . import motionroi as M

    moved = None
    try:
        source.open()
        n, (h, w) = source.n_frames, source.size
        if shake is None:
            boxes = M.scan((x for x, _ in source.pictures(range(n))), n, (h, w), source.dev, params)
        else:
            from . import shake as SH

            if n < 1:
                raise ValueError(f"no frames to scan, got {n}")
            steady, run = SH.Registrar(source.dev, h, w, n, shake), M.MotionScan(source.dev, h, w, n, params)
            with torch.no_grad():
                for x, _ in source.pictures(range(n)):
                    run.add(steady.add(x))
            if run.n != n:
                raise ValueError(f"the scan pass saw {run.n} pictures of {n}")
            log = steady.log()
            boxes = M.boxes_of_scan(SH.mask_border(run.counts(), log, h, w), h, w, params)
            moved = SH.document(log, shake, h, w)
    finally:
        source.close()
    M.write_boxes(root, boxes, params, h, w, None if moved is None else dict(moved["params"], **moved["summary"]))
    S.write_sidecar(root, SHAKE_JSON, moved)
    return boxes


def motion_boxes_folder(frames_dir, root, params, device="cuda:0", io_workers=8, max_frames=None, shake=None):
    """run_codec boxes --frames: the motion boxes (vcm_ts_amd/motionroi.py) of a PNG folder, written to `root` as
    motion_coords/%05d and motion.json -- then a roi.PickleBoxes root.  A pass of its own over the source, for the reason
    the scene-cut scan is one: the background model is a recursion over the whole sequence, while GOP streams and GOP
    sharding code GOPs independently.  The pictures come through the reader and conversion of encode_folder's coding
    pass.  Returns the list of (n, 4) box arrays."""
    return _motion_boxes(_PngSource(frames_dir, device, io_workers, max_frames), root, params, shake)


def motion_boxes_video(video, root, params, device="cuda:0", size=None, spec=None, quantize8=False, bit_depth=8, fps=None,
                       max_frames=None, deinterlace=None, shake=None):
    """motion_boxes_folder for a `.y4m` file, or a raw I420 `.yuv` file with size=(width, height): the pictures come
    through the ring, copy and colour conversion (spec, quantize8) of encode_video's coding pass -- with deinterlace
    (encode_video's) through its deinterlacer too, so the boxes are numbered as the pictures it codes."""
    return _motion_boxes(_VideoSource(video, device, size, spec, quantize8, bit_depth, fps, max_frames, deinterlace), root, params, shake)


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode")
    b = sub.add_parser("boxes", description="Motion ROI boxes of a fixed-camera sequence: a scan pass of its own over the "
                       "source (a background model of the luma on the GPU, vcm_ts_amd/motionroi.py) that writes "
                       "ROOT/motion_coords/%%05d and ROOT/motion.json; ROOT is then an ordinary --roi-root whose third box "
                       "class is \"motion\".  The mechanism only: nothing is claimed about detection quality")
    n = sub.add_parser("noise", description="The sensor noise of a fixed-camera source, measured from the source alone: a scan "
                       "pass (two small kernels on the GPU, vcm_ts_amd/noise.py) over consecutive pictures' luma difference "
                       "per 16x16 cell, the lower quartile of it, and the threshold encode --tnr-auto K would choose, as JSON on "
                       "stdout.  Fixed camera only: a pan is measured as noise and nothing warns of it")
    k = sub.add_parser("shake", description="The shake of a fixed camera, measured from the source alone: every picture is "
                       "searched for in picture 0 (a 2-D whole-pixel search on a sparse sample of every 64x64 tile and a median "
                       "vote over the tiles, vcm_ts_amd/shake.py) and the per-picture records and their summary are printed as "
                       "JSON.  The registration of boxes / noise / encode --tnr-auto --shake R on its own")
    for p in (e, b, n, k):
        p.add_argument("--frames", help="folder of im1.png / im00001.png ... (exactly one of --frames and --video)")
        p.add_argument("--video", metavar="FILE", help="a .y4m file, or a raw I420 .yuv file with --size")
        p.add_argument("--size", metavar="WxH", help="picture size of a raw .yuv file")
        p.add_argument("--bit-depth", type=int, default=8, choices=[8, 10], help="sample depth of a raw .yuv file")
        p.add_argument("--fps", default=None, help="frame rate of a raw .yuv file, N or N:D (recorded, and written to a .y4m output)")
        p.add_argument("--matrix", default=None, choices=["bt709", "bt601"], help="default bt709")
        p.add_argument("--range", default=None, choices=["limited", "full"], help="default: the Y4M header's XCOLORRANGE, else limited")
        p.add_argument("--siting", default=None, choices=["left", "center"], help="chroma siting; default: the Y4M header's, else left")
        p.add_argument("--deinterlace", default=None, choices=["frame", "field"],
                       help="with --video: the file is interlaced 4:2:0 material; make progressive pictures from its fields on the "
                            "GPU (a motion-adaptive deinterlacer on the sample planes, vcm_ts_amd/deint.py) and code those: one per "
                            "frame (the earlier field kept) or one per field (twice the pictures, twice the frame rate).  "
                            "Every picture number then counts output pictures.  Untuned; no inverse telecine")
        p.add_argument("--field-order", default=None, choices=["tff", "bff"],
                       help="with --deinterlace: which field of a frame is earlier.  A Y4M header (It / Ib) decides and this "
                            "overrides it; required for a .yuv file, for Im and for a file whose header says Ip")
        p.add_argument("--quantize8", action="store_true",
                       help="with --video: round the converted picture to 8-bit RGB before coding it (what a PNG of it would hold)")
    b.add_argument("--out", required=True, metavar="ROOT", help="where motion_coords/ and motion.json go")
    b.add_argument("--threshold", type=int, required=True, metavar="T",
                   help="a pixel is foreground when its luma is more than T 8-bit codes from the background model, 1 .. 254 "
                        "(no default exists -- the right value depends on the content)")
    b.add_argument("--learn", type=int, nargs=2, default=None, metavar=("KB", "KF"),
                   help="the model moves by |difference| >> K toward each picture: KB at background pixels, KF at foreground "
                        "ones, 0 .. 16 each (default 4 8, untuned placeholders)")
    b.add_argument("--min-pixels", type=int, default=None, metavar="P",
                   help="a 16x16 cell is active from P foreground pixels, 1 .. 256 (default 8, an untuned placeholder)")
    b.add_argument("--grow", type=int, default=None, metavar="G",
                   help="dilate the active cells by G cells before joining them, 0 .. 8 (default 1, an untuned placeholder)")
    b.add_argument("--min-cells", type=int, default=None, metavar="C", help="drop a region of fewer than C active cells (default 1)")
    b.add_argument("--max-boxes", type=int, default=None, metavar="N", help="keep the N strongest boxes of a picture (default 64)")
    b.add_argument("--device", default="cuda:0")
    b.add_argument("--io-workers", type=int, default=8, help="host threads for PNG decoding (0: inline)")
    n.add_argument("--out", metavar="FILE", help="also write the JSON there")
    n.add_argument("--max-frames", type=int, default=None, metavar="N", help="scan the first N pictures only")
    n.add_argument("--min-cells", type=int, default=None, metavar="N",
                   help="the counted cells an estimate needs (default 1024, an untuned placeholder)")
    n.add_argument("--scale", type=float, default=None, metavar="K",
                   help="the K of encode --tnr-auto K whose threshold is reported, 0.50 .. 16.00 (default 3.0, an untuned placeholder)")
    n.add_argument("--device", default="cuda:0")
    n.add_argument("--io-workers", type=int, default=8, help="host threads for PNG decoding (0: inline)")
    k.add_argument("--radius", type=int, required=True, metavar="R",
                   help="the search range in whole pixels per axis, 1 .. 16 (no default exists -- the largest shake expected; a "
                        "vector AT the radius is taken for a pan and the picture is lost)")
    k.add_argument("--min-votes", type=int, default=None, metavar="N",
                   help="a picture with fewer voting tiles is lost (default 8, an untuned placeholder)")
    k.add_argument("--out", metavar="FILE", help="also write the JSON there")
    k.add_argument("--max-frames", type=int, default=None, metavar="N", help="scan the first N pictures only")
    k.add_argument("--device", default="cuda:0")
    k.add_argument("--io-workers", type=int, default=8, help="host threads for PNG decoding (0: inline)")
    for p, what in ((b, "the motion scan"), (n, "the noise scan"), (e, "with --tnr-auto: the noise scan")):
        p.add_argument("--shake", type=int, default=None, metavar="R",
                       help=f"the camera is fixed but shakes: register every picture onto picture 0 by one whole-pixel vector "
                            f"within +-R (1 .. 16; vcm_ts_amd/shake.py: a tile search and a median vote on the GPU) before "
                            f"{what} sees it.  shake.json holds the records.  Whole pixels, translation only, no "
                            f"re-anchoring; the coding pass is not touched.  Untuned; no real video was seen")
        p.add_argument("--shake-min-votes", type=int, default=None, metavar="N",
                       help="with --shake: a picture with fewer voting tiles is lost and passed on unmoved (default 8, an "
                            "untuned placeholder)")
    e.add_argument("--bins", required=True)
    e.add_argument("--recon")
    e.add_argument("--png-device", action="store_true",
                   help="with --recon: make the PNGs on the GPU (filter and deflate kernels; the same pixels, other files) and "
                        "leave the host threads only the write()")
    e.add_argument("--recon-video", metavar="FILE", help="with --video: reconstructions as .y4m / .yuv")
    e.add_argument("--q", type=float, nargs=3, default=None, metavar=("I", "MV_Y", "Y"),
                   help="explicit q-scales (default 1 1 1 when no rate point is selected)")
    e.add_argument("--rate-count", type=int, default=None,
                   help="with --quality: the reference's rate-point selection (video_coder.py RATE_COUNT / QUALITY): "
                        "q-scales interpolated in log space between the anchors stored in the checkpoints")
    e.add_argument("--quality", type=int, default=None)
    e.add_argument("--gop-streams", type=int, default=1,
                   help="GOPs of the folder in flight together on the GPU (same .bin bytes; ~33 GB of workspace each at 1080p)")
    e.add_argument("--coder", default="host", choices=["host", "device"],
                   help="host: the reference's bitstream (default); device: opt-in GPU entropy coder, own format")
    e.add_argument("--report", metavar="JSON",
                   help="write bpp, PSNR and MS-SSIM of every picture and their I / P / all averages (the key layout of "
                        "the reference's test harness); measured on the device, the .bin files are the same with or without")
    e.add_argument("--bit-map", nargs="?", const=True, default=None, metavar="DIR",
                   help="where the bits of every picture went: --report gains frame_bits_mv_z / _mv_y / _z / _y and, with "
                        "--roi-root, frame_bits_roi / frame_bits_bg / frame_roi_cells; with DIR also im%%05d.npy, the bits per "
                        "16x16 cell of each picture.  Needs --report or DIR; the .bin files are the same with or without")
    e.add_argument("--target-bpp", type=float, default=None, metavar="B",
                   help="rate control: aim at B bits per pixel by moving q_y from P picture to P picture inside each GOP "
                        "(--q, or 1 1 1, is the starting point and stays the I and mv_y setting; the I picture is not "
                        "controlled).  The step is chosen from a sweep of the picture's own code lengths, no fitted model; "
                        "--report gains frame_q_y and frame_bits_target; decode needs nothing new")
    e.add_argument("--q-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="with --target-bpp: the q-scales q_y may take (default the wire range 0.01 655)")
    e.add_argument("--scenecut", type=float, default=None, metavar="T",
                   help="also open a GOP with an I picture where consecutive pictures differ by more than T, 0 < T <= 1 (0: "
                        "identical regional luma histograms, 1: disjoint; no default exists -- the right value depends on "
                        "the content).  A scan pass reads the source once before coding; --gop becomes the longest GOP; the "
                        "I pictures are listed in gops.json beside the .bin files, which decode follows")
    e.add_argument("--min-gop", type=int, default=None, metavar="N",
                   help="with --scenecut: no I picture closer than N pictures behind the last one (default 1, at most --gop); "
                        "a cut that falls inside stays a P picture")
    e.add_argument("--plate-q", type=float, default=None, metavar="F",
                   help="with --roi-root: ROI-weighted quantisation -- multiply the quantisation step of the latent y by F "
                        "(0.1 .. 10, snapped to hundredths; below 1 is finer) in every 16x16 cell a plate box touches.  Any of "
                        "--plate-q, --face-q, --background-q switches it on, the others default to 1.00 (no tuned values "
                        "exist); the factors go to roiq.json beside the .bin files and decode then needs --roi-root")
    e.add_argument("--face-q", type=float, default=None, metavar="F", help="the same for face boxes")
    e.add_argument("--motion-q", type=float, default=None, metavar="F",
                   help="the same for motion boxes; only with a --roi-root that holds motion_coords (run_codec boxes)")
    e.add_argument("--background-q", type=float, default=None, metavar="F", help="the factor of the cells no box touches")
    e.add_argument("--roi-q-grow", type=int, default=None, metavar="N",
                   help="with one of the three above: grow every box by N pixels (0 .. 255, default 0) before it is laid on the cells")
    e.add_argument("--picture-hash", action="store_true",
                   help="write hashes.json beside the .bin files: two CRC-32 digests per coded picture, taken on the GPU from the "
                        "encoder's own reconstruction -- of the 8-bit picture (the bytes of its PNG) and of the fp32 reference "
                        "picture -- which decode follows; the .bin files are the same with or without")
    e.add_argument("--base-scale", default=None, metavar="N/D",
                   help="code the base layer at N/D of the source's size, 1/4 <= N/D < 1 (each side rounded to the nearest "
                        "sample): pictures are scaled down on the GPU before the codec and up again for --recon, --recon-video, "
                        "--report, --residuals, --residual-bins and --picture-hash, all of which keep speaking of the full "
                        "size, as does --target-bpp; scale.json beside the .bin files tells decode.  Not with --plate-q, "
                        "--face-q, --background-q, nor with --bit-map and --roi-root together")
    e.add_argument("--aq-strength", type=int, default=None, metavar="A",
                   help="backward-adaptive quantisation: code every P picture with a q-scale map made on the GPU from its own "
                        "reference picture -- a 16x16 cell flatter than the reference's mean activity gets a finer step of the "
                        "latent y, a busier one a coarser step; A, 1 .. 400, is in hundredths of a QP per doubling of the cell's "
                        "variance (x265's --aq-strength times 100; no tuned value exists).  The decoder rebuilds the maps from its "
                        "own reference pictures: the .bin format is unchanged, nothing is stored per picture, and aq.json beside "
                        "the .bin files tells decode.  I pictures are not adapted")
    e.add_argument("--aq-clamp", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                   help="with --aq-strength: the factors a cell may get, in hundredths, 10 <= LO <= 100 <= HI <= 1000 "
                        "(default 10 1000)")
    e.add_argument("--tnr", type=int, default=None, metavar="T",
                   help="motion-adaptive temporal noise prefilter for fixed-camera content: hand the codec every P picture "
                        "blended on the GPU with the previous filtered picture wherever their luma differs by fewer than T 8-bit "
                        "codes on average over a 5x5 window, and untouched wherever something moves; T, 1 .. 64 (no default "
                        "exists -- the right value depends on the noise).  Encoder side only: the .bin format is unchanged, no "
                        "file is written and decode needs nothing; --report keeps measuring against the unfiltered source and "
                        "gains tnr, frame_tnr_held and frame_tnr_mad.  Motion compensation is opt-in (--tnr-search); nothing is "
                        "claimed about rate or quality")
    e.add_argument("--tnr-floor", type=int, default=None, metavar="W",
                   help="with --tnr: the weight of the current picture, in 1/256ths, where nothing differs, 1 .. 255 (default 64, "
                        "an untuned placeholder)")
    e.add_argument("--tnr-pixel", type=int, default=None, metavar="P",
                   help="with --tnr: a pixel whose own luma differs by more than P codes is passed through whatever its window "
                        "says, 0 .. 255 (default min(255, 3 T), an untuned placeholder)")
    e.add_argument("--tnr-search", type=int, default=None, metavar="R",
                   help="with --tnr: motion-compensate the filter -- search every 16x16 cell of a P picture in the previous "
                        "filtered picture within +-R whole pixels (luma SAD, full search on the GPU), move that picture cell by "
                        "cell and blend against the moved picture, so that a moving object is blended with where it was; R, "
                        "1 .. 32 (no default: without the option nothing is searched).  --report gains frame_tnr_moved and "
                        "frame_tnr_mad_zero.  Whole-pixel vectors, no overlapped blocks")
    e.add_argument("--tnr-penalty", type=int, default=None, metavar="L",
                   help="with --tnr-search: what a pixel of vector length costs the search, in luma codes of the cell's SAD, "
                        "0 .. 255 (default 4, an untuned placeholder)")
    e.add_argument("--tnr-subpel", action="store_true",
                   help="with --tnr-search: refine every cell's vector to quarter pixels (dcvc_me_refine: the 49 candidates "
                        "around the whole-pel vector, luma SAD against a 7/8-tap interpolation) and move the previous filtered "
                        "picture through that interpolation (dcvc_me_compensate_sub): four kernels per P picture.  --report "
                        "gains frame_tnr_subpel.  No overlapped blocks; nothing is claimed about rate or quality")
    e.add_argument("--tnr-split", action="store_true",
                   help="with --tnr-search: let every 8 x 8 quarter of a cell choose again among its cell's vector and the eight "
                        "neighbours' (dcvc_me_split) and move the previous filtered picture sub-cell by sub-cell "
                        "(dcvc_me_compensate_split): one more kernel per P picture.  --report gains frame_tnr_split.  Cells on "
                        "an object's edge stay worse than the unfiltered source; nothing is claimed about rate or quality")
    e.add_argument("--tnr-levels", type=int, default=None, metavar="L",
                   help="with --tnr-search: search hierarchically over L coarser levels of 2 x 2 luma means, 1 or 2 "
                        "(dcvc_me_pyramid, dcvc_me_coarse, dcvc_me_descend in place of dcvc_me_search: 3 + L more kernels per P "
                        "picture); --tnr-search may then be 2 .. 64 (L = 1) or 4 .. 128 (L = 2).  --report gains frame_tnr_far.  "
                        "Fine texture defeats it; --tnr-subpel and --tnr-split stop at R = 32; untuned, and nothing is claimed "
                        "about rate or quality")
    e.add_argument("--tnr-intra", type=int, default=None, metavar="K",
                   help="with --tnr: filter I pictures too -- blend every I picture in one pass (dcvc_tnr_fuse) with up to K "
                        "pictures that follow it in its own GOP, each moved onto it first with --tnr-search, and start the "
                        "recursive filter from the filtered picture; 1 .. 4 (no default: without the option I pictures are "
                        "passed through).  --report gains frame_tnr_refs.  Untuned; nothing is claimed about rate or quality")
    e.add_argument("--tnr-auto", type=float, nargs="?", const=3.0, default=None, metavar="K",
                   help="in place of --tnr T: measure the source's noise level first (vcm_ts_amd/noise.py: a scan pass over "
                        "the whole source, shared with --scenecut's; the lower quartile of the 16x16 cells' mean absolute luma "
                        "difference of consecutive pictures) and filter with T = ceil(K x that level), clamped to 1 .. 64; K "
                        "within 0.50 .. 16.00 (default 3.0, an UNTUNED PLACEHOLDER).  Every --tnr-* option belongs to either.  "
                        "noise.json beside the .bin files and --report's `noise` hold the estimate and the chosen T.  Fixed "
                        "camera only: a pan is measured as noise.  A source without an estimate is refused: pass --tnr T")
    e.add_argument("--tnr-auto-min-cells", type=int, default=None, metavar="N",
                   help="with --tnr-auto: the counted cells an estimate needs (default 1024, an untuned placeholder)")
    e.add_argument("--grain", action="store_true",
                   help="with --tnr: film-grain synthesis, the encoder's half (vcm_ts_amd/grain.py) -- measure on the GPU what the "
                        "prefilter took out of every P picture and leave grain.json beside the .bin files: per GOP eight "
                        "strengths by intensity and two taps.  decode --grain synthesises from it.  Every other output is that "
                        "of an encode without the option.  P pictures only; nothing is tuned, nothing is claimed")
    e.add_argument("--grain-min-samples", type=int, default=None, metavar="N",
                   help="with --grain: an intensity bin with fewer pixels than N in a GOP takes its nearest populated "
                        "neighbour's strength (default 1024, an untuned placeholder)")
    e.add_argument("--redact", nargs="+", default=None, metavar="NAME",
                   help="with --roi-root: ROI redaction -- hand the codec every picture with the boxes of the named classes "
                        "(liplates, faces, motion) replaced on the GPU by a mosaic (--redact-tile) or a solid fill "
                        "(--redact-fill); exactly one of the two must be given, neither has a default.  Encoder side only: the "
                        ".bin format is unchanged and decode needs nothing; redact.json beside the .bin files records the "
                        "setting; --report keeps measuring against the unredacted source and gains redact and frame_redacted.  "
                        "A mosaic is not a security guarantee (small tiles over text can be partly inverted: use the fill); "
                        "boxes are taken as given, so whatever the detector misses stays untouched")
    e.add_argument("--redact-tile", type=int, default=None, metavar="N",
                   help="with --redact: a mosaic of N x N tiles on a picture-aligned grid, N one of 2, 4, 8, 16, 32, 64")
    e.add_argument("--redact-fill", type=int, default=None, metavar="K",
                   help="with --redact: a solid fill of the 8-bit code K, 0 .. 255, on all three channels")
    e.add_argument("--redact-grow", type=int, default=None, metavar="G", help="with --redact: grow every box by G pixels, 0 .. 255 (default 0)")
    e.add_argument("--redact-hold", type=int, default=None, metavar="N",
                   help="with --redact: also redact inside the boxes of the N pictures before and after, 0 .. 32 (default 0): "
                        "narrows, not closes, the gap a detector leaves when it misses a picture")
    e.add_argument("--redact-restorable", action="store_true",
                   help="with --redact: allow --residuals / --residual-bins, whose files then hold what was removed inside the "
                        "boxes (decode --roi-root --residual-bins puts it back); whoever holds them holds the content")
    d = sub.add_parser("decode")
    d.add_argument("--base-only", action="store_true",
                   help="ignore a scale.json beside the .bin files (encode --base-scale) and write the base-size pictures; "
                        "--height / --width stay the full size.  Not with --roi-root")
    d.add_argument("--verify", default=None, choices=["strict", "pixels", "warn", "off"],
                   help="what to do with a hashes.json beside the .bin files (encode --picture-hash), which is followed without "
                        "this option as 'pixels': stop at the first picture whose 8-bit digest differs and warn once when only "
                        "the reference picture's does; strict: stop on either; warn: never stop; off: launch nothing.  "
                        "Refused without the file, except off")
    d.add_argument("--grain", type=int, nargs="?", const=100, default=None, metavar="PERCENT",
                   help="film-grain synthesis, the decoder's half: add to every P picture that is written noise of the strength "
                        "and shape the folder's grain.json (encode --tnr T --grain) measured, at PERCENT of that strength, "
                        "1 .. 200 (default 100).  Opt-in: the file is never followed without the option.  Display side only: "
                        "--verify keeps checking the ungrained picture, and a grained folder deliberately does not pass the "
                        "`verify` command, whose digests are of the ungrained picture.  Achromatic, a 3-tap separable shape, "
                        "per-GOP parameters; I pictures are grained only where the record's tnr entry says intra (encode --tnr-intra).  "
                        "Refused without a grain.json and with --base-only; "
                        "not implemented with --residuals / --residual-bins")
    v = sub.add_parser("verify", description="Hold a folder of decoded PNGs against the `pixels` digests of a hashes.json, on "
                       "the host alone (zlib.crc32 of every picture's RGB bytes; no GPU).  For unfused base-layer PNG folders "
                       "only: a picture fused with a ROI residual layer is not the picture the digests are of.")
    v.add_argument("--bins", required=True, help="the folder whose hashes.json encode --picture-hash wrote")
    v.add_argument("--recon", required=True, help="a folder of im%%05d.png as decode --recon (or encode --recon) writes them, "
                                                  "unfused base layer only")
    d.add_argument("--bins", required=True)
    d.add_argument("--recon", help="folder for PNGs (exactly one of --recon and --recon-video)")
    d.add_argument("--png-device", action="store_true", help="with --recon: make the PNGs on the GPU, as encode --png-device does")
    d.add_argument("--recon-video", metavar="FILE", help=".y4m / .yuv output; size and colour from the bins' sequence.json")
    d.add_argument("--height", type=int, help="required unless sequence.json lies beside the .bin files")
    d.add_argument("--width", type=int)
    d.add_argument("--matrix", default=None, choices=["bt709", "bt601"])
    d.add_argument("--range", default=None, choices=["limited", "full"])
    d.add_argument("--siting", default=None, choices=["left", "center"])
    d.add_argument("--bit-depth", type=int, default=None, choices=[8, 10])
    e.add_argument("--residuals", metavar="PATH",
                   help="with --roi-root: write the residual layer, FILE.gbrp (raw planes for ffmpeg -f rawvideo -pix_fmt gbrp) "
                        "or a folder for im%%05d.png")
    d.add_argument("--residuals", metavar="PATH",
                   help="with --roi-root: the decoded residual layer (FILE.gbrp or a folder of im%%05d.png) to fuse into the output")
    e.add_argument("--residual-bins", metavar="DIR",
                   help="with --roi-root: code the residual layer on the GPU into DIR/im%%05d.rl (DIR may be --bins): a box-local "
                        "coder of its own, not HEVC; --report gains frame_bits_enh, frame_bpp_enh, ave_all_frame_bpp_enh and "
                        "ave_all_frame_bpp_total.  May be given together with --residuals")
    e.add_argument("--residual-step", type=int, default=None, metavar="S",
                   help="with --residual-bins: the integer quantisation step of the residual, 1 .. 64 (default 1: lossless; S keeps "
                        "every sample within S // 2; no tuned value exists)")
    d.add_argument("--residual-bins", metavar="DIR",
                   help="with --roi-root: the coded residual layer (DIR/im%%05d.rl) to decode and fuse into the output, in place "
                        "of --residuals")
    for p in (e, d):
        p.add_argument("--roi-root", metavar="DIR",
                       help="the reference's box files: DIR/liplates_coords/%%05d and DIR/faces_coords/%%05d (either may be absent)")
        p.add_argument("--plate-border", type=int, default=None, metavar="N",
                       help="the reference's LIPLATES.PADDING: feather width and metric shrink of plate boxes "
                            "(default 0; decode: the sequence.json's)")
        p.add_argument("--face-border", type=int, default=None, metavar="N", help="the same for face boxes")
        p.add_argument("--motion-border", type=int, default=None, metavar="N",
                       help="the same for motion boxes; only with a --roi-root that holds motion_coords (run_codec boxes)")
        p.add_argument("--gop", type=int, default=None,
                       help="default 32 (decode: the sequence.json's, else 32; refused if a gops.json beside the .bin files says otherwise)")
        p.add_argument("--io-workers", type=int, default=8, help="host threads for PNG decoding / encoding (0: inline)")
        p.add_argument("--device", default="cuda:0")
        p.add_argument("--precision", default=None, choices=["fp32", "fp16x3"])
        p.add_argument("--i-ckpt")
        p.add_argument("--p-ckpt")
    return ap


def _verify_command(ap, a):
    from . import picturehash as PH

    try:
        first = PH.verify_pngs(a.bins, a.recon)
    except ValueError as ex:
        ap.error(str(ex))
    if first is not None:
        t, name, want, got = first
        print(f"picture {t} ({name}): the pixels digest is {got:08x}, {PH.HASHES_JSON} says {want:08x}")
        raise SystemExit(1)
    print(f"{len(PH.read_hashes(a.bins)['pixels'])} pictures verified")


def _shake_option(ap, radius, min_votes, names="--shake / --shake-min-votes"):
    """The shake.ShakeParams of --shake R [--shake-min-votes N] (or of `run_codec shake`'s --radius R [--min-votes N]); None
    without a radius."""
    if radius is None:
        if min_votes is not None:
            ap.error("--shake-min-votes belongs to --shake")
        return None
    from . import shake as SH

    try:
        return SH.ShakeParams(radius, **({} if min_votes is None else {"min_votes": min_votes}))
    except ValueError as ex:
        ap.error(f"{names}: {ex}")


def _boxes_command(ap, a):
    from . import motionroi as M
    from . import yuv as Y

    if (a.frames is None) == (a.video is None):
        ap.error("give exactly one of --frames and --video")
    if a.video is None and (a.size or a.quantize8 or a.matrix or a.range or a.siting):
        ap.error("--size, --quantize8, --matrix, --range and --siting belong to --video")
    given = {k: v for k, v in (("learn", None if a.learn is None else tuple(a.learn)), ("min_pixels", a.min_pixels),
                               ("grow", a.grow), ("min_cells", a.min_cells), ("max_boxes", a.max_boxes)) if v is not None}
    try:
        params = M.MotionParams(a.threshold, **given)
    except ValueError as ex:
        ap.error(f"boxes: {ex}")
    shake = _shake_option(ap, a.shake, a.shake_min_votes)
    more, setting = _deint_option(ap, a)
    try:
        if a.video is not None:
            size, fps = _video_args(ap, a)
            with Y.open_video(a.video, size, a.bit_depth, fps, **more) as reader:
                boxes = motion_boxes_video(reader, a.out, params, a.device, quantize8=a.quantize8, deinterlace=setting(reader),
                                           spec=reader.spec(a.matrix, None if a.range is None else a.range == "full", a.siting),
                                           shake=shake)
        else:
            boxes = motion_boxes_folder(a.frames, a.out, params, a.device, io_workers=a.io_workers, shake=shake)
    except (ValueError, OSError) as ex:
        ap.error(f"boxes: {ex}")
    print(f"{len(boxes)} pictures, {sum(len(x) for x in boxes)} boxes -> {os.path.join(a.out, M.COORDS)}")


def noise_scan(source, auto, shake=None):
    """(the noise.NoiseEstimate, what shake.json says or None) of a source (a _PngSource or a _VideoSource, opened here and
    closed on every exit) for the tnr.AutoTNR `auto`: the scan pass of encode --tnr-auto on its own -- every picture once,
    through the reader and conversion of the coding pass, with shake (a shake.ShakeParams) registered first."""
    try:
        source.open()
        steady = _registrar(source, shake)
        est = _scan_pass(source, 1, None, 1, auto, steady)[1]
        return est, _shake_document(steady, source)
    finally:
        source.close()


def noise_estimate(source, auto):
    """The noise.NoiseEstimate of noise_scan without a registration."""
    return noise_scan(source, auto)[0]


def _noise_command(ap, a):
    import json

    from . import tnr as N
    from . import yuv as Y

    if (a.frames is None) == (a.video is None):
        ap.error("give exactly one of --frames and --video")
    if a.video is None and (a.size or a.quantize8 or a.matrix or a.range or a.siting):
        ap.error("--size, --quantize8, --matrix, --range and --siting belong to --video")
    try:
        auto = N.AutoTNR(**({} if a.scale is None else {"scale": a.scale}), **({} if a.min_cells is None else {"min_cells": a.min_cells}))
    except ValueError as ex:
        ap.error(f"noise: --scale / --min-cells: {ex}")
    shake = _shake_option(ap, a.shake, a.shake_min_votes)
    more, setting = _deint_option(ap, a)
    try:
        if a.video is not None:
            size, fps = _video_args(ap, a)
            with Y.open_video(a.video, size, a.bit_depth, fps, **more) as reader:
                spec = reader.spec(a.matrix, None if a.range is None else a.range == "full", a.siting)
                est, moved = noise_scan(_VideoSource(reader, a.device, None, spec, a.quantize8, 8, None, a.max_frames, setting(reader)), auto, shake)
        else:
            est, moved = noise_scan(_PngSource(a.frames, a.device, a.io_workers, a.max_frames), auto, shake)
        _, record = _resolve_tnr(auto, est, moved)
    except (ValueError, OSError) as ex:
        ap.error(f"noise: {ex}")
    text = json.dumps(record, indent=2)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def shake_records(source, params):
    """What `run_codec shake` prints for a source (a _PngSource or a _VideoSource, opened here and closed on every exit): every
    picture once through a shake.Registrar, through the reader and conversion of the coding pass, and nothing else."""
    from . import shake as SH

    try:
        source.open()
        steady = _registrar(source, params)
        with torch.no_grad():
            for x, _ in source.pictures(range(source.n_frames)):
                steady.add(x)
        if steady.n != source.n_frames:
            raise ValueError(f"the scan pass saw {steady.n} pictures of {source.n_frames}")
        return SH.document(steady.log(), params, *source.size)
    finally:
        source.close()


def _shake_command(ap, a):
    import json

    from . import yuv as Y

    if (a.frames is None) == (a.video is None):
        ap.error("give exactly one of --frames and --video")
    if a.video is None and (a.size or a.quantize8 or a.matrix or a.range or a.siting):
        ap.error("--size, --quantize8, --matrix, --range and --siting belong to --video")
    params = _shake_option(ap, a.radius, a.min_votes, "--radius / --min-votes")
    more, setting = _deint_option(ap, a)
    try:
        if a.video is not None:
            size, fps = _video_args(ap, a)
            with Y.open_video(a.video, size, a.bit_depth, fps, **more) as reader:
                spec = reader.spec(a.matrix, None if a.range is None else a.range == "full", a.siting)
                record = shake_records(_VideoSource(reader, a.device, None, spec, a.quantize8, 8, None, a.max_frames, setting(reader)), params)
        else:
            record = shake_records(_PngSource(a.frames, a.device, a.io_workers, a.max_frames), params)
    except (ValueError, OSError) as ex:
        ap.error(f"shake: {ex}")
    text = json.dumps(record, indent=2)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def _motion_option(ap, a):
    """Whether --roi-root holds motion boxes; --motion-border and --motion-q are refused without them."""
    from .roi import PickleBoxes

    motion = a.roi_root is not None and PickleBoxes.has_motion(a.roi_root)
    if not motion and (a.motion_border is not None or getattr(a, "motion_q", None) is not None):
        ap.error("--motion-border and --motion-q need a --roi-root that holds motion_coords (run_codec boxes writes one)")
    return motion


def _needs_roi_root(ap, a):
    if a.roi_root is None and (a.residuals or a.residual_bins or a.plate_border is not None or a.face_border is not None):
        ap.error("--residuals, --residual-bins, --plate-border and --face-border belong to --roi-root")


def _roi_option(ap, a, motion, recorded):
    """The roi.Roi of --roi-root (None without); recorded: {class name: border} where an option does not say."""
    if a.roi_root is None:
        return None
    from . import roi as X

    borders = [given if given is not None else recorded.get(name, 0)
               for given, name in ((a.plate_border, "liplates"), (a.face_border, "faces")) +
               (((a.motion_border, "motion"),) if motion else ())]
    try:
        classes = tuple(X.RoiClass(b) for b in borders)
        return X.Roi(X.PickleBoxes(a.roi_root, classes), classes)
    except (ValueError, OSError) as ex:
        ap.error(str(ex))


def _encode_command(ap, a):
    roi_q = aq = tnr = redact = None
    motion = _motion_option(ap, a)
    if a.aq_clamp is not None and a.aq_strength is None:
        ap.error("--aq-clamp belongs to --aq-strength")
    if a.aq_strength is not None:
        from . import aq as A

        try:
            aq = A.AQ(a.aq_strength, *(a.aq_clamp or (A.MIN_Q, A.MAX_Q)))
        except ValueError as ex:
            ap.error(f"--aq-strength / --aq-clamp: {ex}")
    if a.tnr is not None and a.tnr_auto is not None:
        ap.error("give one of --tnr T and --tnr-auto [K]: the threshold is either given or measured")
    if a.tnr_auto is None and a.tnr_auto_min_cells is not None:
        ap.error("--tnr-auto-min-cells belongs to --tnr-auto")
    if a.tnr_auto is None and (a.shake is not None or a.shake_min_votes is not None):
        ap.error("--shake and --shake-min-votes belong to --tnr-auto: they steady the noise scan (the coding pass is not touched; "
                 "--tnr-search finds the shake cell by cell)")
    shake = _shake_option(ap, a.shake, a.shake_min_votes)
    filtered = a.tnr is not None or a.tnr_auto is not None  # (every --tnr-* option below belongs to either)
    if not filtered and (a.tnr_floor is not None or a.tnr_pixel is not None):
        ap.error("--tnr-floor and --tnr-pixel belong to --tnr")
    if not filtered and (a.tnr_search is not None or a.tnr_penalty is not None):
        ap.error("--tnr-search and --tnr-penalty belong to --tnr")
    if a.tnr_search is None and a.tnr_penalty is not None:
        ap.error("--tnr-penalty belongs to --tnr-search")
    if a.tnr_search is None and a.tnr_subpel:
        ap.error("--tnr-subpel belongs to --tnr-search")
    if a.tnr_search is None and a.tnr_split:
        ap.error("--tnr-split belongs to --tnr-search")
    if a.tnr_search is None and a.tnr_levels is not None:
        ap.error("--tnr-levels belongs to --tnr-search")
    if not filtered and a.tnr_intra is not None:
        ap.error("--tnr-intra belongs to --tnr")
    if filtered:
        from . import tnr as N

        shared = dict(**({} if a.tnr_floor is None else {"floor": a.tnr_floor}), pixel=a.tnr_pixel, search=a.tnr_search,
                      **({} if a.tnr_penalty is None else {"penalty": a.tnr_penalty}), intra=a.tnr_intra,
                      **({"subpel": True} if a.tnr_subpel else {}), **({"split": True} if a.tnr_split else {}),
                      **({} if a.tnr_levels is None else {"levels": a.tnr_levels}))
        first = "--tnr" if a.tnr is not None else "--tnr-auto / --tnr-auto-min-cells"
        try:
            tnr = N.TNR(a.tnr, **shared) if a.tnr is not None else \
                N.AutoTNR(a.tnr_auto, **({} if a.tnr_auto_min_cells is None else {"min_cells": a.tnr_auto_min_cells}), **shared)
        except ValueError as ex:
            ap.error(f"{first} / --tnr-floor / --tnr-pixel / --tnr-search / --tnr-penalty / --tnr-intra / --tnr-subpel / --tnr-split / --tnr-levels: {ex}")
    grain = None
    if a.grain_min_samples is not None and not a.grain:
        ap.error("--grain-min-samples belongs to --grain")
    if a.grain:
        from . import grain as GR

        if tnr is None:
            ap.error("--grain needs --tnr: what is measured is what the prefilter took out")
        try:
            grain = GR.Grain(**({} if a.grain_min_samples is None else {"min_samples": a.grain_min_samples}))
        except ValueError as ex:
            ap.error(f"--grain-min-samples: {ex}")
    factors = [a.plate_q, a.face_q, a.background_q] + ([a.motion_q] if motion else [])
    if a.base_scale is not None:
        from . import scale as SC

        try:
            a.base_scale = SC.as_ratio(a.base_scale)
        except ValueError as ex:
            ap.error(f"--base-scale: {ex}")
    if a.roi_root is None and (any(f is not None for f in factors) or a.roi_q_grow is not None):
        ap.error("--plate-q, --face-q, --background-q and --roi-q-grow belong to --roi-root")
    if a.roi_q_grow is not None and all(f is None for f in factors):
        ap.error("--roi-q-grow belongs to --plate-q, --face-q or --background-q")
    if any(f is not None for f in factors):
        from . import roi as X

        try:
            plate, face, ground, *moving = (100 if f is None else X.RoiQ.hundredths(f, n) for f, n in
                                            zip(factors, ("--plate-q", "--face-q", "--background-q", "--motion-q")))
            roi_q = X.RoiQ(ground, (plate, face, *moving), 0 if a.roi_q_grow is None else a.roi_q_grow)
        except ValueError as ex:
            ap.error(f"ROI-weighted quantisation: {ex}")
    _needs_roi_root(ap, a)
    if a.residual_step is not None and not a.residual_bins:
        ap.error("--residual-step belongs to --residual-bins")
    a.residual_step = 1 if a.residual_step is None else a.residual_step
    if not 1 <= a.residual_step <= 64:
        ap.error("--residual-step must be within 1..64")
    roi = _roi_option(ap, a, motion, {})
    if a.redact is None and (a.redact_tile is not None or a.redact_fill is not None or a.redact_grow is not None or
                             a.redact_hold is not None or a.redact_restorable):
        ap.error("--redact-tile, --redact-fill, --redact-grow, --redact-hold and --redact-restorable belong to --redact")
    if a.redact is not None:
        from . import redact as RD

        if roi is None:
            ap.error("--redact needs --roi-root (the boxes to redact)")
        try:
            redact = RD.Redact(tuple(a.redact), a.redact_tile, a.redact_fill, a.redact_grow or 0, a.redact_hold or 0,
                               a.redact_restorable)
            _redact_args(redact, roi, a.residuals, a.residual_bins)
        except ValueError as ex:
            ap.error(f"--redact: {ex}")
    if (a.frames is None) == (a.video is None):
        ap.error("give exactly one of --frames and --video")
    if a.bit_map is True and not a.report:
        ap.error("--bit-map needs --report (where the regional bit counts go) or a DIR for the per-cell maps")
    if a.video is None and (a.recon_video or a.size or a.quantize8 or a.matrix or a.range or a.siting):
        ap.error("--recon-video, --size, --quantize8, --matrix, --range and --siting belong to --video")
    if a.video is not None and a.recon:
        ap.error("--recon (a PNG folder) belongs to --frames; use --recon-video with --video")
    if a.png_device and not a.recon:
        ap.error("--png-device belongs to --recon (the PNG folder)")
    more, setting = _deint_option(ap, a)
    size = fps = None
    if a.video is not None:
        from . import yuv as Y

        size, fps = _video_args(ap, a)
    a.gop = a.gop or 32
    if a.min_gop is not None and a.scenecut is None:
        ap.error("--min-gop belongs to --scenecut")
    a.min_gop = 1 if a.min_gop is None else a.min_gop
    try:
        from .scenecut import check_options

        check_options(a.gop, a.scenecut, a.min_gop)
    except ValueError as ex:
        ap.error(str(ex))
    if (a.rate_count is None) != (a.quality is None) or (a.q is not None and a.rate_count is not None):
        ap.error("give either --q, or --rate-count together with --quality")
    if a.q_range is not None and a.target_bpp is None:
        ap.error("--q-range belongs to --target-bpp")
    if a.target_bpp is not None:
        if a.rate_count is not None and a.rate_count > 1:
            ap.error("--target-bpp controls one rate point; --rate-count selects several (give --q as the starting point)")
        try:
            _rate_args(a.target_bpp, a.q_range, 1, 1, a.gop)
        except ValueError as ex:
            ap.error(f"--target-bpp / --q-range: {ex}")
    q = tuple(a.q) if a.q is not None else (1.0, 1.0, 1.0)
    if a.rate_count is not None:
        from .dmc import DMC
        from .intra import IntraNoAR
        from .params import dmc_spec, intra_spec, seeded_state_dict

        if a.i_ckpt and a.p_ckpt:
            i_qs = IntraNoAR.get_q_scales_from_ckpt(a.i_ckpt)
            y_qs, mv_qs = DMC.get_q_scales_from_ckpt(a.p_ckpt)
        else:  # no checkpoint: the anchors of the name-seeded synthetic weights the nets are built with
            i_qs = seeded_state_dict(intra_spec())["q_scale"].reshape(-1)
            sd = seeded_state_dict(dmc_spec())
            y_qs, mv_qs = sd["y_q_scale"].reshape(-1), sd["mv_y_q_scale"].reshape(-1)
        q = rate_point_q_scales(i_qs, y_qs, mv_qs, a.rate_count, a.quality)
        print(f"rate point {a.quality} of {a.rate_count}: q_i {q[0]:.4f}  q_mv_y {q[1]:.4f}  q_y {q[2]:.4f}")
    options = dict(gop=a.gop, q=q, device=a.device, precision=a.precision, i_ckpt=a.i_ckpt, p_ckpt=a.p_ckpt, coder=a.coder,
                   io_workers=a.io_workers, gop_streams=a.gop_streams, report=a.report, roi=roi, residuals=a.residuals,
                   scenecut=a.scenecut, min_gop=a.min_gop, roi_q=roi_q, bit_map=a.bit_map, target_bpp=a.target_bpp,
                   q_range=a.q_range, residual_bins=a.residual_bins, residual_step=a.residual_step, picture_hash=a.picture_hash,
                   base_scale=a.base_scale, aq=aq, tnr=tnr, redact=redact, grain=grain, shake=shake)
    if a.video is not None:
        try:
            reader = Y.open_video(a.video, size, a.bit_depth, fps, **more)
        except ValueError as ex:
            if not more:
                raise
            ap.error(f"--deinterlace: {ex}")
        with reader:
            spec = reader.spec(a.matrix, None if a.range is None else a.range == "full", a.siting)
            bits, size, *rd = encode_video(reader, a.bins, a.recon_video, spec=spec, quantize8=a.quantize8, **options,
                                           **({"deinterlace": setting(reader)} if more else {}))
    else:
        bits, size, *rd = encode_folder(a.frames, a.bins, a.recon, png_device=a.png_device, **options)
    if rd:
        yuv_part = f", PSNR-YUV {rd[0]['ave_all_frame_psnr_yuv']:.3f} dB" if "ave_all_frame_psnr_yuv" in rd[0] else ""
        print(f"PSNR {rd[0]['ave_all_frame_psnr']:.3f} dB, MS-SSIM {rd[0]['ave_all_frame_msssim']:.5f}{yuv_part} -> {a.report}")
    print(f"{len(bits)} pictures, {size[0]}x{size[1]}, {sum(bits)} bits, {sum(bits) / (len(bits) * size[0] * size[1]):.4f} bpp")


def _decode_command(ap, a):
    motion = _motion_option(ap, a)
    if a.base_only and a.roi_root is not None:
        ap.error("--base-only takes no --roi-root: boxes and the residual layer live at full size")
    if a.roi_root is None and os.path.exists(os.path.join(a.bins, ROIQ_JSON)):
        ap.error(f"{os.path.join(a.bins, ROIQ_JSON)}: these pictures were coded with q-scale maps made from ROI boxes; "
                 f"decode needs --roi-root")
    _needs_roi_root(ap, a)
    if a.residuals and a.residual_bins:
        ap.error("give one of --residuals and --residual-bins")
    if a.roi_root is not None and not a.residuals and not a.residual_bins and not os.path.exists(os.path.join(a.bins, ROIQ_JSON)):
        ap.error("decode --roi-root needs --residuals (the decoded residual layer) or --residual-bins (the coded one)")
    if a.grain is not None:
        from . import grain as GR

        if not 1 <= a.grain <= GR.MAX_PERCENT:
            ap.error(f"--grain: PERCENT must be within 1..{GR.MAX_PERCENT}, got {a.grain}")
        if a.base_only:
            ap.error("--base-only takes no --grain: the grain was measured at display size")
        if a.residuals or a.residual_bins:
            ap.error("--grain with --residuals / --residual-bins is not implemented: inside lossless boxes the source's own "
                     "noise is already there")
        if not os.path.exists(os.path.join(a.bins, GR.GRAIN_JSON)):
            ap.error(f"--grain: no {GR.GRAIN_JSON} in {a.bins} (encode --tnr T --grain writes one)")
    roi = _roi_option(ap, a, motion, {c["name"]: c["border"] for c in
                                      ((read_sequence_info(a.bins) or {}).get("roi") or {}).get("classes", [])})
    if (a.recon is None) == (a.recon_video is None):
        ap.error("give exactly one of --recon and --recon-video")
    if a.png_device and a.recon is None:
        ap.error("--png-device belongs to --recon (the PNG folder)")
    info = read_sequence_info(a.bins)
    if info is None and (a.height is None or a.width is None):
        ap.error(f"--height and --width are required (no {SEQUENCE_JSON} beside the .bin files)")
    if a.recon_video is not None:
        from . import yuv as Y

        if os.path.splitext(a.recon_video)[1].lower() not in (".y4m", ".yuv"):
            ap.error("--recon-video takes a .y4m or a .yuv file")
        spec = None
        if a.matrix or a.range or a.siting or a.bit_depth:
            base = info["color"] if info else Y.ColorSpec()
            spec = Y.ColorSpec(a.matrix or base.matrix, base.full_range if a.range is None else a.range == "full",
                               a.siting or base.siting, a.bit_depth or base.bit_depth)
        n = decode_video(a.bins, a.recon_video, a.height, a.width, a.gop, spec, None, a.device, a.precision, a.i_ckpt, a.p_ckpt,
                         roi=roi, residuals=a.residuals, residual_bins=a.residual_bins, verify=a.verify,
                         base_scale=None if a.base_only else "file", grain=a.grain)
    else:
        if a.matrix or a.range or a.siting or a.bit_depth:
            ap.error("--matrix, --range, --siting and --bit-depth belong to --recon-video")
        height, width = a.height or info["height"], a.width or info["width"]
        n = decode_folder(a.bins, a.recon, height, width, a.gop or (info or {}).get("gop"), a.device, a.precision,
                          a.i_ckpt, a.p_ckpt, io_workers=a.io_workers, roi=roi, residuals=a.residuals,
                          residual_bins=a.residual_bins, verify=a.verify, base_scale=None if a.base_only else "file",
                          png_device=a.png_device, grain=a.grain)
    print(f"{n} pictures decoded")


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    {"verify": _verify_command, "boxes": _boxes_command, "noise": _noise_command, "shake": _shake_command, "encode": _encode_command, "decode": _decode_command}[a.cmd](ap, a)


if __name__ == "__main__":
    from .picturehash import PictureHashMismatch

    try:
        main()
    except PictureHashMismatch as ex:  # (the pictures before it, and maybe some after, have been written)
        raise SystemExit(f"run_codec decode: {ex}") from None
