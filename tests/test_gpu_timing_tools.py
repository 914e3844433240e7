"""Every mode of every tools/*_time.py tool, run in-process on a real MI355X at the smallest picture and counts that still
run every line: a rename in the package that breaks a measuring tool fails here, not on the day a measurement is wanted.

The picture is 720 x 1024: the smallest in which the tools' fixed 384 x 256 rectangle at rows 400..656 and its travel of
W - 512 columns fit, and one that pads (to 768 x 1024), so the crop path that 1080 -> 1088 takes is taken.  `kernels`
modes get 2 launches and 1 round; file modes get GOP + 2 = 34 pictures and 1 repeat, the smallest count for which the
tools' own warm-up of GOP + 2 pictures and a second GOP both exist.  Each case asserts that the mode's variant labels
appear in its output in order, each followed by finite positive numbers; the checks the tools make themselves (equal
.bin totals, equal digests, the resampler against its numpy restatement) are assertions inside them and fail the case."""
import math
import os
import re
import sys

import pytest

from tests.util import load_tool
from tools import timing

pytestmark = pytest.mark.gpu
SIZE, N = (720, 1024), 34

CACHE = ", one picture (cache-resident)", ", rotating over 16 pictures (HBM)"
SETS = ", one set of pictures (cache-resident)", ", rotating over 16 sets (HBM)"
REDACT = ["redact, no block touched, tile 8", "redact, 10 boxes, tile 8", "redact, the whole picture, tile 8",
          "redact, the whole picture, tile 64", "redact, the whole picture, fill"]
RATIO = "# with / without = x"
CASES = {
    ("aq_time", "kernels"): ((2,), ["dcvc_aq_activity" + CACHE[0], "dcvc_aq_activity" + CACHE[1], "dcvc_aq_map",
                                    "AqMaps.map (memset + both launches, from Python)"]),
    ("aq_time", "files"): ((N, 1), ["# encode_video", "  without", "  aq=AQ(100)"]),
    ("aq_time", "decode"): ((N, 1, True), ["# decode_video", "  without", "  aq=AQ(100)"]),
    ("motion_time", "kernels"): ((2, 1), ["motion_step" + CACHE[0], "aq_activity" + CACHE[0], "motion_step" + CACHE[1],
                                          "aq_activity" + CACHE[1], "motion_step / aq_activity = x", "motion_step / aq_activity = x"]),
    ("motion_time", "boxes"): ((N, 1), ["boxes pass (read, convert, scan, box rule, write)"]),
    ("picturehash_time", "kernels"): ((2,), ["  pixels, the 1080x1920 crop (6.2 MB of codes from 24.9 MB of fp32)",
                                             "  state, all of 3x1088x1920 fp32 (25.1 MB)"]),
    ("picturehash_time", "files"): ((N, 1), ["without picture_hash", "picture_hash=True"]),
    ("ratectl_time", "model"): ((6,), ["# target 0.50 x", "predicted / actual over", "# target 0.75 x", "predicted / actual over",
                                       "# target 1.50 x", "predicted / actual over"]),
    ("ratectl_time", "files"): ((N, 1), ["without target_bpp", "target_bpp="]),
    ("ratectl_time", "write_clip"): ((None, 2), []),
    ("redact_time", "kernels"): ((2, 1), [r + SETS[0] for r in REDACT] + ["tnr_step" + SETS[0]] + [r + SETS[1] for r in REDACT] + ["tnr_step" + SETS[1]]),
    ("redact_time", "encode"): ((N, 1), ["  encode_video --roi-root  ", "  encode_video --roi-root --redact motion --redact-tile 16", RATIO]),
    ("roi_time", "kernels"): ((2, 8), ["# 8 boxes, 2 launches each"]),
    ("roi_time", "host"): ((1,), ["  0 boxes", "  8 boxes", " 64 boxes"]),
    ("roi_time", "files"): ((N, 1), ["without roi", "roi,  8 boxes a picture, residuals to .gbrp", "roi, 64 boxes a picture, residuals to .gbrp"]),
    ("roil_time", "kernels"): ((2, 8, 1), ["# 8 boxes, step 1"]),
    ("roil_time", "files"): ((N, 1), ["without roi"] + [f"{b:2d} boxes a picture, {how}" for b in (0, 8, 64)
                                                        for how in ("residuals to .gbrp", "residual_bins (.rl)")] +
                             [f"# {b:2d} boxes: records of" for b in (0, 8, 64)]),
    ("scale_time", "kernels"): ((2,), ["3840x2160 -> 1920x1080", "1920x1080 -> 960x540", "960x540 -> 1920x1080"]),
    ("scale_time", "files"): ((N, 1), ["without base_scale", "base_scale=1/2"]),
    ("scale_time", "workspace"): ((), ["coded at 1/2 (a 1920x1080 base layer), fp16x3:", "peak reserved"]),
    ("scenecut_time", "kernels"): ((1,), ["scene_hist random", "roi_sse random", "scene_hist constant", "roi_sse constant"]),
    ("scenecut_time", "scan"): ((N, 1), ["scan pass alone, Y4M file", "scan pass alone, PNG folder, 8 readers", "encode (Y4M), plain",
                                         "encode (Y4M), --scenecut 0.5"]),
    ("tnr_time", "kernels"): ((2, 1), ["tnr_step" + SETS[0], "motion_step" + SETS[0], "tnr_step" + SETS[1], "motion_step" + SETS[1],
                                       "tnr_step / motion_step = x", "tnr_step / motion_step = x"]),
    ("tnr_time", "encode"): ((N, 1), ["  encode_video ", "  encode_video --tnr 8", RATIO]),
    ("yuv_io_time", "files"): ((N, 1), ["encode_folder, PNG folder, 8 I/O threads       bins only", "encode_video,  Y4M file,  no helper threads    bins only",
                                        "encode_folder, PNG folder, 8 I/O threads     + reconstruction output",
                                        "encode_video,  Y4M file,  no helper threads  + reconstruction output",
                                        "encode_folder io_workers=0   bins only", "encode_video  io_workers=0   bins only",
                                        "encode_folder io_workers=0 + reconstruction output", "encode_video  io_workers=0 + reconstruction output"]),
    ("yuv_io_time", "kernels"): ((2, "plain"), ["# variant plain: 2 launches each"]),
    ("yuv_io_time", "kernels full"): ((2, "full"), ["# variant full: 2 launches each"]),
}


def numbers_after(label, lines, start):
    """(the index of the first line from `start` on that holds `label`, the numbers that follow it on that line): the
    signed per-cent column, the only figure that may be negative, is left out."""
    for at in range(start, len(lines)):
        if label in lines[at]:
            rest = re.sub(r"[-+]\d+\.\d+ % against.*", "", lines[at].split(label, 1)[1])
            assert not re.search(r"\bnan\b|\binf\b|-\d", rest), lines[at]
            return at, [float(x) for x in re.findall(r"(?<![\w.])\d+(?:\.\d+)?(?:e[-+]?\d+)?", rest)]
    raise AssertionError(f"no line with {label!r} after line {start} of:\n" + "\n".join(lines))


@pytest.fixture
def small(monkeypatch):
    monkeypatch.setattr(timing, "SIZE", SIZE)
    monkeypatch.delitem(sys.modules, "tools.roi_time", raising=False)  # (roil_time takes its pictures from it: at this size)
    yield
    sys.modules.pop("tools.roi_time", None)


@pytest.mark.parametrize("tool,mode", list(CASES), ids=[f"{t}-{m.replace(' ', '-')}" for t, m in CASES])
def test_mode_runs_and_reports(tool, mode, small, capsys, tmp_path):
    args, labels = CASES[tool, mode]
    module = load_tool(tool)
    assert (module.H, module.W) == SIZE
    if mode == "write_clip":
        args = (str(tmp_path / "clip.y4m"),) + args[1:]
    if mode == "decode":
        module.files(*args[:2], decode=args[2])
    else:
        getattr(module, mode.split()[0])(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
    if mode == "write_clip":
        assert os.path.getsize(tmp_path / "clip.y4m") > 2 * SIZE[0] * SIZE[1] * 3 // 2
