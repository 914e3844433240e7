"""Both modes of tools/deint_time.py, run in-process on a real MI355X at the smallest picture and counts that still run every
line, in the manner of tests/test_gpu_grain_time.py (tests/test_gpu_timing_tools.py's picture, counts and label check): 720 x
1024, `kernels` with 2 launches and 1 round, `encode` with GOP + 2 = 34 pictures and 1 repeat.  Each case asserts that the
mode's variant labels appear in its output in order, each followed by finite positive numbers.  No time is asserted."""
import math

import pytest

from tests.test_gpu_timing_tools import N, RATIO, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

WHERE = ", one set of frames (cache-resident)", ", rotating over 16 sets (HBM)"
CASES = {
    "kernels": ((2, 1), [f"{k}, {depth} bits{field}{where}" for depth in (8, 10) for where in WHERE
                         for k, field in (("deinterlace420", ", earlier field"), ("deinterlace420", ", later field"), ("yuv420_to_rgb", ""))]),
    "encode": ((N, 1), ["  encode_video, the file labelled Ip", "  encode_video --deinterlace frame, labelled It", RATIO]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("deint_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
