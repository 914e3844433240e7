"""Both modes of tools/shake_time.py, run in-process on a real MI355X at the smallest picture and counts that still run every
line, in the manner of tests/test_gpu_noise_time.py (tests/test_gpu_timing_tools.py's picture, counts and label check): 720 x
1024, `kernels` with 2 launches and 1 round, `boxes` with 34 pictures of either camera and 1 repeat.  Each case asserts that the mode's
variant labels appear in its output in order, each followed by finite positive numbers.  No time is asserted."""
import math

import pytest

from tests.test_gpu_timing_tools import N, RATIO, SETS, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

KERNELS = "shake_plane", "shake_tiles R = 8", "shake_tiles R = 16", "shake_vote", "me_compensate", "noise_cells", "me_search R = 8"
CASES = {
    "kernels": ((2, 1), [k + where for where in SETS for k in KERNELS] +
                ["shake_tiles R = 8 / me_search R = 8 = x", "shake_tiles R = 8 / me_search R = 8 = x"]),
    "boxes": ((N, 1), [label for camera in ("still", "shaking")
                       for label in (f"  {camera} camera, boxes pass  ", f"  {camera} camera, boxes pass --shake 8", RATIO)]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("shake_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
