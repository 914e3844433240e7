"""Both modes of tools/noise_time.py, run in-process on a real MI355X at the smallest picture and counts that still run every
line, in the manner of tests/test_gpu_deint_time.py (tests/test_gpu_timing_tools.py's picture, counts and label check): 720 x
1024, `kernels` with 2 launches and 1 round, `encode` with GOP + 2 = 34 pictures and 1 repeat.  Each case asserts that the
mode's variant labels appear in its output in order, each followed by finite positive numbers.  No time is asserted."""
import math

import pytest

from tests.test_gpu_timing_tools import N, RATIO, SETS, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

INPUTS = "the noisy pictures' own words", "words spread over 3584 bins", "ALL WORDS IN ONE BIN"
CASES = {
    "kernels": ((2, 1), [k + where for where in SETS for k in ("noise_cells", "motion_step")] +
                ["noise_cells / motion_step = x", "noise_cells / motion_step = x"] +
                [f"noise_hist, {p}, {name}" for p in (" 1 picture ", "64 pictures") for name in INPUTS]),
    "encode": ((N, 1), ["  encode_video --tnr ", "  encode_video --tnr-auto", RATIO]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("noise_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
