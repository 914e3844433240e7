"""Both modes of tools/tnr_intra_time.py, run in-process on a real MI355X at the smallest picture and counts that still
run every line, in the manner of tests/test_gpu_grain_time.py (tests/test_gpu_timing_tools.py's picture, counts and label
check): 720 x 1024, `kernels` with 2 launches and 2 rounds, `encode` with GOP + 2 = 34 pictures and 2 repeats.  Each case
asserts that the mode's variant labels appear in its output in order, each followed by finite positive numbers."""
import math

import pytest

from tests.test_gpu_timing_tools import N, RATIO, SETS, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

KERNELS = ["tnr_step", "tnr_fuse n=1", "tnr_fuse n=2", "tnr_fuse n=4"]
CASES = {
    "kernels": ((2, 2), [k + SETS[0] for k in KERNELS] + [k + SETS[1] for k in KERNELS] +
                [f"# {where[2:]}: {k} / tnr_step = x" for where in SETS for k in KERNELS[1:]]),
    "encode": ((N, 2), ["  encode_video --tnr 8 --tnr-search 16 ", "  encode_video --tnr 8 --tnr-search 16 --tnr-intra 2", RATIO]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("tnr_intra_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
