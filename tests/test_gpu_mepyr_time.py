"""Both modes of tools/mepyr_time.py, run in-process on a real MI355X at the smallest picture and counts that still run every
line, in the manner of tests/test_gpu_timing_tools.py (whose picture, counts and label check these are): 720 x 1024,
`kernels` with 2 launches and 1 round, `encode` with GOP + 2 = 34 pictures and 1 repeat.  Each case asserts that the mode's
variant labels appear in its output in order, each followed by finite positive numbers."""
import math

import pytest

from tests.test_gpu_timing_tools import N, RATIO, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

TAGS = [" L=2 R=32", " L=1 R=64", " L=2 R=128"]
CASES = {
    "kernels": ((2, 1), ["  me_pyramid"] + [f"  {k}{tag}" for tag in TAGS for k in ("me_coarse", "me_descend", "chain")] + ["  me_search R=32"] +
                [f"# chain{tag}: " for tag in TAGS]),
    "encode": ((N, 1), ["  encode_video --tnr 8 --tnr-search 32 ", "  encode_video --tnr 8 --tnr-search 32 --tnr-levels 2", RATIO]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("mepyr_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
