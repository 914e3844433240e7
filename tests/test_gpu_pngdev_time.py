"""Both modes of tools/pngdev_time.py, run in-process on a real MI355X at the smallest picture and counts that still run
every line, in the manner of tests/test_gpu_timing_tools.py (whose picture and label check these are): 720 x 1024,
`kernels` with 2 launches and 1 round, `files` with 4 pictures, 1 repeat and 2 writer threads.  Each case asserts that the
mode's labels appear in its output in order, each followed by finite positive numbers; no time is asserted."""
import math

import pytest

from tests.test_gpu_timing_tools import CACHE, SIZE, numbers_after, small  # noqa: F401 (small: a fixture)
from tests.util import load_tool

pytestmark = pytest.mark.gpu

CASES = {
    "kernels": ((2, 1), ["png_encode" + CACHE[0], "hash_pixels" + CACHE[0], "png_encode" + CACHE[1], "hash_pixels" + CACHE[1],
                         "# png_encode / hash_pixels = x", "# png_encode / hash_pixels = x", "synthetic.frames, noise-free",
                         "sigma 1.5 codes", "flat 77"]),
    "files": ((4, 1, 2), ["# folder sizes: ", "  without png_device", "  png_device=True", "  without png_device", "  png_device=True"]),
}


@pytest.mark.parametrize("mode", list(CASES))
def test_mode_runs_and_reports(mode, small, capsys):
    args, labels = CASES[mode]
    module = load_tool("pngdev_time")
    assert (module.H, module.W) == SIZE
    getattr(module, mode)(*args)
    lines = capsys.readouterr().out.splitlines()
    at = -1
    for label in labels:
        at, found = numbers_after(label, lines, at + 1)
        assert found and all(math.isfinite(x) and x > 0 for x in found), lines[at]
