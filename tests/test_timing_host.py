"""tools/timing.py without a GPU: the two report tables give the committed records' lines when those records' numbers
are fed back in, the alternating loop keeps dict order in every round, the command line parses and refuses as the tools'
own tails did, scenecut_time's `trace` mode reads a kernel trace, and a picture too small for the fixed boxes is refused."""
import sys

import pytest
import torch

from tests.util import load_tool
from tools import timing


def test_rate_table_gives_the_lines_of_profiles_aq_1080p(capsys):
    timing.rate_table({"without": [39.58, 40.83, 40.76], "aq=AQ(100)": [40.80, 40.70, 40.69]}, baseline="without", width=28)
    assert capsys.readouterr().out.splitlines() == [
        "  without                       40.39  (39.58 .. 40.83)   39.58 40.83 40.76",
        "  aq=AQ(100)                    40.73  (40.69 .. 40.80)   40.80 40.70 40.69   +0.8 % against without"]


def test_rate_table_gives_the_lines_of_profiles_redact_1080p(capsys):
    timing.rate_table({"encode_video --roi-root": [15.93, 15.92, 15.91],
                       "encode_video --roi-root --redact motion --redact-tile 16": [15.87, 15.86, 15.84]}, width=58, fmt="7.2f", ratio=True)
    assert capsys.readouterr().out.splitlines() == [
        "  encode_video --roi-root                                      15.92  (15.91 .. 15.93)   15.93 15.92 15.91",
        "  encode_video --roi-root --redact motion --redact-tile 16     15.86  (15.84 .. 15.87)   15.87 15.86 15.84",
        "# with / without = x0.996 in frames/s; the spread of the repeats without the option is x0.999 .. x1.001 of their mean"]


def test_kernel_table_gives_the_lines_of_profiles_redact_1080p(capsys):
    nbytes = {"redact": 24 * 1080 * 1920, "tnr_step": (24 * (20 * 260 / (16 * 256)) + 12) * 1080 * 1920}
    med = timing.kernel_table({"redact, 10 boxes, tile 8, one set of pictures (cache-resident)": [13.02, 12.98, 13.07, 13.02, 13.02],
                               "tnr_step, one set of pictures (cache-resident)": [25.96, 26.20, 25.91, 25.96, 25.95]},
                              lambda name: nbytes[name.split(",")[0]], width=78)
    assert capsys.readouterr().out.splitlines() == [
        "  redact, 10 boxes, tile 8, one set of pictures (cache-resident)                   13.02  (12.98 .. 13.07)     3.82 TB/s",
        "  tnr_step, one set of pictures (cache-resident)                                   25.96  (25.91 .. 26.20)     3.39 TB/s"]
    assert list(med.values()) == [13.02, 25.96]


def test_alternating_keeps_dict_order_in_every_round():
    seen = []
    got = timing.alternating({"b": 2, "a": 1, "c": 3}, 3, lambda v: seen.append(v) or 10 * v + len(seen))
    assert seen == [2, 1, 3] * 3
    assert list(got) == ["b", "a", "c"] and got == {"b": [21, 24, 27], "a": [12, 15, 18], "c": [33, 36, 39]}
    assert timing.alternating({"a": 1}, 0, lambda v: v) == {"a": []}


@pytest.fixture
def command(monkeypatch):
    """main() on a command line, on a machine with or without a GPU: what was called, or what it exited with"""
    def run(argv, modes, default=None, gpu=True):
        monkeypatch.setattr(sys, "argv", ["x_time.py"] + argv)
        monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu)
        try:
            return timing.main("the usage text", "x_time.py", modes, default)
        except SystemExit as e:
            return e
    return run


def test_main_prints_the_doc_for_an_unknown_mode_and_refuses_without_a_gpu(command):
    modes = {"kernels": (lambda *a: ("kernels",) + a, (200, 5)), "clip": (lambda *a: ("clip",) + a, (str, 64))}
    for argv in (["nonsense"], [], ["clip"]):  # (no default mode here; `clip` needs its path)
        got = command(argv, modes)
        assert isinstance(got, SystemExit) and got.code == "the usage text", argv
    got = command(["kernels", "3"], modes, gpu=False)
    assert isinstance(got, SystemExit) and got.code == "x_time.py measures on the GPU; none is visible"
    got = command(["nonsense"], modes, gpu=False)  # the usage text needs no GPU
    assert isinstance(got, SystemExit) and got.code == "the usage text"


def test_main_parses_integers_and_defaults(command):
    modes = {"kernels": (lambda *a: ("kernels",) + a, (200, 5)), "files": (lambda *a: ("files",) + a, (64, 3)),
             "colour": (lambda *a: ("colour",) + a, (20, "plain")), "clip": (lambda *a: ("clip",) + a, (str, 64)),
             "workspace": (lambda *a: ("workspace",) + a, ())}
    assert command(["kernels"], modes) == ("kernels", 200, 5)
    assert command(["kernels", "7"], modes) == ("kernels", 7, 5)
    assert command(["kernels", "7", "2"], modes) == ("kernels", 7, 2)
    assert command([], modes, default="files") == ("files", 64, 3)
    assert command(["colour", "4", "full"], modes) == ("colour", 4, "full")
    assert command(["clip", "a.y4m"], modes) == ("clip", "a.y4m", 64)
    assert command(["workspace"], modes) == ("workspace",)
    with pytest.raises(ValueError):
        command(["kernels", "many"], modes)


def test_scenecut_trace_prints_the_medians_it_was_given(tmp_path, capsys):
    """12 warm-up dispatches, then 2 rounds of 4 variants x 20 dispatches: dispatch j of variant k lasts
    10000 (k + 1) + 100 j ns in both rounds, so its 40 times have the median 10 (k + 1) + 0.95 us."""
    tool = load_tool("scenecut_time")
    names = ("void scene_hist_kernel<4>(Args)", "void roi_kernel<2, false>(Args)")
    rows, now = ["Kind,Kernel_Name,Start_Timestamp,End_Timestamp"], 1000
    for i in range(12):
        rows.append(f'KERNEL_DISPATCH,"{names[(i // 3) % 2]}",{now},{now + 77777}')
        now += 100000
    rows.append(f'KERNEL_DISPATCH,"void some_other_kernel(Args)",{now},{now + 5}')  # (the trace holds torch's kernels too)
    for _ in range(2):
        for k in range(4):
            for j in range(tool.BATCH):
                rows.append(f'KERNEL_DISPATCH,"{names[k % 2]}",{now},{now + 10000 * (k + 1) + 100 * j}')
                now += 100000
    path = tmp_path / "kernel_trace.csv"
    path.write_text("\n".join(rows) + "\n")
    tool.trace(str(path))
    assert capsys.readouterr().out.splitlines() == [
        "# kernel times from a rocprofv3 kernel trace, 1920x1080, 40 dispatches per variant, us: median (min .. max), bytes/s at the median",
        "  scene_hist random        10.95  (10.00 .. 11.90)     2.27 TB/s",
        "  roi_sse random           20.95  (20.00 .. 21.90)     2.38 TB/s",
        "  scene_hist constant      30.95  (30.00 .. 31.90)     0.80 TB/s",
        "  roi_sse constant         40.95  (40.00 .. 41.90)     1.22 TB/s",
        "# random: scene_hist / roi_sse = 0.52  (within the yardstick)",
        "# constant: scene_hist / roi_sse = 0.76  (within the yardstick)"]


def test_a_picture_smaller_than_720_x_1024_is_refused_by_name(monkeypatch, tmp_path):
    assert timing.padded(timing.SIZE) == (1088, 1920) and timing.padded((720, 1024)) == (768, 1024)
    for size in ((704, 1024), (720, 960)):
        monkeypatch.setattr(timing, "SIZE", size)
        with pytest.raises(ValueError, match="at least 720 x 1024"):
            timing.padded(timing.SIZE)
        with pytest.raises(ValueError, match="at least 720 x 1024"):
            timing.moving_box_clip(str(tmp_path), 1, timing.SIZE, noise=1)
        with pytest.raises(ValueError, match="at least 720 x 1024"):
            load_tool("motion_time")  # (a tool takes its size when it is loaded)
