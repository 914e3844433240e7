"""Build guards that need no GPU.

The product library must hold NO packed-FP32 VALU instruction (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32): round 2
traced a run-to-run difference of one kernel to such code running beside another stream's 16-bit MFMA kernels
(DESIGN.md 4b), and an encoder and a decoder must compute the same bits whatever runs beside them.  The build switches
the target feature off (vcm_ts_amd/csrc/Makefile, NOPK); this test checks the RESULT -- the shipped ISA -- so that a
toolchain that stops honouring the flag, or a build that drops it, fails here and not in a decoder.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_isa  # noqa: E402

CSRC = os.path.join(ROOT, "vcm_ts_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_toolchain = pytest.mark.skipif(not (os.path.exists(check_isa.OBJDUMP) and os.path.exists(HIPCC)),
                                     reason="ROCm LLVM tools not installed")


@needs_toolchain
def test_product_library_has_no_packed_fp32_instructions():
    census = check_isa.packed_fp32_census(os.path.join(CSRC, "libdcvc_hip.so"))
    # one gfx950 code object per translation unit of the Makefile's HIPSRC
    hipsrc = [ln for ln in open(os.path.join(CSRC, "Makefile")) if ln.startswith("HIPSRC")][0].split(":=")[1].split()
    assert len(census) == len(hipsrc), (sorted(census), hipsrc)
    assert sum(c["mfma"] for c in census.values()) > 1000  # the disassembly really is the kernels
    offenders = {obj: c["packed"] for obj, c in census.items() if c["packed"]}
    assert not offenders, offenders


@needs_toolchain
def test_the_guard_sees_packed_fp32_when_it_is_there(tmp_path):
    """The same source with and without the build's flag: the checker must tell them apart (it is not vacuous), and
    the device pass must accept the flag silently (the Makefile fails the build on its 'not a recognized feature')."""
    src = tmp_path / "pk.hip"
    src.write_text("#include <hip/hip_runtime.h>\n"
                   "__global__ void k(float2 *a, const float2 *b) { int i = threadIdx.x; float2 x = a[i], y = b[i];\n"
                   "  x.x = x.x * y.x + 1.f; x.y = x.y * y.y + 1.f; a[i] = x; }\n")
    nopk = [ln for ln in open(os.path.join(CSRC, "Makefile")) if ln.startswith("NOPK")][0].split("?=")[1].split()
    counts = {}
    for tag, extra in (("plain", []), ("nopk", nopk)):
        fb = tmp_path / f"{tag}.hipfb"
        dev = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-cuid=t", "--offload-device-only", *extra,
                              "-c", str(src), "-o", str(fb)], capture_output=True, text=True)
        assert dev.returncode == 0, dev.stderr
        assert "not a recognized feature" not in dev.stderr, dev.stderr
        obj, so = tmp_path / f"{tag}.o", tmp_path / f"lib{tag}.so"
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-cuid=t", "--offload-host-only", "-Xclang",
                        "-fcuda-include-gpubinary", "-Xclang", str(fb), "-c", str(src), "-o", str(obj)], check=True,
                       capture_output=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(so), str(obj)], check=True,
                       capture_output=True)
        census = check_isa.packed_fp32_census(str(so))
        assert len(census) == 1
        counts[tag] = sum(sum(c["packed"].values()) for c in census.values())
    assert counts["plain"] > 0 and counts["nopk"] == 0, counts


def test_makefile_does_not_filter_compiler_diagnostics():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "grep -v" not in mk
    assert "check-isa" in mk.split("all:")[1].splitlines()[0]


@needs_toolchain
def test_dominant_kernel_keeps_its_occupancy_and_does_not_spill():
    """conv_k32<3,4,8> (half of the GPU time of a P picture) is built for FOUR waves per SIMD and TWO workgroups per CU:
    at most 128 registers per lane and 80 KB of LDS -- and nothing in scratch: round 3 found two spilled staging offsets
    whose reloads (vector-memory loads behind vmcnt(0)) sat in front of every chunk's patch request in the main loop
    (DESIGN.md 4.1 item 3e).  Read from the shipped code object's metadata, so a compiler or source change that brings
    a spill back or drops the occupancy fails here."""
    res = check_isa.kernel_resources(os.path.join(CSRC, "libdcvc_hip.so"))
    main = [v for k, v in res.items() if "conv_k32ILi3ELi4ELi8E" in k]
    assert len(main) == 1, sorted(k for k in res if "conv_k32" in k)
    k = main[0]
    assert k["vgpr_count"] + k["agpr_count"] <= 128, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] <= 160 * 1024 // 2, k
    assert k["max_flat_workgroup_size"] == 512, k
    # every kernel of the library: metadata present, and no kernel needs more than a few dwords of scratch
    assert len(res) > 50
    worst = max(res.items(), key=lambda kv: kv[1]["vgpr_spill_count"])
    assert worst[1]["vgpr_spill_count"] <= 16, worst


def _k32_args(H, W, cs=64, ps=0, cout=64):
    """Arguments that pass every check of dcvc_conv2d_k32 except possibly the picture-size limits; the pointers are
    aligned dummies -- a refused call returns before anything is launched or dereferenced."""
    from vcm_ts_amd import lib

    a = lib.ConvArgs()
    a.nseg, a.N, a.Hin, a.Win = 1, 1, H, W
    a.seg[0].ptr, a.seg[0].C, a.seg[0].cs = 0x1000, 32, cs
    a.wpack, a.bpack, a.out = 0x2000, 0x3000, 0x4000
    a.ks, a.stride, a.Cout, a.Cout_pad, a.out_cs = 3, 1, cout, 64, 64
    a.pixel_shuffle, a.precision = ps, lib.PRECISIONS["fp16x3"]
    return a


def test_conv_k32_refuses_pictures_beyond_its_24_bit_address_arithmetic():
    """the kernel multiplies pixel index by channel stride with 24-bit multiplies (conv_k32.hip load_patch /
    out_off); a 6144x3456 picture passes the 4 GiB checks at 32..63 channels and used to be addressed wrongly.  The
    entry point now refuses (DCVC_E_ARG, callers fall back to dcvc_conv2d).  Host-only: a refused call launches nothing."""
    import ctypes as C

    from vcm_ts_amd import lib

    L = lib.hip()
    E_ARG = -1
    assert L.dcvc_conv2d_k32(C.byref(_k32_args(3456, 6144, cs=32)), None) == E_ARG        # 21.2 M pixels, 2.7 GB image
    assert L.dcvc_conv2d_k32(C.byref(_k32_args(4096, 4096, cs=32)), None) == E_ARG        # exactly 2^24 pixels
    assert L.dcvc_conv2d_k32(C.byref(_k32_args(2048, 2048 + 64, cs=64, ps=1)), None) == E_ARG  # 4 x 4.3 M after the shuffle
    assert L.dcvc_conv2d_k32(C.byref(_k32_args(64, 64, cs=1 << 22)), None) == E_ARG        # channel stride in bytes >= 2^24
    assert L.dcvc_conv_k32_set_waves(6) == E_ARG
    assert L.dcvc_conv_k32_set_waves(8) == 0


def test_engine_routing_ignores_stray_environment(monkeypatch):
    """Which kernel serves a layer is part of the arithmetic: the developer switches are honoured only with DCVC_DEV=1."""
    src = open(os.path.join(ROOT, "vcm_ts_amd", "engine.py")).read()
    for name in ("DCVC_SMALL", "DCVC_K32", "DCVC_PAIR_TAPS", "DCVC_K32_SIZES"):
        assert f'sw("{name}"' in src and f'os.environ.get("{name}"' not in src, name
    k32 = open(os.path.join(CSRC, "conv_k32.hip")).read()
    assert "getenv" not in k32
    # the C library: launch-geometry A/B switches (never a result bit) go through dev_env_long, which reads them only
    # when DCVC_DEV=1 -- no other getenv in the product sources
    import glob
    import re
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        text = open(path).read()
        body = re.sub(r"inline long dev_env_long\(.*?\n}\n", "", text, flags=re.S)
        assert "getenv" not in body, os.path.basename(path)


def test_developer_switch_patch_applies_to_the_product_kernel(tmp_path):
    """__graft_entry__.build() also builds tools/probes, whose conv_k32_dev.hip is the product kernel with
    tools/probes/conv_k32_dev_switches.patch applied: an edit of conv_k32.hip that the patch no longer fits would fail the
    round's build check (it did once, round 4) -- so it fails here first."""
    if shutil.which("patch") is None:
        pytest.skip("patch not installed")
    out = tmp_path / "conv_k32_dev.hip"
    r = subprocess.run(["patch", "-s", "-o", str(out), os.path.join(CSRC, "conv_k32.hip"),
                        os.path.join(ROOT, "tools", "probes", "conv_k32_dev_switches.patch")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = out.read_text()
    assert "K32_ABLATE" in text and "slot_pixel" in text


@pytest.mark.parametrize("sizes", [0, 8], ids=["zero-sizes", "null-pointers"])
def test_every_entry_point_refuses_null_and_empty_arguments(sizes):
    """Every status-returning entry point of include/dcvc_hip*.h, called with NULL pointers (zeroed argument structs) and
    either zero or plausible sizes, must answer DCVC_E_ARG before anything is launched or dereferenced -- a caller's bug
    must not become a GPU fault (which on this pool can reset a whole node).  Host-only: a refused call touches no GPU."""
    import ctypes as C

    from vcm_ts_amd import lib

    L = lib.hip()
    for name, sig in lib._SIGS.items():
        if name in ("dcvc_conv_k32_set_waves", "dcvc_pack_plan_destroy"):  # a mode switch; a void destructor (NULL is a no-op)
            continue
        args, keep = [], []
        for t in sig:
            if t in (lib.i32, lib.i64):
                args.append(sizes)
            elif t is lib.f32:
                args.append(1.0)
            elif t is lib.vp:
                args.append(None)
            else:  # POINTER(argument struct): all fields zero
                keep.append(t._type_())
                args.append(C.byref(keep[-1]))
        assert getattr(L, name)(*args) == -1, name
    L.dcvc_pack_plan_destroy(None)


# argument order of the forward entry points below; pointers are aligned dummies (a refused call returns before anything is
# launched or dereferenced), every other value is plausible unless a case overrides it
_FWD_ABI = {
    "dcvc_scale_channels": ("src src_cs out out_cs q_basic q_scale mode N HW C", {"src_cs": 8, "out_cs": 8, "mode": 0}),
    "dcvc_round_symbols": ("z z_cs z_hat zh_cs sym N H W C", {"z_cs": 8, "zh_cs": 8}),
    "dcvc_symbols_to_nhwc": ("sym out out_cs N H W C", {"out_cs": 8}),
    "dcvc_scale_bits": ("y_q scales_hat out scratch kind N per_sample", {"kind": 0}),
    "dcvc_factorized_bits": ("z_hat z_cs params out scratch N HW C", {"z_cs": 8}),
    "dcvc_sq_err": ("a a_cs b b_cs out scratch N HW C", {"a_cs": 8, "b_cs": 8}),
    "dcvc_se_gate": ("mean w1 w2 gate N C Cr", {"Cr": 2}),
    "dcvc_down2": ("src src_cs out out_cs N H W C scale avgpool_order", {"src_cs": 8, "out_cs": 8, "scale": 1.0, "avgpool_order": 0}),
    "dcvc_maxpool2": ("src src_cs out out_cs N H W C", {"src_cs": 8, "out_cs": 8}),
    "dcvc_warp": ("src src_cs flow flow_cs out out_cs N H W C", {"src_cs": 8, "flow_cs": 4, "out_cs": 8}),
    "dcvc_channel_mean": ("src src_cs mean scratch N HW C", {"src_cs": 8}),
}
_FWD_SIZES = {"N": 2, "H": 4, "W": 6, "HW": 24, "C": 8, "per_sample": 24}
_FWD_POINTERS = ("src", "out", "q_basic", "q_scale", "z", "z_hat", "sym", "y_q", "scales_hat", "scratch", "params", "a", "b",
                 "mean", "w1", "w2", "gate", "flow")


def _fwd_call(L, name, **override):
    from vcm_ts_amd import lib

    order, fixed = _FWD_ABI[name]
    assert len(order.split()) + 1 == len(lib._SIGS[name]), name  # the order above is the header's, plus the stream
    vals = dict(_FWD_SIZES, **fixed)
    vals.update({p: 0x10000 * (k + 1) for k, p in enumerate(_FWD_POINTERS)})
    assert set(override) <= set(order.split()), (name, override)
    vals.update(override)
    return getattr(L, name)(*[vals[k] for k in order.split()], None)


def test_forward_entry_points_refuse_non_positive_sizes_and_short_strides():
    """dcvc_scale_channels, dcvc_round_symbols, dcvc_symbols_to_nhwc, dcvc_scale_bits, dcvc_factorized_bits, dcvc_sq_err and
    dcvc_se_gate used to launch with whatever sizes they were given: N = 0 reached the runtime as a zero-sized grid
    (DCVC_E_LAUNCH), a channel stride below C made neighbouring pixels overlap.  They answer DCVC_E_ARG now, like their
    siblings, for every size <= 0 and every channel stride < C.  Host-only: a refused call launches nothing."""
    from vcm_ts_amd import lib

    L = lib.hip()
    sizes = {"dcvc_scale_channels": ("N", "HW", "C"), "dcvc_round_symbols": ("N", "H", "W", "C"),
             "dcvc_symbols_to_nhwc": ("N", "H", "W", "C"), "dcvc_scale_bits": ("N", "per_sample"),
             "dcvc_factorized_bits": ("N", "HW", "C"), "dcvc_sq_err": ("N", "HW", "C"), "dcvc_se_gate": ("N", "C", "Cr")}
    strides = {"dcvc_scale_channels": ("src_cs", "out_cs"), "dcvc_round_symbols": ("z_cs", "zh_cs"),
               "dcvc_symbols_to_nhwc": ("out_cs",), "dcvc_factorized_bits": ("z_cs",), "dcvc_sq_err": ("a_cs", "b_cs")}
    for name, keys in sizes.items():
        for key in keys:
            for bad in (0, -1, -(2 ** 31)):
                assert _fwd_call(L, name, **{key: bad}) == -1, (name, key, bad)
    for name, keys in strides.items():
        for key in keys:
            for bad in (7, 0, -8):
                assert _fwd_call(L, name, **{key: bad}) == -1, (name, key, bad)
    # a z_hat stride is only looked at when there is a z_hat -- and without z_hat AND sym there is nothing to do
    assert _fwd_call(L, "dcvc_round_symbols", z_hat=None, sym=None) == -1
    assert _fwd_call(L, "dcvc_se_gate", C=257) == -1 and _fwd_call(L, "dcvc_se_gate", Cr=65) == -1


def test_resamplers_refuse_odd_and_degenerate_pictures():
    """dcvc_down2 / dcvc_maxpool2 need even H and W (a 2x2 block per output), dcvc_warp needs H, W >= 2 (its
    normalised grid divides by (size - 1) / 2)."""
    from vcm_ts_amd import lib

    L = lib.hip()
    for name in ("dcvc_down2", "dcvc_maxpool2"):
        for bad in ({"H": 5}, {"W": 7}, {"H": 1}, {"W": 1}, {"H": 0}, {"W": 0}, {"N": 0}, {"C": 0}):
            assert _fwd_call(L, name, **bad) == -1, (name, bad)
    for bad in ({"H": 1}, {"W": 1}, {"H": 0}, {"W": -3}, {"N": 0}, {"C": 0}):
        assert _fwd_call(L, "dcvc_warp", **bad) == -1, bad


def test_channel_mean_accepts_only_power_of_two_channel_counts_and_aligned_views():
    """channel_partial gives 16 bytes (4 channels) to a lane and 256 / (C / 4) pixels to a pass: C must be one of
    4, 8, ..., 256, the channel stride a multiple of 4 floats and the view 16-byte aligned."""
    from vcm_ts_amd import lib

    L = lib.hip()
    for C_ in (3, 12, 96, 512, 0, -4):
        assert _fwd_call(L, "dcvc_channel_mean", C=C_, src_cs=512) == -1, C_
    for cs in (9, 10, 11, 66):
        assert _fwd_call(L, "dcvc_channel_mean", src_cs=cs) == -1, cs
    for off in (4, 8, 12, 1):
        assert _fwd_call(L, "dcvc_channel_mean", src=0x10000 + off) == -1, off
    for key in ("N", "HW"):
        assert _fwd_call(L, "dcvc_channel_mean", **{key: 0}) == -1, key
