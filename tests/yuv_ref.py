"""Not a test: the yardstick of tests/test_yuv_host.py and tests/test_gpu_yuv.py.

Two restatements of include/dcvc_hip_color.h written from its formulas (not from the kernels): `dtype=np.float64`
evaluates them with double-precision constants; `dtype=np.float32` uses the fp32 constants (each derived in double and
rounded once) and one rounded numpy operation per operation of the header, in the header's order, which is what the
kernels must reproduce bit for bit.  Plus the seeded inputs both test files use, and a plain-Python Y4M writer / reader
so that test inputs do not come from the code under test.
"""
import itertools

import numpy as np

MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}


def constants(matrix, full_range, depth, dtype):
    kr, kb = MATRIX[matrix]
    kg = (1.0 - kr) - kb
    s, mx = float(1 << (depth - 8)), float((1 << depth) - 1)
    y_off, c_off = (0.0 if full_range else 16.0 * s), 128.0 * s
    y_range, c_range = (mx, mx) if full_range else (219.0 * s, 224.0 * s)
    k = dict(y_off=y_off, c_off=c_off, y_scale=1.0 / y_range, c_scale=1.0 / c_range, crr=2.0 * (1.0 - kr),
             cgb=2.0 * kb * (1.0 - kb) / kg, cgr=2.0 * kr * (1.0 - kr) / kg, cbb=2.0 * (1.0 - kb), kr=kr, kg=kg, kb=kb,
             icb=1.0 / (2.0 * (1.0 - kb)), icr=1.0 / (2.0 * (1.0 - kr)), y_range=y_range, c_range=c_range)
    k = {n: dtype(v) for n, v in k.items()}
    k["max"] = (1 << depth) - 1
    return k


def upsample16(c, siting):
    """(H/2, W/2) integer chroma -> (H, W) weighted sums in sixteenths, edges clamped."""
    c = c.astype(np.int64)
    up, dn = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    v = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    v[0::2], v[1::2] = 3 * c + up, 3 * c + dn
    lf, rt = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
    out = np.empty((v.shape[0], 2 * v.shape[1]), np.int64)
    if siting == "center":
        out[:, 0::2], out[:, 1::2] = 3 * v + lf, 3 * v + rt
    else:
        out[:, 0::2], out[:, 1::2] = 4 * v, 2 * v + 2 * rt
    return out


def clamp01(v):
    return np.minimum(np.maximum(v, v.dtype.type(0)), v.dtype.type(1))


def to_rgb(y, u, v, matrix="bt709", full_range=False, siting="left", depth=8, dtype=np.float32, quantize8=False):
    """(3, H, W) in `dtype`; with quantize8 the fp32 path returns the table values, the fp64 path the float code k."""
    k = constants(matrix, full_range, depth, dtype)
    sixteenth = dtype(0.0625)
    yp = (y.astype(dtype) - k["y_off"]) * k["y_scale"]
    cb = (upsample16(u, siting).astype(dtype) * sixteenth - k["c_off"]) * k["c_scale"]
    cr = (upsample16(v, siting).astype(dtype) * sixteenth - k["c_off"]) * k["c_scale"]
    rgb = np.stack([clamp01(yp + k["crr"] * cr), clamp01((yp - k["cgb"] * cb) - k["cgr"] * cr), clamp01(yp + k["cbb"] * cb)])
    assert rgb.dtype == dtype
    if quantize8:
        code = np.rint(dtype(255.0) * rgb)
        if dtype is np.float32:
            table = np.arange(256, dtype=np.float32) / np.float32(255.0)
            return table[code.astype(np.int64)]
        return code
    return rgb


def unclamped_mask(y, u, v, matrix="bt709", full_range=False, siting="left", depth=8):
    """Pixels whose RGB triple the fp32 conversion did not clamp (strictly inside (0, 1) before the clamp's effect)."""
    rgb = to_rgb(y, u, v, matrix, full_range, siting, depth, np.float32)
    return ((rgb > 0) & (rgb < 1)).all(axis=0)


def from_rgb(rgb, matrix="bt709", full_range=False, siting="left", depth=8, dtype=np.float32):
    """(3, H, W) floats -> integer planes y (H, W), u, v (H/2, W/2) as int64."""
    k = constants(matrix, full_range, depth, dtype)
    r, g, b = (clamp01(p.astype(dtype)) for p in rgb)
    yp = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    planes = [np.clip(np.rint(yp * k["y_range"] + k["y_off"]), 0, k["max"]).astype(np.int64)]
    for c in ((b - yp) * k["icb"], (r - yp) * k["icr"]):
        if siting == "center":
            f = ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * dtype(0.25)
        else:
            vs = c[0::2] + c[1::2]
            m, rt = vs[:, 0::2], vs[:, 1::2]
            lf = np.concatenate([vs[:, :1], vs[:, 1:-1:2]], 1)
            f = ((lf + rt) + (m + m)) * dtype(0.125)
        assert f.dtype == dtype
        planes.append(np.clip(np.rint(f * k["c_range"] + k["c_off"]), 0, k["max"]).astype(np.int64))
    return planes


def psnr_yuv(src_planes, rec_planes, depth):
    """float64 formula: per-plane PSNR from integer sums and (6 Y + U + V) / 8; also returns the sums."""
    peak = float((1 << depth) - 1) ** 2
    sums = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(src_planes, rec_planes)]
    ps = [10.0 * np.log10(peak / (s / a.size)) if s else float("inf") for s, a in zip(sums, src_planes)]
    return sums, (ps[0], ps[1], ps[2], (6.0 * ps[0] + ps[1] + ps[2]) / 8.0)


# ---------------------------------------------------------------------------------------------------------- inputs
def sample_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def gamut_rgb(seed, n, h, w):
    """In-gamut content: smooth fields plus noise; sizes the generator's octaves do not suit get seeded noise."""
    if min(h, w) < 16:
        return np.random.default_rng(seed).random((n, 3, h, w), dtype=np.float32)
    from vcm_ts_amd.synthetic import frames

    return frames(seed, n, h, w)


def gamut_planes(seed, h, w, matrix="bt709", full_range=False, siting="left", depth=8):
    """(a) in-gamut content taken through the float64 restatement's RGB -> 4:2:0."""
    y, u, v = from_rgb(gamut_rgb(seed, 1, h, w)[0], matrix, full_range, siting, depth, np.float64)
    return tuple(p.astype(sample_dtype(depth)) for p in (y, u, v))


def random_planes(seed, h, w, depth=8):
    """(b) uniformly random samples over the whole code range: exercises the clamps."""
    g = np.random.default_rng(seed)
    return tuple(g.integers(0, 1 << depth, size=s, dtype=np.int64).astype(sample_dtype(depth))
                 for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


SIZES = [(2, 2), (64, 64), (66, 130), (270, 482), (1080, 1920)]
MID = (270, 482)
DEFAULT = dict(matrix="bt709", full_range=False, siting="left", depth=8)


def cases():
    """[(id, h, w, colour keywords)]: the defaults at every size, every combination at the mid size."""
    out = [(f"{h}x{w}-default", h, w, dict(DEFAULT)) for h, w in SIZES if (h, w) != MID]
    for m, fr, st, d in itertools.product(("bt709", "bt601"), (False, True), ("left", "center"), (8, 10)):
        out.append((f"{MID[0]}x{MID[1]}-{m}-{'full' if fr else 'limited'}-{st}-{d}", MID[0], MID[1],
                    dict(matrix=m, full_range=fr, siting=st, depth=d)))
    return out


def case_seed(name):
    import zlib

    return zlib.crc32(name.encode()) % 100000


def case_planes(name, h, w, col, kind):
    seed = case_seed(name)
    return gamut_planes(seed, h, w, **col) if kind == "gamut" else random_planes(seed + 1, h, w, col["depth"])


def case_rgb(name, h, w, kind):
    """RGB inputs of the RGB -> 4:2:0 checks: in-gamut content, or noise reaching beyond [0, 1] (clamped on load)."""
    seed = case_seed(name)
    if kind == "gamut":
        return gamut_rgb(seed + 2, 1, h, w)[0]
    return (np.random.default_rng(seed + 3).random((3, h, w), dtype=np.float32) * np.float32(1.5) - np.float32(0.25))


def to_i420(planes):
    """file order: Y plane, U plane, V plane, as one flat array of samples"""
    return np.concatenate([p.reshape(-1) for p in planes])


def from_i420(flat, h, w):
    n = h * w
    return flat[:n].reshape(h, w), flat[n:n + n // 4].reshape(h // 2, w // 2), flat[n + n // 4:].reshape(h // 2, w // 2)


# ----------------------------------------------------------------------------------------- plain-Python Y4M for tests
def write_y4m(path, frames_planes, w, h, chroma="420mpeg2", fps="25:1", extra="", interlace="p", frame_line=b"FRAME\n"):
    """frames_planes: list of (y, u, v) arrays (uint8, or uint16 written little-endian)."""
    with open(path, "wb") as f:
        head = f"YUV4MPEG2 W{w} H{h} F{fps} I{interlace} A1:1 C{chroma}"
        f.write((head + (" " + extra if extra else "") + "\n").encode())
        for planes in frames_planes:
            f.write(frame_line)
            for p in planes:
                f.write(np.ascontiguousarray(p).astype("<u2" if p.dtype.itemsize == 2 else np.uint8).tobytes())


def read_y4m(path):
    """(header tokens, list of flat sample arrays)"""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    tokens = data[:end].decode().split(" ")
    assert tokens[0] == "YUV4MPEG2"
    fields = {t[0]: t[1:] for t in tokens[1:] if t[0] != "X"}
    fields["X"] = [t[1:] for t in tokens[1:] if t[0] == "X"]
    w, h = int(fields["W"]), int(fields["H"])
    dt = np.dtype("<u2") if fields.get("C", "420") == "420p10" else np.dtype(np.uint8)
    nbytes = w * h * 3 // 2 * dt.itemsize
    frames, at = [], end + 1
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n", at
        frames.append(np.frombuffer(data[at + 6:at + 6 + nbytes], dtype=dt))
        assert frames[-1].size == w * h * 3 // 2
        at += 6 + nbytes
    return fields, frames
