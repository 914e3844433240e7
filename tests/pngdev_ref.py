"""include/dcvc_hip_png.h restated in numpy and plain Python, from the header's text: the row filters and their choice, the
tokens, the prices, the bit packing, the chunks and the file.  zlib.crc32 / zlib.adler32 are used as the format's own
checksums and nothing else of zlib is: what zlib and PIL make of the result is the tests' business.

    codes(rgb)                      (H, W, 3) uint8 of a (3, H, W) float32 picture
    band_string(c, y0, rows)        the filtered rows of one band, with their type bytes
    tokens(string)                  [(literal byte,) or (match length,)] per the greedy rule
    band_data(string, words, force) (the band's deflate bytes, "stored" or the preset's index); force: that coding only
    encode(c, R, words, force)      the file; bands(...) the per-band details
    chunks(file)                    [(type, data)] with every length and CRC checked
"""
import struct
import zlib

import numpy as np

from tests.pixel_ref import code

BAND_MAX, SEG, NSYM, HEADER_WORDS, PRESET_WORDS, SLOT_BYTES = 24576, 64, 286, 72, 360, 24576 + 32
MAX_W, MAX_PRESETS, PREFIX, TRAILER = 8191, 32, 47, 33
SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])


def codes(rgb):
    """(H, W, 3) uint8: code() of a (3, H, W) float32 picture, interleaved."""
    return np.ascontiguousarray(code(np.asarray(rgb, np.float32)).astype(np.uint8).transpose(1, 2, 0))


def default_rows(W):
    return BAND_MAX // (3 * W + 1)


def bound(H, W, R):
    return 80 + H * (3 * W + 1) + 17 * -(-H // R)


# ------------------------------------------------------------------------------------------------------------- filters
def filtered_rows(c, y):
    """The five filtered versions of row y of the (H, W, 3) codes `c`, as (5, 3 W) uint8."""
    W = c.shape[1]
    x = c[y].reshape(-1).astype(np.int32)
    up = c[y - 1].reshape(-1).astype(np.int32) if y > 0 else np.zeros(3 * W, np.int32)
    a, cc = np.zeros_like(x), np.zeros_like(x)
    a[3:], cc[3:] = x[:-3], up[:-3]
    p = a + up - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, cc))
    return (np.stack([x, x - a, x - up, x - ((a + up) >> 1), x - paeth]) & 255).astype(np.uint8)


def row_costs(f):
    v = f.astype(np.int64)
    return np.minimum(v, 256 - v).sum(axis=1)


def band_string(c, y0, rows):
    out = bytearray()
    for y in range(y0, y0 + rows):
        f = filtered_rows(c, y)
        t = int(np.argmin(row_costs(f)))  # (argmin: the first of equals, the smallest type)
        out.append(t)
        out += f[t].tobytes()
    return bytes(out)


# -------------------------------------------------------------------------------------------------------------- tokens
def tokens(s):
    out = []
    for s0 in range(0, len(s), SEG):
        seg, i = s[s0:s0 + SEG], 0
        while i < len(seg):
            L = 0
            if i > 0:
                while i + L < len(seg) and seg[i + L] == seg[i - 1]:
                    L += 1
            if L >= 3:
                out.append(("match", L))
                i += L
            else:
                out.append(("lit", seg[i]))
                i += 1
    return out


def length_symbol(L):
    """(symbol, extra bits, extra value) of a match length 3 .. 63 (RFC 1951, 3.2.5)."""
    assert 3 <= L <= 63
    if L <= 10:
        return 254 + L, 0, 0
    e = 1 if L <= 18 else 2 if L <= 34 else 3
    base = {1: 11, 2: 19, 3: 35}[e]
    return 261 + 4 * e + ((L - base) >> e), e, (L - base) & ((1 << e) - 1)


# ------------------------------------------------------------------------------------------------------------- presets
def preset_fields(words, k):
    """(lengths[286], codes[286] as stored (bit-reversed), header bit count, header bits as an int)."""
    p = [int(v) for v in np.asarray(words, np.uint32).reshape(-1, PRESET_WORDS)[k]]
    hbits = p[NSYM]
    header = sum(w << (32 * j) for j, w in enumerate(p[NSYM + 1:NSYM + 1 + HEADER_WORDS]))
    return [w >> 16 for w in p[:NSYM]], [w & 0xFFFF for w in p[:NSYM]], hbits, header & ((1 << hbits) - 1)


class BitWriter:
    """Bits from bit 0 of byte 0 up; .n counts them, .bytes() pads the last byte with zeros."""

    def __init__(self):
        self.out, self.acc, self.fill, self.n = bytearray(), 0, 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits)
        self.acc |= value << self.fill
        self.fill += bits
        self.n += bits
        if self.fill >= 8:
            whole = self.fill // 8
            self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.fill -= 8 * whole

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.fill else b"")


def token_bits(toks, lens):
    """The bits of the tokens under a preset's lengths: every literal its code, every match its length's code, the extra
    bits and the one-bit distance code."""
    return sum(lens[t[1]] if t[0] == "lit" else lens[length_symbol(t[1])[0]] + length_symbol(t[1])[1] + 1 for t in toks)


def dynamic_size(toks, words, k):
    """The bytes preset k takes, from the header's formula."""
    lens, _, hbits, _ = preset_fields(words, k)
    D = 3 + hbits + token_bits(toks, lens) + lens[256]
    return D // 8 if D % 8 == 0 else -(-(D + 3) // 8) + 4


def dynamic_block(toks, words, k):
    """The band's data with preset k: the dynamic block, and the empty stored block where it does not end on a byte."""
    lens, cds, hbits, header = preset_fields(words, k)
    w = BitWriter()
    w.put(0, 1)  # BFINAL
    w.put(2, 2)  # BTYPE = 10: the bits 0, 1
    w.put(header, hbits)
    for t in toks:
        if t[0] == "lit":
            w.put(cds[t[1]], lens[t[1]])
        else:
            sym, eb, ev = length_symbol(t[1])
            w.put(cds[sym], lens[sym])
            w.put(ev, eb)
            w.put(0, 1)  # the one distance code: distance 1
    w.put(cds[256], lens[256])
    if w.n % 8:
        w.put(0, 3)
        return w.bytes() + b"\x00\x00\xff\xff"
    return w.bytes()


def stored_block(s):
    return b"\x00" + struct.pack("<HH", len(s), 65535 - len(s)) + s


def band_data(s, words, force=None):
    K = np.asarray(words).size // PRESET_WORDS
    toks = tokens(s)
    if force == "stored":
        return stored_block(s), "stored"
    if force is not None:
        out = dynamic_block(toks, words, force)
        assert len(out) == dynamic_size(toks, words, force)
        return out, force
    best, which = 5 + len(s), "stored"
    for k in range(K):
        size = dynamic_size(toks, words, k)
        if size < best:
            best, which = size, k
    out = stored_block(s) if which == "stored" else dynamic_block(toks, words, which)
    assert len(out) == best
    return out, which


# ---------------------------------------------------------------------------------------------------------------- file
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def bands(c, R, words, force=None):
    """[(string, data, choice)] of every band of the (H, W, 3) codes."""
    H, W = c.shape[:2]
    assert 1 <= W <= MAX_W and R >= 1 and R * (3 * W + 1) <= BAND_MAX
    out = []
    for y0 in range(0, H, R):
        s = band_string(c, y0, min(R, H - y0))
        out.append((s,) + band_data(s, words, force))
    return out


def encode(c, R, words, force=None):
    H, W = c.shape[:2]
    bs = bands(c, R, words, force)
    adler = zlib.adler32(b"".join(s for s, _, _ in bs)) & 0xFFFFFFFF
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")
    assert len(out) == PREFIX
    for _, d, _ in bs:
        out += chunk(b"IDAT", d)
    tail = chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler)) + chunk(b"IEND", b"")
    assert len(tail) == TRAILER
    return out + tail


def chunks(data):
    """[(type, data)] of a PNG file, its signature, lengths and CRCs checked, nothing left over."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(body) == n and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, at
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


# ------------------------------------------------------------------------------------------------------------ pictures
def contents(H, W, seed=0):
    """{name: (3, H, W) float32 picture}: a smooth scene with a flat box under noise of sigma 0, 1.5 and 80 codes (the
    last leaves [0, 1] on both sides), a flat picture, the two checkerboards of 0 and 255, and a ramp through every code."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = xx % 256, yy % 256  # (a wide picture repeats the slope instead of leaving the range)
    scene = np.stack([90 + xs / 4 + ys / 8, 60 + xs / 8 + ys / 4, 200 - xs / 8 - ys / 8])
    scene[:, H // 4:H // 4 + max(1, H // 2), W // 4:W // 4 + max(1, W // 2)] = 77
    out = {f"noise{s}": (scene + s * g.standard_normal(scene.shape)) / 255 for s in (0, 1.5, 80)}
    out["flat"] = np.full((3, H, W), 77 / 255)
    board = ((xx + yy) % 2)[None].repeat(3, axis=0)
    out["checker0"], out["checker255"] = board, 1 - board
    out["ramp"] = np.stack([(xx + W * yy + 85 * c) % 256 for c in range(3)]) / 255
    return {k: v.astype(np.float32) for k, v in out.items()}
