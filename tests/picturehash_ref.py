"""A restatement of include/dcvc_hip_hash.h written from its text (not from the kernel): the two byte strings built with
numpy and digested with zlib.crc32, and the header's combine algebra in pure Python -- chunks of a virtually
front-padded string, one crc0 each, folded by  crc0(A || B) = crc0(A) * x^(8 |B|) mod P  xor  crc0(B).

Everything is integer arithmetic after one float32 multiply per sample, so comparisons need no tolerance.
"""
import zlib

import numpy as np

from tests.roi_ref import code

POLY = 0xEDB88320
ONE = 0x80000000  # x^0 in the reflected representation: bit 31 - k is the coefficient of x^k


# --------------------------------------------------------------------------------------------------- the byte strings
def pixel_bytes(rgb):
    """rgb: (3, H, W) float32 -> the 3 H W codes, interleaved R, G, B per pixel, row-major"""
    return code(np.asarray(rgb, dtype=np.float32)).astype(np.uint8).transpose(1, 2, 0).tobytes()


def f32_bytes(t):
    """t: (C, H, W) float32 -> the little-endian bit patterns in the order c, y, x"""
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view("<u4").tobytes()


def crc32_pixels(rgb):
    return zlib.crc32(pixel_bytes(rgb)) & 0xFFFFFFFF


def crc32_f32(t):
    return zlib.crc32(f32_bytes(t)) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the combine algebra
def mulmod(a, b):
    """a(x) * b(x) mod P on reflected 32-bit polynomials"""
    p = 0
    for k in range(32):
        if a & (ONE >> k):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x8n(n):
    """x^(8 n) mod P by square and multiply"""
    out, sq = ONE, ONE >> 8
    while n:
        if n & 1:
            out = mulmod(out, sq)
        sq = mulmod(sq, sq)
        n >>= 1
    return out


def crc0(data):
    """the CRC register after `data`, started from 0, no final xor -- bit by bit"""
    reg = 0
    for byte in bytes(data):
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ (POLY if reg & 1 else 0)
    return reg


def finish(c0, n):
    """crc32(M) from crc0(M) and |M| = n: the init and xorout terms"""
    return c0 ^ mulmod(0xFFFFFFFF, x8n(n)) ^ 0xFFFFFFFF


def chunked_crc32(data, chunk, block):
    """The header's procedure on the host: zero bytes in front up to a whole number of `block` bytes, one crc0 per
    `chunk` bytes, chunks folded into block partials and the partials folded -- left to right, each step one use of the
    combine identity -- then `finish`."""
    data = bytes(data)
    assert block % chunk == 0
    ext = bytes((-len(data)) % block) + data
    if not ext:
        return finish(0, 0)
    xc, xb = x8n(chunk), x8n(block)
    total = 0
    for b0 in range(0, len(ext), block):
        part = 0
        for c0 in range(b0, b0 + block, chunk):
            piece = ext[c0:c0 + chunk]
            # (zlib's register started from 0 is crc0; the bit-by-bit crc0 above is held against it by the host test)
            part = mulmod(part, xc) ^ (zlib.crc32(piece, 0xFFFFFFFF) ^ 0xFFFFFFFF)
        total = mulmod(total, xb) ^ part
    return finish(total, len(data))


# ------------------------------------------------------------------------------------------------------- test inputs
def pixel_values(seed, H, W):
    """(3, H, W) float32 over [-0.5, 1.5] (both clamps act) with 0, 1, negatives, values above 1 and exact half-way codes
    (k + 0.5) / 255 planted at the front"""
    g = np.random.default_rng(seed)
    v = g.uniform(-0.5, 1.5, 3 * H * W).astype(np.float32)
    half = ((np.arange(0, 255, 7, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    special = np.concatenate([np.array([0.0, 1.0, -3.0, 2.5, -0.0, 0.5], np.float32), half])
    pos = g.permutation(v.size)[:special.size]
    v[pos] = special[:pos.size]
    return v.reshape(3, H, W)


def f32_values(seed, C, H, W):
    """(C, H, W) float32 bit patterns: random words (so NaNs with distinct payloads, denormals and infinities occur by
    construction below, not by luck) -- returned as float32, compared as bits"""
    g = np.random.default_rng(seed)
    bits = g.integers(0, 1 << 32, C * H * W, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001,
                        0xFFC12345, 0x7F800001], np.uint32)  # -0, +0, denormals, infinities, NaNs with payloads
    pos = g.permutation(bits.size)[:special.size]
    bits[pos] = special[:pos.size]
    return bits.view(np.float32).reshape(C, H, W)
