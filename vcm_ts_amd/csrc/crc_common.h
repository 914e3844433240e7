// crc_common.h -- the CRC-32 algebra that hash.hip and png.hip share (include/dcvc_hip_hash.h states it): polynomials are
// reflected, bit 31 - k of a word is the coefficient of x^k.
// Internal, like kernel_common.h: every unit is compiled on its own, hence the unnamed namespace.
#ifndef DCVC_CRC_COMMON_H
#define DCVC_CRC_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t POLY = 0xEDB88320u, ONE = 0x80000000u;  // ONE: x^0

// a(x) * b(x) mod P on reflected polynomials, branch-free
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        p ^= b & (0u - ((a >> (31 - k)) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 n) mod P
__host__ __device__ constexpr uint32_t x8n(uint64_t n) {
    uint32_t out = ONE, sq = ONE >> 8;
    for (; n; n >>= 1) {
        if (n & 1) out = mulmod(out, sq);
        sq = mulmod(sq, sq);
    }
    return out;
}

}  // namespace

#endif
