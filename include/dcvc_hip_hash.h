/* dcvc_hip_hash.h -- decoded-picture hashes: the CRC-32 of a picture the codec holds on the device, taken there.
 *
 * Conventions of dcvc_hip_scene.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument.  Planes are fp32 with explicit strides in elements:
 *   element (c, y, x) = src[c * plane_stride + y * row_stride + x],  row_stride >= W,
 *   plane_stride >= (H - 1) * row_stride + W,
 * so the unpadded crop of a padded picture is read in place.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.
 *
 * The digest is the CRC-32 of zlib / PNG / gzip: reflected polynomial P = 0xEDB88320, initial value and final xor
 * 0xFFFFFFFF.  It is taken over a BYTE STRING M that each entry point defines, so zlib's crc32() of the same bytes is the
 * oracle.  Each entry point WRITES (does not add) one uint32_t to device memory; the value is a pure function of the
 * bytes: no floating-point sum, no atomic, nothing that depends on order or on what runs beside the kernels.
 *
 * dcvc_hash_pixels
 *   M = the 3 * H * W 8-bit codes  code(v) = (int) rint(255.0f * clamp01(v)),  clamp01(v) = min(max(v, 0), 1)  -- the
 *   function of dcvc_hip_roi.h: one correctly rounded fp32 multiply, rint is round-half-to-even -- of planar R, G, B,
 *   INTERLEAVED R, G, B per pixel, row-major: byte 3 * (y * W + x) + c is code(rgb[c, y, x]).  These are the bytes of the
 *   8-bit RGB PNG of the picture.  Samples inside the crop are finite; a NaN there is undefined.
 *
 * dcvc_hash_f32
 *   M = the little-endian bit patterns of the C * H * W fp32 elements in the order c, y, x: 4 bytes per element, byte
 *   4 * ((c * H + y) * W + x) + k is bits k * 8 .. k * 8 + 7 of element (c, y, x).  Every bit counts: -0.0 is not +0.0, and
 *   a NaN is its payload.
 *
 * HOW IT IS COMPUTED (the result does not depend on it; the two constants below let a test aim at the seams).
 *   crc0(A) is the CRC register after the bytes A, started from 0, without the final xor: A(x) * x^32 mod P.  Then
 *     crc0(A || B) = crc0(A) * x^(8 |B|) mod P  xor  crc0(B)           ("times x^(8 n) mod P": n zero bytes more)
 *     crc32(M)     = crc0(M)  xor  0xFFFFFFFF * x^(8 |M|) mod P  xor  0xFFFFFFFF
 *   and crc0(0...0 || A) = crc0(A): zero bytes in FRONT change nothing.  M is therefore extended in front, virtually,
 *   by zero bytes to a whole number of DCVC_HASH_BLOCK_BYTES; the extended string is cut into chunks of
 *   DCVC_HASH_CHUNK_BYTES (a multiple of 12: a chunk starts on a pixel and on a word), one per lane, each lane runs a
 *   table-driven CRC from 0 over its chunk, the lanes of a workgroup (256 chunks = one block) are combined with the
 *   first identity, and the workgroup's partial goes to scratch[workgroup].  A second small launch folds the partials
 *   with the same identity and applies the second one.  The kernel boundary is the only synchronisation between
 *   workgroups.
 *
 * scratch: DCVC_HASH_SCRATCH_BYTES of device memory, 4-byte aligned, that the two launches of ONE call own until they
 *   have run: calls on one stream may share it, calls on different streams may not.
 */
#ifndef DCVC_HIP_HASH_H
#define DCVC_HIP_HASH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_HASH_MAX_SIDE 32768
#define DCVC_HASH_CHUNK_BYTES 192                           /* per lane */
#define DCVC_HASH_BLOCK_BYTES (256 * DCVC_HASH_CHUNK_BYTES) /* per workgroup: 49152 */
/* one partial per block of the longest string (2^32 - 1 bytes) */
#define DCVC_HASH_SCRATCH_BYTES (4 * (0xFFFFFFFFu / DCVC_HASH_BLOCK_BYTES + 1))

/* the three constants above as data symbols of the library (for callers that cannot read a header) */
extern const int32_t dcvc_hash_chunk_bytes, dcvc_hash_block_bytes, dcvc_hash_scratch_bytes;

/* Refused with DCVC_E_ARG, before anything else: a NULL rgb, out or scratch; H or W not in 1 .. DCVC_HASH_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; a pointer that is not 4-byte aligned; 3 * H * W >= 2^32 (which
 * no picture within DCVC_HASH_MAX_SIDE reaches: the longest string here is 3 * 2^30 bytes). */
int dcvc_hash_pixels(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, uint32_t *out,
                     uint32_t *scratch, void *stream);

/* Refused with DCVC_E_ARG, before anything else: a NULL src, out or scratch; C, H or W not in 1 .. DCVC_HASH_MAX_SIDE;
 * row_stride < W; plane_stride < (H - 1) * row_stride + W; a pointer that is not 4-byte aligned; 4 * C * H * W >= 2^32. */
int dcvc_hash_f32(const float *src, int32_t row_stride, int64_t plane_stride, int32_t C, int32_t H, int32_t W, uint32_t *out,
                  uint32_t *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
