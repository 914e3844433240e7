/* dcvc_hip_png.h -- a picture the codec holds on the device, written there as a finished 8-bit RGB .png file: PNG's row
 * filters, a deflate coder with preset Huffman tables, CRC-32 and Adler-32.  The host copies `size` bytes and writes them.
 *
 * Conventions of dcvc_hip_hash.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument; planar fp32 with explicit strides in elements,
 *   element (c, y, x) = rgb[c * plane_stride + y * row_stride + x],
 * so the unpadded crop of a padded picture is read in place.  Samples inside the crop are finite.
 *
 * ARITHMETIC AND FORMAT ARE PART OF THE INTERFACE.  After code() everything is integer, and the file is a pure function
 * of (the H x W codes, R, the K presets): tests/pngdev_ref.py restates it and is held against the kernels byte for byte.
 *
 * THE FILE
 *   signature (8 bytes: 89 50 4E 47 0D 0A 1A 0A)
 *   chunk IHDR: W, H big-endian, bit depth 8, colour type 2, compression 0, filter 0, interlace 0
 *   chunk IDAT: 78 01                                         (the zlib header)
 *   chunk IDAT, one per BAND b = 0 .. bands - 1: the band's deflate blocks (below)
 *   chunk IDAT: 01 00 00 FF FF || Adler-32, big-endian        (an empty final stored block, the zlib trailer)
 *   chunk IEND
 * A chunk is: length of its data (4 bytes, big-endian) || type || data || CRC-32 of type || data (big-endian).  The first
 * three items take DCVC_PNG_PREFIX_BYTES = 47 bytes, the last two DCVC_PNG_TRAILER_BYTES = 33, a band's chunk 12 more than its
 * data.
 *
 * BANDS.  A band is R consecutive rows, bands = ceil(H / R), the last band may be shorter.  Bands are independent, except
 * that the first row of band b > 0 is filtered against the SOURCE row above it (codes of the picture, never another
 * band's output).
 *
 * THE BAND'S STRING.  With bpp = 3 and x the row's 3 W codes code(v) = (int) rint(255.0f * min(max(v, 0), 1)) (the function
 * of dcvc_hip_roi.h), interleaved R, G, B per pixel; a = the byte 3 to the left (0 for the first pixel), b = the byte
 * above (0 in the picture's first row), c = the byte above a (0 where either is), all arithmetic mod 256:
 *   type 0  x        type 1  x - a        type 2  x - b        type 3  x - ((a + b) >> 1)  (a + b not reduced)
 *   type 4  x - paeth(a, b, c):  p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|;
 *           a if pa <= pb and pa <= pc, else b if pb <= pc, else c
 * A row takes the type with the smallest  sum over its 3 W filtered bytes v of min(v, 256 - v),  among equals the
 * smallest type.  The band's string is, row after row, the type byte followed by the row's 3 W filtered bytes:
 * n = rows * (3 W + 1) <= DCVC_PNG_BAND_MAX bytes.
 *
 * TOKENS.  The string is cut into segments of DCVC_PNG_SEG = 64 bytes (the last may be shorter); no token crosses a
 * segment.  Inside a segment, from left to right, at a position i that is not the segment's first byte: if the next
 * L >= 3 bytes (L the largest such count inside the segment, so L <= 63) all equal byte i - 1, a match of length L and
 * distance 1 is emitted and i += L; otherwise, and at the segment's first byte, the literal of byte i.  (Equivalently:
 * with e[i] = "byte i equals byte i - 1" and e = 0 at a segment's first byte, every maximal run of e of length >= 3 is
 * one match, every other byte a literal.)  No other match is made.
 *
 * A PRESET is DCVC_PNG_PRESET_WORDS uint32 words:
 *   words 0 .. 285        symbol s of deflate's literal/length alphabet: (length << 16) | code, length in 1 .. 15, the
 *                         286 lengths a COMPLETE prefix code (sum of 2^-length = 1), code = the symbol's canonical
 *                         deflate code (RFC 1951, 3.2.2) with its `length` bits REVERSED, i.e. ready to be written from
 *                         bit 0 up
 *   word 286              hbits: the number of bits of the block header, <= 32 * DCVC_PNG_HEADER_WORDS
 *   words 287 .. 358      the header's bits, bit j in bit j % 32 of word 287 + j / 32, zero beyond hbits: HLIT = 29,
 *                         HDIST = 0, HCLEN, the HCLEN + 4 code-length-code lengths, then the 286 lengths above followed by
 *                         ONE distance code of length 1, coded with the code-length code (symbols 0 .. 18, a complete code)
 *   word 359              0
 * Every match is therefore: the length symbol's code, its extra bits, and the distance code `0` (1 bit, distance 1).
 *
 * A BAND'S DATA is the cheapest of K + 1 codings:
 *   preset k:  bits BFINAL = 0, BTYPE = 10 (the three bits 0, 0, 1 in stream order), the preset's header, the tokens, the code
 *              of symbol 256.  With D bits in all, the data is D / 8 bytes when 8 | D; otherwise an EMPTY STORED block is
 *              appended -- the bits 0, 0, 0, zero bits up to the next byte, then 00 00 FF FF -- ceil((D + 3) / 8) + 4 bytes.
 *   stored:    00 || n (2 bytes, little-endian) || 65535 - n (likewise) || the string: 5 + n bytes.
 * The fewest bytes win; among equals stored, then the smallest k.  Hence the bound
 *   size <= dcvc_png_bound(H, W, R) = 80 + H * (3 W + 1) + 17 * bands.
 *
 * ADLER-32 (s1 = 1 + sum of bytes, s2 = sum of the s1 after every byte, both mod 65521, value s2 << 16 | s1) is taken over
 * all bands' strings in order; zlib's adler32() of the same bytes is the oracle, its crc32() that of every chunk.
 *
 * HOW IT IS COMPUTED.  Two launches, nothing synchronised, no global atomics.
 *   Launch A, one workgroup per band: codes to LDS, row filters chosen by reductions (one wave per row), the string to
 *   LDS, a histogram of the tokens' symbols, the K prices, the winning coding written bit by bit into an LDS image of the
 *   chunk at offsets from a scan, the chunk's CRC-32, and the band's Adler partial.  It writes the band's SLOT of `staging`,
 *   DCVC_PNG_SLOT_BYTES = DCVC_PNG_BAND_MAX + 32 bytes:
 *     words 0 .. 3   { bytes of the band's data, A = sum of the string's bytes mod 65521,
 *                      B = sum over i of (n - i) * byte i mod 65521, n }
 *     from byte 16   the chunk from its type on: "IDAT" || data || CRC-32
 *   Launch B, one workgroup per band and one more: each scans the sizes in front of its band and copies the slot's chunk
 *   to its place behind the prefix; the last writes prefix and trailer (s1 = 1 + sum of A, s2 = N + sum of B_b + A_b * (the
 *   bytes of the strings after band b), N the length of all strings) and the size word.
 *
 * Every byte of file[0, size) is written, nothing at or beyond capacity, and of staging nothing outside the
 * bands * DCVC_PNG_SLOT_BYTES bytes of the slots (a slot's bytes behind its chunk are undefined).  The picture is not written.
 * staging, file and size_word belong to the two launches of ONE call until they have run: calls on one stream may share
 * them, calls on different streams may not.
 */
#ifndef DCVC_HIP_PNG_H
#define DCVC_HIP_PNG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_PNG_BAND_MAX 24576 /* bytes of a band's string */
#define DCVC_PNG_SEG 64
#define DCVC_PNG_MAX_W 8191
#define DCVC_PNG_MAX_H 32768 /* DCVC_HASH_MAX_SIDE */
#define DCVC_PNG_MAX_PRESETS 32
#define DCVC_PNG_SYMBOLS 286
#define DCVC_PNG_HEADER_WORDS 72
#define DCVC_PNG_PRESET_WORDS 360
#define DCVC_PNG_SLOT_BYTES (DCVC_PNG_BAND_MAX + 32)
#define DCVC_PNG_PREFIX_BYTES 47
#define DCVC_PNG_TRAILER_BYTES 33

/* 80 + H * (3 W + 1) + 17 * ceil(H / R), or -1 for sizes that dcvc_png_encode refuses.  HOST only. */
int64_t dcvc_png_bound(int32_t H, int32_t W, int32_t R);

/* HOST only: DCVC_OK when tables_host holds K presets as laid out above, else DCVC_E_ARG: a NULL or misaligned (4 bytes)
 * pointer, K outside 1 .. DCVC_PNG_MAX_PRESETS, a length outside 1 .. 15, lengths that are not a complete code, a code that is
 * not the canonical one bit-reversed, bits set above a word's fields, hbits beyond the room, header bits that do not
 * decode (a code-length code that is not complete, a repeat without a predecessor or past the end) to exactly HLIT = 29,
 * HDIST = 0, those 286 lengths and one distance length 1 in exactly hbits bits, a bit set beyond hbits, a nonzero last word.
 * Reads K * DCVC_PNG_PRESET_WORDS words and nothing else. */
int dcvc_png_tables_check(const uint32_t *tables_host, int32_t K);

/* The file of the H x W picture into file[0, *size_word): two launches on `stream`.  tables_host and tables_dev hold the
 * same K presets, in host and in device memory (the host's are checked here, the device's are read by the kernels).
 * staging: ceil(H / R) * DCVC_PNG_SLOT_BYTES bytes.  size_word: one uint32_t, written.
 * Refused with DCVC_E_ARG, before anything else: a NULL rgb, tables_host, tables_dev, staging, file or size_word; one of them
 * not 4-byte aligned; H not in 1 .. DCVC_PNG_MAX_H or W not in 1 .. DCVC_PNG_MAX_W; row_stride < W; plane_stride <
 * (H - 1) * row_stride + W; R < 1 or R * (3 W + 1) > DCVC_PNG_BAND_MAX; K outside 1 .. DCVC_PNG_MAX_PRESETS; tables that fail
 * dcvc_png_tables_check; capacity < dcvc_png_bound(H, W, R). */
int dcvc_png_encode(const float *rgb, int32_t row_stride, int64_t plane_stride, int32_t H, int32_t W, int32_t R,
                    const uint32_t *tables_host, const uint32_t *tables_dev, int32_t K, uint8_t *staging, uint8_t *file,
                    int64_t capacity, uint32_t *size_word, void *stream);

#ifdef __cplusplus
}
#endif
#endif
