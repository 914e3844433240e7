/* dcvc_hip_bits.h -- where inside a picture the bits went: the code length of every coded symbol, summed per cell of the
 * latent grid, and those maps summed over labelled regions.  The inputs are the coder's own integers (symbol planes,
 * CDF-index planes, CDF tables), so the maps are not an estimate: their sum agrees with the length of the byte string the
 * host coder writes inside a bound that follows from the rANS update rule.
 *
 * Conventions of dcvc_hip_roi.h: raw device pointers, a hipStream_t passed as void*, 0 or a negative DCVC_E_* code,
 * nothing launched (and nothing dereferenced) on a bad argument, nothing synchronised.
 *
 * ARITHMETIC IS PART OF THE INTERFACE.  Everything is an integer; the unit of a cost is 2^-16 bit (DCVC_BITS_UNIT).
 *
 * LUT:  LUT[f] = rint((16 - log2(f)) * 65536) for a frequency f in 1 .. 65536, computed by the HOST in float64.  The
 *   device never evaluates a logarithm.  A frequency of 0 or above 65536 cannot come from a valid table; the host refuses
 *   such a table when it builds the cost array.
 *
 * Cost array:  for a CDF table of n_rows rows and `stride` columns (row r: sizes[r] entries, offsets[r]) the host builds
 *   cost[r][s], int32, same rows and stride:  with sentinel = sizes[r] - 2,
 *     cost[r][s] = LUT[cdf[r][s + 1] - cdf[r][s]]  for 0 <= s <= sentinel,  0 elsewhere.
 *
 * Cost of one symbol `sym` coded with row r:  v = sym - offsets[r];
 *     0 <= v < sentinel:  cost[r][v];
 *     otherwise an escape, as the coder writes it (the sentinel, one nibble holding the count, the nibbles of the value):
 *       raw = (uint32) (-2 v - 1) for v < 0, (uint32) (2 (v - sentinel)) otherwise;  nib = the number of 4-bit nibbles of
 *       raw, 0 .. 8;  cost[r][sentinel] + 4 * 65536 * (1 + nib).
 *   A row outside [0, n_rows), or a row whose size is outside [2, stride], is never used as an address: the symbol costs 0
 *   and DCVC_BITS_BAD_INDEX is ORed into *status.
 *
 * Maps:  a scale-coded latent (y, mv_y) of C channels has two pairs of planes (step 0, step 1), each (N, C/2, H, W) with
 *   entry ((n * C/2 + k) * H + y) * W + x as dcvc_dual_prior_enc writes them; every entry of both is a coded symbol at
 *   latent position (y, x), its row is the index plane's entry.  map[n][y][x], int32, (N, H, W), is the sum of the costs
 *   over k and both steps.  A factorised latent (z, mv_z) has one plane (N, C, H, W) whose row is the channel; its map is
 *   the sum over the channels.  C <= DCVC_BITS_MAX_C: 512 symbols of at most 52 bits stay below 2^31 units.  Integer sums
 *   have no order: the result is defined bit for bit.
 *
 * Region sums:  the four maps of a picture in the order mv_z, mv_y, z, y (component 0 .. 3; an absent one is NULL) and a
 *   label map (N, hc, wc) of uint8 labels 0 .. K - 1 on the 16-pixel cell grid of dcvc_hip_roi.h, hc and wc multiples of 4
 *   (the grid of a padded picture).  mv_y and y maps are (N, hc, wc); mv_z and z maps are (N, hc / 4, wc / 4).
 *     sums[n][label][component], int64, in units of 2^-20 bit:  a cell adds 16 * map[n][i][j] of the y-type maps and
 *     map[n][i / 4][j / 4] of the z-type maps to its label, so that a z-type element is split evenly and exactly over the
 *     4 x 4 cells it covers.  A label map of zeros gives the picture's totals (times 16).
 *   A label >= K adds nothing and ORs DCVC_BITS_BAD_LABEL into *status.
 *
 * Ladder sweep:  what the two-step scale-coded latent of one picture would cost by the coder's tables if
 *   its quantisation step were f times as large and the prior rescaled with it, for K factors f_0 .. f_{K-1} at once.
 *   y_res and scales_hat are the dense NHWC planes (N, H, W, C), fp32, that dcvc_dual_prior_enc writes (the residual
 *   before rounding, the predicted scale); after both steps every element has been written once.  Per element and k:
 *     s   = (int32) rintf(res / f_k)                         (round half to even)
 *     row = the number of idx_edges[0 .. 254] <= sc / f_k     (the function the dual-prior kernel uses; 256 edges)
 *     the cost of (row, s) by the rule above;  est[n][k], int64 in 2^-16 bit, is the sum over sample n.
 *   f_k is whatever float the HOST passes; callers form it as float32(h_k) / float32(100) from integer hundredths h_k,
 *   the device never forms a factor.  The two divisions are IEEE correctly rounded fp32 divisions: the library is built
 *   without fast-math and with the compiler's default of correctly rounded division, and it has to stay so -- a
 *   reciprocal-multiply would move symbols across .5 and scales across an edge.  Everything after the two divisions is
 *   an integer, so est is defined bit for bit.  With f_k = 1 the candidate is the coded symbol and the coded row:
 *   est[n][k] equals the sum of dcvc_bits_map_scale's map of sample n.
 *   A res or sc that is not finite, or a quotient res / f_k at or beyond +-2^31 for any k, makes the element cost 0 for
 *   EVERY k and ORs DCVC_BITS_BAD_VALUE into *status.  Rows as above (DCVC_BITS_BAD_INDEX).
 */
#ifndef DCVC_HIP_BITS_H
#define DCVC_HIP_BITS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_BITS_UNIT 65536        /* cost units per bit */
#define DCVC_BITS_MAX_C 512
#define DCVC_BITS_MAX_SIDE 2048     /* latent rows / columns (DCVC_ROI_MAX_SIDE / 16) */
#define DCVC_BITS_MAX_N 65535
#define DCVC_BITS_MAX_ROWS 65536
#define DCVC_BITS_MAX_LABELS 8
#define DCVC_BITS_BAD_INDEX 1       /* a CDF row out of range (or a row of impossible size) */
#define DCVC_BITS_BAD_LABEL 2       /* a label >= K */
#define DCVC_BITS_BAD_VALUE 4       /* sweep: a residual or scale that is not finite, or a symbol that is no int32 */
#define DCVC_BITS_MAX_LADDER 8      /* sweep: factors per call */

/* Writes exactly N * H * W int32 to `map`.  status: one device int32 the kernels OR DCVC_BITS_BAD_* into (never cleared
 * here).  Refused: a NULL pointer; N outside 1 .. DCVC_BITS_MAX_N; H or W outside 1 .. DCVC_BITS_MAX_SIDE; C odd, < 2 or
 * > DCVC_BITS_MAX_C; n_rows outside 1 .. DCVC_BITS_MAX_ROWS; stride < 2. */
int dcvc_bits_map_scale(const int32_t *sym0, const int32_t *idx0, const int32_t *sym1, const int32_t *idx1,
                        const int32_t *cost, int32_t n_rows, int32_t stride, const int32_t *sizes, const int32_t *offsets,
                        int32_t *map, int32_t N, int32_t C, int32_t H, int32_t W, int32_t *status, void *stream);

/* The same for one factorised plane: the row of channel c is c.  Also refused: C < 1, C > n_rows (C may be odd). */
int dcvc_bits_map_factorized(const int32_t *sym, const int32_t *cost, int32_t n_rows, int32_t stride, const int32_t *sizes,
                             const int32_t *offsets, int32_t *map, int32_t N, int32_t C, int32_t H, int32_t W,
                             int32_t *status, void *stream);

/* maps: HOST array of the four DEVICE maps (NULL entries are absent; at least one is present).  WRITES all N * K * 4
 * entries of `sums` (8-byte aligned device memory; an absent component's are 0): one workgroup per n, no global atomics.
 * Refused: NULL maps, labels, sums or status; all four maps absent; K outside 1 .. DCVC_BITS_MAX_LABELS; N outside
 * 1 .. DCVC_BITS_MAX_N; hc or wc outside 4 .. DCVC_BITS_MAX_SIDE or no multiple of 4. */
int dcvc_bits_regions(const int32_t *const *maps, const uint8_t *labels, int32_t K, int64_t *sums, int32_t N, int32_t hc,
                      int32_t wc, int32_t *status, void *stream);

/* The ladder sweep.  factors: HOST array of K floats (read before the launch, not kept).  WRITES all N * K entries of
 * `est` (8-byte aligned device memory) and nothing else: a memset and one launch on `stream`, one 64-bit integer atomic
 * add per workgroup and factor.  Refused: a NULL pointer; est not 8-byte aligned; K outside 1 .. DCVC_BITS_MAX_LADDER; a
 * factor that is not finite or outside [0.1, 10]; N, H, W, n_rows, stride as for dcvc_bits_map_scale; C odd, < 2 or
 * > DCVC_BITS_MAX_C. */
int dcvc_bits_sweep_scale(const float *y_res, const float *scales_hat, const float *idx_edges, const float *factors,
                          int32_t K, const int32_t *cost, int32_t n_rows, int32_t stride, const int32_t *sizes,
                          const int32_t *offsets, int64_t *est, int32_t N, int32_t C, int32_t H, int32_t W, int32_t *status,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif
