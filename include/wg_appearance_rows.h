/* wg_appearance_rows.h -- C-ABI of the appearance MLP over a LIST of rows (the Gaussians that reach the image), forward and backward, and
 * of the device-side compaction that builds such a list from the rasterizer's `radii` without a host synchronisation.
 *
 * The arithmetic is wg_appearance_mlp.h's, unchanged: float32 v_mfma_f32_32x32x2_f32 chains, hidden width 128, 6 outputs, segments read in
 * place through (pointer, width, row stride), the shared segment folded into the first-layer bias, h1 and h2 recomputed backward, weight
 * gradients in registers with one partial per workgroup and a fixed-order finishing launch, no floating-point atomics.
 *
 * THE CONTRACT: entry i of the list takes the place that row i has in the dense walk.  The 64-entry tiles, their assignment to workgroups,
 * the accumulation order and the number of partials the finishing pass adds -- min(ceil(count / 64), workgroups), in workgroup order -- are
 * those of wg_appearance_mlp_* run on P = count rows.  So every result has the bits of the dense operator run on gathered copies of the
 * inputs (x[rows], dL_dout[rows]) with the same max_workgroups.
 *
 * The list: `rows` int32 (never NULL), `M` entries.  With `rows_count` NULL, M is the exact entry count.  With `rows_count` (one int32 on
 * the device, e.g. what wg_appearance_rows_compact wrote) M is the CAPACITY: the grid and the scratch are sized by M on the host, and the
 * kernels read the real count, clamped to [0, M], on the device; workgroups that then have no tile leave at once and are not summed.
 *     forward   writes out[row, 0..5] for listed rows only; no other element of `out` is touched
 *     backward  reads dL_dout[row] and writes grad_segment[i][row] for listed rows only; grad_shared and the six weight gradients are fully
 *               overwritten (zeros for an empty list)
 * An entry outside [0, mlp.P) is never dereferenced and writes nothing: it keeps its slot in its tile and contributes exact zeros (a zero
 * input row under a zero cotangent), which is wg_appearance_colour.h's rule.  Duplicate entries are processed as given (their writes land on
 * the same row); the compaction never produces any.
 *
 * Host contract as wg_appearance_mlp.h: device pointers, explicit HIP stream, no host synchronisation, no allocation, nothing that prevents
 * stream capture.  A malformed call -- everything wg_appearance_mlp.h refuses, a null `rows`, M < 0, M > 2^31 - 1, scratch smaller than
 * wg_appearance_rows_scratch_floats(M, max_workgroups), a struct_size that does not cover the fields -- is refused with
 * WG_ERR_INVALID_ARGUMENT before any device work.
 */
#ifndef WG_APPEARANCE_ROWS_H
#define WG_APPEARANCE_ROWS_H
#include <stddef.h>
#include <stdint.h>
#include "wg_appearance_mlp.h"
#ifdef __cplusplus
extern "C" {
#endif

#define WG_ROWS_COMPACT_BLOCK 2048   /* entries one workgroup of the compaction counts and scatters */

typedef struct wg_appearance_rows_args {
    size_t struct_size;            /* the caller's sizeof(wg_appearance_rows_args) */
    wg_appearance_mlp_args mlp;    /* as for the dense operator; mlp.P is the row count of the tensors, `out`, `dL_dout` and `grad_segment` are
                                      [P, .]; mlp.scratch holds wg_appearance_rows_scratch_floats(M, mlp.max_workgroups) floats */
    const int32_t* rows;           /* [M] on the device */
    int64_t M;                     /* entries of `rows`: the exact count, or the capacity when rows_count is given */
    const int32_t* rows_count;     /* NULL, or one int32 on the device: the real count */
} wg_appearance_rows_args;

/* = wg_appearance_mlp_scratch_floats with the list's capacity in the place of P. */
int64_t wg_appearance_rows_scratch_floats(int64_t capacity, int32_t max_workgroups);
int wg_appearance_rows_forward(const wg_appearance_rows_args* args);
int wg_appearance_rows_backward(const wg_appearance_rows_args* args);

/* The ordered list of the rows that reach the image.  Exactly one of `radii` (int32 [P]: listed iff radii > 0) and `mask` (uint8 [P]: listed
 * iff non-zero) is given.  rows[0 .. count) receives the listed indices in ascending order, `count` (one int32 on the device) their number;
 * rows[count .. P) is not touched.  Three launches -- a count per block of WG_ROWS_COMPACT_BLOCK entries (wave ballot / popcount), an
 * exclusive scan of the block counts by one workgroup, the scatter -- with no waiting between workgroups: ordered and deterministic.  No
 * host read, no allocation, capturable.  P = 0: WG_OK with count = 0.  P < 0, P > 2^31 - 1, both or neither input, a null `rows` (P > 0),
 * `count` or `scratch`, or scratch_bytes < wg_appearance_rows_compact_scratch_bytes(P): WG_ERR_INVALID_ARGUMENT before any device work. */
int64_t wg_appearance_rows_compact_scratch_bytes(int64_t P);   /* = 4 * max(1, ceil(P / WG_ROWS_COMPACT_BLOCK)); negative status for bad P */
int wg_appearance_rows_compact(int64_t P, const int32_t* radii, const uint8_t* mask, int32_t* rows, int32_t* count, void* scratch,
                               int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
