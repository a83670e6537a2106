/* wg_adam_rows.h -- C-ABI of the fused Adam step over a LIST of rows: the optimizer step for the Gaussians a frame reached.
 *
 * The tensors are [P, width] float32 arrays of one Gaussian per row (xyz 3, features_dc 3, opacities 1, scales 3, rotations 4, embeddings 24,
 * features_rest 45 floats in the reference's model); the list names the rows to update (what wg_appearance_rows_compact builds from the
 * rasterizer's `radii`).  For every listed row r and every j < width, param, exp_avg and exp_avg_sq at r * width + j receive exactly
 * wg_adam.h's update with the descriptor's per-step scalars -- the same float32 operations in the same order, compiled without contraction,
 * so a listed row has the bits wg_fused_adam gives on gathered copies x[rows].  No element of an unlisted row is written and the gradient of
 * an unlisted row is never read: its parameter and both moments keep their bits (dense Adam would decay the moments and keep moving the
 * parameter along them although the gradient is exactly zero).  This is the update rule of 3D-GS's `sparse_adam` and gsplat's `SelectiveAdam`;
 * like theirs, the bias correction follows the caller's global step count, not a per-row count.
 *
 * The list follows wg_appearance_rows.h: `rows` int32 on the device, `M` entries.  With `rows_count` NULL, M is the exact entry count.  With
 * `rows_count` (one int32 on the device) M is the CAPACITY: the grid is sized by M on the host and the kernel reads the real count, clamped to
 * [0, M], on the device; workgroups beyond it leave at once.  An entry outside [0, P) is never dereferenced and updates nothing.  Duplicate
 * entries are the caller's error (two lanes would update one row from the same old state, or from each other's, in no defined order); the
 * compaction never produces any.
 *
 * Host contract: device pointers, explicit HIP stream, no allocation, no host synchronisation, nothing that prevents stream capture.  Up to
 * WG_ADAM_MAX_TENSORS tensors go into one launch, more into several.  Element offsets are size_t: P * width may exceed 2^31.
 * WG_ERR_INVALID_ARGUMENT before any device work for: n_tensors < 0 or a null `tensors` with n_tensors > 0; P < 0 or P > 2^31 - 1; M < 0 or
 * M > 2^31 - 1; a null `rows` with M > 0; width < 1; numel != P * width; a null pointer with numel > 0; the two conditions wg_fused_adam
 * refuses (bias_correction2_sqrt <= 0, one_minus_beta1 >= 0.5); a list so long that M * width needs more than 2^31 - 1 workgroups.
 * M == 0 or n_tensors == 0 (after these checks): WG_OK with no launch.  Returns 0 or a negative wg_status (wg_rasterizer.h).
 */
#ifndef WG_ADAM_ROWS_H
#define WG_ADAM_ROWS_H
#include <stddef.h>
#include <stdint.h>
#include "wg_adam.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct wg_adam_rows_tensor {
    wg_adam_tensor t;      /* as wg_adam.h; t.numel == P * width */
    int64_t width;         /* floats per row, >= 1; the row is contiguous */
} wg_adam_rows_tensor;

int wg_adam_rows_step(int n_tensors, const wg_adam_rows_tensor* tensors /* host array */, int64_t P,
                      const int32_t* rows, int64_t M, const int32_t* rows_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
