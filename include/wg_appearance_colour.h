/* wg_appearance_colour.h -- C-ABI of the fused toned-colour operator: from the image's appearance embedding to the [P, 3] precomputed
 * colours in one kernel, and from dL_dcolours to the embedding's gradient in one kernel plus a finishing launch, over a list of rows.
 *
 * Replaces, as an opt-in for callers that fit ONE appearance embedding against frozen geometry (WildGaussians.optimize_embedding,
 * wildgaussians/method.py:1755-1830), the chain of method.py:1555, :1557 and :1592-1598 around EmbeddingModel.forward (:890-900).  For
 * each listed row p, in float32:
 *
 *     fc[k,c]   = min(features[p, 3k+c], pre_clamp_max)                                        k = 0..15, c = 0..2
 *     x         = (fc[0,0..2], gembedding[p, 0..G-1], shared[0..E-1])
 *     om        = out_scale * (W3 . relu(W2 . relu(W1 . x + b1) + b2) + b3)                    offset = om[0..2], mul = om[3..5]
 *     t[k,c]    = min(fc[k,c] * mul[c] + (k == 0 ? offset[c] / C0 : 0), post_clamp_max)
 *     d         = (xyz[p] - campos) / max(|xyz[p] - campos|, 1e-12)
 *     colour[c] = max(0.5 + sum_{k < (deg+1)^2} Y_k(d) * t[k,c], 0)
 *
 * with Y_k the real spherical-harmonics polynomials of eval_sh (method.py:493-548; the constants and signs of include/wg_sh_eval.h) and
 * C0 = Y_0.  A clamp bound of +inf means no clamp.  The MLP is the float32-MFMA tile walk of wg_appearance_mlp.h: hidden width 128,
 * six outputs, the shared segment folded into the first-layer bias, weights in nn.Linear layout, ReLU'(0) = 0.
 *
 * Backward, for the cotangent g = dL_dcolours[p]: g_c passes where 0.5 + sum > 0; dt[k,c] = Y_k g_c passes where the unclamped t is
 * <= post_clamp_max; d mul[c] = sum_k dt[k,c] fc[k,c]; d offset[c] = dt[0,c] / C0; dz3 = out_scale * (d offset, d mul); then back through
 * the two masked transposed products to dz1, and grad_shared = W1[:, 3+G : 3+G+E]^T . sum_rows dz1.  NOTHING ELSE receives a gradient:
 * no weight gradient, no per-row input gradient and no [P, 48] tensor exists in either direction.  That is the operator's contract.
 *
 * Rows: `rows` is an optional list of M int32 row indices, in any order; a 32-row half tile is 32 list entries.  An entry outside
 * [0, P) is skipped: it is never dereferenced, writes nothing and contributes exact zeros.  rows == NULL means rows 0..M-1 in order (M <= P;
 * M = P for all rows).  Forward writes colours[row, 0..2] of the listed rows and touches no other element; backward reads dL_dcolours of
 * the listed rows only.
 *
 * Backward sums dz1 over its rows per workgroup, writes one partial of WG_COLOUR_PARTIAL_FLOATS floats per workgroup to `scratch`, and a
 * second launch adds the partials in workgroup order and forms grad_shared.  No floating-point atomics: two calls on the same inputs
 * and the same max_workgroups give the same bits.
 *
 * Grid: persistent, min(ceil(M / 64), workgroups) workgroups of 256 threads; max_workgroups = 0 takes the device's compute-unit count.
 *
 * Host contract: device pointers (campos too: three floats on the device), explicit HIP stream, no host synchronisation, no allocation,
 * nothing that prevents stream capture.  M = 0: WG_OK, grad_shared zero.  Every call returns 0 or a negative wg_status
 * (wg_rasterizer.h); a malformed call -- a null mandatory pointer, widths out of range, a row stride below its width, deg outside 0..3,
 * M > P with rows == NULL, scratch too small, a struct_size that does not cover the fields -- is refused with WG_ERR_INVALID_ARGUMENT
 * before any device work.
 */
#ifndef WG_APPEARANCE_COLOUR_H
#define WG_APPEARANCE_COLOUR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WG_COLOUR_COEFFS 48             /* floats of `features` read per row: 16 coefficients x 3 channels, coefficient-major */
#define WG_COLOUR_MAX_WIDTH 64          /* of 3 + G, and of the shared segment */
#define WG_COLOUR_TILE_ROWS 64
#define WG_COLOUR_PARTIAL_FLOATS 128    /* one workgroup's partial: the sum of dz1 over its rows */

typedef struct wg_appearance_colour_args {
    size_t struct_size;          /* the caller's sizeof(wg_appearance_colour_args) */
    int64_t P;                   /* rows of features / gembedding / xyz / colours / dL_dcolours; < 2^31 */
    int64_t M;                   /* listed rows */
    const int32_t* rows;         /* [M], or NULL for rows 0..M-1 */
    const float* features;       /* [P, >= 48] */
    int64_t features_row_stride; /* >= 48 */
    int32_t deg;                 /* 0..3 */
    int32_t gembedding_width;    /* G >= 0, 3 + G <= 64 */
    const float* gembedding;     /* [P, G]; NULL iff G == 0 */
    int64_t gembedding_row_stride; /* >= G */
    const float* shared;         /* [E] the image's appearance embedding */
    int32_t shared_width;        /* E, 1..64 */
    int32_t max_workgroups;      /* 0 = automatic */
    const float* xyz;            /* [P, >= 3] */
    int64_t xyz_row_stride;      /* >= 3 */
    const float* campos;         /* [3] on the device */
    const float* W1; const float* b1; const float* W2; const float* b2; const float* W3; const float* b3;   /* W1 is [128, 3 + G + E] */
    float out_scale;
    float pre_clamp_max;
    float post_clamp_max;
    int32_t reserved;
    float* colours;              /* forward: [P, 3] contiguous */
    /* backward only */
    const float* dL_dcolours;    /* [P, 3] contiguous */
    float* grad_shared;          /* [E], fully overwritten */
    float* scratch;
    int64_t scratch_floats;      /* what `scratch` holds */
    void* stream;
} wg_appearance_colour_args;

/* Floats of scratch a backward call over M listed rows needs; a negative wg_status for M < 0 or max_workgroups < 0, or when
 * max_workgroups = 0 and no device can be asked for its compute-unit count.
 * = min(ceil(M / WG_COLOUR_TILE_ROWS), workgroups) * WG_COLOUR_PARTIAL_FLOATS. */
int64_t wg_appearance_colour_scratch_floats(int64_t M, int32_t max_workgroups);
int wg_appearance_colour_forward(const wg_appearance_colour_args* args);
int wg_appearance_colour_backward(const wg_appearance_colour_args* args);

#ifdef __cplusplus
}
#endif
#endif
