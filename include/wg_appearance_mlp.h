/* wg_appearance_mlp.h -- C-ABI of the fused appearance MLP, forward and backward, in float32 on the matrix cores.
 *
 * Replaces, as an opt-in for callers, the arithmetic of EmbeddingModel.forward (wildgaussians/method.py:874-900) up to the final toning
 * statements: `torch.cat((color, gembedding, aembedding))`, Linear(K, 128) - ReLU - Linear(128, 128) - ReLU - Linear(128, 6) and `* 0.01`,
 * with autograd's backward pass.  Hidden width 128 and output width 6 (appearance_model_sh = False) only.
 *
 *     out[P, 6] = out_scale * (W3 . relu(W2 . relu(W1 . x + b1) + b2) + b3)
 *
 * x is never materialised: a row is the concatenation of up to WG_MLP_MAX_SEGMENTS per-row segments, each read in place through
 * (pointer, width, row stride in floats) -- `color` is `features[..., :3]`, a stride-48 view -- followed by an optional SHARED segment, one
 * vector of `shared_width` floats for all rows (the appearance embedding of the image being rendered).  The per-row widths sum to 1..64,
 * shared_width is 0..64, and W1 is [128, K] with K = the sum of both, columns in that order.  Forward the shared segment is folded into the
 * first-layer bias once per workgroup (b1' = b1 + W1[:, shared] . e); backward its gradient is W1[:, shared]^T . db1 and the shared columns
 * of dW1 are db1 (x) e, both formed in the finishing pass.  Weights are in nn.Linear layout, row-major: W1[128, K] b1[128] W2[128, 128]
 * b2[128] W3[6, 128] b3[6].
 *
 * Arithmetic: every product is a float32-input, float32-accumulate MFMA (v_mfma_f32_32x32x2_f32), i.e. fmaf chains with one rounding per
 * term.  There is no reduced-precision path.  ReLU'(0) = 0 as torch's threshold_backward.
 *
 * Backward takes dL_dout[P, 6] and RECOMPUTES h1 and h2 per row tile from the inputs: nothing of size P x 128 is read from or written to
 * device memory, and a caller saves nothing but the inputs.  Outputs, each fully overwritten:
 *     grad_segment[i]  [P, width_i] with row stride grad_row_stride[i] (NULL: skipped, the buffer is not touched)
 *     grad_shared      [shared_width] (NULL: skipped)
 *     dW1 db1 dW2 db2 dW3 db3, all six or none
 * Weight gradients are accumulated per workgroup in registers, written as ONE partial per workgroup to `scratch`, and summed by a second
 * launch in workgroup order; bias gradients likewise.  No floating-point atomics anywhere: two calls on the same inputs and the same
 * max_workgroups give the same bits.
 *
 * Grid: persistent, min(row tiles, workgroups) workgroups of 256 threads over tiles of WG_MLP_TILE_ROWS rows; `max_workgroups` = 0 takes
 * the device's compute-unit count (cached per device), any other positive value caps the grid (tests reach the multi-pass path at tiny P
 * with it).  Workgroups that would have no tile are not launched and contribute no partial.
 *
 * Host contract: device pointers, explicit HIP stream, no host synchronisation, no allocation, nothing that prevents stream capture.
 * `scratch` (backward only) holds at least wg_appearance_mlp_scratch_floats(P, max_workgroups) floats.  P = 0: WG_OK, `out` empty,
 * weight gradients and grad_shared zero.  Every call returns 0 or a negative wg_status (wg_rasterizer.h); a malformed call -- a null
 * mandatory pointer, widths out of range, row_stride < width, some but not all weight gradients, scratch too small, a struct_size that
 * does not cover the fields -- is refused with WG_ERR_INVALID_ARGUMENT before any device work.
 */
#ifndef WG_APPEARANCE_MLP_H
#define WG_APPEARANCE_MLP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WG_MLP_MAX_SEGMENTS 3
#define WG_MLP_HIDDEN 128
#define WG_MLP_OUT 6
#define WG_MLP_MAX_WIDTH 64          /* of the per-row segments together, and of the shared segment */
#define WG_MLP_TILE_ROWS 64
/* floats of one workgroup's partial: dW1 [128, 64] dW2 [128, 128] dW3 [6, 128] db1 [128] db2 [128] db3 [8] */
#define WG_MLP_PARTIAL_FLOATS (128 * 64 + 128 * 128 + 6 * 128 + 128 + 128 + 8)
#define WG_MLP_SCRATCH_HEAD_FLOATS 128   /* the summed db1, which the shared segment's gradient is taken from */

typedef struct wg_appearance_mlp_segment {
    const float* ptr;        /* [P, width] with row stride `row_stride` floats */
    int32_t width;
    int32_t reserved;
    int64_t row_stride;      /* >= width */
} wg_appearance_mlp_segment;

typedef struct wg_appearance_mlp_args {
    size_t struct_size;      /* the caller's sizeof(wg_appearance_mlp_args) */
    int64_t P;
    int32_t num_segments;    /* 1..WG_MLP_MAX_SEGMENTS */
    int32_t shared_width;    /* 0..WG_MLP_MAX_WIDTH */
    wg_appearance_mlp_segment segments[WG_MLP_MAX_SEGMENTS];
    const float* shared;     /* [shared_width]; NULL iff shared_width == 0 */
    const float* W1; const float* b1; const float* W2; const float* b2; const float* W3; const float* b3;
    float out_scale;
    int32_t max_workgroups;  /* 0 = automatic */
    float* out;              /* forward: [P, 6] contiguous */
    /* backward only */
    const float* dL_dout;    /* [P, 6] contiguous */
    float* grad_segment[WG_MLP_MAX_SEGMENTS];       /* NULL = not wanted */
    int64_t grad_row_stride[WG_MLP_MAX_SEGMENTS];   /* >= width where grad_segment is given */
    float* grad_shared;      /* NULL = not wanted */
    float* dW1; float* db1; float* dW2; float* db2; float* dW3; float* db3;   /* all six or none */
    float* scratch;
    int64_t scratch_floats;  /* what `scratch` holds */
    void* stream;
} wg_appearance_mlp_args;

/* Floats of scratch a backward call with this P and max_workgroups needs; a negative wg_status for P < 0 or max_workgroups < 0, or when
 * max_workgroups = 0 and no device can be asked for its compute-unit count.
 * = WG_MLP_SCRATCH_HEAD_FLOATS + min(ceil(P / WG_MLP_TILE_ROWS), workgroups) * WG_MLP_PARTIAL_FLOATS. */
int64_t wg_appearance_mlp_scratch_floats(int64_t P, int32_t max_workgroups);
int wg_appearance_mlp_forward(const wg_appearance_mlp_args* args);
int wg_appearance_mlp_backward(const wg_appearance_mlp_args* args);

#ifdef __cplusplus
}
#endif
#endif
