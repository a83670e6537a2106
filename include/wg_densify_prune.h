/* wg_densify_prune.h -- C-ABI of the fused densify-and-prune (clone, split and prune in one GPU pass), of the exact quantile it needs
 * and of reset_opacity.  Included by wg_densify.h: the entry points below stand beside wg_densification_stats, which produces their inputs.
 *
 * Replaces, as an opt-in for callers, GaussianModel.densify_and_prune with _densify_and_clone, _densify_and_split,
 * _densification_postfix and _prune_points (wildgaussians/method.py:1280-1468) and reset_opacity (:1249-1278).  The reference runs
 * three to four passes over every parameter, both Adam moments and every per-Gaussian buffer, through boolean masks; here one plan
 * (decisions + offsets) and one gather move each byte once, with one host read in between (the new count).
 *
 * Per-Gaussian decisions, for P Gaussians with statistics xyz_grad, denom and (use_abs_gradient) xyz_gradient_accum_abs of P floats:
 *     g  = xyz_grad / denom, NaN -> 0              ga = xyz_gradient_accum_abs / denom, NaN -> 0
 *     ratio = count(|g| >= max_grad) / P           (the exact integer count, converted once, divided in float32)
 *     Q  = quantile(ga, 1 - ratio), linear interpolation (below)
 *     m  = max_k exp(scales_raw[k])                (the plain activation, not the 3-D-filtered scale)
 *     clone = (|g| >= max_grad or |ga| >= Q) and m <= dense_threshold          dense_threshold = percent_dense * extent
 *     split = ( g  >= max_grad or  ga  >= Q) and m >  dense_threshold
 * (the reference takes a norm for the clone test and none for the split test; the statistics are sums of norms, never negative, so the two
 * agree).  Without use_abs_gradient only the first term of either test applies and no quantile is taken.  A clone can never be split: in the
 * reference its padded gradient is 0 and its m is on the clone side of the threshold; the decisions here are taken once, from the P inputs,
 * and rely on that.  Clones are copies of the raw parameters.  Every split Gaussian is replaced by two children c = 0, 1:
 *     xyz_new    = R(normalize(normalize(rotations_raw))) . (z * exp(scales_raw)) + xyz        z: a standard-normal draw the caller supplies
 *     scales_new = log(exp(scales_raw) / 1.6f)                                                 every other parameter copied
 * A survivor of these steps is then removed when sigmoid(opacities_raw) < min_opacity or (enable_size_pruning) max_k exp(scales[k]) >
 * size_threshold (= 0.1 * extent), children with their NEW scales.  Output order: surviving originals in index order, surviving clones,
 * copy-0 children, copy-1 children (kinds 0, 1, 2, 3 of `origin`).  Adam moments and per-Gaussian buffers are copied for originals and
 * zero for every new row (WG_DP_ZERO_NEW).
 *
 * The quantile is an exact order-statistic selection (4 passes of 8-bit digits over order-preserving keys, workgroup-private LDS
 * histograms, one small device-side reduction per pass, no sort); the two adjacent ranks are selected in the same passes.  It follows
 * torch.quantile for n <= 2^24: q as float32, rank = q * (n - 1) in float32, lo = floor(rank), hi = ceil(rank), w = rank - lo,
 * Q = lerp(v[lo], v[hi], w) (torch's lerp: lo + w (hi - lo) for w < 0.5, else hi - (hi - lo)(1 - w)).  Above 2^24 elements torch.quantile
 * refuses and float32 can no longer index the elements: there ratio, q, rank and w are computed in float64 and the lerp is evaluated
 * in float64 and rounded to float32 once.  Values must not be NaN.
 *
 * Nothing allocates inside a call: the caller hands in outputs and scratch (wg_densify_scratch_bytes, 256-byte aligned; one scratch
 * serves plan and the apply that follows it).  Every call takes an explicit stream and returns 0 or a negative wg_status.  wg_densify_plan
 * ends with an asynchronous copy of a wg_densify_counts to `counts_host` (pinned host memory: the call's mailbox); the caller waits for the
 * stream -- the only host wait --, sizes the outputs with n_out and calls wg_densify_apply.  Not supported inside a stream capture (the
 * output size is data-dependent): WG_ERR_INVALID_ARGUMENT.  float32 / int32 device pointers; destinations 16-byte aligned.
 */
#ifndef WG_DENSIFY_PRUNE_H
#define WG_DENSIFY_PRUNE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct wg_densify_params {
    float max_grad;         /* densify_grad_threshold */
    float min_opacity;
    float dense_threshold;  /* float32(percent_dense * extent), the product formed in double as Python forms it */
    float size_threshold;   /* float32(0.1 * extent) */
    int32_t enable_size_pruning;
    int32_t use_abs_gradient;
} wg_densify_params;

typedef struct wg_densify_counts {
    int64_t n_out[4];       /* rows of the output by kind: surviving originals, clones, copy-0 children, copy-1 children */
    int64_t n_cloned;       /* the reference's clone - before */
    int64_t n_split;        /* split parents, the reference's split - clone */
    int64_t n_pruned;       /* the reference's split - prune */
    int64_t n_hot;          /* count(|g| >= max_grad) */
    float ratio;
    float Q;                /* NaN without use_abs_gradient */
    int32_t reserved[2];
} wg_densify_counts;

enum { WG_DP_COPY = 0,       /* every output row is its source row */
       WG_DP_ZERO_NEW = 1,   /* source row for originals, zero for clones and children (Adam moments, per-Gaussian buffers) */
       WG_DP_XYZ = 2,        /* children: the transformed position (3 floats per row) */
       WG_DP_SCALES = 3 };   /* children: log(exp(s) / 1.6f) (3 floats per row) */

typedef struct wg_densify_array {
    const float* src;       /* P rows */
    float* dst;             /* the new number of rows; must not overlap any source */
    int32_t row_floats;
    int32_t role;
} wg_densify_array;

#define WG_DENSIFY_MAX_ARRAYS 48

size_t wg_densify_scratch_bytes(int64_t P);   /* 0 for P < 0; also what wg_quantile needs for any n <= P */

/* Q = quantile(values[0..n), q), 0 <= q <= 1, into *result (device, one float).  scratch: wg_densify_scratch_bytes(0) bytes suffice. */
int wg_quantile(int64_t n, const float* values, double q, float* result, void* scratch, void* stream);

int wg_densify_plan(int64_t P, const wg_densify_params* params, const float* xyz_grad, const float* denom,
                    const float* xyz_gradient_accum_abs, const float* scales_raw, const float* opacities_raw, void* scratch,
                    wg_densify_counts* counts_host, void* stream);

/* After the stream has delivered `counts`: origin is int32 [n_new, 2] = (source index, kind), n_new the sum of counts->n_out; noise is
 * [2 n_split, 3], copy-major (row c * n_split + k serves child c of the k-th split Gaussian in index order).  One launch moves all arrays. */
int wg_densify_apply(int64_t P, const wg_densify_counts* counts, const void* scratch, int num_arrays, const wg_densify_array* arrays,
                     const float* xyz, const float* scales_raw, const float* rotations_raw, const float* noise, int32_t* origin, void* stream);

/* reset_opacity (method.py:1252-1266), elementwise, out may alias opacities_raw:
 *     out = logit(min(sigmoid(o) * coef(exp(s), f), 0.01) / coef(sqrt(exp(s)^2 + f^2), f)),  coef(t, f) = sqrt(prod t^2 / prod (t^2 + f^2))
 * (the reference divides by the coefficient of the already filtered scales).  exp_avg / exp_avg_sq (may be NULL) are zeroed. */
int wg_reset_opacity(int64_t P, const float* opacities_raw, const float* scales_raw, const float* filter_3D, float* out, float* exp_avg,
                     float* exp_avg_sq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
