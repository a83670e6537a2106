/*
 * wg_rasterizer.h -- C-ABI of the MI355X-native differentiable Gaussian-splat rasterizer (libwg_rasterizer.so).
 *
 * The drop-in boundary for the hot path of jkulhanek/wild-gaussians: it replaces the static C++ interface
 * CudaRasterizer::Rasterizer::{forward,backward,markVisible} (submodules/diff-gaussian-rasterization/cuda_rasterizer/
 * rasterizer.h:24-88), i.e. what the reference's torch binding (rasterize_points.cu:35-225) calls.  Differences, all forced by
 * "plain C, no C++ / torch types in the signature": std::function<char*(size_t)> allocators become (function pointer, void* user)
 * pairs; every call takes the HIP stream to launch on (NULL = the default stream; the reference uses the legacy default stream,
 * rasterizer_impl.cu:148,292); errors are negative wg_status codes instead of C++ exceptions (rasterizer_impl.cu:244-247,
 * auxiliary.h:166-173); bool becomes int / unsigned char.
 *
 * All pointers are DEVICE pointers to contiguous float32 / int32 data unless stated otherwise.  NULL means "not provided" exactly as
 * in the reference (shs vs colors_precomp, scales + rotations vs cov3D_precomp; forward.cu:217,253, backward.cu:426,430).  Matrices
 * have the reference's layout: viewmatrix = W2C transposed, projmatrix = (P W2C) transposed, row-major (auxiliary.h:58-77).
 *
 * The surface is TWO pairs of entry points: wg_rasterize_forward / _backward, argument for argument the reference's interface, and
 * wg_rasterize_forward_ex / _backward_ex, which take ONE struct: the same arguments plus optional blocks for everything beyond the
 * reference (NULL = absent) and the PER-CALL options that affect results.  The first pair is the second with no block and default
 * options.  The library keeps no result-affecting process-wide state: wg_set_option only holds tuning switches whose every setting
 * gives bit-identical results (docs/OPTIONS.md).
 *
 * The three scratch buffers (geometry / binning / image state) are opaque (the layout differs from the reference's GeometryState /
 * BinningState / ImageState).  Documented: the image-state buffer starts, at its first 256-byte-aligned address, with final_T as
 * float[H*W], and holds at wg_image_accumulation_offset() behind it accumulation = 1 - final_T as float[H*W], written by the forward
 * pass itself (the reference's Python wrapper computes it from final_T, diff_gaussian_rasterization/__init__.py:101-113).
 */
#ifndef WG_RASTERIZER_H_INCLUDED
#define WG_RASTERIZER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_TILE_X 16 /* config.h:15 */
#define WG_TILE_Y 16 /* config.h:16 */
#define WG_NUM_CHANNELS 3 /* config.h:14 */

typedef enum wg_status {
    WG_OK = 0,
    WG_ERR_INVALID_ARGUMENT = -1, /* bad sizes / missing mandatory pointer / both-or-neither optional inputs / an inconsistent block */
    WG_ERR_ALLOC = -2,            /* an allocator callback returned NULL */
    WG_ERR_HIP = -3,              /* a HIP runtime call or kernel launch failed (wg_last_hip_error() has the text) */
    WG_ERR_OVERFLOW = -4,         /* more than 2^31-1 (tile, Gaussian) instances */
    WG_ERR_SPECULATION = -5       /* "speculative_forward" = 2 only: the calling thread's PREVIOUS forward call did not fit the binning buffer
                                     it had predicted; that call's image is NaN and its gradients are zero -- repeat the step */
} wg_status;

/* Replaces std::function<char*(size_t N)> (rasterizer.h:34-36, rasterize_points.cu:27-33): returns a device pointer to at least
 * `bytes` bytes that stays valid until the matching backward call.  binning_alloc may be called TWICE in one forward call (the
 * speculative forward re-issues a frame that did not fit its predicted buffer); the buffer returned last is the one in use. */
typedef char* (*wg_alloc_fn)(size_t bytes, void* user);

/* Scratch sizes (bytes), for callers that preallocate (the binning size is an upper bound).  wg_geometry_buffer_size_rows: what a forward
 * call with plain SH colours (no tone, no second set) and forward_only = 0 asks geometry_alloc for -- 40 bytes per Gaussian more, rounded up to
 * 256, the frame's backward rows; every other forward call asks for wg_geometry_buffer_size. */
size_t wg_geometry_buffer_size(int P);
size_t wg_geometry_buffer_size_rows(int P);
size_t wg_image_buffer_size(int width, int height);
size_t wg_binning_buffer_size(int num_rendered);
size_t wg_image_accumulation_offset(int width, int height); /* bytes from final_T to accumulation[H*W] */

/* Rasterizer::forward (rasterizer.h:33-59, rasterizer_impl.cu:198-340).  Returns num_rendered (>= 0) or a negative wg_status.
 * out_color: float[3*H*W] planar CHW, fully written.  radii: int[P] or NULL.  subpixel_offset: float[H*W*2], or NULL (beyond the
 * reference: all zero, nothing read).  The reference's one host<->device rendezvous (num_rendered sizes the binning buffer,
 * rasterizer_impl.cu:284) sits behind the call's LAST launch, not in its middle (docs/OPTIONS.md: "speculative_forward"). */
int wg_rasterize_forward(wg_alloc_fn geometry_alloc, void* geometry_user, wg_alloc_fn binning_alloc, void* binning_user,
                         wg_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width, int height,
                         const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                         const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                         const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                         float kernel_size, const float* subpixel_offset, int prefiltered, float* out_color, int* radii, int debug,
                         void* stream);

/* Rasterizer::backward (rasterizer.h:61-88, rasterizer_impl.cu:344-443).  The reference wants all nine gradient outputs zero-filled
 * (rasterize_points.cu:157-165); here (options->grad_record = 1, the default) all nine are fully OVERWRITTEN (zeros for culled
 * Gaussians) -- a caller following the reference's protocol gets the same values -- and dL_dconic (an intermediate of the
 * reference) and, with SH colours, dL_dcolor may be NULL.  dL_dcov3D may be NULL whenever cov3D_precomp is (with scales and rotations
 * it is an intermediate too: its chain rule is applied into dL_dscale / dL_drot either way, only the store is left out) -- with or
 * without the record.  dL_dconic: float[P*4], 16-byte aligned ([0],[1],[3] used);
 * dL_dmean2D: float[P*3] (x, y NDC-scaled, z = abs-gradient, backward.cu:590-595); dL_dsh may be NULL when M == 0. */
int wg_rasterize_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* campos, float tan_fovx, float tan_fovy, float kernel_size, const float* subpixel_offset,
                          const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                          float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                          float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream);

/* Rasterizer::markVisible (rasterizer.h:26-31, rasterizer_impl.cu:141-153). present: unsigned char[P]. */
int wg_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, unsigned char* present, void* stream);

/* ---- optional blocks of the _ex calls (everything beyond the reference; SURVEY.md 8f N3 and the caller's two renders per step) ---- */

/* Result-affecting switches, PER CALL (NULL = WG_CALL_OPTIONS_DEFAULT).  A frame's backward call must carry its forward call's
 * exact_compositing: the library remembers it per image buffer and returns WG_ERR_INVALID_ARGUMENT on a mismatch.
 *   exact_compositing (1): every skip / stop decision of forward.cu:356-372 / backward.cu:536-546 on values computed with the
 *     reference's own float32 operations and hipcc's float32 `exp` expansion: n_contrib, final_T and the blended set equal the
 *     reference's -ffp-contract=off build bit for bit (image within ~2e-7).  0: exp2 of a fused form, ~2 pixels per million flip, 5 % faster.
 *   deterministic_backward (0): 1 = every (tile, Gaussian) instance stores its wave-reduced sums in a slot of its own and a
 *     per-Gaussian pass adds them in a fixed order instead of float atomics: bit-identical gradients run to run.  Its scratch is a block
 *     of the library's own, leased for the call: not inside a stream capture (WG_ERR_INVALID_ARGUMENT -- a replay would write a block others hold).
 *   grad_record (1): the per-tile pass accumulates into a 48-byte record per Gaussian inside geom_buffer (see wg_rasterize_backward);
 *     0 = into dL_dmean2D / dL_dconic / dL_dopacity / dL_dcolor themselves, which must then be non-NULL and zero on entry. */
typedef struct wg_call_options {
    int exact_compositing, deterministic_backward, grad_record;
} wg_call_options;
#define WG_CALL_OPTIONS_DEFAULT {1, 0, 1}

/* Per-Gaussian affine on the SH coefficients inside K1 / K11 ("the appearance MLP output feeds SH eval directly"):
 *   x = min(shs[i][k][c], pre_clamp_max);  t = x * mul[i][c] + (k == 0 ? offset[i][c] : 0);  used = min(t, post_clamp_max)
 * (separate multiply and add: the values of `(features.clamp_max(1) * mul + cat(offset / C0, 0)).clamp_max(1)`,
 * wildgaussians/method.py:890-900, 1590-1595).  INFINITY switches a clamp off; mul / offset may be NULL (1 / 0).  Backward: dL_dsh is
 * then the gradient of the RAW coefficients; dL_dmul / dL_doffset ([P,3], overwritten) are required where mul / offset are given. */
typedef struct wg_sh_tone {
    const float* mul;      /* [P,3] or NULL */
    const float* offset;   /* [P,3] or NULL */
    float pre_clamp_max, post_clamp_max;
    float* dL_dmul;        /* backward only */
    float* dL_doffset;     /* backward only */
} wg_sh_tone;

/* The caller's get_gaussians() (wildgaussians/method.py:1060-1086) inside K1 / K11: `opacities`, `scales`, `rotations` are the RAW
 * parameters (logit, log-scale, unnormalised quaternion); q = r / max(|r|, 1e-12), s = sqrt(exp(ls)^2 + f^2), o = sigmoid(lo) *
 * sqrt(prod exp(ls)^2 / prod s^2).  Backward: dL_dopacity / dL_dscale / dL_drot are the RAW parameters' gradients (needs grad_record).
 * Scale / rotation pairs only.  Same device functions and bits as wg_activations_forward / _backward (include/wg_activations.h). */
typedef struct wg_raw_gaussians {
    const float* filter_3D;       /* [P] */
    const float* raw_opacities;   /* [P], backward only: the forward call's `opacities` */
} wg_raw_gaussians;

/* A SECOND image composited in the same walk (WildGaussians renders raw and toned colours over identical geometry every step,
 * method.py:1573-1611; the decisions do not depend on the colours).  Either a second set of precomputed colours (colors_precomp2, with
 * colors_precomp) or -- sh_second = 1 in the args -- the SAME SH coefficients through `tone2`.  Both images share the background.
 * Backward: dL_dpix2 = out_color2's cotangent (zeros if none); dL_dcolor2 [P,3] out (may be NULL with sh_second); the geometry
 * gradients are those of BOTH images' losses (what autograd adds over the reference's two calls).  Needs grad_record or
 * deterministic_backward. */
typedef struct wg_second_image {
    const float* colors_precomp2;   /* forward; NULL with sh_second */
    float* out_color2;              /* forward: float[3*H*W], fully written */
    const float* dL_dpix2;          /* backward */
    float* dL_dcolor2;              /* backward */
} wg_second_image;

/* Recolouring: a further image of the SAME Gaussians through the SAME camera with other precomputed colours, along the parent
 * call's sorted lists.  parent_*: the three buffers a forward call returned (R = its return value), alive and unmodified.  The call
 * allocates ONE new geometry buffer (geometry_alloc), reads only colors_precomp / background / subpixel_offset / out_color / radii
 * of the args, and returns R; its backward call takes the NEW geometry buffer and the parent's binning and image buffers. */
typedef struct wg_recolor_parent {
    char *geom_buffer, *binning_buffer, *image_buffer;
    int R;
} wg_recolor_parent;

typedef struct wg_forward_args {
    size_t struct_size;   /* the CALLER's sizeof(wg_forward_args): fields are only ever appended (one exception: forward_only, below, took
                             what was padding); a shorter (older) struct is accepted
                             from version 0.5's 288 bytes on, its missing tail reads as absent; a longer (newer) one is refused */
    wg_alloc_fn geometry_alloc; void* geometry_user;
    wg_alloc_fn binning_alloc;  void* binning_user;
    wg_alloc_fn image_alloc;    void* image_user;
    int P, D, M, width, height, prefiltered, debug;
    float scale_modifier, tan_fovx, tan_fovy, kernel_size;
    const float *background, *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *cam_pos, *subpixel_offset;
    float* out_color;
    int* radii;
    void* stream;
    /* beyond the reference: NULL / 0 = absent */
    const wg_sh_tone* tone;            /* with shs */
    const wg_sh_tone* tone2;           /* with sh_second: the second image's tone (NULL = no affine, no clamp) */
    int sh_second;                     /* second image = the same SH coefficients through tone2 (needs `second`->out_color2) */
    const wg_second_image* second;
    const wg_raw_gaussians* raw;
    const wg_recolor_parent* recolor;
    int binning_capacity;              /* > 0: NO host rendezvous at all (hipGraph capture): the caller's capacity in instances; returns it
                                          (hand it to backward as R); a frame that does not fit gives a NaN image and zero gradients,
                                          wg_forward_status() tells afterwards.  <= 36864 tiles, no debug, no deterministic backward. */
    int forward_only;                  /* 1: the caller expects NO backward call for this frame (grad mode off, nothing requires a gradient): a
                                          frame with plain SH colours then skips the 40-byte backward row per Gaussian it would leave for the
                                          per-Gaussian backward kernel, and asks geometry_alloc for wg_geometry_buffer_size(P) instead of
                                          wg_geometry_buffer_size_rows(P).  A hint, not a contract: a backward call on such a frame is served by
                                          the kernel that re-reads the SH block.  The field takes the four bytes that were padding between
                                          binning_capacity and options since version 0.5, so the struct keeps its 288 bytes and its first
                                          published layout: a caller built against an older header, whose structs are zero-initialised, says 0. */
    const wg_call_options* options;
} wg_forward_args;

/* The gradient of the depth pass (wg_render_depth) inside the frame's backward call: one more per-tile walk that adds into the gradient record
 * before the per-Gaussian kernel runs, so that dL_dmean2D / dL_dopacity / dL_dmean3D / dL_dcov3D / dL_dscale / dL_drot come out as the gradients of
 * the image loss PLUS the depth loss (what autograd adds over the image call and a second three-channel call with the scalars as colours).
 *   depth = sum_i v_i alpha_i T_i over the pairs the forward call blended:  dL/dv_g = sum over g's pairs of alpha T dL_ddepth[pixel];
 *   dL/dalpha_i = dL_ddepth[pixel] T_i (v_i - R_i), R_i the reference's accum_rec recursion for one channel (backward.cu:555-561); no background
 *   term; from dL/dalpha on the reference's chain (backward.cu:568-603).  The abs-gradient (dL_dmean2D.z) receives |q_depth| beside |q_image|.
 *   values: float[P], the scalars of the forward depth pass; or NULL = the distance to the camera (reads the call's means3D and campos): dL_dmean3D
 *     then also receives dL_dvalues[g] * (x_g - campos) / v_g (0 where v_g == 0).  campos takes no gradient.
 *   dL_dvalues: float[P], required in both modes, overwritten in full, zero for Gaussians without instances.
 * Needs the atomic gradient record: WG_ERR_INVALID_ARGUMENT, before any launch, with colour_gradients_only != 0, deterministic_backward = 1,
 * grad_record = 0, a struct_size smaller than the struct, a NULL dL_ddepth or (P > 0) dL_dvalues, distance mode without means3D / campos.  R = 0 or
 * P = 0 zero-fill dL_dvalues and launch no walk.  No scratch, no host wait: the call captures like the one without the block. */
typedef struct wg_depth_grad {
    size_t struct_size;       /* the CALLER's sizeof(wg_depth_grad): fields are only ever appended */
    const float* dL_ddepth;   /* [H*W] */
    const float* values;      /* [P] or NULL (distance) */
    float* dL_dvalues;        /* [P], fully overwritten */
} wg_depth_grad;

typedef struct wg_backward_args {
    size_t struct_size;
    int P, D, M, R, width, height, debug;
    float scale_modifier, tan_fovx, tan_fovy, kernel_size;
    const float *background, *means3D, *shs, *colors_precomp, *scales, *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos, *subpixel_offset;
    const int* radii;
    char *geom_buffer, *binning_buffer, *image_buffer;
    const float* dL_dpix;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
    void* stream;
    const wg_sh_tone* tone;
    const wg_sh_tone* tone2;
    int sh_second;
    const wg_second_image* second;
    const wg_raw_gaussians* raw;
    const wg_call_options* options;
    int colour_gradients_only;         /* 1: ONLY dL_dcolor [P,3] is computed (overwritten; zeros for Gaussians without instances) -- frames whose
                                          geometry is frozen and whose colours alone take a gradient.  One front-to-back walk that sums the
                                          forward pass's blend weights times dL_dpix; no per-Gaussian pass.  Needs colors_precomp-mode (shs NULL),
                                          dL_dcolor, dL_dpix, background and the three buffers; every other output pointer may be NULL and is
                                          never written; the grad_record option is ignored.  WG_ERR_INVALID_ARGUMENT with shs, tone, tone2,
                                          sh_second, second, raw, or deterministic_backward = 1.  Absent (a struct of version 0.5's 312
                                          bytes) = 0 = the full backward pass.
                                          2 (WG_COLOUR_GRADIENTS_FIXED_ORDER): the same gradient without float atomics -- every (tile, Gaussian)
                                          term is stored into a slot of the library's leased scratch (16 bytes + 1 flag byte per instance) and
                                          a second kernel adds each Gaussian's terms in an order fixed by the frame: two calls give the same
                                          bits.  Same needs and refusals as 1 (deterministic_backward = 1 included: that option belongs to the
                                          full pass); additionally refused inside a stream capture, like the full pass's deterministic mode.
                                          Any other non-zero value behaves as 1. */
    const wg_depth_grad* depth;        /* the depth pass's gradient in the same call (wg_depth_grad above), or NULL.  Absent (a struct of 320 bytes or
                                          less) = NULL: the call runs no new code and its gradients have the bits they had. */
} wg_backward_args;
#define WG_COLOUR_GRADIENTS_ATOMIC 1
#define WG_COLOUR_GRADIENTS_FIXED_ORDER 2

/* The gradient of the distortion pass (wg_render_distortion, below) inside the frame's backward call: one more per-tile walk that adds into the
 * gradient record before the per-Gaussian kernel runs -- behind the depth block's walk when both are present --, so that the geometry gradients come
 * out as those of the image loss PLUS the distortion loss.  With g = dL_ddistortion[pixel] and the forward pass's moments (A, D', Q', c), u_i = v_i - c:
 *   d dist / d w_i = m_i = Q' + u_i (A u_i - 2 D');  dL/dalpha_i = g T_i (m_i - R_i), R_i the reference's accum_rec recursion (backward.cu:555-561)
 *   for the "channel" m, back to front, no background term; from dL/dalpha on the reference's chain (backward.cu:568-603).  The abs-gradient
 *   (dL_dmean2D.z) receives |q_dist| beside |q_image|.  dL/dv_g = sum over g's pairs of 2 g w_i (A u_i - D'); the pivot takes no gradient.
 *   moments: float[4*H*W], what wg_render_distortion wrote into out_moments for THIS frame with THESE values.
 *   values: float[P], the scalars of the forward distortion pass; or NULL = the distance to the camera (reads the call's means3D and campos):
 *     dL_dmean3D then also receives dL_dvalues[g] * (x_g - campos) / v_g (0 where v_g == 0).  campos takes no gradient.
 *   dL_dvalues: float[P], required in both modes, overwritten in full, zero for Gaussians without instances.
 * Needs the atomic gradient record: WG_ERR_INVALID_ARGUMENT, before any launch, with colour_gradients_only != 0, deterministic_backward = 1,
 * grad_record = 0, a struct_size smaller than the struct, a NULL dL_ddistortion, moments or (P > 0) dL_dvalues, distance mode without means3D /
 * campos.  R = 0 or P = 0 zero-fill dL_dvalues and launch no walk.  No scratch, no host wait: the call captures like the one without the block. */
typedef struct wg_distortion_grad {
    size_t struct_size;            /* the CALLER's sizeof(wg_distortion_grad): fields are only ever appended */
    const float* dL_ddistortion;   /* [H*W] */
    const float* moments;          /* [4*H*W]: the planes A, D', Q', c of the forward distortion pass */
    const float* values;           /* [P] or NULL (distance) */
    float* dL_dvalues;             /* [P], fully overwritten */
} wg_distortion_grad;
/* What a backward call may carry beyond wg_backward_args, whose size tests pin: blocks by pointer, fields only ever appended. */
typedef struct wg_backward_extras {
    size_t struct_size;                     /* the CALLER's sizeof(wg_backward_extras) */
    const wg_distortion_grad* distortion;   /* the distortion pass's gradient in the same call, or NULL */
} wg_backward_extras;

int wg_rasterize_forward_ex(const wg_forward_args* args);
int wg_rasterize_backward_ex(const wg_backward_args* args);
/* wg_rasterize_backward_ex with the blocks of `extras`.  extras = NULL, or every block NULL: exactly wg_rasterize_backward_ex, no new code runs.
 * WG_ERR_INVALID_ARGUMENT for an extras struct smaller than its first published size (16 bytes). */
int wg_rasterize_backward_with(const wg_backward_args* args, const wg_backward_extras* extras);
/* num_rendered and fits (1 / 0) of the forward call that produced image_buffer; synchronises the stream. */
int wg_forward_status(char* image_buffer, int width, int height, int* num_rendered, int* fits, void* stream);

/* ---- introspection used by the parity tests (device pointers into the opaque buffers) ---- */
typedef struct wg_geometry_view {
    const float* depths;          /* [P]   view-space z (forward.cu:262) */
    const int* radii;             /* [P]   internal copy */
    const float* splats;          /* [P*12] 48-byte records: mx,my,conic.x,conic.y | conic.z,opacity*coef,r2,r | g,b,g2,b2 (r2,g2,b2: the second image's colours) */
    const float* cov3D;           /* [P*6] */
    const unsigned char* clamped; /* [P]   bit c: SH colour channel c was clamped at 0 (forward.cu:67-69); bits 3-5: the second image's */
    const uint32_t* tiles_touched;/* [P] */
    const uint32_t* point_offsets;/* [P]   inclusive prefix sum (global-sort and deterministic paths) */
} wg_geometry_view;
typedef struct wg_binning_view {
    const uint32_t* point_list;   /* [R] Gaussian ids sorted by (tile | depth), stable */
} wg_binning_view;
typedef struct wg_image_view {
    const float* final_T;       /* [H*W] */
    const float* accumulation;  /* [H*W] 1 - final_T */
    const uint32_t* n_contrib;  /* [H*W] */
    const uint32_t* ranges;     /* [tiles*2] (start,end) */
    const uint32_t* tile_last;  /* [tiles] max n_contrib over the tile's pixels */
    const uint32_t* tile_near;  /* [tiles] near / far split: near instances of the tile */
    const uint32_t* split;      /* [2] {depth-code threshold of the split (0xffffffff = off), bands that needed their far instances} */
    const uint32_t* order_fwd;  /* [tiles] launch order of the forward render kernel ("forward_order"; valid when order_key[0] != 0xffffffff) */
    const uint32_t* order_key;  /* [4] {the camera's row in the launch-order table or 0xffffffff = none, tag lo, tag hi, 1 = the row held this camera} */
    const uint32_t* order_bwd;  /* [tiles] launch order of the backward render kernel (written by the frame's backward call) */
} wg_image_view;
int wg_view_geometry(char* geom_buffer, int P, wg_geometry_view* out);
/* The backward rows of a frame with plain SH colours rendered with forward_only = 0: [P*10] floats, per Gaussian nine direction terms
 * T[ch][axis] = sum_k dB_k/d axis * sh[k][ch], then opacity*coef; zeros for a culled Gaussian.  buffer_bytes: the size of the frame's geometry
 * buffer; *rows = NULL when it is too small to hold the array (a frame that left none: its buffer is wg_geometry_buffer_size(P)).  A call of
 * its own, not a field of wg_geometry_view: that struct carries no size, so it cannot grow under callers built against an older header. */
int wg_view_backward_rows(char* geom_buffer, int P, size_t buffer_bytes, const float** rows);
int wg_view_binning(char* binning_buffer, int R, wg_binning_view* out);
int wg_view_image(char* image_buffer, int width, int height, wg_image_view* out);

/* ---- per-stage timing with HIP events on the caller's stream (bench.py's roofline): enable, run, read (synchronises) ---- */
enum { WG_STAGE_PREPROCESS = 0, WG_STAGE_SCAN, WG_STAGE_DUPLICATE_KEYS, WG_STAGE_SORT, WG_STAGE_TILE_RANGES,
       WG_STAGE_RENDER_FORWARD, WG_STAGE_RENDER_BACKWARD, WG_STAGE_PREPROCESS_BACKWARD, WG_STAGE_RENDER_FIXUP, WG_STAGE_RENDER_DEPTH, WG_STAGE_RENDER_DEPTH_BACKWARD,
       WG_STAGE_RENDER_CONTRIBUTIONS, WG_STAGE_COUNT };
typedef struct wg_stage_times {
    double total_ms[WG_STAGE_COUNT];
    long long launches[WG_STAGE_COUNT];
} wg_stage_times;
int wg_profile_enable(int enable);
int wg_profile_read(wg_stage_times* out);
int wg_profile_reset(void);
const char* wg_stage_name(int stage);

/* Tuning / test switches, process-wide, copied once per call; EVERY setting gives bit-identical results (binning strategies, host
 * flow, profiling).  Names, defaults and measurements: docs/OPTIONS.md.  -1 / WG_ERR_INVALID_ARGUMENT for an unknown name --
 * including the three result-affecting switches, which are per call (wg_call_options). */
int wg_set_option(const char* name, int value);
int wg_get_option(const char* name);

const char* wg_status_string(int status);
const char* wg_last_hip_error(void);
const char* wg_version(void);

/* ---- the projection-only pass: a frame's cull decisions before (and without) rendering it ----
 * radii[i] with THE BITS a forward call writes for the same geometry inputs and camera (0 = culled: behind the near plane at view-space
 * z <= 0.2, a singular 2-D covariance, or a tile rectangle that misses the grid), so radii > 0 is the set of Gaussians that reach the
 * image.  It is the per-Gaussian kernel's geometry restated (near cull, projection, 3-D covariance, clamped EWA Jacobian, mip filter,
 * eigenvalue radius, ndc2Pix, getRect), built with that kernel's flags.  wg_mark_visible is NOT this: it is the near-plane test alone.
 * One launch on `stream`; no colour, no SH block, no geometry / binning / image buffer, no allocator, no atomics, no host wait: it can be
 * captured.  Reads 12 + 12 + 16 bytes per Gaussian (12 + 24 with cov3D_precomp; + 4 with filter_3D), writes radii[0 .. P) in full and
 * nothing else.  `prefiltered` is not an input: the pass never traps.
 *   scales + rotations XOR cov3D_precomp, as in the forward call.
 *   filter_3D (only with scales + rotations): those two are then the caller's RAW parameters (wg_raw_gaussians) and get_gaussians() runs
 *     in-kernel.  There is no raw_opacities field: of the activation's outputs only the normalised rotation and sqrt(exp(ls)^2 + f^2)
 *     reach the radius; the opacity reaches neither, so it is not read.
 * WG_ERR_INVALID_ARGUMENT, before any device work: struct_size smaller than the struct, P < 0, width or height <= 0, with P > 0 a NULL
 * means3D / viewmatrix / projmatrix / radii or both / neither covariance source (or half a scales + rotations pair), filter_3D together
 * with cov3D_precomp.  P = 0 returns WG_OK and launches nothing.  Fields are only ever appended. */
typedef struct wg_project_args {
    size_t struct_size;   /* the CALLER's sizeof(wg_project_args) */
    int P, width, height;
    const float *means3D, *scales, *rotations, *cov3D_precomp;
    const float* filter_3D;   /* [P] or NULL */
    float scale_modifier, tan_fovx, tan_fovy, kernel_size;
    const float *viewmatrix, *projmatrix;
    int* radii;               /* [P], fully overwritten */
    void* stream;
} wg_project_args;
int wg_project_radii(const wg_project_args* args);

/* ---- the depth pass: one scalar per Gaussian composited over a FINISHED frame like a colour channel ----
 *   out_depth[pixel] = sum over the (pixel, Gaussian) pairs the frame's forward call blended of  v[Gaussian] * alpha * T
 * with the forward call's own decisions, alpha and T, and the forward kernel's multiply-add: the bits of one channel of a three-channel
 * forward call over the same geometry with colors_precomp = v repeated and an all-zero background (what the caller's depth render,
 * wildgaussians/method.py:1621-1631, keeps of its second rasterizer call).  No background term, no division by the accumulation.
 *   values: float[P], the scalars; or NULL = the distance to the camera, sqrtf(dx*dx + dy*dy + dz*dz) of means3D[i] - campos (means3D float[P*3],
 *     campos float[3], both DEVICE pointers) -- torch.norm(means3D - camera_center[None], dim=-1).  WG_ERR_INVALID_ARGUMENT when both sources
 *     are missing; with values given, means3D / campos are not read.
 *   geom_buffer / binning_buffer / image_buffer, R, subpixel_offset, options: the frame's, as its backward call takes them (a frame served by
 *     a recolouring call: its NEW geometry buffer and the parent's other two).  options->exact_compositing must be the frame's
 *     (WG_ERR_INVALID_ARGUMENT otherwise, as in the backward call); the other two options are not read.
 * One launch on `stream` over each tile's list up to tile_last.  The three buffers are only READ: a backward call of the frame before or after
 * it behaves as without it.  No scratch, no allocator, no atomics, no host wait -- but for a frame of the deferred forward, whose verdict is read
 * first (WG_ERR_SPECULATION: the frame did not fit, nothing is written).  out_depth: float[H*W], fully overwritten, 0 for a pixel without a
 * contributor; P = 0 or R = 0 zero-fill it and return WG_OK.  Two calls give the same bits.
 * WG_ERR_INVALID_ARGUMENT, before any device work: struct_size smaller than the struct, P < 0, R < 0, width or height <= 0, a NULL out_depth,
 * with P > 0 a NULL buffer or no scalar source.  Fields are only ever appended. */
typedef struct wg_depth_args {
    size_t struct_size;   /* the CALLER's sizeof(wg_depth_args) */
    int P, R, width, height;
    char *geom_buffer, *binning_buffer, *image_buffer;
    const float* subpixel_offset;   /* the frame's float[H*W*2], or NULL */
    const float* values;            /* [P] or NULL */
    const float* means3D;           /* [P*3], read when values is NULL */
    const float* campos;            /* [3], device, read when values is NULL */
    const wg_call_options* options; /* NULL = WG_CALL_OPTIONS_DEFAULT */
    float* out_depth;               /* [H*W], fully overwritten */
    int debug;                      /* 1: synchronise behind the launch and report (as the other calls' debug) */
    void* stream;
} wg_depth_args;
int wg_render_depth(const wg_depth_args* args);

/* ---- the distortion pass: the Mip-NeRF 360 / 2DGS distortion term of a FINISHED frame ----
 *   out_distortion[pixel] = sum_{j < i} w_i w_j (v_i - v_j)^2,  w = alpha * T over the (pixel, Gaussian) pairs the frame's forward call blended
 * (the depth pass's predicate, with the forward call's own decisions, alpha and T), computed as A Q' - D'^2 of the CENTRED moments
 *   A = sum w,  D' = sum w u,  Q' = sum w u^2,  u_i = v_i - c (one float32 subtraction),  c = the v of the pixel's first blended instance:
 * the term is invariant under a shift of v, and centred sums do not cancel where the uncentred A Q - D^2 of a three-channel (1, v, v^2) render does
 * (thin surfaces far from the camera).  Not clamped: >= 0 in exact arithmetic, a last-bit negative value can come out.  A pixel without a
 * contributor gives 0; no background term, no normalisation.
 *   values / means3D / campos, geom_buffer / binning_buffer / image_buffer, R, subpixel_offset, options: as wg_render_depth takes them, with its
 *     checks, its refusals, its WG_ERR_SPECULATION behaviour and its exact_compositing match.
 *   out_distortion: float[H*W], required, fully overwritten.
 *   out_moments: float[4*H*W] or NULL: the planes (A, D', Q', c), fully overwritten, what wg_distortion_grad reads in the frame's backward call.
 * One launch on `stream` over each tile's list up to tile_last; the three buffers are only READ.  No scratch, no allocator, no atomics, no host
 * wait (but for a deferred frame's verdict).  P = 0 or R = 0 zero-fill the outputs and return WG_OK.  Two calls give the same bits.
 * Fields are only ever appended. */
typedef struct wg_distortion_args {
    size_t struct_size;   /* the CALLER's sizeof(wg_distortion_args) */
    int P, R, width, height;
    char *geom_buffer, *binning_buffer, *image_buffer;
    const float* subpixel_offset;   /* the frame's float[H*W*2], or NULL */
    const float* values;            /* [P] or NULL */
    const float* means3D;           /* [P*3], read when values is NULL */
    const float* campos;            /* [3], device, read when values is NULL */
    const wg_call_options* options; /* NULL = WG_CALL_OPTIONS_DEFAULT */
    float* out_distortion;          /* [H*W], fully overwritten */
    float* out_moments;             /* [4*H*W] or NULL, fully overwritten */
    int debug;                      /* 1: synchronise behind the launch and report (as the other calls' debug) */
    void* stream;
} wg_distortion_args;
int wg_render_distortion(const wg_distortion_args* args);

/* ---- the contribution pass: what each Gaussian contributed to a FINISHED frame ----
 * Over the (pixel, Gaussian) pairs the frame's forward call blended (the depth pass's predicate), with w = alpha * T the forward call's own
 * blend weight, bit for bit:
 *   max_weight[g]     the largest w, combined by an unsigned-integer atomic max on the float's bit pattern (w > 0: the bit order is the
 *                     value order);
 *   hits[g]           the number of pairs, a 64-bit integer atomic add;
 *   weight_sum_q32[g] the sum of (unsigned long long)(w * 2^32), each term truncated (so within 2^-32 of w), a 64-bit integer atomic add:
 *                     the summed weight is weight_sum_q32 * 2^-32.
 * Integer atomics commute exactly: two calls give the same bits whatever order the tiles ran in.  A NaN weight counts as a hit, adds 0 to the
 * sum and makes max_weight NaN (its bit pattern is above every finite weight's).  Each of the three outputs may be NULL (not all three).
 *   pixel_mask: float[H*W] or NULL; a pixel whose entry compares equal to 0.0f (-0.0f too) takes no part.
 *   accumulate: 0 = the (non-NULL) arrays are zero-filled on `stream` under this call first; 1 = the pass combines into what an earlier call
 *     or a zero fill left (a sweep over many cameras).  max_weight must not hold negative values or the combination is meaningless.
 *   geom_buffer / binning_buffer / image_buffer, R, subpixel_offset, options: the frame's, as wg_render_depth takes them;
 *     options->exact_compositing must be the frame's (WG_ERR_INVALID_ARGUMENT otherwise).
 * One launch on `stream` (behind up to three memsets with accumulate = 0) over each tile's list up to tile_last, at most three atomics per
 * (tile, Gaussian).  The three buffers are only READ.  No scratch, no allocator, no host wait -- but for a frame of the deferred forward, whose
 * verdict is read first (WG_ERR_SPECULATION: nothing is written).  P = 0 or R = 0: WG_OK after the optional zero fill.
 * WG_ERR_INVALID_ARGUMENT, before any device work: struct_size smaller than the struct, P < 0, R < 0, width or height <= 0, all three outputs
 * NULL, accumulate not 0 or 1, with P > 0 a NULL buffer.  Fields are only ever appended. */
typedef struct wg_contrib_args {
    size_t struct_size;   /* the CALLER's sizeof(wg_contrib_args) */
    int P, R, width, height;
    char *geom_buffer, *binning_buffer, *image_buffer;
    const float* subpixel_offset;        /* the frame's float[H*W*2], or NULL */
    const float* pixel_mask;             /* [H*W] or NULL */
    const wg_call_options* options;      /* NULL = WG_CALL_OPTIONS_DEFAULT */
    float* max_weight;                   /* [P] or NULL */
    unsigned long long* hits;            /* [P] or NULL */
    unsigned long long* weight_sum_q32;  /* [P] or NULL */
    int accumulate;                      /* 0: zero-fill first; 1: combine */
    int debug;                           /* 1: synchronise behind the launch and report (as the other calls' debug) */
    void* stream;
} wg_contrib_args;
int wg_render_contributions(const wg_contrib_args* args);

#ifdef __cplusplus
}
#endif
#endif /* WG_RASTERIZER_H_INCLUDED */
