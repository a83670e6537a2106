/* wg_uncertainty.h -- C-ABI of the fused uncertainty head and DINO loss: everything `UncertaintyModel._compute_losses` does AROUND the frozen
 * backbone in its default mode (wildgaussians/method.py:363-433 with :190-201 and :267-323; uncertainty_mode = "dino",
 * uncertainty_dino_max_size = None, a batch of one).  The backbone itself stays the caller's.
 *
 *   prepare        zero padding of (bilinear(img -> h x w) - mean_c) / std_c to hP x wP: one backbone input
 *   head_stats     per channel c of the feature map x [C, N]: the batch mean and biased variance over the N positions (training) or the running
 *                  statistics (eval), the running-statistics update of F.batch_norm, and dropout2d + batch norm + the 1x1 convolution folded
 *                  into one coefficient a_c and one constant q_c:  logit_p = sum_c a_c x_cp + sum_c q_c + bias + log(e - 1)
 *   head_forward   s_p = softplus(logit_p) (torch's threshold 20) and softplus'(logit_p)
 *   maps_forward   u = max(bilinear(s -> hp P x wp P), clip_min) cropped to H x W at the pads; loss_mult = min(1 / (2 u^2), 3) is written, and six
 *                  per-workgroup partial sums: log u, loss_mult, ssim * loss_mult, sum_c (gt - pred)^2 * loss_mult, ssim, msssim
 *   cosine         cos_p = <a_p, b_p> / (max(|a_p|, eps) max(|b_p|, eps)) over the C channels of two feature maps
 *   dino_loss      dino_part = clip(1 - (cos^ - 0.5) / 0.5, 0, 1) on the nh x nw downsampled grid (cos^: cos upsampled bilinearly to the padded
 *                  downsampled size and cropped), times bilinear(1 / (2 u^2) -> nh x nw) whose four taps are recomputed from s; per-workgroup
 *                  partial sums of the product; dino_part is written for the backward pass
 *   finish         the partials added in a fixed order (in double) -> loss and the six metrics, one vector of 8 floats
 *   maps_backward  dL/ds: the adjoint of both bilinear maps as a gather per cell of s (the clamp passes a gradient where bilinear(s) >= clip_min)
 *   head_backward  dlogit = ds * softplus'; the gradients of conv.weight, conv.bias, bn.weight, bn.bias from sum_p dlogit_p and
 *                  sum_p dlogit_p x_cp.  The features are constants: no batch-statistics backward exists
 *
 * "Bilinear" is F.interpolate(mode = "bilinear", align_corners = False) without antialiasing; its source index (dst + 0.5) in / out - 0.5 is
 * evaluated in integers, so the interpolation weight is rounded once.  The identity resize (in == out) needs no special case.
 * No atomics: every cross-workgroup sum goes through per-workgroup partials added in a fixed order, and a repeated call is bit-identical.
 * Layout: planar float32, device pointers, explicit HIP stream; scratch is caller-provided (the library never allocates).
 * Returns 0 or a negative wg_status (wg_rasterizer.h); invalid arguments (a size < 1, a null required pointer, clip_min <= 0, pads that do
 * not fit, sizes whose index arithmetic would leave 31 bits) are refused before any device work.
 */
#ifndef WG_UNCERTAINTY_H
#define WG_UNCERTAINTY_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* img [C, H, W] -> out [C, hP, wP]: rows pad_top .. pad_top + h - 1 and columns pad_left .. pad_left + w - 1 hold the normalised image resized
 * to h x w (h == H and w == W: no resize), everything else is 0.  mean, std [C] on the device. */
int wg_uncertainty_prepare(int C, int H, int W, int h, int w, int pad_top, int pad_left, int hP, int wP, const float* img, const float* mean,
                           const float* std, float* out, void* stream);

/* x [C, N]; kdrop [C] the dropout2d channel factors (0 or 1 / (1 - p); all 1 in eval).  training != 0 (N >= 2 required): batch statistics
 * m_c = k_c mean, v_c = k_c^2 var; running_mean / running_var [C] are updated with `momentum` (the variance unbiased, N / (N - 1)).
 * training == 0: m, v are the running statistics, which stay unchanged.  coef [2 C] receives a_c then q_c, stats [2 C] m_c then 1 / sqrt(v_c + eps). */
int wg_uncertainty_head_stats(int C, int N, int training, const float* x, const float* kdrop, const float* bn_weight, const float* bn_bias,
                              const float* conv_weight, float eps, float momentum, float* running_mean, float* running_var, float* coef,
                              float* stats, void* stream);

/* s [N], dsdl [N] (softplus' at the logit).  conv_bias [1] on the device. */
int wg_uncertainty_head_forward(int C, int N, const float* x, const float* coef, const float* conv_bias, float* s, float* dsdl, void* stream);

/* ds [N] = dL/ds.  d_bn_weight, d_bn_bias, d_conv_weight [C] and d_conv_bias [1] are written (not accumulated). */
int wg_uncertainty_head_backward(int C, int N, const float* x, const float* ds, const float* dsdl, const float* kdrop, const float* stats,
                                 const float* bn_weight, const float* bn_bias, const float* conv_weight, float* d_bn_weight, float* d_bn_bias,
                                 float* d_conv_weight, float* d_conv_bias, void* stream);

/* Floats `partials` of wg_uncertainty_maps_forward must hold (0 for invalid sizes): six per workgroup. */
size_t wg_uncertainty_maps_scratch_floats(int H, int W);

/* s [hp, wp]; gt, pred [C, H, W]; ssim, msssim, loss_mult [H, W].  P is the patch size: s is upsampled to hp P x wp P and cropped at
 * (pad_top, pad_left); pad_top + H <= hp P and pad_left + W <= wp P are required. */
int wg_uncertainty_maps_forward(int C, int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, const float* s,
                                const float* gt, const float* pred, const float* ssim, const float* msssim, float* loss_mult, float* partials,
                                void* stream);

/* a, b [C, N] -> cos [N]. */
int wg_uncertainty_cosine(int C, int N, float eps, const float* a, const float* b, float* cos, void* stream);

/* Floats `partials` of wg_uncertainty_dino_loss must hold (0 for invalid sizes): one per workgroup. */
size_t wg_uncertainty_dino_scratch_floats(int nh, int nw);

/* cos [hd, wd] is upsampled to hd P x wd P and cropped to nh x nw at (dpad_top, dpad_left); s and the first nine arguments are those of
 * maps_forward; nh x nw is the size dino_downsample gives the frame (nh == H and nw == W: no resize; rounding up to
 * a multiple of 14 can make a side larger than the frame's, and one side may stay while the other shrinks).  dino_part [nh, nw] is written. */
int wg_uncertainty_dino_loss(int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, const float* s, int nh, int nw,
                             int hd, int wd, int dpad_top, int dpad_left, const float* cos, float* dino_part, float* partials, void* stream);

/* result [8]: loss, mean ssim, mean msssim, ssim_discounted, mse_discounted, psnr_discounted, beta, uncertainty_loss. */
int wg_uncertainty_finish(int H, int W, int nh, int nw, float regularizer_weight, const float* maps_partials, const float* dino_partials,
                          float* result, void* stream);

/* ds [hp, wp] = grad_loss[0] * d(uncertainty_loss + regularizer_weight * beta) / ds; grad_loss [1] on the device. */
int wg_uncertainty_maps_backward(int H, int W, int P, int hp, int wp, int pad_top, int pad_left, float clip_min, float regularizer_weight,
                                 const float* s, int nh, int nw, const float* dino_part, const float* grad_loss, float* ds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
