/* wg_step_loss.h -- C-ABI of the fused train-step image loss with mask, multiplier schedule and every logged metric.
 *
 * Replaces, as an opt-in for callers, the block of the reference's train_iteration between the render and loss.backward() and the logging
 * block behind it (wildgaussians/method.py:1920-1992), for the default configuration (uncertainty_scale_grad and uncertainty_center_mult off):
 *
 *     image, image_toned = scale_grads(image, mask), scale_grads(image_toned, mask)          # gradients * mask; value unchanged
 *     loss_mult = (loss_mult > 1); 1 before the warm-up; 1 + p * (loss_mult - 1) during it   # the effective multiplier m
 *     loss = (1 - lambda) * mean(|image_toned - gt| * m) + lambda * mean((1 - ssim(image, gt)) * m)
 *     l1_loss, ssim, mse, psnr, mask_percentage, ssim_masked, mse_masked, psnr_masked, l1_loss_masked
 *
 * Two launches forward (the 32x16-tile SSIM stencil with nine partial sums per workgroup, then a one-workgroup finishing kernel), one
 * backward.  No float atomics: per-workgroup partial sums go to `scratch` and are added in workgroup order in float64, so a repeated call
 * gives the same bits.  Layout: planar float32 [C, H, W] images, [H*W] mask and multiplier, device pointers, explicit HIP stream.
 * Returns 0 or a negative wg_status (wg_rasterizer.h); every argument check is made before any launch.
 *
 * The effective multiplier of a pixel, in float32 and in this order (the bits of the reference's tensors):
 *     m = mult ? mult[p] : 1
 *     if threshold_enabled:  m = (m > mult_threshold) ? 1 : 0          (NaN gives 0, as `>` does)
 *     if mult_blend != 1:    m = 1 + mult_blend * (m - 1)              (mult_blend = 0: exactly 1; 0 < mult_blend < 1: the warm-up)
 * threshold_enabled = 0 with mult_blend = 1 passes a ready-made multiplier through untouched.
 *
 * The forward value of scale_grads is taken as the identity: it is that exactly for 0/1 masks and within one float32 rounding otherwise.
 */
#ifndef WG_STEP_LOSS_H
#define WG_STEP_LOSS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* stats[WG_STEP_STATS] (float64, device).  With S over all C*H*W elements, d = img_l1 - gt, s = the SSIM value of img_ssim against gt:
 * the five masked entries are NaN without a mask; an all-zero mask gives NaN (0/0) in the four ratios; mse == 0 gives psnr = +inf. */
enum wg_step_stat {
    WG_STEP_LOSS = 0,             /* (1 - lambda) * l1_weighted + lambda * dssim_weighted */
    WG_STEP_L1 = 1,               /* sum |d| / (C*H*W)                 -- "l1_loss" */
    WG_STEP_SSIM = 2,             /* sum s / (C*H*W)                   -- "ssim" */
    WG_STEP_MSE = 3,              /* sum d*d / (C*H*W)                 -- "mse" */
    WG_STEP_PSNR = 4,             /* -10 log10(mse)                    -- "psnr" */
    WG_STEP_L1_WEIGHTED = 5,      /* sum |d| * m / (C*H*W) */
    WG_STEP_DSSIM_WEIGHTED = 6,   /* sum (1 - s) * m / (C*H*W) */
    WG_STEP_MASK_PERCENTAGE = 7,  /* sum mask / (H*W)                  -- "mask_percentage" */
    WG_STEP_SSIM_MASKED = 8,      /* sum s * mask / (C * sum mask)     -- "ssim_masked" (the channel mean, then the masked mean) */
    WG_STEP_MSE_MASKED = 9,       /* sum d*d * mask / sum mask         -- "mse_masked" (all channels summed, NO division by C) */
    WG_STEP_PSNR_MASKED = 10,     /* -10 log10(mse_masked)             -- "psnr_masked" */
    WG_STEP_L1_MASKED = 11,       /* sum |d| * mask / sum mask         -- "l1_loss_masked" (as mse_masked) */
    WG_STEP_STATS = 12
};

/* Number of float32 words `scratch` must hold (nine float64 partial sums per workgroup); 0 for sizes the operator refuses. */
size_t wg_step_loss_scratch_floats(int C, int H, int W);

/* img_l1 (the appearance-toned render), img_ssim (the raw one; may be the same pointer), gt: [C*H*W].  mask, mult: [H*W] or NULL.
 * scratch: wg_step_loss_scratch_floats(C, H, W) floats, 8-byte aligned.  loss_out: one float32 (for autograd).  stats: WG_STEP_STATS float64.
 * dm_dmu1, dm_dsigma1_sq, dm_dsigma12 [C*H*W]: all three (a backward call will follow) or none. */
int wg_step_loss_forward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mask,
                         const float* mult, int threshold_enabled, float mult_threshold, float mult_blend, double lambda, float* scratch,
                         float* loss_out, double* stats, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);

/* dL_dloss is a DEVICE scalar (autograd's grad_output).  dL_dimg_l1 and dL_dimg_ssim [C*H*W] are overwritten; pass the same pointer for
 * both exactly when img_l1 == img_ssim, and the two terms' gradients are summed into it.  Both gradients are multiplied by mask[pixel]
 * when a mask is given (all that scale_grads does to a gradient); the effective multiplier is recomputed, not read. */
int wg_step_loss_backward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mask,
                          const float* mult, int threshold_enabled, float mult_threshold, float mult_blend, double lambda,
                          const float* dL_dloss, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                          float* dL_dimg_l1, float* dL_dimg_ssim, void* stream);

#ifdef __cplusplus
}
#endif
#endif
