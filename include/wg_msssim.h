/* wg_msssim.h -- C-ABI of the fused, forward-only multi-scale SSIM map and of ssim_down (the uncertainty model's two metrics).
 *
 * Replaces, as an opt-in for callers, the reference's `msssim()` (wildgaussians/method.py:171-187, with `_ssim_parts`, :138-168)
 * and `ssim_down()` (:126-135), which `UncertaintyModel._compute_losses` calls on every training step on detached images:
 *
 *   msssim     optional area resize to h0 x w0; level 0 contributes luminance * contrast * structure of the 11x11 Gaussian window
 *              (sigma 1.5, zero padding 5; sigma = sqrt(max(sigma_sq, 0)); C1 = 1e-4, C2 = 9e-4, C3 = C2 / 2); while both sides are larger
 *              than min_size the images are 2x2 average-pooled (an odd last row / column is dropped) and the level contributes its contrast
 *              and its structure map, each upsampled bilinearly (align_corners = False) to h0 x w0; the product of all maps per channel
 *              is optionally upsampled bilinearly to H x W; the channel mean is the result.
 *   ssim_down  optional area resize to h0 x w0 (which may be LARGER than H x W), the product-form SSIM of wg_ssim.h, its channel mean,
 *              optionally upsampled bilinearly to H x W.
 *
 * The caller computes h0 x w0 (the reference does it in Python doubles: floor(H * scale)); the "area" resize is adaptive average pooling
 * with the window [floor(i * in / out), ceil((i + 1) * in / out)).  No gradient is defined.  No atomics: a repeated call is bit-identical.
 * Launches: msssim = levels + 3 (resize, one stencil per level, combine, finish; the resize is skipped when resize == 0 and the combine
 * when there is one level), ssim_down = 3 (resize, SSIM, finish; 2 without the resize).
 * Layout: planar float32 [B, C, H, W], device pointers, explicit HIP stream; `scratch` is caller-provided (the library never allocates).
 * Returns 0 or a negative wg_status (wg_rasterizer.h).
 */
#ifndef WG_MSSSIM_H
#define WG_MSSSIM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Number of pyramid levels of an h0 x w0 level-0 image (>= 1), or 0 for invalid arguments (a size < 1, min_size < 1). */
int wg_msssim_levels(int h0, int w0, int min_size);

/* Floats `scratch` must hold for wg_msssim_forward with the same arguments (0 for invalid arguments): the resized images, every coarser
 * level's pooled images and its two maps, the level-0 map and the per-channel product. */
size_t wg_msssim_scratch_floats(int B, int C, int H, int W, int h0, int w0, int min_size);

/* x, y [B*C*H*W]; out [B*H*W].  resize != 0: x and y are area-resized to h0 x w0 first (the reference's `if max_size is not None`);
 * resize == 0 requires h0 == H and w0 == W.  final_upsample != 0: the per-channel product is upsampled bilinearly to H x W before the
 * channel mean (the reference's second `if max_size is not None`, taken even at scale 1); final_upsample == 0 requires h0 == H, w0 == W. */
int wg_msssim_forward(int B, int C, int H, int W, int h0, int w0, int resize, int final_upsample, int min_size, const float* x,
                      const float* y, float* scratch, float* out, void* stream);

/* Floats `scratch` must hold for wg_ssim_down_forward (0 for invalid arguments): the resized images and the per-channel SSIM map. */
size_t wg_ssim_down_scratch_floats(int B, int C, int h0, int w0);

/* x, y [B*C*H*W]; out [B*H*W].  resize != 0: area resize to h0 x w0, SSIM there, channel mean, bilinear upsampling to H x W;
 * resize == 0 (h0 == H, w0 == W required): the channel mean of the SSIM map. */
int wg_ssim_down_forward(int B, int C, int H, int W, int h0, int w0, int resize, const float* x, const float* y, float* scratch,
                         float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
