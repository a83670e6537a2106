/* wg_metrics.h -- C-ABI of the fused evaluation metrics: what the reference computes per test image on the host
 * (wildgaussians/evaluation.py:156-234 behind compute_metrics :331-352, after render() :1832-1866 and image_to_srgb utils.py:130-151),
 * on the device.
 *
 *   wg_frame_quantize   float32 planar [C, HW] -> uint8 pixel-major [HW, C] with the BITS of the reference's chain
 *                       torch.clamp(x, 0, 1).nan_to_num_(0) -> np.clip(x * 255.0, 0, 255).astype(np.uint8): one float32 multiplication by 255.0f
 *                       and a truncation.  NaN -> 0, +inf -> 255, -inf, negatives and -0.0 -> 0.
 *   wg_image_metrics    MSE, MAE and the mean SSIM (dm_pix's: an 11-tap Gaussian over "valid" windows) of one image pair over a rectangle,
 *                       as three doubles.  Values are float32 and so are a*a, b*b, a*b, a-b and (a-b)^2, as in NumPy; the filtering and all
 *                       that follows is float64, as in the reference, whose float64 taps promote np.convolve's result.  One partial triple
 *                       per workgroup, added in a fixed order by a finishing launch: no float atomics, two calls give the same bits.
 *
 * Device pointers (the taps are a HOST array), an explicit HIP stream, no allocation.  Returns 0 or a negative wg_status (wg_rasterizer.h);
 * invalid arguments are refused before any device work.
 */
#ifndef WG_METRICS_H
#define WG_METRICS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WG_METRICS_TAPS 11          /* the window; a rectangle must be at least this high and wide */
#define WG_METRICS_MAX_SIDE 32768   /* H and W of an image */

enum wg_image_kind {
    WG_IMAGE_U8 = 0,         /* uint8: value = (float)byte / 255.0f, one correctly rounded float32 division */
    WG_IMAGE_F32 = 1,        /* float32: value = min(max(x, 0), 1) (NaN stays NaN, as np.clip leaves it) */
    WG_IMAGE_F32_RENDER = 2  /* float32, a raw render: quantised as wg_frame_quantize does, then read as WG_IMAGE_U8 */
};

/* One image: element (y, x, c) lies `y * row_stride + x * pixel_stride + c * channel_stride` ELEMENTS (bytes for U8, floats otherwise) after
 * `data`.  A planar [C, H, W] tensor has strides (W, 1, H * W), a pixel-major [H, W, C'] array (C' >= C) has (W * C', C', 1). */
typedef struct wg_image_desc {
    const void* data;
    int32_t kind;
    int32_t reserved;   /* 0 */
    int64_t row_stride, pixel_stride, channel_stride;
} wg_image_desc;

/* src [C, HW] float32, contiguous -> dst [HW, C] uint8.  C = 1..4. */
int wg_frame_quantize(int C, size_t HW, const float* src, uint8_t* dst, void* stream);

/* Bytes `scratch` of wg_image_metrics must hold for a rectangle of h x w pixels and C channels (0 for invalid sizes). */
size_t wg_image_metrics_scratch_bytes(int C, int h, int w);

/* out[3] = {mse, mae, ssim} of images a and b, both H x W with C channels, over rows y0 .. y1 - 1 and columns x0 .. x1 - 1 (both images
 * cropped first).  taps: WG_METRICS_TAPS doubles on the HOST; c1, c2: SSIM's constants.  scratch: 8-byte aligned device memory of
 * wg_image_metrics_scratch_bytes(C, y1 - y0, x1 - x0) bytes; out: 8-byte aligned device memory.  Refused: C outside 1..4, a side above
 * WG_METRICS_MAX_SIDE, a rectangle outside the image or with a side under WG_METRICS_TAPS, a null pointer, an unknown kind, a negative stride. */
int wg_image_metrics(const wg_image_desc* a, const wg_image_desc* b, int H, int W, int C, int y0, int y1, int x0, int x1, const double* taps,
                     double c1, double c2, void* scratch, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
