/* wg_lpips.h -- C-ABI of the fused LPIPS v0.1 (AlexNet and VGG16 trunks): what `evaluation._lpips` (wildgaussians/evaluation.py:255-291) asks
 * of `LPIPS.forward` (wildgaussians/_metrics_lpips.py:149-180) with lpips=True, spatial=False, forward only, float32 throughout.
 *
 * Covered trunks, exactly as _metrics_lpips.py:286-364 slices them; a tap is taken after the ReLU that ends each slice:
 *
 *   WG_LPIPS_ALEX   conv 3->64 k11 s4 p2 | pool 3 s2, conv 64->192 k5 p2 | pool 3 s2, conv 192->384 k3 p1 | conv 384->256 k3 p1 |
 *                   conv 256->256 k3 p1                                              (5 convolutions; H, W >= 31)
 *   WG_LPIPS_VGG    64, 64 | pool 2 s2, 128, 128 | pool 2 s2, 256, 256, 256 | pool 2 s2, 512, 512, 512 | pool 2 s2, 512, 512, 512
 *                   (13 convolutions k3 p1; H, W >= 16)
 *
 * Every convolution is followed by ReLU; pools floor and do not pad.  The predicted and the true images go through the trunk as ONE batch of
 * 2 B (images 0..B-1 the first argument's, B..2B-1 the second's), channels-last: activations are [2B, h, w, C].
 *
 * Weights.  conv_w[i] is the i-th convolution's weight REPACKED as [Cout][KH][KW][Cin], each row padded with zeros to Kpad = the next multiple
 * of 4 of K = KH KW Cin (only the first layers pad: 363 -> 364, 27 -> 28); conv_b[i] is [Cout]; lin_w[l] is tap l's 1x1 `lin` weight, [C_l].
 *
 * First layer.  Each image is read in place through (pointer, batch stride and three strides, in floats), as wg_metrics.h describes images: a
 * planar [B, 3, H, W] tensor and a pixel-major [B, H, W, 3] array are both read without a copy.  On load the caller's float32 operations are
 * applied in the caller's order, each rounded on its own: clip to [0, 1] (NaN stays NaN), * 2, - 1, - shift[c], / scale[c] (a correctly rounded
 * division).  The convolution's zero padding applies AFTER this scaling.
 *
 * Arithmetic.  A convolution is an implicit GEMM, M = 2B OH OW output pixels x N = Cout x K = KH KW Cin, every product a chain of
 * v_mfma_f32_32x32x2_f32 in ascending k = (ky, kx, ci); padding taps contribute exactly 0; bias and ReLU in the epilogue.  No value depends on
 * where its pixel lies in a tile: image b of a batch gives the bits of the single call.  Head, per tap and pixel over the C channels of both
 * images: n = sqrt(sum f^2), g = f / (n + 1e-10), sum_c lin[c] (g0 - g1)^2 in float32; pixels are then added in float64, one partial per
 * workgroup of WG_LPIPS_HEAD_PIXELS pixels of one image, the partials in a fixed order by a finishing launch, divided by h_l w_l, and the five
 * layers summed.  No reduced-precision path, no atomics: two calls give the same bits.
 *
 * Host contract: device pointers, an explicit HIP stream, no host synchronisation, no allocation, nothing that prevents stream capture.
 * Every call returns 0 or a negative wg_status (wg_rasterizer.h).  A malformed call -- a struct_size that does not cover the fields, a NULL
 * required pointer, an unknown net, H or W below the trunk's minimum, B < 1, a scratch that is too small or not 16-byte aligned, sizes whose
 * index arithmetic would leave 31 bits -- is refused with WG_ERR_INVALID_ARGUMENT before any device work.
 */
#ifndef WG_LPIPS_H
#define WG_LPIPS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WG_LPIPS_ALEX 0
#define WG_LPIPS_VGG 1
#define WG_LPIPS_TAPS 5
#define WG_LPIPS_MAX_CONVS 13
#define WG_LPIPS_ALEX_MIN_SIDE 31
#define WG_LPIPS_VGG_MIN_SIDE 16
#define WG_LPIPS_HEAD_PIXELS 256     /* pixels of one image per workgroup of the head, i.e. per float64 partial */

/* Images [B, 3, H, W]: element (b, c, y, x) lies b * batch_stride + y * row_stride + x * pixel_stride + c * channel_stride FLOATS after
 * `data`.  Strides are non-negative. */
typedef struct wg_lpips_image {
    const float* data;
    int64_t batch_stride, row_stride, pixel_stride, channel_stride;
} wg_lpips_image;

typedef struct wg_lpips_args {
    size_t struct_size;      /* the caller's sizeof(wg_lpips_args) */
    int32_t net;             /* WG_LPIPS_ALEX or WG_LPIPS_VGG */
    int32_t B, H, W;
    wg_lpips_image in0, in1; /* values in [0, 1] (clipped on load) */
    const float* shift;      /* [3] each: the ScalingLayer's buffers */
    const float* scale;
    const float* conv_w[WG_LPIPS_MAX_CONVS];   /* the first 5 (alex) or 13 (vgg) are read; 16-byte aligned */
    const float* conv_b[WG_LPIPS_MAX_CONVS];
    const float* lin_w[WG_LPIPS_TAPS];
    float* scratch;          /* 16-byte aligned */
    int64_t scratch_floats;  /* what `scratch` holds */
    float* out;              /* [B] */
    float* per_layer;        /* [B, 5], or NULL */
    void* stream;
} wg_lpips_args;

/* Floats of scratch of wg_lpips = 2 A + 2 P.  A = the trunk's largest activation, 2 B * 64 * oh * ow floats, with (oh, ow) = (H, W) for vgg and
 * ((H - 7) / 4 + 1, (W - 7) / 4 + 1) for alex: two ping-pong buffers (every stage reads one and writes the other).  P = B * sum over the five
 * taps of ceil(h_l w_l / WG_LPIPS_HEAD_PIXELS): the head's float64 partials (two floats each).  A 1600x1200 pair on vgg needs 2 * 245.76 M
 * floats, 1.97 GB.  Host arithmetic only; WG_ERR_INVALID_ARGUMENT for an unknown net, B < 1 or a side under the minimum, WG_ERR_OVERFLOW when
 * A or the count of input values, 6 B H W, leaves 31 bits (such a call is refused by wg_lpips too). */
int64_t wg_lpips_scratch_floats(int32_t net, int32_t B, int32_t H, int32_t W);

/* out[b] = LPIPS(in0[b], in1[b]); per_layer[b, l] = layer l's spatial average. */
int wg_lpips(const wg_lpips_args* args);

/* ---- the stages alone (tests, feature extraction) ---- */

typedef struct wg_lpips_conv_args {
    size_t struct_size;
    int32_t N, IH, IW;       /* N images of IH x IW */
    int32_t Cin, Cout;       /* Cin 3 or a multiple of 64; Cout a multiple of 64 */
    int32_t K, stride, pad;  /* a K x K window, K = 1..11, stride >= 1, 0 <= pad < K */
    const float* x;          /* [N, IH, IW, Cin] channels-last; or NULL: the input is images (Cin = 3), scaled on load as described above */
    wg_lpips_image in0;      /* x == NULL: images 0 .. N0 - 1 */
    wg_lpips_image in1;      /* x == NULL: images N0 .. N - 1 (not read when N0 == N) */
    int32_t N0;
    const float* shift;      /* x == NULL: [3] each */
    const float* scale;
    const float* w;          /* [Cout][K][K][Cin] padded to rows of Kpad floats; 16-byte aligned */
    const float* bias;       /* [Cout] */
    float* y;                /* [N, OH, OW, Cout], OH = (IH + 2 pad - K) / stride + 1; must not overlap x */
    void* stream;
} wg_lpips_conv_args;

/* y = relu(conv(x, w) + bias). */
int wg_lpips_conv(const wg_lpips_conv_args* args);

/* Max pool, window x window, stride 2, floor, no padding: x [N, IH, IW, C] -> y [N, (IH - window) / 2 + 1, (IW - window) / 2 + 1, C], both
 * channels-last.  window 2 or 3, C a multiple of 4, IH, IW >= window.  NaN propagates. */
int wg_lpips_pool(const float* x, int32_t N, int32_t IH, int32_t IW, int32_t C, int32_t window, float* y, void* stream);

/* One tap's head: f [2 B, h, w, C] channels-last (images b and B + b are compared), lin [C] -> out[b] = the tap's spatial average, as float32.
 * C a multiple of 64, at most 512.  partials: 8-byte aligned device memory of B * ceil(h w / WG_LPIPS_HEAD_PIXELS) doubles. */
int wg_lpips_head(const float* f, int32_t B, int32_t h, int32_t w, int32_t C, const float* lin, double* partials, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
