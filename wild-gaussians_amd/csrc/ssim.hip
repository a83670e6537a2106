// Fused SSIM map, forward and backward, for gfx950 (include/wg_ssim.h); below it, the forward-only msssim / ssim_down
// of the uncertainty path (include/wg_msssim.h).
// Reference semantics: wildgaussians/method.py:644-673 -- depthwise 11x11 Gaussian window (sigma 1.5, normalised 1-D
// taps, outer product), zero padding 5, C1 = 0.01^2, C2 = 0.03^2.
//
// HBM-bound stencil: the forward pass reads 8 B and writes 16 B per (channel, pixel), the backward pass reads 24 B and
// writes 4 B; everything in between lives in LDS.  One 256-thread workgroup owns a 32x16 output tile of one channel:
//   1. the 42x26 halo of both images goes to LDS (zero outside the frame = the reference's zero padding);
//   2. horizontal pass: the five running sums (x, y, xx, yy, xy) of the 11 taps for 26 rows x 32 columns -> LDS;
//   3. vertical pass: 11 taps over those rows -> mu1, mu2, E[xx], E[yy], E[xy] -> SSIM and its three partial derivatives.
// The backward pass is the same separable convolution applied to dL_dmap * (the three derivative maps).
#include <hip/hip_runtime.h>
#include <cmath>
#include <stddef.h>
#include "wg_ssim.h"
#include "wg_msssim.h"
#include "wg_rasterizer.h"

namespace wg {

constexpr int SS_TW = 32, SS_TH = 16, SS_R = 5, SS_K = 11;
constexpr int SS_HW = SS_TW + 2 * SS_R, SS_HH = SS_TH + 2 * SS_R;  // 42 x 26 halo

struct SsimTaps {
    float w[SS_K];
};

// LOSS (include/wg_ssim.h: wg_l1_ssim_loss_*): instead of writing the SSIM map, the workgroup sums (1 - ssim) * mult and
// |img_l1 - img2| * mult over its tile (img2 = the ground truth) and leaves the two partial sums in partials[2 * block]; a second
// tiny kernel adds the partials in block order (deterministic) and forms the reference's loss (method.py:1948-1965).
template <bool LOSS>
__global__ void __launch_bounds__(256) ssim_forward_kernel(int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                                                           float* __restrict__ ssim_map, float* __restrict__ dm_dmu1,
                                                           float* __restrict__ dm_dsigma1_sq, float* __restrict__ dm_dsigma12, SsimTaps taps,
                                                           const float* __restrict__ img_l1, const float* __restrict__ mult,
                                                           float* __restrict__ partials) {
    __shared__ float sx[SS_HH][SS_HW + 1], sy[SS_HH][SS_HW + 1];
    __shared__ float hs[5][SS_HH][SS_TW + 1];
    __shared__ float red[2][4];
    float acc_s = 0.f, acc_l = 0.f;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SS_TW, y0 = blockIdx.y * SS_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    img1 += plane; img2 += plane;
    for (int i = tid; i < SS_HH * SS_HW; i += 256) {
        const int ly = i / SS_HW, lx = i % SS_HW;
        const int gy = y0 + ly - SS_R, gx = x0 + lx - SS_R;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[ly][lx] = in ? img1[(size_t)gy * W + gx] : 0.f;
        sy[ly][lx] = in ? img2[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SS_HH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k], u = sx[ly][lx + k], v = sy[ly][lx + k];
            a += w * u; b += w * v; aa += w * u * u; bb += w * v * v; ab += w * u * v;
        }
        hs[0][ly][lx] = a; hs[1][ly][lx] = b; hs[2][ly][lx] = aa; hs[3][ly][lx] = bb; hs[4][ly][lx] = ab;
    }
    __syncthreads();
    for (int i = tid; i < SS_TH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k];
            mu1 += w * hs[0][ly + k][lx]; mu2 += w * hs[1][ly + k][lx];
            e11 += w * hs[2][ly + k][lx]; e22 += w * hs[3][ly + k][lx]; e12 += w * hs[4][ly + k][lx];
        }
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
        const float A = 2.f * mu12 + C1, B = 2.f * s12 + C2, Cc = mu1_sq + mu2_sq + C1, D = s1 + s2 + C2;
        const size_t o = plane + (size_t)gy * W + gx;
        const float m = (A * B) / (Cc * D);
        if (LOSS) {
            const float wgt = mult ? mult[(size_t)gy * W + gx] : 1.0f;
            acc_s += (1.0f - m) * wgt;
            acc_l += fabsf(img_l1[o] - sy[ly + SS_R][lx + SS_R]) * wgt;
        } else {
            ssim_map[o] = m;
        }
        if (dm_dmu1) {
            // total derivative w.r.t. mu1, including sigma1_sq = E[xx] - mu1^2 and sigma12 = E[xy] - mu1*mu2
            const float iCD = 1.f / (Cc * D);
            dm_dmu1[o] = 2.f * mu2 * B * iCD - 2.f * mu2 * A * iCD - 2.f * mu1 * A * B / (Cc * Cc * D) + 2.f * mu1 * A * B / (Cc * D * D);
            dm_dsigma1_sq[o] = -A * B / (Cc * D * D);
            dm_dsigma12[o] = 2.f * A * iCD;
        }
    }
    if (LOSS) {  // workgroup sum in a fixed order: lanes (xor butterfly), then the four waves
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            acc_s += __shfl_xor(acc_s, d);
            acc_l += __shfl_xor(acc_l, d);
        }
        if ((tid & 63) == 0) { red[0][tid >> 6] = acc_s; red[1][tid >> 6] = acc_l; }
        __syncthreads();
        if (tid == 0) {
            const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            partials[2 * b] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
            partials[2 * b + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        }
    }
}

// loss_out = { (1 - lambda) * l1_mean + lambda * dssim_mean, l1_mean, ssim_mean } from the per-workgroup partial sums
__global__ void __launch_bounds__(1024) l1_ssim_finish_kernel(const float* __restrict__ partials, int nblocks, float inv_count, float lambda,
                                                              float* __restrict__ loss_out) {
    __shared__ double red[2][16];
    double s = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 1024) { s += partials[2 * i]; l += partials[2 * i + 1]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_xor(s, d);
        l += __shfl_xor(l, d);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = l; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0; l = 0.0;
        for (int w = 0; w < 16; w++) { s += red[0][w]; l += red[1][w]; }
        const float dssim = (float)(s * inv_count), l1 = (float)(l * inv_count);
        loss_out[0] = (1.0f - lambda) * l1 + lambda * dssim;
        loss_out[1] = l1;
        loss_out[2] = 1.0f - dssim;   // mean SSIM when mult == 1 (what the reference logs, method.py:1972)
    }
}

// dL_dimg1(q) = sum_p w(p - q) g(p) [ dm_dmu1(p) + 2 img1(q) dm_dsigma1_sq(p) + img2(q) dm_dsigma12(p) ]
// LOSS: dL_dmap is not a tensor but  -lambda * inv_count * (*dL_dloss) * mult[pixel]  (the loss is lambda * mean((1 - ssim) mult)),
// and the L1 branch's gradient  (1 - lambda) * inv_count * (*dL_dloss) * mult * sign(img_l1 - img2)  is written alongside.
template <bool LOSS>
__global__ void __launch_bounds__(256) ssim_backward_kernel(int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                                                            const float* __restrict__ dL_dmap, const float* __restrict__ dm_dmu1,
                                                            const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12,
                                                            float* __restrict__ dL_dimg1, SsimTaps taps, const float* __restrict__ img_l1,
                                                            const float* __restrict__ mult, const float* __restrict__ dL_dloss, float lambda,
                                                            float inv_count, float* __restrict__ dL_dimg_l1) {
    const float gl = LOSS ? dL_dloss[0] * inv_count : 0.f;
    __shared__ float t[3][SS_HH][SS_HW + 1];
    __shared__ float hs[3][SS_HH][SS_TW + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SS_TW, y0 = blockIdx.y * SS_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    for (int i = tid; i < SS_HH * SS_HW; i += 256) {
        const int ly = i / SS_HW, lx = i % SS_HW;
        const int gy = y0 + ly - SS_R, gx = x0 + lx - SS_R;
        float a = 0.f, b = 0.f, c = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = plane + (size_t)gy * W + gx;
            const float g = LOSS ? -lambda * gl * (mult ? mult[(size_t)gy * W + gx] : 1.0f) : dL_dmap[o];
            a = g * dm_dmu1[o]; b = g * dm_dsigma1_sq[o]; c = g * dm_dsigma12[o];
        }
        t[0][ly][lx] = a; t[1][ly][lx] = b; t[2][ly][lx] = c;
    }
    __syncthreads();
    for (int i = tid; i < SS_HH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k];
            a += w * t[0][ly][lx + k]; b += w * t[1][ly][lx + k]; c += w * t[2][ly][lx + k];
        }
        hs[0][ly][lx] = a; hs[1][ly][lx] = b; hs[2][ly][lx] = c;
    }
    __syncthreads();
    for (int i = tid; i < SS_TH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k];
            a += w * hs[0][ly + k][lx]; b += w * hs[1][ly + k][lx]; c += w * hs[2][ly + k][lx];
        }
        const size_t o = plane + (size_t)gy * W + gx;
        const float gt = img2[o];
        const float gs = a + 2.f * img1[o] * b + gt * c;
        if (LOSS) {
            const float d = img_l1[o] - gt;
            const float gl1 = (1.0f - lambda) * gl * (mult ? mult[(size_t)gy * W + gx] : 1.0f) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
            if (dL_dimg_l1 == dL_dimg1) {  // one image feeds both terms: a single gradient
                dL_dimg1[o] = gs + gl1;
            } else {
                dL_dimg1[o] = gs;
                dL_dimg_l1[o] = gl1;
            }
        } else {
            dL_dimg1[o] = gs;
        }
    }
}

static SsimTaps make_taps() {  // method.py:648-649: exp(-(x - 5)^2 / (2 sigma^2)), normalised, in float32 like torch.Tensor
    SsimTaps t;
    float sum = 0.f;
    for (int k = 0; k < SS_K; k++) {
        t.w[k] = (float)std::exp(-(double)((k - SS_R) * (k - SS_R)) / (2.0 * 1.5 * 1.5));
        sum += t.w[k];
    }
    for (int k = 0; k < SS_K; k++) t.w[k] /= sum;
    return t;
}

}  // namespace wg

extern "C" {

int wg_ssim_forward(int C, int H, int W, const float* img1, const float* img2, float* ssim_map, float* dm_dmu1,
                    float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !ssim_map) return WG_ERR_INVALID_ARGUMENT;
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr)) return WG_ERR_INVALID_ARGUMENT;
    const dim3 grid((W + wg::SS_TW - 1) / wg::SS_TW, (H + wg::SS_TH - 1) / wg::SS_TH, C);
    hipLaunchKernelGGL(wg::ssim_forward_kernel<false>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H, W, img1, img2, ssim_map,
                       dm_dmu1, dm_dsigma1_sq, dm_dsigma12, wg::make_taps(), (const float*)nullptr, (const float*)nullptr, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

int wg_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* dL_dmap, const float* dm_dmu1,
                     const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dL_dmap || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return WG_ERR_INVALID_ARGUMENT;
    const dim3 grid((W + wg::SS_TW - 1) / wg::SS_TW, (H + wg::SS_TH - 1) / wg::SS_TH, C);
    hipLaunchKernelGGL(wg::ssim_backward_kernel<false>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H, W, img1, img2, dL_dmap,
                       dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, wg::make_taps(), (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, 0.f, 0.f, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

size_t wg_l1_ssim_loss_scratch_floats(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * (size_t)((W + wg::SS_TW - 1) / wg::SS_TW) * (size_t)((H + wg::SS_TH - 1) / wg::SS_TH) * (size_t)C;
}

int wg_l1_ssim_loss_forward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mult,
                            float lambda, float* scratch, float* loss_out, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                            void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img_l1 || !img_ssim || !gt || !scratch || !loss_out) return WG_ERR_INVALID_ARGUMENT;
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr)) return WG_ERR_INVALID_ARGUMENT;
    const dim3 grid((W + wg::SS_TW - 1) / wg::SS_TW, (H + wg::SS_TH - 1) / wg::SS_TH, C);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wg::ssim_forward_kernel<true>, grid, dim3(256), 0, st, H, W, img_ssim, gt, (float*)nullptr, dm_dmu1, dm_dsigma1_sq,
                       dm_dsigma12, wg::make_taps(), img_l1, mult, scratch);
    hipLaunchKernelGGL(wg::l1_ssim_finish_kernel, dim3(1), dim3(1024), 0, st, scratch, (int)(grid.x * grid.y * grid.z),
                       1.0f / ((float)C * (float)H * (float)W), lambda, loss_out);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

int wg_l1_ssim_loss_backward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mult,
                             float lambda, const float* dL_dloss, const float* dm_dmu1, const float* dm_dsigma1_sq,
                             const float* dm_dsigma12, float* dL_dimg_l1, float* dL_dimg_ssim, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || !img_l1 || !img_ssim || !gt || !dL_dloss || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 ||
        !dL_dimg_l1 || !dL_dimg_ssim)
        return WG_ERR_INVALID_ARGUMENT;
    if ((img_l1 == img_ssim) != (dL_dimg_l1 == dL_dimg_ssim)) return WG_ERR_INVALID_ARGUMENT;  // one image <-> one gradient
    const dim3 grid((W + wg::SS_TW - 1) / wg::SS_TW, (H + wg::SS_TH - 1) / wg::SS_TH, C);
    hipLaunchKernelGGL(wg::ssim_backward_kernel<true>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H, W, img_ssim, gt,
                       (const float*)nullptr, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg_ssim, wg::make_taps(), img_l1, mult, dL_dloss, lambda,
                       1.0f / ((float)C * (float)H * (float)W), dL_dimg_l1);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// Fused multi-scale SSIM map and ssim_down, forward only (include/wg_msssim.h).  In this file because it shares the tile, the taps and
// ssim_forward_kernel with the code above.
// Reference semantics: wildgaussians/method.py:126-187 -- `ssim_down`, `_ssim_parts`, `msssim`, as UncertaintyModel._compute_losses calls
// them on detached images every training step.
//
// msssim in levels + 3 launches:
//   1. area_resize_pair_kernel: the adaptive-average ("area") resize of BOTH images to the level-0 size;
//   2. msssim_level_kernel, once per level: the 32x16 tile / 42x26 LDS halo / separable 11-tap stencil of ssim_forward_kernel over the five sums;
//      level 0 writes luminance * contrast * structure, a coarser level its contrast and its structure map; every level but the last also
//      writes the next level's 2x2-pooled images from the tile it already holds (the tile origin is even: a pooled pixel never straddles tiles);
//   3. msssim_combine_kernel: at level-0 resolution, the level-0 map times the bilinear samples of every coarser level's two maps;
//   4. msssim_finish_kernel: the final bilinear upsampling fused with the channel mean.
// ssim_down in 3: the same resize, ssim_forward_kernel (the product form), the finish kernel (channel mean first, then the upsampling, as the reference
// orders them).  No atomics anywhere: every output element is written by exactly one thread, so a repeated call is bit-identical.
namespace wg {
namespace {

constexpr int MS_MAX_LEVELS = 32;                                   // an int side halves at most 31 times
constexpr int MS_MAX_PLANES = 65535;                                // B * C planes ride in gridDim.z

struct MsPlan {  // level sizes: h[0] x w[0] is level 0
    int n;
    int h[MS_MAX_LEVELS], w[MS_MAX_LEVELS];
};

struct MsCoarse {  // the coarser levels' maps, for the combine kernel (by value in the kernel arguments)
    int n;
    int h[MS_MAX_LEVELS], w[MS_MAX_LEVELS];
    const float* c[MS_MAX_LEVELS];
    const float* s[MS_MAX_LEVELS];
};

// "area" interpolation = adaptive average pooling: output i averages the input window [floor(i*in/out), ceil((i+1)*in/out)).
// One thread per output pixel of one plane, both images; out may be smaller or larger than in.
__global__ void __launch_bounds__(256) area_resize_pair_kernel(int H, int W, int h, int w, const float* __restrict__ x, const float* __restrict__ y,
                                                               float* __restrict__ ox, float* __restrict__ oy) {
    const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (px >= w || py >= h) return;
    const int ys = (int)(((long long)py * H) / h), ye = (int)(((long long)(py + 1) * H + h - 1) / h);
    const int xs = (int)(((long long)px * W) / w), xe = (int)(((long long)(px + 1) * W + w - 1) / w);
    const size_t in_plane = (size_t)blockIdx.z * H * W;
    float a = 0.f, b = 0.f;
    for (int iy = ys; iy < ye; iy++) {
        const size_t row = in_plane + (size_t)iy * W;
        for (int ix = xs; ix < xe; ix++) { a += x[row + ix]; b += y[row + ix]; }
    }
    const float kh = (float)(ye - ys), kw = (float)(xe - xs);
    const size_t o = ((size_t)blockIdx.z * h + py) * w + px;
    ox[o] = a / kh / kw;
    oy[o] = b / kh / kw;
}

// One pyramid level of one plane per 32x16 tile.  FIRST: map_a = luminance * contrast * structure; else map_a = contrast, map_b = structure.
// pool1 / pool2 (both or neither): the next level's images, [planes, H/2, W/2].
template <bool FIRST>
__global__ void __launch_bounds__(256) msssim_level_kernel(int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                                                           float* __restrict__ map_a, float* __restrict__ map_b, float* __restrict__ pool1,
                                                           float* __restrict__ pool2, SsimTaps taps) {
    __shared__ float sx[SS_HH][SS_HW + 1], sy[SS_HH][SS_HW + 1];
    __shared__ float hs[5][SS_HH][SS_TW + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SS_TW, y0 = blockIdx.y * SS_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    img1 += plane; img2 += plane;
    for (int i = tid; i < SS_HH * SS_HW; i += 256) {
        const int ly = i / SS_HW, lx = i % SS_HW;
        const int gy = y0 + ly - SS_R, gx = x0 + lx - SS_R;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[ly][lx] = in ? img1[(size_t)gy * W + gx] : 0.f;
        sy[ly][lx] = in ? img2[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    if (pool1) {  // avg_pool2d(2): 16x8 pooled pixels per image per tile; waves 0-1 take img1, waves 2-3 img2
        const int Hp = H / 2, Wp = W / 2;
        const int t = tid & 127, ply = t >> 4, plx = t & 15;
        const int gy = y0 / 2 + ply, gx = x0 / 2 + plx;
        if (gy < Hp && gx < Wp) {  // then rows 2gy, 2gy+1 < H and columns 2gx, 2gx+1 < W: all four are frame pixels in LDS
            const float(*s)[SS_HW + 1] = tid < 128 ? sx : sy;
            const int ly = 2 * ply + SS_R, lx = 2 * plx + SS_R;
            const float v = (s[ly][lx] + s[ly][lx + 1] + s[ly + 1][lx] + s[ly + 1][lx + 1]) * 0.25f;
            (tid < 128 ? pool1 : pool2)[((size_t)blockIdx.z * Hp + gy) * Wp + gx] = v;
        }
    }
    for (int i = tid; i < SS_HH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k], u = sx[ly][lx + k], v = sy[ly][lx + k];
            a += w * u; b += w * v; aa += w * u * u; bb += w * v * v; ab += w * u * v;
        }
        hs[0][ly][lx] = a; hs[1][ly][lx] = b; hs[2][ly][lx] = aa; hs[3][ly][lx] = bb; hs[4][ly][lx] = ab;
    }
    __syncthreads();
    for (int i = tid; i < SS_TH * SS_TW; i += 256) {
        const int ly = i / SS_TW, lx = i % SS_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const float w = taps.w[k];
            mu1 += w * hs[0][ly + k][lx]; mu2 += w * hs[1][ly + k][lx];
            e11 += w * hs[2][ly + k][lx]; e22 += w * hs[3][ly + k][lx]; e12 += w * hs[4][ly + k][lx];
        }
        // method.py:151-167.  The window variances cancel to about 0 on flat image regions and can come out negative: clamp before sqrt.
        constexpr float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03), C3 = (float)(0.03 * 0.03 / 2);
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
        const float sd1 = sqrtf(fmaxf(s1, 0.f)), sd2 = sqrtf(fmaxf(s2, 0.f));
        const float contrast = (2.f * sd1 * sd2 + C2) / (s1 + s2 + C2);
        const float structure = (s12 + C3) / (sd1 * sd2 + C3);
        const size_t o = plane + (size_t)gy * W + gx;
        if (FIRST) {
            const float luminance = (2.f * mu12 + C1) / (mu1_sq + mu2_sq + C1);
            map_a[o] = luminance * contrast * structure;
        } else {
            map_a[o] = contrast;
            map_b[o] = structure;
        }
    }
}

// Bilinear sampling with align_corners = False: src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out in float32.
struct MsLerp {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ MsLerp ms_lerp(int dst, float scale, int in) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    MsLerp r;
    r.i0 = min((int)src, in - 1);
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

__device__ __forceinline__ float ms_bilinear(const float* __restrict__ p, int w, const MsLerp& ly, const MsLerp& lx) {
    const float* r0 = p + (size_t)ly.i0 * w;
    const float* r1 = p + (size_t)ly.i1 * w;
    return ly.l0 * (lx.l0 * r0[lx.i0] + lx.l1 * r0[lx.i1]) + ly.l1 * (lx.l0 * r1[lx.i0] + lx.l1 * r1[lx.i1]);
}

// prod[plane, y, x] = m0 * prod over coarser levels of bilinear(contrast_l) * bilinear(structure_l), in the reference's order
__global__ void __launch_bounds__(256) msssim_combine_kernel(int h0, int w0, const float* __restrict__ m0, MsCoarse lv, float* __restrict__ prod) {
    const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (px >= w0 || py >= h0) return;
    const size_t o = ((size_t)blockIdx.z * h0 + py) * w0 + px;
    float v = m0[o];
    for (int l = 0; l < lv.n; l++) {
        const int h = lv.h[l], w = lv.w[l];
        const MsLerp ly = ms_lerp(py, (float)h / (float)h0, h), lx = ms_lerp(px, (float)w / (float)w0, w);
        const size_t plane = (size_t)blockIdx.z * h * w;
        v *= ms_bilinear(lv.c[l] + plane, w, ly, lx);
        v *= ms_bilinear(lv.s[l] + plane, w, ly, lx);
    }
    prod[o] = v;
}

// out[b, y, x] = channel mean of maps[b, :, h, w], upsampled bilinearly to H x W when `upsample` (else h == H and w == W).
// MEAN_FIRST: the mean is taken before the upsampling (ssim_down), else after it (msssim).
template <bool MEAN_FIRST>
__global__ void __launch_bounds__(256) msssim_finish_kernel(int C, int h, int w, int H, int W, int upsample, const float* __restrict__ maps,
                                                            float* __restrict__ out) {
    const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (px >= W || py >= H) return;
    const size_t hw = (size_t)h * w;
    const float* base = maps + (size_t)blockIdx.z * C * hw;
    float v = 0.f;
    if (!upsample) {
        for (int c = 0; c < C; c++) v += base[c * hw + (size_t)py * w + px];
        v = v / (float)C;
    } else {
        const MsLerp ly = ms_lerp(py, (float)h / (float)H, h), lx = ms_lerp(px, (float)w / (float)W, w);
        if (MEAN_FIRST) {
            float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
            for (int c = 0; c < C; c++) {
                const float* r0 = base + c * hw + (size_t)ly.i0 * w;
                const float* r1 = base + c * hw + (size_t)ly.i1 * w;
                v00 += r0[lx.i0]; v01 += r0[lx.i1]; v10 += r1[lx.i0]; v11 += r1[lx.i1];
            }
            const float n = (float)C;
            v = ly.l0 * (lx.l0 * (v00 / n) + lx.l1 * (v01 / n)) + ly.l1 * (lx.l0 * (v10 / n) + lx.l1 * (v11 / n));
        } else {
            for (int c = 0; c < C; c++) v += ms_bilinear(base + c * hw, w, ly, lx);
            v = v / (float)C;
        }
    }
    out[((size_t)blockIdx.z * H + py) * W + px] = v;
}

bool make_plan(int h0, int w0, int min_size, MsPlan& p) {  // method.py:180-182
    p.n = 0;
    if (h0 <= 0 || w0 <= 0 || min_size < 1) return false;
    int h = h0, w = w0;
    p.h[p.n] = h; p.w[p.n] = w; p.n++;
    while (h > min_size && w > min_size && p.n < MS_MAX_LEVELS) {
        h /= 2; w /= 2;  // avg_pool2d(2) drops an odd last row / column; h, w > min_size >= 1 keeps both >= 1
        p.h[p.n] = h; p.w[p.n] = w; p.n++;
    }
    return true;
}

bool sizes_ok(int B, int C, int H, int W, int h0, int w0) {
    return B > 0 && C > 0 && H > 0 && W > 0 && h0 > 0 && w0 > 0 && (long long)B * C <= MS_MAX_PLANES;
}

dim3 pixel_grid(int h, int w, int planes) { return dim3((w + 31) / 32, (h + 7) / 8, planes); }
dim3 tile_grid(int h, int w, int planes) { return dim3((w + SS_TW - 1) / SS_TW, (h + SS_TH - 1) / SS_TH, planes); }

}  // namespace
}  // namespace wg

extern "C" {

int wg_msssim_levels(int h0, int w0, int min_size) {
    wg::MsPlan p;
    return wg::make_plan(h0, w0, min_size, p) ? p.n : 0;
}

size_t wg_msssim_scratch_floats(int B, int C, int H, int W, int h0, int w0, int min_size) {
    wg::MsPlan p;
    if (!wg::sizes_ok(B, C, H, W, h0, w0) || !wg::make_plan(h0, w0, min_size, p)) return 0;
    const size_t planes = (size_t)B * C, n0 = planes * h0 * w0;
    size_t total = 2 * n0 + n0;                                                       // resized pair, level-0 map
    for (int l = 1; l < p.n; l++) total += 4 * planes * (size_t)p.h[l] * p.w[l];      // pooled pair, contrast and structure maps
    if (p.n > 1) total += n0;                                                         // per-channel product
    return total;
}

int wg_msssim_forward(int B, int C, int H, int W, int h0, int w0, int resize, int final_upsample, int min_size, const float* x,
                      const float* y, float* scratch, float* out, void* stream) {
    wg::MsPlan p;
    if (!wg::sizes_ok(B, C, H, W, h0, w0) || !wg::make_plan(h0, w0, min_size, p) || !x || !y || !scratch || !out) return WG_ERR_INVALID_ARGUMENT;
    if ((!resize || !final_upsample) && (h0 != H || w0 != W)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int planes = B * C;
    const size_t n0 = (size_t)planes * h0 * w0;
    const wg::SsimTaps taps = wg::make_taps();
    float* cur = scratch;
    const float *lx = x, *ly = y;
    if (resize) {
        hipLaunchKernelGGL(wg::area_resize_pair_kernel, wg::pixel_grid(h0, w0, planes), dim3(256), 0, st, H, W, h0, w0, x, y, cur, cur + n0);
        lx = cur; ly = cur + n0;
    }
    cur += 2 * n0;
    float* m0 = cur;
    cur += n0;
    wg::MsCoarse lv;
    lv.n = p.n - 1;
    for (int l = 0; l < p.n; l++) {
        const bool last = l + 1 == p.n;
        float *nx = nullptr, *ny = nullptr;
        if (!last) {  // the next level's block: pooled pair, then its two maps
            const size_t nn = (size_t)planes * p.h[l + 1] * p.w[l + 1];
            nx = cur; ny = cur + nn;
            lv.h[l] = p.h[l + 1]; lv.w[l] = p.w[l + 1];
            lv.c[l] = cur + 2 * nn; lv.s[l] = cur + 3 * nn;
            cur += 4 * nn;
        }
        const dim3 grid = wg::tile_grid(p.h[l], p.w[l], planes);
        if (l == 0)
            hipLaunchKernelGGL(wg::msssim_level_kernel<true>, grid, dim3(256), 0, st, p.h[0], p.w[0], lx, ly, m0, (float*)nullptr, nx, ny, taps);
        else
            hipLaunchKernelGGL(wg::msssim_level_kernel<false>, grid, dim3(256), 0, st, p.h[l], p.w[l], lx, ly, const_cast<float*>(lv.c[l - 1]),
                               const_cast<float*>(lv.s[l - 1]), nx, ny, taps);
        lx = nx; ly = ny;
    }
    const float* prod = m0;
    if (p.n > 1) {
        hipLaunchKernelGGL(wg::msssim_combine_kernel, wg::pixel_grid(h0, w0, planes), dim3(256), 0, st, h0, w0, (const float*)m0, lv, cur);
        prod = cur;
    }
    hipLaunchKernelGGL(wg::msssim_finish_kernel<false>, wg::pixel_grid(H, W, B), dim3(256), 0, st, C, h0, w0, H, W, final_upsample ? 1 : 0, prod, out);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

size_t wg_ssim_down_scratch_floats(int B, int C, int h0, int w0) {
    if (!wg::sizes_ok(B, C, 1, 1, h0, w0)) return 0;
    return 3 * (size_t)B * C * h0 * w0;
}

int wg_ssim_down_forward(int B, int C, int H, int W, int h0, int w0, int resize, const float* x, const float* y, float* scratch,
                         float* out, void* stream) {
    if (!wg::sizes_ok(B, C, H, W, h0, w0) || !x || !y || !scratch || !out) return WG_ERR_INVALID_ARGUMENT;
    if (!resize && (h0 != H || w0 != W)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int planes = B * C;
    const size_t n0 = (size_t)planes * h0 * w0;
    const float *lx = x, *ly = y;
    if (resize) {
        hipLaunchKernelGGL(wg::area_resize_pair_kernel, wg::pixel_grid(h0, w0, planes), dim3(256), 0, st, H, W, h0, w0, x, y, scratch, scratch + n0);
        lx = scratch; ly = scratch + n0;
    }
    float* map = scratch + 2 * n0;
    const int rc = wg_ssim_forward(planes, h0, w0, lx, ly, map, nullptr, nullptr, nullptr, stream);
    if (rc != WG_OK) return rc;
    hipLaunchKernelGGL(wg::msssim_finish_kernel<true>, wg::pixel_grid(H, W, B), dim3(256), 0, st, C, h0, w0, H, W, resize ? 1 : 0, (const float*)map, out);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // extern "C"
