// Fused train-step image loss for gfx950: mask, multiplier schedule, the loss and every logged metric (include/wg_step_loss.h).
// Reference semantics: wildgaussians/method.py:1920-1992 with uncertainty_scale_grad and uncertainty_center_mult off (the defaults).
//
// ssim.hip's loss tile restated (so that ssim.hip compiles as before): one 256-thread workgroup owns a 32x16 output tile of one channel,
//   1. the 42x26 halo of the raw render and the ground truth goes to LDS (zero outside the frame = the reference's zero padding);
//   2. horizontal pass: the five running sums (x, y, xx, yy, xy) of the 11 taps for 26 rows x 32 columns -> LDS;
//   3. vertical pass: 11 taps over those rows -> SSIM and its three partial derivatives;
// and in step 3 every in-frame pixel adds its nine terms (wg_step_loss.h) to the thread's accumulators.
//
// Precision of the sums.  Every TERM is a float32 value with the bits of the reference's tensor element (|d|, d*d, s, their products with the
// float32 multiplier and mask).  Every SUM is float64 from the first addition on: a thread's two pixels, the wave butterfly, the four waves,
// the workgroups.  A float32 thread partial would save nothing (two additions per thread) and would put a rounding of its own between the
// reference's elements and the float64 total; as it is, each statistic is the float64 sum of the reference's float32 elements.
//
// HBM traffic per (channel, pixel): forward reads 12 B (+ 8 B / C of mask and multiplier) and writes 12 B of derivative maps, backward reads
// 24 B and writes 4 or 8 B.  Nothing of size H x W exists besides the inputs, the maps and the gradients.
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include "wg_step_loss.h"
#include "wg_rasterizer.h"

namespace wg {
namespace {

constexpr int SL_TW = 32, SL_TH = 16, SL_R = 5, SL_K = 11;
constexpr int SL_HW = SL_TW + 2 * SL_R, SL_HH = SL_TH + 2 * SL_R;  // 42 x 26 halo
constexpr int SL_SUMS = 9;
constexpr int SL_FINISH_THREADS = 1024;

struct StepTaps {
    float w[SL_K];
};

struct StepMult {  // how the effective multiplier is formed from mult[pixel]
    const float* mult;
    int threshold_enabled;
    float threshold, blend;
};

// The reference's (loss_mult > 1).to(float32) and 1 + p * (loss_mult - 1), each operation rounded on its own: no contraction here, so that
// a ready-made fractional multiplier under a blend also has the bits PyTorch gives it.
__device__ __forceinline__ float effective_mult(const StepMult& sm, size_t pixel) {
#pragma clang fp contract(off)
    float m = sm.mult ? sm.mult[pixel] : 1.0f;
    if (sm.threshold_enabled) m = (m > sm.threshold) ? 1.0f : 0.0f;
    if (sm.blend != 1.0f) {
        const float t = m - 1.0f;
        const float u = sm.blend * t;
        m = 1.0f + u;
    }
    return m;
}

__global__ void __launch_bounds__(256) step_loss_forward_kernel(int H, int W, const float* __restrict__ img_ssim, const float* __restrict__ gt,
                                                                const float* __restrict__ img_l1, const float* __restrict__ mask, StepMult sm,
                                                                float* __restrict__ dm_dmu1, float* __restrict__ dm_dsigma1_sq,
                                                                float* __restrict__ dm_dsigma12, StepTaps taps, double* __restrict__ partials) {
    __shared__ float sx[SL_HH][SL_HW + 1], sy[SL_HH][SL_HW + 1];
    __shared__ float hs[5][SL_HH][SL_TW + 1];
    __shared__ double red[SL_SUMS][4];
    double acc[SL_SUMS];
#pragma unroll
    for (int k = 0; k < SL_SUMS; k++) acc[k] = 0.0;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SL_TW, y0 = blockIdx.y * SL_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float* img1 = img_ssim + plane;
    const float* img2 = gt + plane;
    for (int i = tid; i < SL_HH * SL_HW; i += 256) {
        const int ly = i / SL_HW, lx = i % SL_HW;
        const int gy = y0 + ly - SL_R, gx = x0 + lx - SL_R;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[ly][lx] = in ? img1[(size_t)gy * W + gx] : 0.f;
        sy[ly][lx] = in ? img2[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SL_HH * SL_TW; i += 256) {
        const int ly = i / SL_TW, lx = i % SL_TW;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < SL_K; k++) {
            const float w = taps.w[k], u = sx[ly][lx + k], v = sy[ly][lx + k];
            a += w * u; b += w * v; aa += w * u * u; bb += w * v * v; ab += w * u * v;
        }
        hs[0][ly][lx] = a; hs[1][ly][lx] = b; hs[2][ly][lx] = aa; hs[3][ly][lx] = bb; hs[4][ly][lx] = ab;
    }
    __syncthreads();
    for (int i = tid; i < SL_TH * SL_TW; i += 256) {
        const int ly = i / SL_TW, lx = i % SL_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < SL_K; k++) {
            const float w = taps.w[k];
            mu1 += w * hs[0][ly + k][lx]; mu2 += w * hs[1][ly + k][lx];
            e11 += w * hs[2][ly + k][lx]; e22 += w * hs[3][ly + k][lx]; e12 += w * hs[4][ly + k][lx];
        }
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
        const float A = 2.f * mu12 + C1, B = 2.f * s12 + C2, Cc = mu1_sq + mu2_sq + C1, D = s1 + s2 + C2;
        const size_t pixel = (size_t)gy * W + gx;
        const size_t o = plane + pixel;
        const float s = (A * B) / (Cc * D);
        const float m = effective_mult(sm, pixel);
        const float d = img_l1[o] - sy[ly + SL_R][lx + SL_R];
        const float ad = fabsf(d), dd = d * d, ds = 1.0f - s;
        // each product is rounded to float32 (the reference's tensor element) before it joins a float64 sum
        const float adm = ad * m, dsm = ds * m;
        acc[0] += (double)adm;
        acc[1] += (double)dsm;
        acc[2] += (double)ad;
        acc[3] += (double)s;
        acc[4] += (double)dd;
        if (mask) {
            const float k = mask[pixel];
            const float sk = s * k, ddk = dd * k, adk = ad * k;
            if (blockIdx.z == 0) acc[5] += (double)k;   // counted once per pixel
            acc[6] += (double)sk;
            acc[7] += (double)ddk;
            acc[8] += (double)adk;
        }
        if (dm_dmu1) {
            // total derivative w.r.t. mu1, including sigma1_sq = E[xx] - mu1^2 and sigma12 = E[xy] - mu1*mu2
            const float iCD = 1.f / (Cc * D);
            dm_dmu1[o] = 2.f * mu2 * B * iCD - 2.f * mu2 * A * iCD - 2.f * mu1 * A * B / (Cc * Cc * D) + 2.f * mu1 * A * B / (Cc * D * D);
            dm_dsigma1_sq[o] = -A * B / (Cc * D * D);
            dm_dsigma12[o] = 2.f * A * iCD;
        }
    }
    // workgroup sums in a fixed order: lanes (xor butterfly), then the four waves
#pragma unroll
    for (int k = 0; k < SL_SUMS; k++) {
        double v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if ((tid & 63) == 0) red[k][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < SL_SUMS) {
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[SL_SUMS * b + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }
}

// One workgroup: the nine sums over all workgroups' partials (strided over the threads in workgroup order, butterfly, the sixteen waves: a fixed
// order), then the loss and the statistics of wg_step_loss.h in float64.
__global__ void __launch_bounds__(SL_FINISH_THREADS) step_loss_finish_kernel(const double* __restrict__ partials, int nblocks, double chw, double hw,
                                                                             double channels, double lambda, int has_mask,
                                                                             float* __restrict__ loss_out, double* __restrict__ stats) {
    __shared__ double red[SL_SUMS][SL_FINISH_THREADS / 64];
    double acc[SL_SUMS];
#pragma unroll
    for (int k = 0; k < SL_SUMS; k++) acc[k] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += SL_FINISH_THREADS) {
#pragma unroll
        for (int k = 0; k < SL_SUMS; k++) acc[k] += partials[(size_t)SL_SUMS * i + k];
    }
#pragma unroll
    for (int k = 0; k < SL_SUMS; k++) {
        double v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S[SL_SUMS];
        for (int k = 0; k < SL_SUMS; k++) {
            double v = 0.0;
            for (int w = 0; w < SL_FINISH_THREADS / 64; w++) v += red[k][w];
            S[k] = v;
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const double l1w = S[0] / chw, dsw = S[1] / chw, mse = S[4] / chw;
        const double loss = (1.0 - lambda) * l1w + lambda * dsw;
        loss_out[0] = (float)loss;
        stats[WG_STEP_LOSS] = loss;
        stats[WG_STEP_L1] = S[2] / chw;
        stats[WG_STEP_SSIM] = S[3] / chw;
        stats[WG_STEP_MSE] = mse;
        stats[WG_STEP_PSNR] = -10.0 * log10(mse);
        stats[WG_STEP_L1_WEIGHTED] = l1w;
        stats[WG_STEP_DSSIM_WEIGHTED] = dsw;
        if (has_mask) {
            const double mse_masked = S[7] / S[5];
            stats[WG_STEP_MASK_PERCENTAGE] = S[5] / hw;
            stats[WG_STEP_SSIM_MASKED] = S[6] / (channels * S[5]);
            stats[WG_STEP_MSE_MASKED] = mse_masked;
            stats[WG_STEP_PSNR_MASKED] = -10.0 * log10(mse_masked);
            stats[WG_STEP_L1_MASKED] = S[8] / S[5];
        } else {
            for (int k = WG_STEP_MASK_PERCENTAGE; k <= WG_STEP_L1_MASKED; k++) stats[k] = nan;
        }
    }
}

// ssim.hip's loss backward restated.  With gl = dL_dloss / (C*H*W):
//   dL_dimg_ssim(q) = mask(q) * sum_p w(p - q) g(p) [ dm_dmu1(p) + 2 img_ssim(q) dm_dsigma1_sq(p) + gt(q) dm_dsigma12(p) ],  g(p) = -lambda gl m(p)
//   dL_dimg_l1(q)   = mask(q) * (1 - lambda) gl m(q) sign(img_l1(q) - gt(q))
__global__ void __launch_bounds__(256) step_loss_backward_kernel(int H, int W, const float* __restrict__ img_ssim, const float* __restrict__ gt,
                                                                 const float* __restrict__ img_l1, const float* __restrict__ mask, StepMult sm,
                                                                 const float* __restrict__ dm_dmu1, const float* __restrict__ dm_dsigma1_sq,
                                                                 const float* __restrict__ dm_dsigma12, const float* __restrict__ dL_dloss,
                                                                 float lambda, float count, float* dL_dimg_ssim, float* dL_dimg_l1,
                                                                 StepTaps taps) {  // the two gradients may be one buffer: not __restrict__
    const float gl = dL_dloss[0] / count;
    __shared__ float t[3][SL_HH][SL_HW + 1];
    __shared__ float hs[3][SL_HH][SL_TW + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SL_TW, y0 = blockIdx.y * SL_TH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    for (int i = tid; i < SL_HH * SL_HW; i += 256) {
        const int ly = i / SL_HW, lx = i % SL_HW;
        const int gy = y0 + ly - SL_R, gx = x0 + lx - SL_R;
        float a = 0.f, b = 0.f, c = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t pixel = (size_t)gy * W + gx;
            const size_t o = plane + pixel;
            const float g = -lambda * gl * effective_mult(sm, pixel);
            a = g * dm_dmu1[o]; b = g * dm_dsigma1_sq[o]; c = g * dm_dsigma12[o];
        }
        t[0][ly][lx] = a; t[1][ly][lx] = b; t[2][ly][lx] = c;
    }
    __syncthreads();
    for (int i = tid; i < SL_HH * SL_TW; i += 256) {
        const int ly = i / SL_TW, lx = i % SL_TW;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < SL_K; k++) {
            const float w = taps.w[k];
            a += w * t[0][ly][lx + k]; b += w * t[1][ly][lx + k]; c += w * t[2][ly][lx + k];
        }
        hs[0][ly][lx] = a; hs[1][ly][lx] = b; hs[2][ly][lx] = c;
    }
    __syncthreads();
    for (int i = tid; i < SL_TH * SL_TW; i += 256) {
        const int ly = i / SL_TW, lx = i % SL_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < SL_K; k++) {
            const float w = taps.w[k];
            a += w * hs[0][ly + k][lx]; b += w * hs[1][ly + k][lx]; c += w * hs[2][ly + k][lx];
        }
        const size_t pixel = (size_t)gy * W + gx;
        const size_t o = plane + pixel;
        const float g2 = gt[o];
        float gs = a + 2.f * img_ssim[o] * b + g2 * c;
        const float d = img_l1[o] - g2;
        // (1 - lambda) * gl * m is rounded before the mask multiplies it: with lambda = 0 and gl = 1 the gradient is m * mask, one rounding
        float gl1 = (1.0f - lambda) * gl * effective_mult(sm, pixel) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        if (mask) {
            const float k = mask[pixel];
            gs *= k;
            gl1 *= k;
        }
        if (dL_dimg_l1 == dL_dimg_ssim) {  // one image feeds both terms: a single gradient
            dL_dimg_ssim[o] = gs + gl1;
        } else {
            dL_dimg_ssim[o] = gs;
            dL_dimg_l1[o] = gl1;
        }
    }
}

StepTaps make_step_taps() {  // method.py:648-649: exp(-(x - 5)^2 / (2 sigma^2)), normalised, in float32 like torch.Tensor
    StepTaps t;
    float sum = 0.f;
    for (int k = 0; k < SL_K; k++) {
        t.w[k] = (float)std::exp(-(double)((k - SL_R) * (k - SL_R)) / (2.0 * 1.5 * 1.5));
        sum += t.w[k];
    }
    for (int k = 0; k < SL_K; k++) t.w[k] /= sum;
    return t;
}

// Number of workgroups, or 0 where the sizes are refused: channels ride in gridDim.z, and the finishing kernel counts workgroups in an int.
size_t step_blocks(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0 || C > 65535) return 0;
    const size_t n = (size_t)((W + SL_TW - 1) / SL_TW) * (size_t)((H + SL_TH - 1) / SL_TH) * (size_t)C;
    return n <= (size_t)INT_MAX / SL_SUMS ? n : 0;
}

dim3 step_grid(int C, int H, int W) { return dim3((W + SL_TW - 1) / SL_TW, (H + SL_TH - 1) / SL_TH, C); }

}  // namespace
}  // namespace wg

extern "C" {

size_t wg_step_loss_scratch_floats(int C, int H, int W) { return 2 * wg::SL_SUMS * wg::step_blocks(C, H, W); }

int wg_step_loss_forward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mask,
                         const float* mult, int threshold_enabled, float mult_threshold, float mult_blend, double lambda, float* scratch,
                         float* loss_out, double* stats, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    const size_t blocks = wg::step_blocks(C, H, W);
    if (blocks == 0 || !img_l1 || !img_ssim || !gt || !scratch || !loss_out || !stats) return WG_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) != 0 || (reinterpret_cast<uintptr_t>(stats) & 7) != 0) return WG_ERR_INVALID_ARGUMENT;
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const wg::StepMult sm{mult, threshold_enabled ? 1 : 0, mult_threshold, mult_blend};
    double* partials = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(wg::step_loss_forward_kernel, wg::step_grid(C, H, W), dim3(256), 0, st, H, W, img_ssim, gt, img_l1, mask, sm, dm_dmu1,
                       dm_dsigma1_sq, dm_dsigma12, wg::make_step_taps(), partials);
    hipLaunchKernelGGL(wg::step_loss_finish_kernel, dim3(1), dim3(wg::SL_FINISH_THREADS), 0, st, (const double*)partials, (int)blocks,
                       (double)C * (double)H * (double)W, (double)H * (double)W, (double)C, lambda, mask ? 1 : 0, loss_out, stats);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

int wg_step_loss_backward(int C, int H, int W, const float* img_l1, const float* img_ssim, const float* gt, const float* mask,
                          const float* mult, int threshold_enabled, float mult_threshold, float mult_blend, double lambda,
                          const float* dL_dloss, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                          float* dL_dimg_l1, float* dL_dimg_ssim, void* stream) {
    if (wg::step_blocks(C, H, W) == 0 || !img_l1 || !img_ssim || !gt || !dL_dloss || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 ||
        !dL_dimg_l1 || !dL_dimg_ssim)
        return WG_ERR_INVALID_ARGUMENT;
    if ((img_l1 == img_ssim) != (dL_dimg_l1 == dL_dimg_ssim)) return WG_ERR_INVALID_ARGUMENT;  // one image <-> one gradient
    const wg::StepMult sm{mult, threshold_enabled ? 1 : 0, mult_threshold, mult_blend};
    hipLaunchKernelGGL(wg::step_loss_backward_kernel, wg::step_grid(C, H, W), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H, W,
                       img_ssim, gt, img_l1, mask, sm, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dloss, (float)lambda,
                       (float)((double)C * (double)H * (double)W), dL_dimg_ssim, dL_dimg_l1, wg::make_step_taps());
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // extern "C"
