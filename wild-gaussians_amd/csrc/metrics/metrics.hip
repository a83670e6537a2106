// Fused evaluation metrics for gfx950 (include/wg_metrics.h): the 8-bit quantisation of a render and MSE / MAE / mean SSIM of an image pair.
//
// This file restates NumPy op for op and is compiled with -ffp-contract=off and no fast-math flag: a float32 product stays a float32 product,
// the division by 255.0f stays correctly rounded, and no multiply-add is fused.
//
// quantize_kernel: streaming, no reuse, one wave per workgroup as in frames.hip.  A thread takes FOUR pixels: C 16-byte loads (one per plane)
// and C dword stores (four pixels of C bytes are exactly C dwords) where HW % 4 == 0 and the addresses allow it, single floats and bytes
// elsewhere; the HW % 4 tail goes pixel by pixel through the thread that owns the last, partial group.
//
// metrics_kernel: 256 threads own a tile of 32 x 16 pixels of one channel, laid from the RECTANGLE's origin (a crop and a copy of the crop
// walk identically).  LDS holds the 42 x 26 halo of both images as float32 (8.5 KB) and five planes of 26 x 32 doubles, the horizontal
// 11-tap sums of a, b, a*a, b*b, a*b (32.5 KB).  A row of a double plane is 32 doubles = 256 bytes = one pass over the 64 banks, and in both
// passes a 32-lane half of a wave touches ONE such row (lane = column), which the 8-byte LDS instructions serve without a conflict; the two
// halves never conflict with each other.  So the planes carry no padding: a pad would move no access off a busy bank.
// The SSIM of the pixel at (y, x) is the window centred on it and counts where the window lies inside the rectangle
// (5 <= y < h - 5, 5 <= x < w - 5): the (h - 10)(w - 10) values of np.convolve(mode="valid").  Halo pixels outside the rectangle are read
// as 0 and only ever feed windows that do not count.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wg_metrics.h"
#include "wg_rasterizer.h"

namespace wgm {

// ------------------------------------------------------------------------------------------------ value loads
// torch.clamp(x, 0, 1).nan_to_num_(0) -> np.clip(x * 255.0, 0, 255).astype(np.uint8)
__device__ inline uint32_t quantize_one(float x) {
    x = x != x ? 0.f : x;
    x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const float t = x * 255.0f;   // within [0, 255]: the outer clip changes nothing
    return (uint32_t)t;           // truncation
}

__device__ inline float byte_to_float(uint32_t b) { return (float)b / 255.0f; }

__device__ inline float load_value(const wg_image_desc& d, int64_t off) {
    if (d.kind == WG_IMAGE_U8) return byte_to_float(static_cast<const uint8_t*>(d.data)[off]);
    const float x = static_cast<const float*>(d.data)[off];
    if (d.kind == WG_IMAGE_F32) return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);   // NaN passes, as through np.clip
    return byte_to_float(quantize_one(x));
}

// ------------------------------------------------------------------------------------------------ quantize
constexpr int Q_TPB = 64;                // one wave
constexpr int PER = 4;                   // pixels per thread and step
constexpr unsigned Q_MAX_BLOCKS = 8192;  // 256 CUs x 32 one-wave workgroups; larger frames stride

template <int C, bool WIDE>
__global__ void __launch_bounds__(Q_TPB) quantize_kernel(size_t HW, const float* __restrict__ src, uint8_t* __restrict__ dst) {
    const size_t full = HW / PER, groups = (HW + PER - 1) / PER, step = (size_t)gridDim.x * Q_TPB;
    for (size_t g = (size_t)blockIdx.x * Q_TPB + threadIdx.x; g < groups; g += step) {
        if (g < full) {
            uint32_t q[C][PER];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* s = src + (size_t)c * HW + PER * g;
                float v[PER];
                if (WIDE) {
                    const float4 t = *reinterpret_cast<const float4*>(s);
                    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                } else {
#pragma unroll
                    for (int p = 0; p < PER; ++p) v[p] = s[p];
                }
#pragma unroll
                for (int p = 0; p < PER; ++p) q[c][p] = quantize_one(v[p]);
            }
            uint8_t* d = dst + PER * g * C;   // 4 C bytes
            if (WIDE) {
                uint32_t w[C];
#pragma unroll
                for (int k = 0; k < C; ++k) w[k] = 0;
#pragma unroll
                for (int p = 0; p < PER; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c) w[(p * C + c) >> 2] |= q[c][p] << (8 * ((p * C + c) & 3));
#pragma unroll
                for (int k = 0; k < C; ++k) reinterpret_cast<uint32_t*>(d)[k] = w[k];
            } else {
#pragma unroll
                for (int p = 0; p < PER; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c) d[p * C + c] = (uint8_t)q[c][p];
            }
        } else {
            for (size_t i = PER * full; i < HW; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) dst[i * C + c] = (uint8_t)quantize_one(src[(size_t)c * HW + i]);
        }
    }
}

template <int C>
inline void launch_quantize(bool wide, unsigned blocks, hipStream_t s, size_t HW, const float* src, uint8_t* dst) {
    if (wide)
        hipLaunchKernelGGL((quantize_kernel<C, true>), dim3(blocks), dim3(Q_TPB), 0, s, HW, src, dst);
    else
        hipLaunchKernelGGL((quantize_kernel<C, false>), dim3(blocks), dim3(Q_TPB), 0, s, HW, src, dst);
}

// ------------------------------------------------------------------------------------------------ metrics
constexpr int TPB = 256;
constexpr int TILE_X = 32, TILE_Y = 16;
constexpr int TAPS = WG_METRICS_TAPS, HALF = TAPS / 2;
constexpr int HALO_X = TILE_X + TAPS - 1, HALO_Y = TILE_Y + TAPS - 1;   // 42 x 26
constexpr int PLANES = 5;                                               // a, b, a*a, b*b, a*b
constexpr int FINISH_TPB = 256;

struct Params {
    wg_image_desc a, b;
    int y0, x0, h, w;   // the rectangle
    double taps[TAPS];
    double c1, c2;
};

// s[0..2] summed over the workgroup in a fixed order -> thread 0
__device__ inline void block_sum3(double (&s)[3], double (*red)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

__global__ void __launch_bounds__(TPB) metrics_kernel(const Params p, double* __restrict__ partials) {
    __shared__ float sa[HALO_Y][HALO_X], sb[HALO_Y][HALO_X];
    __shared__ double hs[PLANES][HALO_Y][TILE_X];
    __shared__ double red[TPB / 64][3];

    const int t = threadIdx.x, c = blockIdx.z;
    const int oy = blockIdx.y * TILE_Y, ox = blockIdx.x * TILE_X;   // the tile's origin inside the rectangle

    // 1. both halos as float32 values; 0 outside the rectangle
    for (int i = t; i < HALO_Y * HALO_X; i += TPB) {
        const int r = i / HALO_X, q = i - r * HALO_X;
        const int y = oy + r - HALF, x = ox + q - HALF;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < p.h && x >= 0 && x < p.w) {
            const int64_t gy = p.y0 + y, gx = p.x0 + x;
            va = load_value(p.a, gy * p.a.row_stride + gx * p.a.pixel_stride + c * p.a.channel_stride);
            vb = load_value(p.b, gy * p.b.row_stride + gx * p.b.pixel_stride + c * p.b.channel_stride);
        }
        sa[r][q] = va, sb[r][q] = vb;
    }
    __syncthreads();

    // 2. - 4. float32 products, then the horizontal sums in double
    for (int i = t; i < HALO_Y * TILE_X; i += TPB) {
        const int r = i / TILE_X, q = i % TILE_X;
        double s0 = 0., s1 = 0., s00 = 0., s11 = 0., s01 = 0.;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float a = sa[r][q + k], b = sb[r][q + k];
            const float aa = a * a, bb = b * b, ab = a * b;
            const double f = p.taps[k];
            s0 += (double)a * f, s1 += (double)b * f, s00 += (double)aa * f, s11 += (double)bb * f, s01 += (double)ab * f;
        }
        hs[0][r][q] = s0, hs[1][r][q] = s1, hs[2][r][q] = s00, hs[3][r][q] = s11, hs[4][r][q] = s01;
    }
    __syncthreads();

    // 5. - 6. the vertical sums and the reference's expression; the squared and absolute differences of the tile's own pixels
    double acc[3] = {0., 0., 0.};   // sum d*d, sum |d|, sum ssim
    const double eps = 0x1p-46;     // np.finfo(np.float32).eps ** 2
    const int q = t % TILE_X;
    for (int r = t / TILE_X; r < TILE_Y; r += TPB / TILE_X) {
        const int y = oy + r, x = ox + q;
        if (y >= p.h || x >= p.w) continue;
        const float d = sa[r + HALF][q + HALF] - sb[r + HALF][q + HALF];
        const float dd = d * d;
        acc[0] += (double)dd;
        acc[1] += (double)fabsf(d);
        if (y < HALF || y >= p.h - HALF || x < HALF || x >= p.w - HALF) continue;
        double v[PLANES];
#pragma unroll
        for (int m = 0; m < PLANES; ++m) {
            double s = 0.;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) s += hs[m][r + k][q] * p.taps[k];
            v[m] = s;
        }
        const double mu0 = v[0], mu1 = v[1];
        const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
        double sigma00 = v[2] - mu00, sigma11 = v[3] - mu11, sigma01 = v[4] - mu01;
        sigma00 = fmax(eps, sigma00), sigma11 = fmax(eps, sigma11);
        const double sgn = sigma01 > 0. ? 1. : (sigma01 < 0. ? -1. : 0.);
        sigma01 = sgn * fmin(sqrt(sigma00 * sigma11), fabs(sigma01));
        const double numer = (2. * mu01 + p.c1) * (2. * sigma01 + p.c2);
        const double denom = (mu00 + mu11 + p.c1) * (sigma00 + sigma11 + p.c2);
        acc[2] += numer / denom;
    }
    block_sum3(acc, red);
    if (t == 0) {
        double* o = partials + 3 * (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
    }
}

// Thread t adds partials t, t + 256, ... in workgroup order, then the 256 sums are folded in a fixed order: the same bits at every call.
__global__ void __launch_bounds__(FINISH_TPB) metrics_finish_kernel(unsigned nb, const double* __restrict__ partials, double n_pixels,
                                                                    double n_windows, double* __restrict__ out) {
    __shared__ double red[FINISH_TPB / 64][3];
    double s[3] = {0., 0., 0.};
    for (unsigned i = threadIdx.x; i < nb; i += FINISH_TPB)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += partials[3 * (size_t)i + k];
    block_sum3(s, red);
    if (threadIdx.x == 0) out[0] = s[0] / n_pixels, out[1] = s[1] / n_pixels, out[2] = s[2] / n_windows;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int done() { return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP; }

inline bool sizes_ok(int C, int h, int w) {
    return C >= 1 && C <= 4 && h >= TAPS && w >= TAPS && h <= WG_METRICS_MAX_SIDE && w <= WG_METRICS_MAX_SIDE;
}

inline dim3 grid_for(int C, int h, int w) { return dim3((w + TILE_X - 1) / TILE_X, (h + TILE_Y - 1) / TILE_Y, C); }

inline bool desc_ok(const wg_image_desc* d) {
    if (!d || !d->data || d->kind < WG_IMAGE_U8 || d->kind > WG_IMAGE_F32_RENDER) return false;
    if (d->row_stride < 0 || d->pixel_stride < 0 || d->channel_stride < 0) return false;
    return d->kind == WG_IMAGE_U8 || aligned(d->data, 4);
}

}  // namespace wgm

using namespace wgm;

extern "C" {

int wg_frame_quantize(int C, size_t HW, const float* src, uint8_t* dst, void* stream) {
    if (C < 1 || C > 4 || HW < 1 || HW > 0xffffffffUL / 4 || !src || !dst || !aligned(src, 4)) return WG_ERR_INVALID_ARGUMENT;
    const bool wide = HW % 4 == 0 && aligned(src, 16) && aligned(dst, 4);
    const size_t groups = (HW + PER - 1) / PER, want = (groups + Q_TPB - 1) / Q_TPB;
    const unsigned blocks = (unsigned)(want < Q_MAX_BLOCKS ? want : Q_MAX_BLOCKS);
    const hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: launch_quantize<1>(wide, blocks, s, HW, src, dst); break;
        case 2: launch_quantize<2>(wide, blocks, s, HW, src, dst); break;
        case 3: launch_quantize<3>(wide, blocks, s, HW, src, dst); break;
        default: launch_quantize<4>(wide, blocks, s, HW, src, dst); break;
    }
    return done();
}

size_t wg_image_metrics_scratch_bytes(int C, int h, int w) {
    if (!sizes_ok(C, h, w)) return 0;
    const dim3 g = grid_for(C, h, w);
    return (size_t)g.x * g.y * g.z * 3 * sizeof(double);
}

int wg_image_metrics(const wg_image_desc* a, const wg_image_desc* b, int H, int W, int C, int y0, int y1, int x0, int x1, const double* taps,
                     double c1, double c2, void* scratch, double* out, void* stream) {
    if (!desc_ok(a) || !desc_ok(b) || !taps || !scratch || !out || !aligned(scratch, 8) || !aligned(out, 8)) return WG_ERR_INVALID_ARGUMENT;
    if (H < 1 || W < 1 || H > WG_METRICS_MAX_SIDE || W > WG_METRICS_MAX_SIDE || y0 < 0 || x0 < 0 || y1 > H || x1 > W || y1 <= y0 || x1 <= x0)
        return WG_ERR_INVALID_ARGUMENT;
    const int h = y1 - y0, w = x1 - x0;
    if (!sizes_ok(C, h, w)) return WG_ERR_INVALID_ARGUMENT;
    Params p;
    p.a = *a, p.b = *b;
    p.y0 = y0, p.x0 = x0, p.h = h, p.w = w;
    for (int k = 0; k < TAPS; ++k) p.taps[k] = taps[k];
    p.c1 = c1, p.c2 = c2;
    const dim3 g = grid_for(C, h, w);
    const unsigned nb = g.x * g.y * g.z;
    double* partials = static_cast<double*>(scratch);
    hipLaunchKernelGGL(metrics_kernel, g, dim3(TPB), 0, (hipStream_t)stream, p, partials);
    if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(FINISH_TPB), 0, (hipStream_t)stream, nb, (const double*)partials,
                       (double)h * (double)w * (double)C, (double)(h - 2 * HALF) * (double)(w - 2 * HALF) * (double)C, out);
    return done();
}

}  // extern "C"
