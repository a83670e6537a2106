// Fused LPIPS v0.1 on the AlexNet and VGG16 trunks (include/wg_lpips.h): forward only, float32 on the matrix cores.  Reference semantics:
// LPIPS.forward (wildgaussians/_metrics_lpips.py:149-180) behind evaluation._lpips (wildgaussians/evaluation.py:255-291).
//
// Every product is a chain of v_mfma_f32_32x32x2_f32: lane l = (r = l & 31, h = l >> 5) hands in A[i = r][k = h] and B[k = h][j = r] and
// receives D[crow(reg, h)][j = r] in 16 registers (the tile walk of csrc/dino/vit.hip, restated here).
//
//   conv_kernel   an implicit GEMM: M = N OH OW output pixels x Cout x K = KH KW Cin, activations channels-last, weights [Cout][KH][KW][Cin].
//                 128 pixels x 64 output channels per workgroup of 4 waves, each wave 64 x 32 (two MFMA tiles, 32 accumulator registers); k in
//                 slices of 32 through LDS images sA[128][34], sB[64][34] (row stride 34: the 64 lanes of an operand read, (34 r + h) mod 64,
//                 fall in 64 different banks); the next slice travels global -> registers while the current one is multiplied.  Cin a multiple
//                 of 64: a slice lies inside one window tap, so a thread's four float4 loads of a slice share one (ky, kx) and are contiguous
//                 in Cin.  Cin = 3 (the first layers): every element is decoded on its own and read through the image's strides, with the
//                 caller's scaling applied.  A tap outside the image, a row past M and a k past K load 0.  The pixel is the accumulator's row
//                 and the output channel its lane, so the bias is one per-lane read and a pixel's 32 results are stored as one 128-byte run.
//   pool_kernel   max pool, a float4 of channels per thread.
//   head_kernel   one wave per pixel: both images' C channels (C / 64 per lane), three butterflies (the two norms, the weighted squared
//                 difference); a wave adds its pixels in float64 in pixel order, the four waves of a workgroup are added in wave order: one
//                 partial per workgroup.
//   finish_kernel one workgroup per image adds each tap's partials (thread t those at t, t + 256, ..., then a fixed tree), divides by the
//                 tap's pixel count and sums the five taps.
// No atomics; every reduction is a fixed butterfly or a fixed order.  Compiled with -ffp-contract=off: the scaling chain of the first layer
// and the head are float32 operations rounded one by one (the MFMA chains are intrinsics and do not care).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wg_lpips.h"
#include "wg_rasterizer.h"

namespace wg {
namespace lpips {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TM = 128, TN = 64, GK = 32, GS = GK + 2;   // conv tile: pixels, output channels, k slice, LDS row stride
constexpr int HP = WG_LPIPS_HEAD_PIXELS;
constexpr int MAXC = 512;
constexpr float EPS = 1e-10f;

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
    return c;
#endif
}
// row of accumulator register i in the 32x32 result (the column is lane & 31)
__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
__device__ __forceinline__ void put4(float* dst, const float4& v) {   // dst is 8-byte aligned
    *reinterpret_cast<float2*>(dst) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(dst + 2) = make_float2(v.z, v.w);
}

// ---- convolution ----------------------------------------------------------------------------------------------------------------------------
enum { IN_CHANNELS_LAST = 0, IN_STRIDED = 1, IN_STRIDED_SCALED = 2 };

struct Img {
    const float* data;
    long long bs, rs, ps, cs;
};

struct CArgs {
    const float* x;      // IN_CHANNELS_LAST: [N, IH, IW, Cin]
    Img in0, in1;        // IN_STRIDED*: images 0..n0-1 and n0..N-1
    int n0;
    const float* shift;  // IN_STRIDED_SCALED: [3] each
    const float* scale;
    const float* w;      // [Cout][Kpad]
    const float* bias;   // [Cout]
    float* y;            // [M, Cout]
    int IH, IW, Cin, Cout, KW, stride, pad, OH, OW, M, K, Kpad, nct;
};

// one input value of the first layer: the caller's chain, each operation rounded on its own
__device__ __forceinline__ float scaled(float v, float shift, float scale) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);   // np.clip: NaN stays
    v = v * 2.f;
    v = v - 1.f;
    v = v - shift;
    return v / scale;
}

template <int MODE>
__device__ __forceinline__ float load_elem(const CArgs& a, int n, int iy0, int ix0, int k) {
    if (k >= a.K) return 0.f;
    const int tap = k / 3, c = k - 3 * tap, ky = tap / a.KW, kx = tap - ky * a.KW;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= a.IH || ix < 0 || ix >= a.IW) return 0.f;
    // the choice is made on values (unary + makes each operand a value): a choice between the two OBJECTS would be an address computed at run
    // time, and the argument block would be copied to scratch memory for it
    const bool first = n < a.n0;
    const float* data = first ? +a.in0.data : +a.in1.data;
    const long long nb = first ? n * a.in0.bs : (n - a.n0) * a.in1.bs;
    const long long rs = first ? +a.in0.rs : +a.in1.rs, ps = first ? +a.in0.ps : +a.in1.ps, cs = first ? +a.in0.cs : +a.in1.cs;
    const long long off = nb + iy * rs + ix * ps + c * cs;
    const float v = data[off];
    if (MODE != IN_STRIDED_SCALED) return v;
    return scaled(v, a.shift[c], a.scale[c]);
}

template <int MODE>
__global__ void __launch_bounds__(256) conv_kernel(const CArgs a) {
    __shared__ float sA[TM * GS];
    __shared__ float sB[TN * GS];
    const int t = threadIdx.x, wv = t >> 6, l = t & 63, r = l & 31, h = l >> 5, wr = wv >> 1, wc = wv & 1;
    const int ct = blockIdx.x % a.nct, mt = blockIdx.x / a.nct;
    const int row0 = mt * TM, col0 = ct * TN;
    const int lr = t >> 3, lk = (t & 7) * 4;   // this thread's row (plus 32 per pass) and k offset in a slice

    // the four pixels this thread loads: image, and the window's top-left corner in the input
    int pn[4], py[4], px[4];
    bool pok[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = row0 + lr + 32 * p;
        pok[p] = m < a.M;
        const int mm = pok[p] ? m : 0;
        const int n = mm / (a.OH * a.OW), rem = mm - n * (a.OH * a.OW), oy = rem / a.OW, ox = rem - oy * a.OW;
        pn[p] = n;
        py[p] = oy * a.stride - a.pad;
        px[p] = ox * a.stride - a.pad;
    }

    f32x16 acc[2] = {zero16(), zero16()};
    float4 ra[4], rb[2];
    auto fetch = [&](int k0) {
        if (MODE == IN_CHANNELS_LAST) {   // Cin is a multiple of 64: the slice lies in one window tap
            const int tap = k0 / a.Cin, ci = k0 - tap * a.Cin + lk, ky = tap / a.KW, kx = tap - ky * a.KW;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int iy = py[p] + ky, ix = px[p] + kx;
                const bool ok = pok[p] && iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW;
                ra[p] = ok ? *reinterpret_cast<const float4*>(a.x + ((size_t)(pn[p] * a.IH + iy) * a.IW + ix) * a.Cin + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int k = k0 + lk;
                ra[p] = pok[p] ? make_float4(load_elem<MODE>(a, pn[p], py[p], px[p], k), load_elem<MODE>(a, pn[p], py[p], px[p], k + 1),
                                             load_elem<MODE>(a, pn[p], py[p], px[p], k + 2), load_elem<MODE>(a, pn[p], py[p], px[p], k + 3))
                               : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)   // col0 + 63 < Cout: Cout is a multiple of 64
            rb[p] = k0 + lk < a.Kpad ? *reinterpret_cast<const float4*>(a.w + (size_t)(col0 + lr + 32 * p) * a.Kpad + k0 + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += GK) {
#pragma unroll
        for (int p = 0; p < 4; ++p) put4(sA + (lr + 32 * p) * GS + lk, ra[p]);
#pragma unroll
        for (int p = 0; p < 2; ++p) put4(sB + (lr + 32 * p) * GS + lk, rb[p]);
        __syncthreads();
        if (k0 + GK < a.K) fetch(k0 + GK);
        const float* pa = sA + (64 * wr + r) * GS + h;
        const float* pb = sB + (32 * wc + r) * GS + h;
#pragma unroll
        for (int s = 0; s < GK / 2; ++s) {
            const float a0 = pa[2 * s], a1 = pa[32 * GS + 2 * s], b = pb[2 * s];
            acc[0] = mfma(a0, b, acc[0]);
            acc[1] = mfma(a1, b, acc[1]);
        }
        __syncthreads();
    }

    const int col = col0 + 32 * wc + r;
    const float bias = a.bias[col];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = row0 + 64 * wr + 32 * ti + crow(i, h);
            if (row >= a.M) continue;
            const float v = acc[ti][i] + bias;
            a.y[(size_t)row * a.Cout + col] = v < 0.f ? 0.f : v;   // ReLU; NaN stays
        }
    }
}

// ---- max pool ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pool_kernel(const float* __restrict__ x, float* __restrict__ y, int IH, int IW, int C4, int window, int OH,
                                                   int OW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    const long long pix = i / C4;
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), n = (int)(pix / ((long long)OW * OH));
    const float4* src = reinterpret_cast<const float4*>(x) + ((size_t)(n * IH + 2 * oy) * IW + 2 * ox) * C4 + c;
    float4 m = src[0];
    for (int dy = 0; dy < window; ++dy)
        for (int dx = 0; dx < window; ++dx) {
            const float4 v = src[((size_t)dy * IW + dx) * C4];
            m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x;
            m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
            m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z;
            m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
        }
    reinterpret_cast<float4*>(y)[i] = m;
}

// ---- head -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// f [2 B, hw, C]; partials [B, nchunks]: workgroup (chunk, b) adds pixels chunk * HP .. of image b
template <int CJ>   // C = 64 CJ
__global__ void __launch_bounds__(256) head_kernel(const float* __restrict__ f, const float* __restrict__ lin, double* __restrict__ partials, int B,
                                                   int hw) {
    __shared__ double sw[4];
    constexpr int C = 64 * CJ;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, b = blockIdx.y, chunk = blockIdx.x;
    float wl[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) wl[j] = lin[lane + 64 * j];
    const int p_end = min(hw, (chunk + 1) * HP);
    double sum = 0.0;
    for (int p = chunk * HP + wv; p < p_end; p += 4) {   // uniform over the wave
        const float* f0 = f + ((size_t)b * hw + p) * C;
        const float* f1 = f + ((size_t)(B + b) * hw + p) * C;
        float v0[CJ], v1[CJ], q0 = 0.f, q1 = 0.f;
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            v0[j] = f0[lane + 64 * j];
            v1[j] = f1[lane + 64 * j];
            q0 += v0[j] * v0[j];
            q1 += v1[j] * v1[j];
        }
        const float d0 = sqrtf(wave_sum(q0)) + EPS, d1 = sqrtf(wave_sum(q1)) + EPS;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            const float d = v0[j] / d0 - v1[j] / d1;
            s += wl[j] * (d * d);
        }
        sum += (double)wave_sum(s);
    }
    if (lane == 0) sw[wv] = sum;
    __syncthreads();
    if (t == 0) partials[(size_t)b * gridDim.x + chunk] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

struct FArgs {
    const double* partials[WG_LPIPS_TAPS];   // [B, nchunks[l]]
    int nchunks[WG_LPIPS_TAPS], hw[WG_LPIPS_TAPS];
    int taps;
    float* out;         // [B], or NULL
    float* per_layer;   // [B, taps], or NULL
};

__global__ void __launch_bounds__(256) finish_kernel(const FArgs a) {
    __shared__ double sd[256];
    const int t = threadIdx.x, b = blockIdx.x;
    double total = 0.0;
    for (int l = 0; l < a.taps; ++l) {
        double s = 0.0;
        for (int i = t; i < a.nchunks[l]; i += 256) s += a.partials[l][(size_t)b * a.nchunks[l] + i];
        sd[t] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) sd[t] += sd[t + o];
            __syncthreads();
        }
        const double layer = sd[0] / (double)a.hw[l];
        __syncthreads();
        if (t == 0 && a.per_layer) a.per_layer[b * a.taps + l] = (float)layer;
        total += layer;
    }
    if (t == 0 && a.out) a.out[b] = (float)total;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool launched() { return hipGetLastError() == hipSuccess; }

struct Conv { int cin, cout, k, stride, pad; bool pool_before; int pool; bool tap_after; };
static const Conv ALEX[5] = {{3, 64, 11, 4, 2, false, 0, true}, {64, 192, 5, 1, 2, true, 3, true}, {192, 384, 3, 1, 1, true, 3, true},
                             {384, 256, 3, 1, 1, false, 0, true}, {256, 256, 3, 1, 1, false, 0, true}};
static const Conv VGG[13] = {{3, 64, 3, 1, 1, false, 0, false}, {64, 64, 3, 1, 1, false, 0, true},
                             {64, 128, 3, 1, 1, true, 2, false}, {128, 128, 3, 1, 1, false, 0, true},
                             {128, 256, 3, 1, 1, true, 2, false}, {256, 256, 3, 1, 1, false, 0, false}, {256, 256, 3, 1, 1, false, 0, true},
                             {256, 512, 3, 1, 1, true, 2, false}, {512, 512, 3, 1, 1, false, 0, false}, {512, 512, 3, 1, 1, false, 0, true},
                             {512, 512, 3, 1, 1, true, 2, false}, {512, 512, 3, 1, 1, false, 0, false}, {512, 512, 3, 1, 1, false, 0, true}};

static bool image_ok(const wg_lpips_image& im) { return im.data && im.batch_stride >= 0 && im.row_stride >= 0 && im.pixel_stride >= 0 && im.channel_stride >= 0; }
static Img img(const wg_lpips_image& im) { return Img{im.data, im.batch_stride, im.row_stride, im.pixel_stride, im.channel_stride}; }

// the shape checks of one convolution, shared by the stage entry point and the trunk; -> OH, OW
static bool conv_shape_ok(int64_t N, int64_t IH, int64_t IW, int Cin, int Cout, int K, int stride, int pad, int* OH, int* OW) {
    if (N < 1 || IH < 1 || IW < 1 || Cout < 64 || Cout % 64 != 0 || !(Cin == 3 || (Cin >= 64 && Cin % 64 == 0))) return false;
    if (K < 1 || K > 11 || stride < 1 || pad < 0 || pad >= K || IH + 2 * pad < K || IW + 2 * pad < K) return false;
    const int64_t oh = (IH + 2 * pad - K) / stride + 1, ow = (IW + 2 * pad - K) / stride + 1;
    if (N * IH * IW * Cin > INT32_MAX || N * oh * ow * Cout > INT32_MAX || (int64_t)K * K * Cin + 3 > INT32_MAX / Cout) return false;
    *OH = (int)oh;
    *OW = (int)ow;
    return true;
}

static int conv(CArgs& c, int N, int mode, hipStream_t stream) {
    c.M = N * c.OH * c.OW;
    c.Kpad = (c.K + 3) & ~3;
    c.nct = c.Cout / TN;
    const int64_t blocks = (int64_t)((c.M + TM - 1) / TM) * c.nct;
    if (blocks > INT32_MAX) return WG_ERR_INVALID_ARGUMENT;
    const dim3 grid((unsigned)blocks), block(256);
    if (mode == IN_CHANNELS_LAST) hipLaunchKernelGGL((conv_kernel<IN_CHANNELS_LAST>), grid, block, 0, stream, c);
    else if (mode == IN_STRIDED) hipLaunchKernelGGL((conv_kernel<IN_STRIDED>), grid, block, 0, stream, c);
    else hipLaunchKernelGGL((conv_kernel<IN_STRIDED_SCALED>), grid, block, 0, stream, c);
    return launched() ? WG_OK : WG_ERR_HIP;
}

static int pool(const float* x, int N, int IH, int IW, int C, int window, float* y, hipStream_t stream) {
    const int OH = (IH - window) / 2 + 1, OW = (IW - window) / 2 + 1;
    const long long total = (long long)N * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, y, IH, IW, C / 4, window, OH, OW, total);
    return launched() ? WG_OK : WG_ERR_HIP;
}

static int head_chunks(int64_t hw) { return (int)((hw + HP - 1) / HP); }

static int head(const float* f, int B, int hw, int C, const float* lin, double* partials, hipStream_t stream) {
    const dim3 grid(head_chunks(hw), B), block(256);
    switch (C / 64) {
#define WG_HEAD_CASE(J) case J: hipLaunchKernelGGL((head_kernel<J>), grid, block, 0, stream, f, lin, partials, B, hw); break;
        WG_HEAD_CASE(1) WG_HEAD_CASE(2) WG_HEAD_CASE(3) WG_HEAD_CASE(4) WG_HEAD_CASE(5) WG_HEAD_CASE(6) WG_HEAD_CASE(7) WG_HEAD_CASE(8)
#undef WG_HEAD_CASE
        default: return WG_ERR_INVALID_ARGUMENT;
    }
    return launched() ? WG_OK : WG_ERR_HIP;
}

// The trunk's geometry: the largest activation (floats) and, per tap, its size.  false: a side under the minimum.
struct Plan { int64_t A; int th[WG_LPIPS_TAPS], tw[WG_LPIPS_TAPS], tc[WG_LPIPS_TAPS]; int64_t P; };
static bool plan(int net, int64_t B, int H, int W, Plan* pl) {
    const Conv* cv = net == WG_LPIPS_ALEX ? ALEX : VGG;
    const int n = net == WG_LPIPS_ALEX ? 5 : 13;
    int64_t h = H, w = W;
    int tap = 0;
    pl->A = 0;
    pl->P = 0;
    for (int i = 0; i < n; ++i) {
        if (cv[i].pool_before) {
            if (h < cv[i].pool || w < cv[i].pool) return false;
            h = (h - cv[i].pool) / 2 + 1;
            w = (w - cv[i].pool) / 2 + 1;
        }
        if (h + 2 * cv[i].pad < cv[i].k || w + 2 * cv[i].pad < cv[i].k) return false;
        h = (h + 2 * cv[i].pad - cv[i].k) / cv[i].stride + 1;
        w = (w + 2 * cv[i].pad - cv[i].k) / cv[i].stride + 1;
        const int64_t act = 2 * B * h * w * cv[i].cout;
        if (act > pl->A) pl->A = act;
        if (cv[i].tap_after) {
            pl->th[tap] = (int)h; pl->tw[tap] = (int)w; pl->tc[tap] = cv[i].cout;
            pl->P += B * head_chunks(h * w);
            ++tap;
        }
    }
    return true;
}

}  // namespace lpips
}  // namespace wg

using namespace wg::lpips;

static bool trunk_sizes_ok(int32_t net, int32_t B, int32_t H, int32_t W) {
    if (net != WG_LPIPS_ALEX && net != WG_LPIPS_VGG) return false;
    const int min_side = net == WG_LPIPS_ALEX ? WG_LPIPS_ALEX_MIN_SIDE : WG_LPIPS_VGG_MIN_SIDE;
    return B >= 1 && H >= min_side && W >= min_side;
}

extern "C" int64_t wg_lpips_scratch_floats(int32_t net, int32_t B, int32_t H, int32_t W) {
    if (!trunk_sizes_ok(net, B, H, W)) return WG_ERR_INVALID_ARGUMENT;
    if ((int64_t)H * W > INT32_MAX / 6 / B) return WG_ERR_OVERFLOW;   // the 2 B x 3 x H x W input values are indexed in 31 bits
    Plan pl;
    if (!plan(net, B, H, W, &pl)) return WG_ERR_INVALID_ARGUMENT;
    return pl.A > INT32_MAX ? (int64_t)WG_ERR_OVERFLOW : 2 * pl.A + 2 * pl.P;
}

extern "C" int wg_lpips_conv(const wg_lpips_conv_args* p) {
    if (!p || p->struct_size < sizeof(wg_lpips_conv_args)) return WG_ERR_INVALID_ARGUMENT;
    CArgs c = {};
    if (!conv_shape_ok(p->N, p->IH, p->IW, p->Cin, p->Cout, p->K, p->stride, p->pad, &c.OH, &c.OW)) return WG_ERR_INVALID_ARGUMENT;
    if (!p->w || !p->bias || !p->y || !aligned16(p->w) || !aligned16(p->y)) return WG_ERR_INVALID_ARGUMENT;
    int mode;
    if (p->x) {
        if (!aligned16(p->x)) return WG_ERR_INVALID_ARGUMENT;
        mode = p->Cin == 3 ? IN_STRIDED : IN_CHANNELS_LAST;
        c.x = p->x;
        c.in0 = c.in1 = Img{p->x, (long long)p->IH * p->IW * p->Cin, (long long)p->IW * p->Cin, p->Cin, 1};
        c.n0 = p->N;
    } else {
        if (!p->shift || !p->scale || p->Cin != 3 || p->N0 < 0 || p->N0 > p->N || (p->N0 > 0 && !image_ok(p->in0)) || (p->N0 < p->N && !image_ok(p->in1)))
            return WG_ERR_INVALID_ARGUMENT;
        mode = IN_STRIDED_SCALED;
        c.in0 = img(p->N0 > 0 ? p->in0 : p->in1);
        c.in1 = img(p->N0 < p->N ? p->in1 : p->in0);
        c.n0 = p->N0;
    }
    c.shift = p->shift; c.scale = p->scale;
    c.w = p->w; c.bias = p->bias; c.y = p->y;
    c.IH = p->IH; c.IW = p->IW; c.Cin = p->Cin; c.Cout = p->Cout; c.KW = p->K; c.stride = p->stride; c.pad = p->pad;
    c.K = p->K * p->K * p->Cin;
    return conv(c, p->N, mode, static_cast<hipStream_t>(p->stream));
}

extern "C" int wg_lpips_pool(const float* x, int32_t N, int32_t IH, int32_t IW, int32_t C, int32_t window, float* y, void* stream) {
    if (!x || !y || !aligned16(x) || !aligned16(y) || N < 1 || C < 4 || C % 4 != 0 || (window != 2 && window != 3) || IH < window || IW < window)
        return WG_ERR_INVALID_ARGUMENT;
    if ((int64_t)N * IH * IW * C > INT32_MAX) return WG_ERR_INVALID_ARGUMENT;
    return pool(x, N, IH, IW, C, window, y, static_cast<hipStream_t>(stream));
}

extern "C" int wg_lpips_head(const float* f, int32_t B, int32_t h, int32_t w, int32_t C, const float* lin, double* partials, float* out, void* stream) {
    if (!f || !lin || !partials || !out || (reinterpret_cast<uintptr_t>(partials) & 7) || B < 1 || h < 1 || w < 1 || C < 64 || C % 64 != 0 || C > MAXC)
        return WG_ERR_INVALID_ARGUMENT;
    if (2 * (int64_t)B * h * w * C > INT32_MAX || B > 65535) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int st = head(f, B, h * w, C, lin, partials, s);
    if (st != WG_OK) return st;
    FArgs fa = {};
    fa.partials[0] = partials; fa.nchunks[0] = head_chunks((int64_t)h * w); fa.hw[0] = h * w; fa.taps = 1;
    fa.out = nullptr; fa.per_layer = out;
    hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(256), 0, s, fa);
    return launched() ? WG_OK : WG_ERR_HIP;
}

extern "C" int wg_lpips(const wg_lpips_args* p) {
    if (!p || p->struct_size < sizeof(wg_lpips_args)) return WG_ERR_INVALID_ARGUMENT;
    if (!trunk_sizes_ok(p->net, p->B, p->H, p->W) || p->B > 32767) return WG_ERR_INVALID_ARGUMENT;
    const Conv* cv = p->net == WG_LPIPS_ALEX ? ALEX : VGG;
    const int nconv = p->net == WG_LPIPS_ALEX ? 5 : 13;
    if (!image_ok(p->in0) || !image_ok(p->in1) || !p->shift || !p->scale || !p->scratch || !aligned16(p->scratch) || !p->out) return WG_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < nconv; ++i)
        if (!p->conv_w[i] || !p->conv_b[i] || !aligned16(p->conv_w[i])) return WG_ERR_INVALID_ARGUMENT;
    for (int l = 0; l < WG_LPIPS_TAPS; ++l)
        if (!p->lin_w[l]) return WG_ERR_INVALID_ARGUMENT;
    const int64_t need = wg_lpips_scratch_floats(p->net, p->B, p->H, p->W);
    if (need < 0 || p->scratch_floats < need) return WG_ERR_INVALID_ARGUMENT;
    Plan pl;
    if (!plan(p->net, p->B, p->H, p->W, &pl)) return WG_ERR_INVALID_ARGUMENT;
    // every convolution's shape, before any device work
    {
        int64_t h = p->H, w = p->W;
        for (int i = 0; i < nconv; ++i) {
            if (cv[i].pool_before) { h = (h - cv[i].pool) / 2 + 1; w = (w - cv[i].pool) / 2 + 1; }
            int oh, ow;
            if (!conv_shape_ok(2 * (int64_t)p->B, h, w, cv[i].cin, cv[i].cout, cv[i].k, cv[i].stride, cv[i].pad, &oh, &ow)) return WG_ERR_INVALID_ARGUMENT;
            h = oh; w = ow;
        }
    }

    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    const int N = 2 * p->B;
    float* buf[2] = {p->scratch, p->scratch + pl.A};
    double* partials = reinterpret_cast<double*>(p->scratch + 2 * pl.A);   // A is a multiple of 64: 16-byte aligned
    FArgs fa = {};
    fa.taps = WG_LPIPS_TAPS; fa.out = p->out; fa.per_layer = p->per_layer;
    int cur = -1, h = p->H, w = p->W, tap = 0, st;   // cur: the buffer that holds the current activation (-1: the images)
    for (int i = 0; i < nconv; ++i) {
        if (cv[i].pool_before) {
            if ((st = pool(buf[cur], N, h, w, cv[i].cin, cv[i].pool, buf[cur ^ 1], stream)) != WG_OK) return st;
            h = (h - cv[i].pool) / 2 + 1; w = (w - cv[i].pool) / 2 + 1;
            cur ^= 1;
        }
        CArgs c = {};
        c.IH = h; c.IW = w; c.Cin = cv[i].cin; c.Cout = cv[i].cout; c.KW = cv[i].k; c.stride = cv[i].stride; c.pad = cv[i].pad;
        c.OH = (h + 2 * c.pad - c.KW) / c.stride + 1; c.OW = (w + 2 * c.pad - c.KW) / c.stride + 1;
        c.K = c.KW * c.KW * c.Cin;
        c.w = p->conv_w[i]; c.bias = p->conv_b[i];
        const int dst = cur < 0 ? 0 : cur ^ 1;
        c.y = buf[dst];
        if (cur < 0) {
            c.in0 = img(p->in0); c.in1 = img(p->in1); c.n0 = p->B;
            c.shift = p->shift; c.scale = p->scale;
        } else {
            c.x = buf[cur];
        }
        if ((st = conv(c, N, cur < 0 ? IN_STRIDED_SCALED : IN_CHANNELS_LAST, stream)) != WG_OK) return st;
        cur = dst; h = c.OH; w = c.OW;
        if (cv[i].tap_after) {
            fa.partials[tap] = partials; fa.nchunks[tap] = head_chunks((int64_t)h * w); fa.hw[tap] = h * w;
            if ((st = head(buf[cur], p->B, h * w, cv[i].cout, p->lin_w[tap], partials, stream)) != WG_OK) return st;
            partials += (size_t)p->B * fa.nchunks[tap];
            ++tap;
        }
    }
    hipLaunchKernelGGL(finish_kernel, dim3(p->B), dim3(256), 0, stream, fa);
    return launched() ? WG_OK : WG_ERR_HIP;
}
