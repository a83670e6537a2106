// Fused frozen DINOv2 ViT-S/14 feature extractor (include/wg_dino.h): forward only, float32 on the matrix cores, stopping at the block the
// caller reads.  Reference semantics: DinoVisionTransformer.get_intermediate_layers(x, n=[k], reshape=True) (wildgaussians/dinov2.py:789-813)
// with prepare_tokens_with_masks (:704-723), Block / Attention / Mlp / LayerScale of the same file.
//
// Every product is a chain of v_mfma_f32_32x32x2_f32: lane l = (r = l & 31, h = l >> 5) hands in A[i = r][k = h] and B[k = h][j = r] and
// receives D[crow(reg, h)][j = r] in 16 registers (the layout csrc/appearance/mlp.hip uses).
//
//   gemm_kernel   Y[rows, M] = X[rows, K] . W^T with W in nn.Linear layout.  128 x 128 output tile per workgroup of 4 waves, each wave 2 x 2
//                 MFMA tiles (64 accumulator registers) -- or, where that tiling has fewer than 128 workgroups, 64 x 64 and one MFMA tile per
//                 wave, which changes no bit; k in slices of 32 through LDS images sA[128][34], sB[128][34] (row stride 34: the
//                 64 lanes of an operand read, (34 r + h) mod 64, fall in 64 different banks); the next slice travels global -> registers
//                 while the current one is multiplied.  The token is the accumulator's row and the output feature its lane, so bias, LayerScale
//                 and the residual are per-lane reads and a row's 32 results are stored as one 128-byte run.  Epilogues: + bias; + bias, GELU
//                 (erf); (. + bias) * gamma + residual (in place); and the patch embedding's, which gathers its A rows from the image and
//                 writes behind the 5 leading tokens with the position embedding added.
//   attn_kernel   softmax(q k^T / 8) v for 128 queries of one (image, head) per workgroup, 32 queries per wave, keys in tiles of 64.
//                 S^T [key][query] = K . Q^T puts the QUERY on the lane: row maximum and row sum are 32 in-lane operations and one exchange
//                 between the lane halves, and the probabilities are, as they stand, the B operand of O^T [d][query] = V^T . P^T (a product that
//                 sums over the accumulator's row index needs no lane movement).  Q (scaled by 1/8) lives in 32 registers, O^T in 32, the
//                 scores of a tile in 32; K [64][66] and V [64][72] tiles lie in LDS (strides chosen so that both operand reads are
//                 conflict-free), prefetched through registers.  Keys past N are loaded as zeros and their scores set to -inf before the
//                 row maximum; queries past N are computed on zeros and not stored.
//   ln_kernel     one wave per token row (6 values per lane), two passes in registers.  A separate launch, not a GEMM load stage: the
//                 statistics need the whole row before the first product, and normalising on load would repeat it for each of the 3..12
//                 column tiles, while the separate pass moves 2 x 1.5 KB per token.
//   final_kernel  the last LayerNorm of 32 patch tokens into an LDS image [384][33], written out channel-major: [B, 384, h, w].
// No atomics; every reduction is a fixed butterfly or a fixed in-lane order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wg_dino.h"
#include "wg_rasterizer.h"

namespace wg {
namespace dino {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int E = WG_DINO_EMBED, HEADS = WG_DINO_HEADS, HD = WG_DINO_HEAD_DIM, HID = WG_DINO_HIDDEN, LEAD = WG_DINO_LEAD_TOKENS, PS = WG_DINO_PATCH;
constexpr int QKV = 3 * E;                  // floats of one token's packed q, k, v
constexpr int PK = 3 * PS * PS;             // 588: the patch embedding's K
constexpr int GT = 128, GK = 32, GS = GK + 2;   // GEMM tile (the large one), k slice, LDS row stride
constexpr int GEMM_BIG_MIN_WORKGROUPS = 128;   // below this many 128 x 128 tiles the 64 x 64 tiling runs: half the device's compute units
constexpr int AQ = 128, AK = 64;            // attention: queries per workgroup, keys per tile
constexpr int SK = HD + 2, SV = HD + 8;     // LDS row strides of the K and V tiles
constexpr int FT = 32, FS = FT + 1;         // final kernel: tokens per workgroup, LDS row stride
constexpr float LOG2E = 1.44269504088896340736f;
static_assert(E % GT == 0 && QKV % GT == 0 && HID % GT == 0, "every output width is a whole number of GEMM tiles");
static_assert(E % 4 == 0 && HID % 4 == 0 && PK % 4 == 0, "k is read in float4");
static_assert(AQ * SK <= AK * SK + AK * SV, "the Q tile is staged in the K / V tiles' LDS");

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

// ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
enum { EP_BIAS = 0, EP_GELU = 1, EP_RESIDUAL = 2, EP_PATCH = 3 };

struct GArgs {
    const float* A;        // [rows, K]; EP_PATCH: the image [B, 3, H, W]
    const float* Wt;       // [M, K]
    const float* bias;     // [M]
    const float* gamma;    // EP_RESIDUAL: [M]
    const float* res;      // EP_RESIDUAL: [rows, M] (may be Y); EP_PATCH: pos [1 + hw, M]
    float* Y;              // [rows, M]; EP_PATCH: the token buffer [B, N, M]
    int rows, K, M;
    int hw, wq, H, W, N;   // EP_PATCH: patches per image, patches per row, image size, tokens per image
};

template <int EP>
__device__ __forceinline__ float4 load_a(const GArgs& a, int row, int k) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= a.rows || k >= a.K) return v;
    if (EP != EP_PATCH) return *reinterpret_cast<const float4*>(a.A + (size_t)row * a.K + k);
    const int b = row / a.hw, p = row - b * a.hw, ph = p / a.wq, pw = p - ph * a.wq;
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kk = k + j, c = kk / (PS * PS), rem = kk - c * (PS * PS), py = rem / PS, px = rem - py * PS;
        e[j] = a.A[((size_t)(b * 3 + c) * a.H + (ph * PS + py)) * a.W + (pw * PS + px)];
    }
    return make_float4(e[0], e[1], e[2], e[3]);
}

__device__ __forceinline__ void put4(float* dst, const float4& v) {   // dst is 8-byte aligned
    *reinterpret_cast<float2*>(dst) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(dst + 2) = make_float2(v.z, v.w);
}

// T x T MFMA tiles per wave: a (64 T) x (64 T) output tile per workgroup.  T = 2 where there is enough work to fill the device (one operand read
// feeds two products), T = 1 for the small passes (four times the workgroups, a quarter of the serial MFMA chain per wave).  The k order of
// every output element is the same in both, so which one runs changes no bit.
template <int EP, int T>
__global__ void __launch_bounds__(256) gemm_kernel(const GArgs a) {
    constexpr int TILE = 64 * T;
    __shared__ float sA[TILE * GS];
    __shared__ float sB[TILE * GS];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5, wr = w >> 1, wc = w & 1;
    const int row0 = blockIdx.y * TILE, col0 = blockIdx.x * TILE;
    const int lr = t >> 3, lk = (t & 7) * 4;   // this thread's row (plus 32 per pass) and k offset in a slice

    f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = zero16();

    float4 ra[2 * T], rb[2 * T];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 2 * T; ++p) {
            ra[p] = load_a<EP>(a, row0 + lr + 32 * p, k0 + lk);
            const int col = col0 + lr + 32 * p;
            rb[p] = (col < a.M && k0 + lk < a.K) ? *reinterpret_cast<const float4*>(a.Wt + (size_t)col * a.K + k0 + lk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += GK) {
#pragma unroll
        for (int p = 0; p < 2 * T; ++p) {
            put4(sA + (lr + 32 * p) * GS + lk, ra[p]);
            put4(sB + (lr + 32 * p) * GS + lk, rb[p]);
        }
        __syncthreads();
        if (k0 + GK < a.K) fetch(k0 + GK);
        const float* pa = sA + (32 * T * wr + r) * GS + h;
        const float* pb = sB + (32 * T * wc + r) * GS + h;
#pragma unroll
        for (int s = 0; s < GK / 2; ++s) {
            float av[T], bv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                av[i] = pa[32 * i * GS + 2 * s];
                bv[i] = pb[32 * i * GS + 2 * s];
            }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = mfma(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int tj = 0; tj < T; ++tj) {
        const int col = col0 + 32 * T * wc + 32 * tj + r;
        if (col >= a.M) continue;
        const float bias = a.bias[col];
        const float gamma = EP == EP_RESIDUAL ? a.gamma[col] : 1.f;
#pragma unroll
        for (int ti = 0; ti < T; ++ti) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = row0 + 32 * T * wr + 32 * ti + crow(i, h);
                if (row >= a.rows) continue;
                float v = acc[ti][tj][i] + bias;
                if (EP == EP_GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
                if (EP == EP_RESIDUAL) {
                    const size_t o = (size_t)row * a.M + col;
                    a.Y[o] = v * gamma + a.res[o];
                } else if (EP == EP_PATCH) {
                    const int b = row / a.hw, p = row - b * a.hw;
                    a.Y[((size_t)b * a.N + LEAD + p) * a.M + col] = v + a.res[(size_t)(1 + p) * a.M + col];
                } else {
                    a.Y[(size_t)row * a.M + col] = v;
                }
            }
        }
    }
}

// ---- attention ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 load4_or_zero(const float* p, bool valid) {
    return valid ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// one tile of 64 keys x 64 floats of K and of V -> 4 + 4 float4 per thread; keys past N read as zeros
__device__ __forceinline__ void fetch_kv(const float* base, int tile, int N, int lrow, int lc, float4 (&rk)[4], float4 (&rv)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int key = tile * AK + lrow + 16 * p;
        const float* src = base + (size_t)key * QKV + lc;
        rk[p] = load4_or_zero(src + E, key < N);
        rv[p] = load4_or_zero(src + 2 * E, key < N);
    }
}

__global__ void __launch_bounds__(256) attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N) {
    __shared__ float lds[AK * SK + AK * SV];
    float* const sK = lds;
    float* const sV = lds + AK * SK;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;
    const int b = blockIdx.y / HEADS, head = blockIdx.y - b * HEADS;
    const int q0 = blockIdx.x * AQ;
    const float* const base = qkv + (size_t)b * N * QKV + head * HD;

    // ---- Q tile -> LDS -> registers, scaled by 1/8 (exact)
    for (int i = t; i < AQ * (HD / 4); i += 256) {
        const int row = i >> 4, c = (i & 15) * 4, q = q0 + row;
        put4(lds + row * SK + c, load4_or_zero(base + (size_t)q * QKV + c, q < N));
    }
    __syncthreads();
    float qr[HD / 2];
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) qr[s] = lds[(32 * w + r) * SK + 2 * s + h] * 0.125f;
    __syncthreads();

    f32x16 o0 = zero16(), o1 = zero16();
    float m = -INFINITY, lsum = 0.f;
    const int ntiles = (N + AK - 1) / AK;
    const int lrow = t >> 4, lc = (t & 15) * 4;   // this thread's key (plus 16 per pass) and d offset in a tile
    float4 rk[4], rv[4];
    fetch_kv(base, 0, N, lrow, lc, rk, rv);
    for (int tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            put4(sK + (lrow + 16 * p) * SK + lc, rk[p]);
            *reinterpret_cast<float4*>(sV + (lrow + 16 * p) * SV + lc) = rv[p];
        }
        __syncthreads();
        if (tile + 1 < ntiles) fetch_kv(base, tile + 1, N, lrow, lc, rk, rv);

        // ---- S^T [key][query] = K . Q^T: two blocks of 32 keys
        f32x16 s0 = zero16(), s1 = zero16();
        {
            const float* pk = sK + r * SK + h;
#pragma unroll
            for (int s = 0; s < HD / 2; ++s) {
                s0 = mfma(pk[2 * s], qr[s], s0);
                s1 = mfma(pk[32 * SK + 2 * s], qr[s], s1);
            }
        }
        const int kb = tile * AK;
        if (kb + AK > N) {   // the ragged last tile: -inf before the row maximum
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kb + crow(i, h);
                if (key >= N) s0[i] = -INFINITY;
                if (key + 32 >= N) s1[i] = -INFINITY;
            }
        }
        // ---- online softmax; the query is this lane's (both halves), the keys are split between the halves
        float mt = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mt = fmaxf(mt, fmaxf(s0[i], s1[i]));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);   // finite: key 0 is in the first tile
        const float alpha = exp2f((m - mn) * LOG2E);
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s0[i] = exp2f((s0[i] - mn) * LOG2E);
            s1[i] = exp2f((s1[i] - mn) * LOG2E);
            rs += s0[i] + s1[i];
        }
        lsum = lsum * alpha + rs;
        m = mn;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o0[i] *= alpha;
            o1[i] *= alpha;
        }
        // ---- O^T [d][query] += V^T . P^T: step s of key block j sums over keys 32 j + crow(s, h), which is what this lane's s_j[s] holds
        {
            const float* pv = sV + r;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int key = crow(s, h);
                o0 = mfma(pv[key * SV], s0[s], o0);
                o1 = mfma(pv[key * SV + 32], s0[s], o1);
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int key = 32 + crow(s, h);
                o0 = mfma(pv[key * SV], s1[s], o0);
                o1 = mfma(pv[key * SV + 32], s1[s], o1);
            }
        }
        __syncthreads();
    }

    const float ltot = lsum + __shfl_xor(lsum, 32);
    const int q = q0 + 32 * w + r;
    if (q < N) {   // the ragged last query tile does not store
        float* dst = out + ((size_t)b * N + q) * E + head * HD + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<float4*>(dst + 8 * g) = make_float4(o0[4 * g] / ltot, o0[4 * g + 1] / ltot, o0[4 * g + 2] / ltot, o0[4 * g + 3] / ltot);
            *reinterpret_cast<float4*>(dst + 32 + 8 * g) = make_float4(o1[4 * g] / ltot, o1[4 * g + 1] / ltot, o1[4 * g + 2] / ltot, o1[4 * g + 3] / ltot);
        }
    }
}

// ---- LayerNorm, leading tokens, final norm ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// y[lane + 64 j] of LayerNorm(x row); every lane of the wave takes part
__device__ __forceinline__ void ln_row(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta, float eps, int lane,
                                       float (&y)[E / 64]) {
    float v[E / 64], s = 0.f;
#pragma unroll
    for (int j = 0; j < E / 64; ++j) {
        v[j] = x[lane + 64 * j];
        s += v[j];
    }
    const float mean = wave_sum(s) * (1.f / E);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < E / 64; ++j) {
        v[j] -= mean;
        q += v[j] * v[j];
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / E) + eps);
#pragma unroll
    for (int j = 0; j < E / 64; ++j) y[j] = v[j] * rstd * g[lane + 64 * j] + bta[lane + 64 * j];
}

__global__ void __launch_bounds__(256) ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta, float eps,
                                                 float* __restrict__ y, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;   // uniform over the wave
    float o[E / 64];
    ln_row(x + (size_t)row * E, g, bta, eps, lane, o);
#pragma unroll
    for (int j = 0; j < E / 64; ++j) y[(size_t)row * E + lane + 64 * j] = o[j];
}

__global__ void __launch_bounds__(256) lead_kernel(const float* __restrict__ cls, const float* __restrict__ reg, const float* __restrict__ pos,
                                                   float* __restrict__ x, int B, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * LEAD * E) return;
    const int c = i % E, tok = (i / E) % LEAD, b = i / (E * LEAD);
    x[((size_t)b * N + tok) * E + c] = tok == 0 ? cls[c] + pos[c] : reg[(tok - 1) * E + c];
}

__global__ void __launch_bounds__(256) final_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta, float eps,
                                                    float* __restrict__ out, int N, int hw) {
    __shared__ float sT[E * FS];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, b = blockIdx.y, p0 = blockIdx.x * FT;
    for (int k = 0; k < FT / 4; ++k) {
        const int pr = w * (FT / 4) + k, p = p0 + pr;
        if (p >= hw) break;   // uniform over the wave
        float o[E / 64];
        ln_row(x + ((size_t)b * N + LEAD + p) * E, g, bta, eps, lane, o);
#pragma unroll
        for (int j = 0; j < E / 64; ++j) sT[(lane + 64 * j) * FS + pr] = o[j];
    }
    __syncthreads();
    for (int i = t; i < E * FT; i += 256) {
        const int c = i >> 5, pr = i & 31, p = p0 + pr;
        if (p < hw) out[((size_t)b * E + c) * hw + p] = sT[c * FS + pr];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int EP>
static int gemm(const GArgs& g, int tiling, hipStream_t stream) {
    const int big = ((g.M + GT - 1) / GT) * ((g.rows + GT - 1) / GT);   // workgroups of the 128 x 128 tiling
    if (tiling == WG_DINO_TILING_128 || (tiling == WG_DINO_TILING_AUTO && big >= GEMM_BIG_MIN_WORKGROUPS))
        hipLaunchKernelGGL((gemm_kernel<EP, 2>), dim3((g.M + GT - 1) / GT, (g.rows + GT - 1) / GT), dim3(256), 0, stream, g);
    else
        hipLaunchKernelGGL((gemm_kernel<EP, 1>), dim3((g.M + GT / 2 - 1) / (GT / 2), (g.rows + GT / 2 - 1) / (GT / 2)), dim3(256), 0, stream, g);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

static GArgs linear(const float* A, const float* Wt, const float* bias, float* Y, int rows, int K, int M) {
    GArgs g = {};
    g.A = A; g.Wt = Wt; g.bias = bias; g.Y = Y; g.rows = rows; g.K = K; g.M = M;
    return g;
}

static int attention(const float* qkv, int B, int N, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(attn_kernel, dim3((N + AQ - 1) / AQ, B * HEADS), dim3(256), 0, stream, qkv, out, N);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

static int layer_norm(const float* x, const float* g, const float* b, float eps, float* y, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, g, b, eps, y, rows);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

static int64_t scratch_floats(int64_t B, int64_t h, int64_t w) { return B * (LEAD + h * w) * WG_DINO_SCRATCH_FLOATS_PER_TOKEN; }

}  // namespace dino
}  // namespace wg

using namespace wg::dino;

extern "C" int64_t wg_dino_scratch_floats(int32_t B, int32_t h, int32_t w) {
    if (B < 0 || h < 0 || w < 0) return WG_ERR_INVALID_ARGUMENT;
    if ((int64_t)h * w > INT32_MAX / WG_DINO_SCRATCH_FLOATS_PER_TOKEN) return WG_ERR_OVERFLOW;
    const int64_t n = scratch_floats(B, h, w);
    return n > INT32_MAX ? WG_ERR_OVERFLOW : n;
}

extern "C" int wg_dino_attention(const float* qkv, int32_t B, int32_t N, float* out, void* stream) {
    if (!qkv || !out || B < 1 || N < 1 || !aligned16(qkv) || !aligned16(out)) return WG_ERR_INVALID_ARGUMENT;
    if ((int64_t)B * N * QKV > INT32_MAX || (int64_t)B * HEADS > 65535) return WG_ERR_INVALID_ARGUMENT;
    return attention(qkv, B, N, out, static_cast<hipStream_t>(stream));
}

extern "C" int wg_dino_features(const wg_dino_args* p) {
    if (!p || p->struct_size < sizeof(wg_dino_args)) return WG_ERR_INVALID_ARGUMENT;
    if (p->B < 1 || p->H < PS || p->W < PS || p->H % PS != 0 || p->W % PS != 0) return WG_ERR_INVALID_ARGUMENT;
    if (p->num_blocks < 1 || p->num_blocks > WG_DINO_MAX_BLOCKS || !(p->eps > 0.f)) return WG_ERR_INVALID_ARGUMENT;
    if (p->gemm_tiling < WG_DINO_TILING_AUTO || p->gemm_tiling > WG_DINO_TILING_128) return WG_ERR_INVALID_ARGUMENT;
    if (!p->image || !p->patch_w || !p->patch_b || !p->pos || !p->cls_token || !p->reg_tokens || !p->norm_w || !p->norm_b || !p->scratch || !p->out)
        return WG_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < p->num_blocks; ++i) {
        const wg_dino_block& k = p->blocks[i];
        if (!k.norm1_w || !k.norm1_b || !k.qkv_w || !k.qkv_b || !k.proj_w || !k.proj_b || !k.ls1 || !k.norm2_w || !k.norm2_b || !k.fc1_w || !k.fc1_b ||
            !k.fc2_w || !k.fc2_b || !k.ls2)
            return WG_ERR_INVALID_ARGUMENT;
        if (!aligned16(k.qkv_w) || !aligned16(k.proj_w) || !aligned16(k.fc1_w) || !aligned16(k.fc2_w)) return WG_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(p->scratch) || !aligned16(p->patch_w)) return WG_ERR_INVALID_ARGUMENT;
    const int h = p->H / PS, w = p->W / PS;
    if ((int64_t)p->B * 3 * p->H * p->W > INT32_MAX || (int64_t)p->B * HEADS > 65535) return WG_ERR_INVALID_ARGUMENT;
    const int64_t need = wg_dino_scratch_floats(p->B, h, w);
    if (need < 0 || p->scratch_floats < need) return WG_ERR_INVALID_ARGUMENT;

    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    const int hw = h * w, N = LEAD + hw, T = p->B * N;
    float* const X = p->scratch;               // the residual stream [B, N, 384]
    float* const Y = X + (size_t)T * E;        // LayerNorm output, then the attention output [B, N, 384]
    float* const Z = Y + (size_t)T * E;        // packed QKV [B, N, 1152], then the FFN's hidden layer [B, N, 1536]
    int st;

    hipLaunchKernelGGL(lead_kernel, dim3((p->B * LEAD * E + 255) / 256), dim3(256), 0, stream, p->cls_token, p->reg_tokens, p->pos, X, p->B, N);
    if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    {
        GArgs g = linear(p->image, p->patch_w, p->patch_b, X, p->B * hw, PK, E);
        g.res = p->pos; g.hw = hw; g.wq = w; g.H = p->H; g.W = p->W; g.N = N;
        if ((st = gemm<EP_PATCH>(g, p->gemm_tiling, stream)) != WG_OK) return st;
    }
    for (int i = 0; i < p->num_blocks; ++i) {
        const wg_dino_block& k = p->blocks[i];
        if ((st = layer_norm(X, k.norm1_w, k.norm1_b, p->eps, Y, T, stream)) != WG_OK) return st;
        if ((st = gemm<EP_BIAS>(linear(Y, k.qkv_w, k.qkv_b, Z, T, E, QKV), p->gemm_tiling, stream)) != WG_OK) return st;
        if ((st = attention(Z, p->B, N, Y, stream)) != WG_OK) return st;
        {
            GArgs g = linear(Y, k.proj_w, k.proj_b, X, T, E, E);
            g.gamma = k.ls1; g.res = X;
            if ((st = gemm<EP_RESIDUAL>(g, p->gemm_tiling, stream)) != WG_OK) return st;
        }
        if ((st = layer_norm(X, k.norm2_w, k.norm2_b, p->eps, Y, T, stream)) != WG_OK) return st;
        if ((st = gemm<EP_GELU>(linear(Y, k.fc1_w, k.fc1_b, Z, T, E, HID), p->gemm_tiling, stream)) != WG_OK) return st;
        {
            GArgs g = linear(Z, k.fc2_w, k.fc2_b, X, T, HID, E);
            g.gamma = k.ls2; g.res = X;
            if ((st = gemm<EP_RESIDUAL>(g, p->gemm_tiling, stream)) != WG_OK) return st;
        }
    }
    hipLaunchKernelGGL(final_kernel, dim3((hw + FT - 1) / FT, p->B), dim3(256), 0, stream, X, p->norm_w, p->norm_b, p->eps, p->out, N, hw);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}
