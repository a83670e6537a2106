// Fused toned-colour operator (include/wg_appearance_colour.h): appearance embedding -> [P, 3] precomputed colours, and dL_dcolours -> the
// embedding's gradient, over a list of rows.  Reference semantics: wildgaussians/method.py:1555, :1557, :890-900 and :1592-1598.
//
// The MLP is the persistent-workgroup tile walk of mlp.hip (same LDS images, same MFMA chains, same summation orders: read that file's
// head first) with three additions:
//   gather    a half tile is 32 entries of the row list; sRow holds the tile's 64 row indices, -1 for an entry past M or outside [0, P).
//             A -1 row loads zeros, writes nothing, and its dz3 is exact zeros, so it adds exact zeros to the row sum.
//   forward   after z3: 96 lanes, one per (row, channel), tone the row's 16 staged coefficients, clamp, and sum them against the SH
//             basis at the row's view direction.  colours[row, c] is the only write.
//   backward  forms z3 as well (mul and offset decide the clamp masks), the same 96 lanes turn dL_dcolours[row] into dz3, then steps B6
//             and B8 of mlp.hip run without weight-gradient accumulators and without dx.  Each workgroup writes its 128-float sum of dz1;
//             finish_kernel adds the partials in workgroup order and multiplies by W1[:, shared]^T.  No atomics.
// The row's 48 coefficients (192 contiguous bytes) are staged, pre-clamped, in LDS by the same pass that loads x, so the epilogue waits
// for no global load.
#include <hip/hip_runtime.h>
#include <climits>
#include <map>
#include <mutex>
#include "wg_appearance_colour.h"
#include "wg_rasterizer.h"

namespace wg {
namespace colour {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HID = 128, NOUT = 6, KMAX = WG_COLOUR_MAX_WIDTH, SUB = 32, NC = WG_COLOUR_COEFFS;
constexpr int TS = SUB + 1;    // row stride of the activation images T[unit][row]
constexpr int S1 = KMAX + 1;   // row stride of W1 in LDS
constexpr int S2 = HID + 1;    // row stride of W2 and W3 in LDS
constexpr int FS = NC + 1;     // row stride of the staged coefficients
// LDS map, in floats
constexpr int O_W1 = 0;
constexpr int O_W2 = O_W1 + HID * S1;
constexpr int O_W3 = O_W2 + HID * S2;
constexpr int O_B1 = O_W3 + NOUT * S2;
constexpr int O_B2 = O_B1 + HID;
constexpr int O_B3 = O_B2 + HID;
constexpr int O_X = O_B3 + 8;               // x^T   [64][33]
constexpr int O_H1 = O_X + KMAX * TS;       // h1^T, later dz1^T [128][33]
constexpr int O_H2 = O_H1 + HID * TS;       // h2^T, later dz2^T [128][33]
constexpr int O_D3 = O_H2 + HID * TS;       // dz3^T [8][33], rows 6 and 7 zero
constexpr int O_P3 = O_D3 + 8 * TS;         // the four K-quarters of z3^T [4][6][33]
constexpr int O_F = O_P3 + 4 * NOUT * TS;   // the half tile's coefficients, pre-clamped [32][49]
constexpr int O_V = O_F + SUB * FS;         // xyz - campos [32][3]
constexpr int O_ROW = O_V + SUB * 3;        // the tile's row indices [64] (int)
constexpr int LDS_FLOATS = O_ROW + WG_COLOUR_TILE_ROWS;
static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "LDS image exceeds a compute unit's 160 KiB");
static_assert(WG_COLOUR_TILE_ROWS == 2 * SUB, "a row tile is two 32-row halves");
static_assert(WG_COLOUR_PARTIAL_FLOATS == HID, "a partial is the 128 sums of dz1");

// eval_sh's constants (method.py:462-479), as csrc/sh_eval.hip holds them
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                            -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

struct KArgs {
    long long P, M;
    const int* rows;
    const float* features; long long fstr;
    const float* gemb; long long gstr;
    int G, Kr, E, K;         // Kr = 3 + G, K = Kr + E (W1's row length)
    int ncoef;               // (deg + 1)^2
    const float* shared;
    const float* xyz; long long xstr;
    const float* campos;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    float out_scale, pre, post;
    float* colours;
    const float* dcol;
    float* partial;
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
    return c;
#endif
}
// row of accumulator register i in the 32x32 result (the column is lane & 31)
__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// all 16 basis values at a direction: the polynomials of sh_eval.hip's sh_basis<3>; the caller uses the first (deg + 1)^2
__device__ __forceinline__ void sh_basis16(float x, float y, float z, float* b) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[0] = SH_C0;
    b[1] = -SH_C1 * y;
    b[2] = SH_C1 * z;
    b[3] = -SH_C1 * x;
    b[4] = SH_C2[0] * xy;
    b[5] = SH_C2[1] * yz;
    b[6] = SH_C2[2] * (2.0f * zz - xx - yy);
    b[7] = SH_C2[3] * xz;
    b[8] = SH_C2[4] * (xx - yy);
    b[9] = SH_C3[0] * y * (3.0f * xx - yy);
    b[10] = SH_C3[1] * xy * z;
    b[11] = SH_C3[2] * y * (4.0f * zz - xx - yy);
    b[12] = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    b[13] = SH_C3[4] * x * (4.0f * zz - xx - yy);
    b[14] = SH_C3[5] * z * (xx - yy);
    b[15] = SH_C3[6] * x * (xx - 3.0f * yy);
}

template <bool BWD>
__global__ void __launch_bounds__(256) colour_kernel(const KArgs a) {
    extern __shared__ float lds[];
    float* const sW1 = lds + O_W1;
    float* const sW2 = lds + O_W2;
    float* const sW3 = lds + O_W3;
    float* const sB1 = lds + O_B1;
    float* const sB2 = lds + O_B2;
    float* const sB3 = lds + O_B3;
    float* const sX = lds + O_X;
    float* const sH1 = lds + O_H1;
    float* const sH2 = lds + O_H2;
    float* const sD3 = lds + O_D3;
    float* const sP3 = lds + O_P3;
    float* const sF = lds + O_F;
    float* const sV = lds + O_V;
    int* const sRow = reinterpret_cast<int*>(lds + O_ROW);
    const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 31, h = l >> 5;

    // ---- weights -> LDS, once per workgroup; the shared segment folded into b1
    for (int i = t; i < HID * KMAX; i += 256) {
        const int u = i >> 6, k = i & 63;
        sW1[u * S1 + k] = k < a.Kr ? a.W1[(size_t)u * a.K + k] : 0.f;
    }
    for (int i = t; i < HID * HID; i += 256) sW2[(i >> 7) * S2 + (i & 127)] = a.W2[i];
    for (int i = t; i < NOUT * HID; i += 256) sW3[(i >> 7) * S2 + (i & 127)] = a.W3[i];
    if (t < HID) {
        float b = a.b1[t];
        for (int j = 0; j < a.E; ++j) b = fmaf(a.W1[(size_t)t * a.K + a.Kr + j], a.shared[j], b);
        sB1[t] = b;
        sB2[t] = a.b2[t];
    }
    if (t < 8) sB3[t] = t < NOUT ? a.b3[t] : 0.f;
    if (BWD)
        for (int i = t; i < 8 * TS; i += 256) sD3[i] = 0.f;
    const float cam0 = a.campos[0], cam1 = a.campos[1], cam2 = a.campos[2];

    float db1 = 0.f;
    const int ks1 = ((a.Kr + 7) >> 3) << 2;   // k-steps of layer 1, a multiple of 4; columns >= Kr are zero in sW1 and sX
    const long long ntiles = (a.M + WG_COLOUR_TILE_ROWS - 1) / WG_COLOUR_TILE_ROWS;

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // ---- 0. the tile's rows (the previous half's closing barrier has every reader of sRow behind it)
        if (t < WG_COLOUR_TILE_ROWS) {
            const long long e = tile * WG_COLOUR_TILE_ROWS + t;
            long long row = -1;
            if (e < a.M) row = a.rows ? (long long)a.rows[e] : e;
            sRow[t] = (row >= 0 && row < a.P) ? (int)row : -1;
        }
        __syncthreads();   // also orders the weights' image before its first use

        for (int sub = 0; sub < 2; ++sub) {
            if (tile * WG_COLOUR_TILE_ROWS + sub * SUB >= a.M) break;   // uniform over the workgroup
            const int* const rowp = sRow + sub * SUB;

            // ---- 1. x^T, the coefficients and xyz - campos -> LDS (skipped rows and columns past Kr are zero)
            for (int i = t; i < SUB * KMAX; i += 256) {
                const int k = i & 63, row = i >> 6;
                const int gr = rowp[row];
                float v = 0.f;
                if (gr >= 0 && k < a.Kr) {
                    if (k >= 3) v = a.gemb[gr * a.gstr + (k - 3)];
                    else {
                        v = a.features[gr * a.fstr + k];
                        v = v > a.pre ? a.pre : v;
                    }
                }
                sX[k * TS + row] = v;
            }
            for (int i = t; i < SUB * NC; i += 256) {
                const int row = i / NC, j = i - row * NC;
                const int gr = rowp[row];
                float v = 0.f;
                if (gr >= 0) {
                    v = a.features[gr * a.fstr + j];
                    v = v > a.pre ? a.pre : v;
                }
                sF[row * FS + j] = v;
            }
            if (t < SUB * 3) {
                const int row = t / 3, c = t - row * 3;
                const int gr = rowp[row];
                sV[t] = gr >= 0 ? a.xyz[gr * a.xstr + c] - (c == 0 ? cam0 : c == 1 ? cam1 : cam2) : 0.f;
            }
            __syncthreads();

            // ---- 2. h1^T = relu(W1 . x^T + b1')
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const float* pa = sW1 + (32 * w + r) * S1 + h;
                const float* pb = sX + h * TS + r;
#pragma unroll 4
                for (int s = 0; s < ks1; ++s) acc = mfma(pa[2 * s], pb[2 * s * TS], acc);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int u = 32 * w + crow(i, h);
                    const float v = acc[i] + sB1[u];
                    sH1[u * TS + r] = v <= 0.f ? 0.f : v;
                }
            }
            __syncthreads();

            // ---- 3. h2^T = relu(W2 . h1^T + b2)
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const float* pa = sW2 + (32 * w + r) * S2 + h;
                const float* pb = sH1 + h * TS + r;
#pragma unroll 8
                for (int s = 0; s < HID / 2; ++s) acc = mfma(pa[2 * s], pb[2 * s * TS], acc);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int u = 32 * w + crow(i, h);
                    const float v = acc[i] + sB2[u];
                    sH2[u * TS + r] = v <= 0.f ? 0.f : v;
                }
            }
            __syncthreads();

            // ---- 4. z3^T [6 (of 32), rows] = W3 . h2^T, the K = 128 sum split in quarters over the waves (each wave reads its own 32
            // units of the image), summed in wave order by the epilogue
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 8
                for (int s = 0; s < 16; ++s) {
                    const int k = 32 * w + 2 * s + h;
                    const float av = r < NOUT ? sW3[r * S2 + k] : 0.f;
                    acc = mfma(av, sH2[k * TS + r], acc);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = i + 4 * h;
                    if (m < NOUT) sP3[(w * NOUT + m) * TS + r] = acc[i];
                }
            }
            __syncthreads();

            // ---- 5. one lane per (row, channel): tone, clamp, SH sum; forward writes the colour, backward writes dz3^T
            if (t < SUB * 3) {
                const int row = t / 3, c = t - row * 3;
                const int gr = rowp[row];
                float d_off = 0.f, d_mul = 0.f;
                if (gr >= 0) {
                    const float z_off = (((sP3[c * TS + row] + sP3[(NOUT + c) * TS + row]) + sP3[(2 * NOUT + c) * TS + row]) +
                                         sP3[(3 * NOUT + c) * TS + row]) + sB3[c];
                    const float z_mul = (((sP3[(3 + c) * TS + row] + sP3[(NOUT + 3 + c) * TS + row]) + sP3[(2 * NOUT + 3 + c) * TS + row]) +
                                         sP3[(3 * NOUT + 3 + c) * TS + row]) + sB3[3 + c];
                    const float off = (z_off * a.out_scale) / SH_C0, mul = z_mul * a.out_scale;
                    const float vx = sV[row * 3], vy = sV[row * 3 + 1], vz = sV[row * 3 + 2];
                    const float len = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
                    float Y[16];
                    sh_basis16(vx / len, vy / len, vz / len, Y);
                    const float* f = sF + row * FS + c;
                    float sum = 0.f;
                    unsigned pass = 0;   // bit k: the unclamped t[k, c] is <= post
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (k < a.ncoef) {
                            float tv = f[3 * k] * mul;
                            if (k == 0) tv += off;
                            if (tv > a.post) tv = a.post;
                            else pass |= 1u << k;
                            sum = fmaf(Y[k], tv, sum);
                        }
                    const float col = 0.5f + sum;
                    if (!BWD) a.colours[(long long)gr * 3 + c] = col > 0.f ? col : 0.f;
                    else if (col > 0.f) {
                        const float g = a.dcol[(long long)gr * 3 + c];
#pragma unroll
                        for (int k = 0; k < 16; ++k)
                            if (k < a.ncoef && ((pass >> k) & 1u)) {
                                const float dt = Y[k] * g;
                                d_mul = fmaf(dt, f[3 * k], d_mul);
                                if (k == 0) d_off = dt / SH_C0;
                            }
                    }
                }
                if (BWD) {
                    sD3[c * TS + row] = d_off * a.out_scale;
                    sD3[(3 + c) * TS + row] = d_mul * a.out_scale;
                }
            }
            if (!BWD) {
                __syncthreads();   // closes the half: the next one overwrites every image read above
                continue;
            }
            __syncthreads();

            // ---- B6. dz2^T = (W3^T . dz3^T) masked by h2 > 0, in place over h2^T (each wave its own 32 units)
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {   // k = 0..7: dz3^T rows 6, 7 are zero; W3 has no rows 6, 7
                    const int k = 2 * s + h;
                    const float av = k < NOUT ? sW3[k * S2 + 32 * w + r] : 0.f;
                    acc = mfma(av, sD3[k * TS + r], acc);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int idx = (32 * w + crow(i, h)) * TS + r;
                    sH2[idx] = sH2[idx] > 0.f ? acc[i] : 0.f;
                }
            }
            __syncthreads();

            // ---- B8. dz1^T = (W2^T . dz2^T) masked by h1 > 0, in place over h1^T
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const float* pa = sW2 + h * S2 + 32 * w + r;
                const float* pb = sH2 + h * TS + r;
#pragma unroll 8
                for (int s = 0; s < HID / 2; ++s) acc = mfma(pa[2 * s * S2], pb[2 * s * TS], acc);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int idx = (32 * w + crow(i, h)) * TS + r;
                    sH1[idx] = sH1[idx] > 0.f ? acc[i] : 0.f;   // h1 is read by no other step of the backward half: no barrier before this
                }
            }
            __syncthreads();

            // ---- B9. the row sum of dz1 (skipped rows hold exact zeros)
            if (t < HID)
                for (int row = 0; row < SUB; ++row) db1 += sH1[t * TS + row];
            __syncthreads();
        }
    }

    if (BWD && t < HID) a.partial[(size_t)blockIdx.x * WG_COLOUR_PARTIAL_FLOATS + t] = db1;
}

// db1 = the partials added in workgroup order; grad_shared = W1[:, shared]^T . db1
__global__ void __launch_bounds__(128) finish_kernel(const float* partial, int nwg, const float* W1, int K, int Kr, int E, float* grad_shared) {
    __shared__ float head[HID];
    const int t = threadIdx.x;
    float s = 0.f;
    for (int g = 0; g < nwg; ++g) s += partial[(size_t)g * WG_COLOUR_PARTIAL_FLOATS + t];
    head[t] = s;
    __syncthreads();
    if (t < E) {
        float v = 0.f;
        for (int u = 0; u < HID; ++u) v = fmaf(W1[(size_t)u * K + Kr + t], head[u], v);
        grad_shared[t] = v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static std::mutex g_mu;

static int device_workgroups(int* out) {   // one workgroup per compute unit (the LDS image allows no more); cached per device
    static std::map<int, int> cus;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return WG_ERR_HIP; }
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = cus.find(dev);
    if (it == cus.end()) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); return WG_ERR_HIP; }
        it = cus.emplace(dev, n).first;
    }
    *out = it->second;
    return WG_OK;
}

static int ensure_lds(const void* fn) {
    static std::map<std::pair<int, const void*>, bool> granted;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return WG_ERR_HIP; }
    std::lock_guard<std::mutex> lock(g_mu);
    bool& have = granted[{dev, fn}];
    if (have) return WG_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_FLOATS * sizeof(float))) != hipSuccess) {
        (void)hipGetLastError();
        return WG_ERR_HIP;
    }
    have = true;
    return WG_OK;
}

static int workgroups_for(int64_t M, int32_t max_workgroups, int64_t* nwg) {
    if (M < 0 || max_workgroups < 0) return WG_ERR_INVALID_ARGUMENT;
    const int64_t tiles = (M + WG_COLOUR_TILE_ROWS - 1) / WG_COLOUR_TILE_ROWS;
    int cap = max_workgroups;
    if (cap == 0 && tiles > 0) {
        const int st = device_workgroups(&cap);
        if (st != WG_OK) return st;
    }
    *nwg = tiles < cap ? tiles : (tiles == 0 ? 0 : cap);
    return WG_OK;
}

// everything that can be judged without a device; fills the kernel's arguments
static int check(const wg_appearance_colour_args* p, bool bwd, KArgs* k) {
    if (!p || p->struct_size < sizeof(wg_appearance_colour_args)) return WG_ERR_INVALID_ARGUMENT;
    if (p->P < 0 || p->P > INT_MAX || p->M < 0 || p->max_workgroups < 0) return WG_ERR_INVALID_ARGUMENT;
    if (!p->rows && p->M > p->P) return WG_ERR_INVALID_ARGUMENT;
    if (p->deg < 0 || p->deg > 3) return WG_ERR_INVALID_ARGUMENT;
    const int G = p->gembedding_width;
    if (G < 0 || 3 + G > WG_COLOUR_MAX_WIDTH || (G > 0) != (p->gembedding != nullptr) || (G > 0 && p->gembedding_row_stride < G)) return WG_ERR_INVALID_ARGUMENT;
    if (p->shared_width < 1 || p->shared_width > WG_COLOUR_MAX_WIDTH || !p->shared) return WG_ERR_INVALID_ARGUMENT;
    if (!p->features || p->features_row_stride < WG_COLOUR_COEFFS) return WG_ERR_INVALID_ARGUMENT;
    if (!p->xyz || p->xyz_row_stride < 3 || !p->campos) return WG_ERR_INVALID_ARGUMENT;
    if (!p->W1 || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3) return WG_ERR_INVALID_ARGUMENT;
    if (!bwd && !p->colours) return WG_ERR_INVALID_ARGUMENT;
    if (bwd && (!p->dL_dcolours || !p->grad_shared || p->scratch_floats < 0)) return WG_ERR_INVALID_ARGUMENT;
    k->P = p->P; k->M = p->M; k->rows = p->rows;
    k->features = p->features; k->fstr = p->features_row_stride;
    k->gemb = p->gembedding; k->gstr = p->gembedding_row_stride;
    k->G = G; k->Kr = 3 + G; k->E = p->shared_width; k->K = 3 + G + p->shared_width;
    k->ncoef = (p->deg + 1) * (p->deg + 1);
    k->shared = p->shared;
    k->xyz = p->xyz; k->xstr = p->xyz_row_stride; k->campos = p->campos;
    k->W1 = p->W1; k->b1 = p->b1; k->W2 = p->W2; k->b2 = p->b2; k->W3 = p->W3; k->b3 = p->b3;
    k->out_scale = p->out_scale; k->pre = p->pre_clamp_max; k->post = p->post_clamp_max;
    k->colours = p->colours; k->dcol = bwd ? p->dL_dcolours : nullptr; k->partial = bwd ? p->scratch : nullptr;
    return WG_OK;
}

template <bool BWD>
static int launch(const KArgs& k, int nwg, hipStream_t stream) {
    const void* fn = reinterpret_cast<const void*>(colour_kernel<BWD>);
    const int st = ensure_lds(fn);
    if (st != WG_OK) return st;
    hipLaunchKernelGGL((colour_kernel<BWD>), dim3(nwg), dim3(256), LDS_FLOATS * sizeof(float), stream, k);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // namespace colour
}  // namespace wg

extern "C" {

int64_t wg_appearance_colour_scratch_floats(int64_t M, int32_t max_workgroups) {
    int64_t nwg = 0;
    const int st = wg::colour::workgroups_for(M, max_workgroups, &nwg);
    if (st != WG_OK) return st;
    return nwg * (int64_t)WG_COLOUR_PARTIAL_FLOATS;
}

int wg_appearance_colour_forward(const wg_appearance_colour_args* p) {
    using namespace wg::colour;
    KArgs k;
    int st = check(p, false, &k);
    if (st != WG_OK) return st;
    if (p->M == 0) return WG_OK;
    int64_t nwg = 0;
    st = workgroups_for(p->M, p->max_workgroups, &nwg);
    if (st != WG_OK) return st;
    return launch<false>(k, (int)nwg, (hipStream_t)p->stream);
}

int wg_appearance_colour_backward(const wg_appearance_colour_args* p) {
    using namespace wg::colour;
    KArgs k;
    int st = check(p, true, &k);
    if (st != WG_OK) return st;
    int64_t nwg = 0;
    st = workgroups_for(p->M, p->max_workgroups, &nwg);
    if (st != WG_OK) return st;
    const int64_t need = nwg * (int64_t)WG_COLOUR_PARTIAL_FLOATS;
    if (p->scratch_floats < need || (need > 0 && !p->scratch)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)p->stream;
    if (nwg > 0) {
        st = launch<true>(k, (int)nwg, stream);
        if (st != WG_OK) return st;
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(HID), 0, stream, (const float*)p->scratch, (int)nwg, p->W1, k.K, k.Kr, k.E, p->grad_shared);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // extern "C"
