// Fused appearance MLP, forward and backward (include/wg_appearance_mlp.h): K -> 128 -> 128 -> 6 in float32 on the matrix cores.
// Reference semantics: EmbeddingModel.forward (wildgaussians/method.py:890-897) up to `* 0.01`, and autograd's backward of it.
//
// One persistent workgroup of 4 waves per compute unit keeps all weights in LDS (W1 [128][65], W2 [128][129], W3 [6][129]: odd row
// strides, so that both W[i][k] with i on the lanes and W[k][i] with i on the lanes read conflict-free) and walks 64-row tiles as two
// halves of 32 rows.  Every product is a chain of v_mfma_f32_32x32x2_f32 with the DATA ROW on the lanes (n = lane & 31):
//     Z^T [units, rows] = W [units, k] . H^T [k, rows]
// so a wave owns 32 output units x 32 rows in one 16-register accumulator and writes them back to an LDS image T[unit][row] (row stride
// 33) that is the next product's B operand as it stands.  The backward pass recomputes h1, h2 in these images, then overwrites them in
// place with dz2, dz1 (each element is read for its ReLU mask and written by the same lane), and feeds the weight-gradient products
//     dW [units_out, units_in] += dZ^T [units_out, rows] . H [rows, units_in]
// from the same images (A and B both with the unit on the lanes).  dW2 (4 accumulators), dW1 (2) and dW3 (1) stay in registers for the
// whole launch; each workgroup writes one partial and reduce_kernel sums the partials in workgroup order.  No atomics.
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include "wg_appearance_mlp.h"
#include "wg_rasterizer.h"

namespace wg {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HID = WG_MLP_HIDDEN, NOUT = WG_MLP_OUT, KMAX = WG_MLP_MAX_WIDTH, SUB = 32;
constexpr int TS = SUB + 1;    // row stride of the activation images T[unit][row]
constexpr int S1 = KMAX + 1;   // row stride of W1 in LDS
constexpr int S2 = HID + 1;    // row stride of W2 and W3 in LDS
// LDS map, in floats
constexpr int O_W1 = 0;
constexpr int O_W2 = O_W1 + HID * S1;
constexpr int O_W3 = O_W2 + HID * S2;
constexpr int O_B1 = O_W3 + NOUT * S2;
constexpr int O_B2 = O_B1 + HID;
constexpr int O_B3 = O_B2 + HID;
constexpr int O_X = O_B3 + 8;               // x^T   [64][33]
constexpr int O_H1 = O_X + KMAX * TS;       // h1^T, later dz1^T [128][33]
constexpr int O_H2 = O_H1 + HID * TS;       // h2^T, later dz2^T, later the two K-halves of dx^T [2][64][33]
constexpr int O_D3 = O_H2 + HID * TS;       // dz3^T [8][33], rows 6 and 7 zero
constexpr int O_P3 = O_D3 + 8 * TS;         // forward: the four K-quarters of z3^T [4][6][33]
constexpr int LDS_FLOATS = O_P3 + 4 * NOUT * TS;
static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "LDS image exceeds a compute unit's 160 KiB");
// one workgroup's partial, in floats (WG_MLP_PARTIAL_FLOATS)
constexpr int P_W1 = 0;
constexpr int P_W2 = P_W1 + HID * KMAX;
constexpr int P_W3 = P_W2 + HID * HID;
constexpr int P_B1 = P_W3 + NOUT * HID;
constexpr int P_B2 = P_B1 + HID;
constexpr int P_B3 = P_B2 + HID;
static_assert(P_B3 + 8 == WG_MLP_PARTIAL_FLOATS, "partial layout and header disagree");
static_assert(WG_MLP_TILE_ROWS == 2 * SUB, "a row tile is two 32-row halves");

struct KArgs {
    long long P;
    int Kr, E, K;            // per-row width, shared width, K = Kr + E (W1's row length)
    int beg1, beg2;          // first column of segments 1 and 2 (Kr where the segment is absent)
    const float *seg0, *seg1, *seg2;
    long long str0, str1, str2;
    const float* shared;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    float out_scale;
    float* out;
    const float* dout;
    float *g0, *g1, *g2;
    long long gs0, gs1, gs2;
    float* partial;
    int need_dx;
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

template <bool BWD, bool WGRAD>
__global__ void __launch_bounds__(256) mlp_kernel(const KArgs a) {
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
    __syncthreads();

    f32x16 aW2[4], aW1[2], aW3;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        aW3[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) aW2[j][i] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) aW1[j][i] = 0.f;
    }
    float db1 = 0.f, db2 = 0.f, db3 = 0.f;
    const int ks1 = ((a.Kr + 7) >> 3) << 2;   // k-steps of layer 1, a multiple of 4; columns >= Kr are zero in sW1 and sX
    const long long ntiles = (a.P + WG_MLP_TILE_ROWS - 1) / WG_MLP_TILE_ROWS;

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int sub = 0; sub < 2; ++sub) {
            const long long row0 = tile * WG_MLP_TILE_ROWS + sub * SUB;
            if (row0 >= a.P) break;   // uniform over the workgroup
            const int nvalid = (int)((a.P - row0) < SUB ? (a.P - row0) : SUB);

            // ---- 1. x^T -> LDS (rows past P and columns past Kr are zero)
            for (int i = t; i < SUB * KMAX; i += 256) {
                const int k = i & 63, row = i >> 6;
                float v = 0.f;
                if (row < nvalid && k < a.Kr) {
                    const long long gr = row0 + row;
                    if (k >= a.beg2) v = a.seg2[gr * a.str2 + (k - a.beg2)];
                    else if (k >= a.beg1) v = a.seg1[gr * a.str1 + (k - a.beg1)];
                    else v = a.seg0[gr * a.str0 + k];
                }
                sX[k * TS + row] = v;
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

            if (!BWD) {
                // ---- 4. z3^T [6 (of 32), rows] = W3 . h2^T, the K = 128 sum split in quarters over the waves, then summed in wave order
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
                __syncthreads();
                if (t < nvalid * NOUT) {
                    const int row = t / NOUT, o = t - row * NOUT;
                    const float z = (((sP3[o * TS + row] + sP3[(NOUT + o) * TS + row]) + sP3[(2 * NOUT + o) * TS + row]) +
                                     sP3[(3 * NOUT + o) * TS + row]) + sB3[o];
                    a.out[row0 * NOUT + t] = z * a.out_scale;
                }
                continue;   // the next half's barriers order every reuse of these images
            }

            // ---- B4. dz3^T = out_scale * dL_dout^T (rows past P zero: they then contribute exact zeros everywhere)
            if (t < SUB * NOUT) {
                const int row = t / NOUT, o = t - row * NOUT;
                sD3[o * TS + row] = row < nvalid ? a.dout[row0 * NOUT + t] * a.out_scale : 0.f;
            }
            __syncthreads();

            // ---- B5. dW3 [6 (of 32), units of this wave] += dz3^T . h2;  db3
            if (WGRAD) {
                const float* pb = sH2 + (32 * w + r) * TS + h;
#pragma unroll 8
                for (int s = 0; s < SUB / 2; ++s) {
                    const float av = r < NOUT ? sD3[r * TS + 2 * s + h] : 0.f;
                    aW3 = mfma(av, pb[2 * s], aW3);
                }
                if (t < NOUT)
                    for (int row = 0; row < SUB; ++row) db3 += sD3[t * TS + row];
            }
            // ---- B6. dz2^T = (W3^T . dz3^T) masked by h2 > 0, in place over h2^T.  B5 above read only this wave's 32 units of the image
            // and this step writes only those, so no barrier is needed between the two.
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

            // ---- B7. dW2 [units of this wave, all 128] += dz2^T . h1;  db2
            if (WGRAD) {
                const float* pa = sH2 + (32 * w + r) * TS + h;
                const float* pb = sH1 + r * TS + h;
#pragma unroll 4
                for (int s = 0; s < SUB / 2; ++s) {
                    const float av = pa[2 * s];
#pragma unroll
                    for (int j = 0; j < 4; ++j) aW2[j] = mfma(av, pb[32 * j * TS + 2 * s], aW2[j]);
                }
                if (t < HID)
                    for (int row = 0; row < SUB; ++row) db2 += sH2[t * TS + row];
            }
            // ---- B8. dz1^T = (W2^T . dz2^T) masked by h1 > 0, in place over h1^T once every wave is through B7
            {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const float* pa = sW2 + h * S2 + 32 * w + r;
                const float* pb = sH2 + h * TS + r;
#pragma unroll 8
                for (int s = 0; s < HID / 2; ++s) acc = mfma(pa[2 * s * S2], pb[2 * s * TS], acc);
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int idx = (32 * w + crow(i, h)) * TS + r;
                    sH1[idx] = sH1[idx] > 0.f ? acc[i] : 0.f;
                }
            }
            __syncthreads();

            // ---- B9. dW1 [units of this wave, 64 columns] += dz1^T . x;  db1 (always: the shared segment's gradient comes from it)
            if (WGRAD) {
                const float* pa = sH1 + (32 * w + r) * TS + h;
                const float* pb = sX + r * TS + h;
#pragma unroll 4
                for (int s = 0; s < SUB / 2; ++s) {
                    const float av = pa[2 * s];
#pragma unroll
                    for (int j = 0; j < 2; ++j) aW1[j] = mfma(av, pb[32 * j * TS + 2 * s], aW1[j]);
                }
            }
            if (t < HID)
                for (int row = 0; row < SUB; ++row) db1 += sH1[t * TS + row];

            // ---- B10. dx^T [64 columns, rows] = W1^T . dz1^T: wave (mt, kh) takes 32 columns and one half of the 128-unit sum; the two
            // halves meet in the (now free) h2 image and are added on the way out
            if (a.need_dx) {
                const int mt = w & 1, kh = w >> 1;
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                const float* pa = sW1 + (64 * kh + h) * S1 + 32 * mt + r;
                const float* pb = sH1 + (64 * kh + h) * TS + r;
#pragma unroll 8
                for (int s = 0; s < 32; ++s) acc = mfma(pa[2 * s * S1], pb[2 * s * TS], acc);
#pragma unroll
                for (int i = 0; i < 16; ++i) sH2[(kh * KMAX + 32 * mt + crow(i, h)) * TS + r] = acc[i];
                __syncthreads();
                for (int i = t; i < SUB * KMAX; i += 256) {
                    const int k = i & 63, row = i >> 6;
                    if (row < nvalid && k < a.Kr) {
                        const long long gr = row0 + row;
                        const float v = sH2[k * TS + row] + sH2[(KMAX + k) * TS + row];
                        if (k >= a.beg2) { if (a.g2) a.g2[gr * a.gs2 + (k - a.beg2)] = v; }
                        else if (k >= a.beg1) { if (a.g1) a.g1[gr * a.gs1 + (k - a.beg1)] = v; }
                        else if (a.g0) a.g0[gr * a.gs0 + k] = v;
                    }
                }
            }
            __syncthreads();
        }
    }

    if (BWD) {
        float* part = a.partial + (size_t)blockIdx.x * WG_MLP_PARTIAL_FLOATS;
        if (WGRAD) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = 32 * w + crow(i, h);
#pragma unroll
                for (int j = 0; j < 4; ++j) part[P_W2 + m * HID + 32 * j + r] = aW2[j][i];
#pragma unroll
                for (int j = 0; j < 2; ++j) part[P_W1 + m * KMAX + 32 * j + r] = aW1[j][i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = i + 4 * h;
                if (m < NOUT) part[P_W3 + m * HID + 32 * w + r] = aW3[i];
            }
            if (t < HID) part[P_B2 + t] = db2;
            if (t < 8) part[P_B3 + t] = t < NOUT ? db3 : 0.f;
        }
        if (t < HID) part[P_B1 + t] = db1;
    }
}

struct RArgs {
    const float* partial;
    int nwg, Kr, E, K, wgrad;
    float* head;   // [128] the summed db1
    float *dW1, *db1, *dW2, *db2, *dW3, *db3;
    const float *W1, *shared;
    float* grad_shared;
};

// element q of the partial layout, summed over the workgroups in workgroup order, to its place in the outputs
__global__ void __launch_bounds__(256) reduce_kernel(const RArgs a, int qbeg, int qend) {
    const int q = qbeg + blockIdx.x * 256 + threadIdx.x;
    if (q >= qend) return;
    float s = 0.f;
    for (int g = 0; g < a.nwg; ++g) s += a.partial[(size_t)g * WG_MLP_PARTIAL_FLOATS + q];
    if (q >= P_B1 && q < P_B2) {
        a.head[q - P_B1] = s;
        if (a.wgrad) a.db1[q - P_B1] = s;
        return;
    }
    if (!a.wgrad) return;
    if (q < P_W2) {
        const int u = q >> 6, c = q & 63;
        if (c < a.Kr) a.dW1[(size_t)u * a.K + c] = s;
    } else if (q < P_W3) a.dW2[q - P_W2] = s;
    else if (q < P_B1) a.dW3[q - P_W3] = s;
    else if (q < P_B3) a.db2[q - P_B2] = s;
    else if (q < P_B3 + NOUT) a.db3[q - P_B3] = s;
}

// the shared segment: dW1[:, Kr + j] = db1 (x) e and dL/de = W1[:, shared]^T . db1, from the summed db1
__global__ void __launch_bounds__(256) shared_kernel(const RArgs a) {
    const int t = threadIdx.x;
    if (a.wgrad)
        for (int i = t; i < HID * a.E; i += 256) {
            const int u = i / a.E, j = i - u * a.E;
            a.dW1[(size_t)u * a.K + a.Kr + j] = a.head[u] * a.shared[j];
        }
    if (a.grad_shared && t < a.E) {
        float s = 0.f;
        for (int u = 0; u < HID; ++u) s = fmaf(a.W1[(size_t)u * a.K + a.Kr + t], a.head[u], s);
        a.grad_shared[t] = s;
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

static int workgroups_for(int64_t P, int32_t max_workgroups, int64_t* nwg) {
    if (P < 0 || max_workgroups < 0) return WG_ERR_INVALID_ARGUMENT;
    const int64_t tiles = (P + WG_MLP_TILE_ROWS - 1) / WG_MLP_TILE_ROWS;
    int cap = max_workgroups;
    if (cap == 0 && tiles > 0) {
        const int st = device_workgroups(&cap);
        if (st != WG_OK) return st;
    }
    *nwg = tiles < cap ? tiles : (tiles == 0 ? 0 : cap);
    return WG_OK;
}

// everything that can be judged without a device; fills the kernel's arguments
static int check(const wg_appearance_mlp_args* p, bool bwd, KArgs* k) {
    if (!p || p->struct_size < sizeof(wg_appearance_mlp_args)) return WG_ERR_INVALID_ARGUMENT;
    if (p->P < 0 || p->max_workgroups < 0) return WG_ERR_INVALID_ARGUMENT;
    if (p->num_segments < 1 || p->num_segments > WG_MLP_MAX_SEGMENTS) return WG_ERR_INVALID_ARGUMENT;
    if (p->shared_width < 0 || p->shared_width > WG_MLP_MAX_WIDTH || (p->shared_width > 0) != (p->shared != nullptr)) return WG_ERR_INVALID_ARGUMENT;
    int beg[WG_MLP_MAX_SEGMENTS + 1] = {0, 0, 0, 0};
    for (int i = 0; i < p->num_segments; ++i) {
        const wg_appearance_mlp_segment& s = p->segments[i];
        if (s.width < 1 || s.width > WG_MLP_MAX_WIDTH || s.row_stride < s.width || (p->P > 0 && !s.ptr)) return WG_ERR_INVALID_ARGUMENT;
        beg[i + 1] = beg[i] + s.width;
        if (beg[i + 1] > WG_MLP_MAX_WIDTH) return WG_ERR_INVALID_ARGUMENT;
        if (bwd && p->grad_segment[i] && p->grad_row_stride[i] < s.width) return WG_ERR_INVALID_ARGUMENT;
    }
    if (!p->W1 || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3) return WG_ERR_INVALID_ARGUMENT;
    if (!bwd && p->P > 0 && !p->out) return WG_ERR_INVALID_ARGUMENT;
    if (bwd) {
        if (p->P > 0 && !p->dL_dout) return WG_ERR_INVALID_ARGUMENT;
        const int n = (p->dW1 != nullptr) + (p->db1 != nullptr) + (p->dW2 != nullptr) + (p->db2 != nullptr) + (p->dW3 != nullptr) + (p->db3 != nullptr);
        if (n != 0 && n != 6) return WG_ERR_INVALID_ARGUMENT;
        if (p->grad_shared && p->shared_width == 0) return WG_ERR_INVALID_ARGUMENT;
        if (!p->scratch || p->scratch_floats < WG_MLP_SCRATCH_HEAD_FLOATS) return WG_ERR_INVALID_ARGUMENT;
    }
    const int ns = p->num_segments, Kr = beg[ns];
    k->P = p->P; k->Kr = Kr; k->E = p->shared_width; k->K = Kr + p->shared_width;
    k->beg1 = ns > 1 ? beg[1] : Kr; k->beg2 = ns > 2 ? beg[2] : Kr;
    k->seg0 = p->segments[0].ptr; k->str0 = p->segments[0].row_stride;
    k->seg1 = ns > 1 ? p->segments[1].ptr : nullptr; k->str1 = ns > 1 ? p->segments[1].row_stride : 0;
    k->seg2 = ns > 2 ? p->segments[2].ptr : nullptr; k->str2 = ns > 2 ? p->segments[2].row_stride : 0;
    k->shared = p->shared;
    k->W1 = p->W1; k->b1 = p->b1; k->W2 = p->W2; k->b2 = p->b2; k->W3 = p->W3; k->b3 = p->b3;
    k->out_scale = p->out_scale; k->out = p->out; k->dout = nullptr;
    k->g0 = k->g1 = k->g2 = nullptr; k->gs0 = k->gs1 = k->gs2 = 0; k->partial = nullptr; k->need_dx = 0;
    if (bwd) {
        k->dout = p->dL_dout;
        k->g0 = p->grad_segment[0]; k->gs0 = p->grad_row_stride[0];
        if (ns > 1) { k->g1 = p->grad_segment[1]; k->gs1 = p->grad_row_stride[1]; }
        if (ns > 2) { k->g2 = p->grad_segment[2]; k->gs2 = p->grad_row_stride[2]; }
        k->need_dx = (k->g0 || k->g1 || k->g2) ? 1 : 0;
        k->partial = p->scratch + WG_MLP_SCRATCH_HEAD_FLOATS;
    }
    return WG_OK;
}

template <bool BWD, bool WGRAD>
static int launch(const KArgs& k, int nwg, hipStream_t stream) {
    const void* fn = reinterpret_cast<const void*>(mlp_kernel<BWD, WGRAD>);
    const int st = ensure_lds(fn);
    if (st != WG_OK) return st;
    hipLaunchKernelGGL((mlp_kernel<BWD, WGRAD>), dim3(nwg), dim3(256), LDS_FLOATS * sizeof(float), stream, k);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // namespace mlp
}  // namespace wg

extern "C" {

int64_t wg_appearance_mlp_scratch_floats(int64_t P, int32_t max_workgroups) {
    int64_t nwg = 0;
    const int st = wg::mlp::workgroups_for(P, max_workgroups, &nwg);
    if (st != WG_OK) return st;
    return WG_MLP_SCRATCH_HEAD_FLOATS + nwg * (int64_t)WG_MLP_PARTIAL_FLOATS;
}

int wg_appearance_mlp_forward(const wg_appearance_mlp_args* p) {
    using namespace wg::mlp;
    KArgs k;
    int st = check(p, false, &k);
    if (st != WG_OK) return st;
    if (p->P == 0) return WG_OK;
    int64_t nwg = 0;
    st = workgroups_for(p->P, p->max_workgroups, &nwg);
    if (st != WG_OK) return st;
    return launch<false, false>(k, (int)nwg, (hipStream_t)p->stream);
}

int wg_appearance_mlp_backward(const wg_appearance_mlp_args* p) {
    using namespace wg::mlp;
    KArgs k;
    int st = check(p, true, &k);
    if (st != WG_OK) return st;
    int64_t nwg = 0;
    st = workgroups_for(p->P, p->max_workgroups, &nwg);
    if (st != WG_OK) return st;
    if (p->scratch_floats < WG_MLP_SCRATCH_HEAD_FLOATS + nwg * (int64_t)WG_MLP_PARTIAL_FLOATS) return WG_ERR_INVALID_ARGUMENT;
    const bool wgrad = p->dW1 != nullptr;
    hipStream_t stream = (hipStream_t)p->stream;
    if (nwg > 0) {
        st = wgrad ? launch<true, true>(k, (int)nwg, stream) : launch<true, false>(k, (int)nwg, stream);
        if (st != WG_OK) return st;
    }
    RArgs r;
    r.partial = k.partial; r.nwg = (int)nwg; r.Kr = k.Kr; r.E = k.E; r.K = k.K; r.wgrad = wgrad ? 1 : 0;
    r.head = p->scratch;
    r.dW1 = p->dW1; r.db1 = p->db1; r.dW2 = p->dW2; r.db2 = p->db2; r.dW3 = p->dW3; r.db3 = p->db3;
    r.W1 = p->W1; r.shared = p->shared; r.grad_shared = p->grad_shared;
    const int qbeg = wgrad ? 0 : P_B1, qend = wgrad ? (int)WG_MLP_PARTIAL_FLOATS : P_B2;
    if (wgrad || p->grad_shared) {
        hipLaunchKernelGGL(reduce_kernel, dim3((qend - qbeg + 255) / 256), dim3(256), 0, stream, r, qbeg, qend);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    if (k.E > 0 && (wgrad || p->grad_shared)) {
        hipLaunchKernelGGL(shared_kernel, dim3(1), dim3(256), 0, stream, r);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    return WG_OK;
}

}  // extern "C"
