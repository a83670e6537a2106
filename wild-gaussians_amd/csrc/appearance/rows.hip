// The appearance MLP over a list of rows, forward and backward, and the device-side compaction that builds the list from `radii`
// (include/wg_appearance_rows.h).  mlp_kernel is mlp.hip's tile walk, statement for statement, with ONE difference: the 64 rows of a tile are
// not tile * 64 + 0..63 but the tile's 64 list entries, held in sRow (-1 for an entry past the count or outside [0, P): such a slot loads
// zeros, reads a zero cotangent and writes nothing).  Tiles, their assignment to workgroups, every MFMA chain and the order of the partials
// are the dense operator's on P = count rows, so the results have the bits of the dense operator on gathered inputs.  The count may live
// on the device (rows_count): the host then sizes the grid by the capacity, workgroups without a tile return at once, and the finishing
// pass sums min(ceil(count / 64), workgroups) partials.  The next tile's 64 indices are loaded into a register before the current tile's
// MFMA chains and stored to sRow (two images, alternating) after them, so that only the row loads, not index-then-row, sit in front of a tile.
// The device code is duplicated from mlp.hip on purpose: the dense kernels' code and resource usage stay untouched.
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <climits>
#include "wg_appearance_rows.h"
#include "wg_rasterizer.h"

namespace wg {
namespace rows {

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
constexpr int O_ROW = O_P3 + 4 * NOUT * TS;   // two tiles' 64 row indices (int), -1 = skipped; a workgroup's tiles alternate between them
constexpr int LDS_FLOATS = O_ROW + 2 * WG_MLP_TILE_ROWS;
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
    long long P, M;          // rows of the tensors; entries (or capacity) of the list
    const int* rows;
    const int* rows_count;   // NULL: M is the count
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

    long long cnt = a.M;
    if (a.rows_count) {
        const long long c = *a.rows_count;
        cnt = c < 0 ? 0 : (c < a.M ? c : a.M);
    }
    const long long ntiles = (cnt + WG_MLP_TILE_ROWS - 1) / WG_MLP_TILE_ROWS;
    if ((long long)blockIdx.x >= ntiles) return;   // uniform over the workgroup: no tile, no partial (the finishing pass does not read it)
    // the first tile's entries; from then on the next tile's are fetched one tile ahead
    int nxt = -1, image = 1;
    if (t < WG_MLP_TILE_ROWS) {
        const long long e = (long long)blockIdx.x * WG_MLP_TILE_ROWS + t;
        if (e < cnt) nxt = a.rows[e];
    }

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

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // ---- 0. the tile's rows, then the next tile's indices.  The image written is not the one the previous tile read (the forward pass
        // ends a tile without a barrier), and the one before that has this tile's barriers behind it
        image ^= 1;
        int* const sRow = reinterpret_cast<int*>(lds + O_ROW) + image * WG_MLP_TILE_ROWS;
        if (t < WG_MLP_TILE_ROWS) {
            sRow[t] = (nxt >= 0 && nxt < a.P) ? nxt : -1;
            const long long e = (tile + gridDim.x) * WG_MLP_TILE_ROWS + t;
            nxt = e < cnt ? a.rows[e] : -1;
        }
        __syncthreads();

        for (int sub = 0; sub < 2; ++sub) {
            if (tile * WG_MLP_TILE_ROWS + sub * SUB >= cnt) break;   // uniform over the workgroup
            const int* const rowp = sRow + sub * SUB;

            // ---- 1. x^T -> LDS (skipped slots and columns past Kr are zero)
            for (int i = t; i < SUB * KMAX; i += 256) {
                const int k = i & 63, row = i >> 6;
                float v = 0.f;
                const long long gr = rowp[row];
                if (gr >= 0 && k < a.Kr) {
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
                if (t < SUB * NOUT) {
                    const int row = t / NOUT, o = t - row * NOUT;
                    const long long gr = rowp[row];
                    if (gr >= 0) {
                    const float z = (((sP3[o * TS + row] + sP3[(NOUT + o) * TS + row]) + sP3[(2 * NOUT + o) * TS + row]) +
                                     sP3[(3 * NOUT + o) * TS + row]) + sB3[o];
                    a.out[gr * NOUT + o] = z * a.out_scale;
                    }
                }
                continue;   // the next half's barriers order every reuse of these images
            }

            // ---- B4. dz3^T = out_scale * dL_dout^T (skipped slots zero: they then contribute exact zeros everywhere)
            if (t < SUB * NOUT) {
                const int row = t / NOUT, o = t - row * NOUT;
                const long long gr = rowp[row];
                sD3[o * TS + row] = gr >= 0 ? a.dout[gr * NOUT + o] * a.out_scale : 0.f;
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
                    const long long gr = rowp[row];
                    if (gr >= 0 && k < a.Kr) {
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
    int nwg, Kr, E, K, wgrad;   // nwg: the grid of mlp_kernel
    long long M;
    const int* rows_count;      // NULL: M is the count
    float* head;   // [128] the summed db1
    float *dW1, *db1, *dW2, *db2, *dW3, *db3;
    const float *W1, *shared;
    float* grad_shared;
};

// element q of the partial layout, summed over the workgroups that had a tile, min(ceil(count / 64), grid), in workgroup order, to its place
// in the outputs
__global__ void __launch_bounds__(256) reduce_kernel(const RArgs a, int qbeg, int qend) {
    const int q = qbeg + blockIdx.x * 256 + threadIdx.x;
    if (q >= qend) return;
    long long cnt = a.M;
    if (a.rows_count) {
        const long long c = *a.rows_count;
        cnt = c < 0 ? 0 : (c < a.M ? c : a.M);
    }
    const long long ntiles = (cnt + WG_MLP_TILE_ROWS - 1) / WG_MLP_TILE_ROWS;
    const int n = ntiles < a.nwg ? (int)ntiles : a.nwg;
    float s = 0.f;
    for (int g = 0; g < n; ++g) s += a.partial[(size_t)g * WG_MLP_PARTIAL_FLOATS + q];
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

// the list's part of a call, then the dense operator's own checks; the grid is sized by the capacity M
static int check_rows(const wg_appearance_rows_args* p, bool bwd, KArgs* k, int64_t* nwg) {
    if (!p || p->struct_size < sizeof(wg_appearance_rows_args)) return WG_ERR_INVALID_ARGUMENT;
    if (!p->rows || p->M < 0 || p->M > INT_MAX) return WG_ERR_INVALID_ARGUMENT;
    int st = check(&p->mlp, bwd, k);
    if (st != WG_OK) return st;
    k->M = p->M; k->rows = p->rows; k->rows_count = p->rows_count;
    st = workgroups_for(p->M, p->mlp.max_workgroups, nwg);
    if (st != WG_OK) return st;
    if (bwd && p->mlp.scratch_floats < WG_MLP_SCRATCH_HEAD_FLOATS + *nwg * (int64_t)WG_MLP_PARTIAL_FLOATS) return WG_ERR_INVALID_ARGUMENT;
    return WG_OK;
}

// ---- compaction: count per block, scan of the block counts, scatter ------------------------------------------------------------------
constexpr int CB = WG_ROWS_COMPACT_BLOCK, CT = 256;
static_assert(CB % CT == 0, "a block of the compaction is whole passes of its workgroup");

__device__ __forceinline__ bool listed(const int* radii, const unsigned char* mask, long long i, long long P) {
    return i < P && (radii ? radii[i] > 0 : mask[i] != 0);
}

__global__ void __launch_bounds__(CT) count_kernel(long long P, const int* radii, const unsigned char* mask, int* block_count) {
    __shared__ int sw[CT / 64];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * CB;
    int n = 0;   // the same in every lane of a wave
    for (int it = 0; it < CB / CT; ++it) n += __popcll(__ballot(listed(radii, mask, base + it * CT + t, P)));
    if ((t & 63) == 0) sw[t >> 6] = n;
    __syncthreads();
    if (t == 0) block_count[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// one workgroup: block_count[0 .. nb) -> its exclusive prefix sums, in place; *count = the total
__global__ void __launch_bounds__(CT) scan_kernel(int nb, int* block_count, int* count) {
    __shared__ int s[CT];
    const int t = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += CT) {
        const int i = b0 + t;
        const int v = i < nb ? block_count[i] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < CT; d <<= 1) {
            const int x = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (i < nb) block_count[i] = carry + s[t] - v;
        carry += s[CT - 1];
        __syncthreads();
    }
    if (t == 0) *count = carry;
}

__global__ void __launch_bounds__(CT) scatter_kernel(long long P, const int* radii, const unsigned char* mask, const int* block_offset, int* rows) {
    __shared__ int sw[CT / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long base = (long long)blockIdx.x * CB;
    long long at = block_offset[blockIdx.x];
    for (int it = 0; it < CB / CT; ++it) {
        const long long i = base + it * CT + t;
        const bool f = listed(radii, mask, i, P);
        const unsigned long long b = __ballot(f);
        if (lane == 0) sw[wv] = __popcll(b);
        __syncthreads();
        long long to = at + __popcll(b & ((1ull << lane) - 1ull));
        for (int j = 0; j < wv; ++j) to += sw[j];
        if (f && to >= 0 && to < P) rows[to] = (int)i;   // to < count <= P by construction; the test costs nothing and keeps a store in bounds
        at += sw[0] + sw[1] + sw[2] + sw[3];
        __syncthreads();
    }
}

}  // namespace rows
}  // namespace wg

extern "C" {

int64_t wg_appearance_rows_scratch_floats(int64_t capacity, int32_t max_workgroups) {
    if (capacity > INT_MAX) return WG_ERR_INVALID_ARGUMENT;
    int64_t nwg = 0;
    const int st = wg::rows::workgroups_for(capacity, max_workgroups, &nwg);
    if (st != WG_OK) return st;
    return WG_MLP_SCRATCH_HEAD_FLOATS + nwg * (int64_t)WG_MLP_PARTIAL_FLOATS;
}

int wg_appearance_rows_forward(const wg_appearance_rows_args* p) {
    using namespace wg::rows;
    KArgs k;
    int64_t nwg = 0;
    const int st = check_rows(p, false, &k, &nwg);
    if (st != WG_OK) return st;
    if (nwg == 0 || p->mlp.P == 0) return WG_OK;   // no entry, or none that can be in range
    return launch<false, false>(k, (int)nwg, (hipStream_t)p->mlp.stream);
}

int wg_appearance_rows_backward(const wg_appearance_rows_args* p) {
    using namespace wg::rows;
    KArgs k;
    int64_t nwg = 0;
    int st = check_rows(p, true, &k, &nwg);
    if (st != WG_OK) return st;
    const wg_appearance_mlp_args& m = p->mlp;
    const bool wgrad = m.dW1 != nullptr;
    hipStream_t stream = (hipStream_t)m.stream;
    if (nwg > 0) {
        st = wgrad ? launch<true, true>(k, (int)nwg, stream) : launch<true, false>(k, (int)nwg, stream);
        if (st != WG_OK) return st;
    }
    RArgs r;
    r.partial = k.partial; r.nwg = (int)nwg; r.Kr = k.Kr; r.E = k.E; r.K = k.K; r.wgrad = wgrad ? 1 : 0;
    r.M = p->M; r.rows_count = p->rows_count;
    r.head = m.scratch;
    r.dW1 = m.dW1; r.db1 = m.db1; r.dW2 = m.dW2; r.db2 = m.db2; r.dW3 = m.dW3; r.db3 = m.db3;
    r.W1 = m.W1; r.shared = m.shared; r.grad_shared = m.grad_shared;
    const int qbeg = wgrad ? 0 : P_B1, qend = wgrad ? (int)WG_MLP_PARTIAL_FLOATS : P_B2;
    if (wgrad || m.grad_shared) {
        hipLaunchKernelGGL(reduce_kernel, dim3((qend - qbeg + 255) / 256), dim3(256), 0, stream, r, qbeg, qend);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    if (k.E > 0 && (wgrad || m.grad_shared)) {
        hipLaunchKernelGGL(shared_kernel, dim3(1), dim3(256), 0, stream, r);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    return WG_OK;
}

int64_t wg_appearance_rows_compact_scratch_bytes(int64_t P) {
    if (P < 0 || P > INT_MAX) return WG_ERR_INVALID_ARGUMENT;
    const int64_t nb = (P + WG_ROWS_COMPACT_BLOCK - 1) / WG_ROWS_COMPACT_BLOCK;
    return 4 * (nb > 0 ? nb : 1);
}

int wg_appearance_rows_compact(int64_t P, const int32_t* radii, const uint8_t* mask, int32_t* rows, int32_t* count, void* scratch,
                               int64_t scratch_bytes, void* stream_) {
    using namespace wg::rows;
    if (P < 0 || P > INT_MAX || !count || !scratch) return WG_ERR_INVALID_ARGUMENT;
    if (P > 0 && ((radii != nullptr) == (mask != nullptr) || !rows)) return WG_ERR_INVALID_ARGUMENT;
    if (radii && mask) return WG_ERR_INVALID_ARGUMENT;
    if (scratch_bytes < wg_appearance_rows_compact_scratch_bytes(P)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const int nb = (int)((P + CB - 1) / CB);
    int* const blocks = static_cast<int*>(scratch);
    if (nb > 0) {
        hipLaunchKernelGGL(count_kernel, dim3(nb), dim3(CT), 0, stream, (long long)P, radii, mask, blocks);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(CT), 0, stream, nb, blocks, count);
    if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    if (nb > 0) {
        hipLaunchKernelGGL(scatter_kernel, dim3(nb), dim3(CT), 0, stream, (long long)P, radii, mask, (const int*)blocks, rows);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    return WG_OK;
}

}  // extern "C"

