// Fused Adam step over a list of rows (include/wg_adam_rows.h): the optimizer step for the Gaussians a frame reached, the update rule of
// 3D-GS's sparse_adam / gsplat's SelectiveAdam with adam.hip's arithmetic.  A streaming kernel like adam.hip's: per listed element 4 B of
// index (shared by a row), 16 B read and 12 B written, nothing else; no LDS, no atomics.  One launch covers up to WG_ADAM_MAX_TENSORS row
// tensors: workgroup b finds its tensor in a prefix table of workgroup counts.  Within a tensor the work is the flat range count * width:
// consecutive lanes take consecutive floats of a row and then the next listed row, so a wide row (24, 45 floats) is one coalesced run and a
// narrow one (1, 3, 4) shares its wave instruction with its neighbours in the list.  The flat index is split into (entry, j) without an
// integer division (gfx950 has no divide instruction): once per workgroup a 64-bit multiply-high by a reciprocal the host computed, on
// wave-uniform values, and per element a 32-bit multiply-high of a number below 2048.
//
// In csrc/adam/, not next to adam.hip: the top level of csrc/ is the list of files bench.py's byte model names.  adam.hip's adam_one is
// restated below, so that adam.hip compiles from the text it always had; both files are built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "wg_adam_rows.h"
#include "wg_rasterizer.h"

namespace wg {

constexpr int ROWS_ADAM_THREADS = 256;
constexpr int ROWS_ADAM_PER_THREAD = 4;                                          // independent elements in flight per thread
constexpr uint32_t ROWS_ADAM_PER_BLOCK = ROWS_ADAM_THREADS * ROWS_ADAM_PER_THREAD;   // flat elements one workgroup updates
constexpr uint64_t ROWS_ADAM_MAGIC64_WIDTHS = 1ull << 20;                        // widths below this take the 64-bit reciprocal

struct AdamRowsBatch {
    wg_adam_tensor t[WG_ADAM_MAX_TENSORS];
    uint64_t width[WG_ADAM_MAX_TENSORS];
    uint64_t magic64[WG_ADAM_MAX_TENSORS];   // ceil(2^64 / width) for 2 <= width < 2^20, else 0: floor(n / width) = mulhi(n, magic) while n * width < 2^64
    uint32_t magic32[WG_ADAM_MAX_TENSORS];   // ceil(2^32 / width) for 2 <= width < ROWS_ADAM_PER_BLOCK, else 0: the same for n * width < 2^32
    uint32_t first_block[WG_ADAM_MAX_TENSORS + 1];   // exclusive prefix of the tensors' workgroup counts (sized by the list's capacity)
    const int32_t* rows;
    const int32_t* rows_count;
    int32_t M, P;
    int n;
};

// adam.hip's adam_one, statement for statement (torch/optim/adam.py's single-tensor update in float32)
__device__ __forceinline__ void adam_rows_one(float& p, float g, float& m, float& v, const wg_adam_tensor& d) {
    g = d.weight_decay != 0.0f ? g + d.weight_decay * p : g;
    m = m + d.one_minus_beta1 * (g - m);          // exp_avg.lerp_(grad, 1 - beta1)   (weight < 0.5: start + weight * (end - start))
    v = d.beta2 * v + d.one_minus_beta2 * (g * g);  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / d.bias_correction2_sqrt + d.eps;
    p = p - d.step_size * (m / denom);            // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ void __launch_bounds__(ROWS_ADAM_THREADS) adam_rows_kernel(const AdamRowsBatch batch) {
    // the workgroup's tensor: a short linear search over wave-uniform values (SGPRs), as fused_adam_kernel does
    int k = 0;
    while (k + 1 < batch.n && blockIdx.x >= batch.first_block[k + 1]) k++;
    const wg_adam_tensor& d = batch.t[k];
    const uint64_t w = batch.width[k];
    int32_t count = batch.M;
    if (batch.rows_count != nullptr) {   // M is the capacity: the real count lives on the device
        const int32_t c = *batch.rows_count;
        count = c < 0 ? 0 : (c > batch.M ? batch.M : c);
    }
    const uint64_t total = (uint64_t)count * w;   // < 2^31 * width, which the host holds below 2^41
    const uint64_t base = (uint64_t)(blockIdx.x - batch.first_block[k]) * ROWS_ADAM_PER_BLOCK;
    if (base >= total) return;   // a workgroup the capacity paid for and the count does not need
    // (entry0, j0) of the workgroup's first element; all wave-uniform.  base < 2^41 and width < 2^20 keep base * width below 2^64
    uint64_t entry0;
    if (w == 1) entry0 = base;
    else if (batch.magic64[k] != 0) entry0 = __umul64hi(base, batch.magic64[k]);
    else entry0 = base / w;   // rows of a million floats and more: once per workgroup, on uniform values
    const uint64_t j0 = base - entry0 * w;

    const int32_t* __restrict__ const rows = batch.rows;
    float* __restrict__ const P = d.param;
    const float* __restrict__ const G = d.grad;
    float* __restrict__ const M = d.exp_avg;
    float* __restrict__ const V = d.exp_avg_sq;
    const uint32_t magic32 = batch.magic32[k];

    // every load of the thread is requested before anything is computed or stored: the row indices first, then p, g, m, v of
    // ROWS_ADAM_PER_THREAD independent elements (adam.hip's discipline; the arrays may alias as far as the compiler knows)
    bool ok[ROWS_ADAM_PER_THREAD];
    uint64_t j[ROWS_ADAM_PER_THREAD];
    int32_t row[ROWS_ADAM_PER_THREAD];
#pragma unroll
    for (int r = 0; r < ROWS_ADAM_PER_THREAD; r++) {
        const uint32_t lane = (uint32_t)r * ROWS_ADAM_THREADS + threadIdx.x;
        ok[r] = base + lane < total;   // then entry0 + e < count
        uint64_t e;
        if (w < ROWS_ADAM_PER_BLOCK) {   // local < width + 1024 < 2048: local * width < 2^21
            const uint32_t local = (uint32_t)j0 + lane;
            const uint32_t q = w == 1 ? local : __umulhi(local, magic32);
            e = q;
            j[r] = local - q * (uint32_t)w;
        } else {   // local < 2 * width
            const uint64_t local = j0 + lane;
            const bool next = local >= w;
            e = next ? 1 : 0;
            j[r] = next ? local - w : local;
        }
        row[r] = ok[r] ? rows[entry0 + e] : -1;
    }
    size_t off[ROWS_ADAM_PER_THREAD];
    float p[ROWS_ADAM_PER_THREAD], g[ROWS_ADAM_PER_THREAD], m[ROWS_ADAM_PER_THREAD], v[ROWS_ADAM_PER_THREAD];
#pragma unroll
    for (int r = 0; r < ROWS_ADAM_PER_THREAD; r++) {
        ok[r] = ok[r] && (uint32_t)row[r] < (uint32_t)batch.P;   // an entry outside [0, P) is never dereferenced (P <= 2^31 - 1: negatives fail too)
        off[r] = (size_t)(uint32_t)row[r] * w + j[r];
        p[r] = g[r] = m[r] = v[r] = 0.0f;
        if (ok[r]) {
            p[r] = P[off[r]];
            g[r] = __builtin_nontemporal_load(G + off[r]);   // read once, by nobody else
            m[r] = M[off[r]];
            v[r] = V[off[r]];
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS_ADAM_PER_THREAD; r++) adam_rows_one(p[r], g[r], m[r], v[r], d);
#pragma unroll
    for (int r = 0; r < ROWS_ADAM_PER_THREAD; r++) {
        if (ok[r]) {
            P[off[r]] = p[r];
            M[off[r]] = m[r];
            V[off[r]] = v[r];
        }
    }
}

}  // namespace wg

extern "C" int wg_adam_rows_step(int n_tensors, const wg_adam_rows_tensor* tensors, int64_t P, const int32_t* rows, int64_t M,
                                 const int32_t* rows_count, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr)) return WG_ERR_INVALID_ARGUMENT;
    if (P < 0 || P > 0x7fffffffll || M < 0 || M > 0x7fffffffll) return WG_ERR_INVALID_ARGUMENT;
    if (M > 0 && rows == nullptr) return WG_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n_tensors; i++) {
        const wg_adam_rows_tensor& r = tensors[i];
        const wg_adam_tensor& d = r.t;
        if (r.width < 1) return WG_ERR_INVALID_ARGUMENT;
        const uint64_t w = (uint64_t)r.width;
        if (P == 0 ? d.numel != 0 : (w > SIZE_MAX / (uint64_t)P || d.numel != (size_t)P * w)) return WG_ERR_INVALID_ARGUMENT;
        if (d.numel == 0) continue;
        if (!d.param || !d.grad || !d.exp_avg || !d.exp_avg_sq) return WG_ERR_INVALID_ARGUMENT;
        if (!(d.bias_correction2_sqrt > 0.0f) || !(d.one_minus_beta1 < 0.5f)) return WG_ERR_INVALID_ARGUMENT;  // as wg_fused_adam
        if (M > 0 && w > 0x7fffffffull * wg::ROWS_ADAM_PER_BLOCK / (uint64_t)M) return WG_ERR_INVALID_ARGUMENT;   // the grid limit, per tensor
    }
    if (M == 0 || n_tensors == 0) return WG_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int i = 0;
    while (i < n_tensors) {
        wg::AdamRowsBatch b;
        b.n = 0;
        b.rows = rows;
        b.rows_count = rows_count;
        b.M = (int32_t)M;
        b.P = (int32_t)P;
        uint64_t blocks = 0;
        while (i < n_tensors && b.n < WG_ADAM_MAX_TENSORS) {
            const wg_adam_rows_tensor& r = tensors[i];
            if (r.t.numel == 0) { i++; continue; }
            const uint64_t w = (uint64_t)r.width;
            const uint64_t nb = ((uint64_t)M * w + wg::ROWS_ADAM_PER_BLOCK - 1) / wg::ROWS_ADAM_PER_BLOCK;   // >= 1 and <= 2^31 - 1 (checked above)
            if (blocks + nb > 0x7fffffffull) break;  // grid limit: the rest goes into the next launch
            b.t[b.n] = r.t;
            b.width[b.n] = w;
            b.magic64[b.n] = (w >= 2 && w < wg::ROWS_ADAM_MAGIC64_WIDTHS) ? ~0ull / w + 1 : 0;
            b.magic32[b.n] = (w >= 2 && w < wg::ROWS_ADAM_PER_BLOCK) ? (uint32_t)(0xffffffffull / w + 1) : 0;
            b.first_block[b.n] = (uint32_t)blocks;
            blocks += nb;
            b.n++;
            i++;
        }
        if (b.n == 0) break;   // only empty tensors were left (a single tensor always fits a launch: checked above)
        b.first_block[b.n] = (uint32_t)blocks;
        hipLaunchKernelGGL(wg::adam_rows_kernel, dim3((uint32_t)blocks), dim3(wg::ROWS_ADAM_THREADS), 0, s, b);
        if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    }
    return WG_OK;
}
