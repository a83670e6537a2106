// Fused densification statistics (include/wg_densify.h).  Reference semantics:
// wildgaussians/method.py:1995-1998 and :1470-1477.  One Gaussian per lane; invisible Gaussians (radii <= 0) touch nothing
// but their radius, so a sparse view reads 4 B per Gaussian and the read-modify-write traffic scales with the visible count.
#include <hip/hip_runtime.h>
#include "wg_densify.h"
#include "wg_rasterizer.h"

namespace wg {

template <bool ABS, bool RADII>
__global__ void __launch_bounds__(256) densification_stats_kernel(int P, const int* __restrict__ radii, const float* __restrict__ grad,
                                                                  float* __restrict__ xyz_grad, float* __restrict__ accum_abs,
                                                                  float* __restrict__ accum_abs_max, float* __restrict__ denom,
                                                                  float* __restrict__ max_radii) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = grad[3 * i], gy = grad[3 * i + 1];
    xyz_grad[i] += sqrtf(gx * gx + gy * gy);  // torch.norm(g[:, :2], dim=-1)
    if (ABS) {
        const float n = fabsf(grad[3 * i + 2]);  // the norm of a single element
        accum_abs[i] += n;
        accum_abs_max[i] = fmaxf(accum_abs_max[i], n);
    }
    denom[i] += 1.0f;
    if (RADII) max_radii[i] = fmaxf(max_radii[i], (float)r);  // torch.max(float, int32) promotes to float
}

}  // namespace wg

extern "C" int wg_densification_stats(int P, const int* radii, const float* viewspace_grad, float* xyz_grad, float* xyz_gradient_accum_abs,
                                      float* xyz_gradient_accum_abs_max, float* denom, float* max_radii2D, void* stream) {
    if (P < 0 || P > 0x7fffffff / 4) return WG_ERR_INVALID_ARGUMENT;  // per-Gaussian element indices (3 i, 4 i) are 32-bit
    if (P == 0) return WG_OK;
    if (!radii || !viewspace_grad || !xyz_grad || !denom) return WG_ERR_INVALID_ARGUMENT;
    if ((xyz_gradient_accum_abs == nullptr) != (xyz_gradient_accum_abs_max == nullptr)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((P + 255) / 256), block(256);
    const bool a = xyz_gradient_accum_abs != nullptr, m = max_radii2D != nullptr;
#define WG_LAUNCH(A, M) \
    wg::densification_stats_kernel<A, M><<<grid, block, 0, s>>>(P, radii, viewspace_grad, xyz_grad, xyz_gradient_accum_abs, \
                                                                xyz_gradient_accum_abs_max, denom, max_radii2D)
    if (a && m) WG_LAUNCH(true, true);
    else if (a) WG_LAUNCH(true, false);
    else if (m) WG_LAUNCH(false, true);
    else WG_LAUNCH(false, false);
#undef WG_LAUNCH
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}


// ==== Fused densify-and-prune, its exact quantile and reset_opacity (include/wg_densify_prune.h) ==========================================
// Reference semantics: wildgaussians/method.py:1249-1468.  No FMA contraction from here to the end of the file (the kernel above keeps the
// file's default), as activations.hip is built: exp, sigmoid and the normalised quaternion are wg_act.h's functions and the remaining
// arithmetic follows the reference's statements operation for operation.
//
//   plan    ga + count  ->  4 x (histogram, pick)  ->  decide (one byte per Gaussian + five counts per block)  ->  scan of the block counts
//   apply   origin (source index and kind of every output row)  ->  ONE gather over a table of arrays
//
// Scratch: a header (selection state, totals), ga as floats (P; reused for the split ranks once Q is known), the decision bytes (P) and
// the per-block counts / offsets (2 x 5 x blocks).
#pragma clang fp contract(off)
#include <stdint.h>
#include "wg_act.h"

#ifndef WG_DENSIFY_NT_LOADS   // A/B: non-temporal loads of the source rows in the gather (EXPERIMENTS.md)
#define WG_DENSIFY_NT_LOADS 0
#endif

namespace wg {
namespace dp {

constexpr int BLOCK = 256;
constexpr int NCOUNT = 5;   // per block: surviving originals, surviving clones, surviving children (per copy), split parents, clones
enum : uint8_t { F_ORIG = 1, F_CLONE = 2, F_CHILD = 4, F_SPLIT = 8, F_CLONED = 16 };

struct SelState {
    uint32_t prefix[2];   // key bits fixed so far for rank lo / rank hi
    uint32_t rank[2];     // rank of the wanted element among the keys that share its prefix
    uint32_t hot;         // count(|g| >= max_grad)
    float w32;
    double w64;
    float ratio, Q;
    uint32_t hist[2][256];
};

struct Header {
    SelState sel;
    wg_densify_counts counts;
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

struct Layout {
    size_t ga, flags, counts, offsets, total;
    uint32_t blocks;
    __host__ __device__ explicit Layout(int64_t P) {
        blocks = static_cast<uint32_t>((P + BLOCK - 1) / BLOCK);
        ga = align256(sizeof(Header));
        flags = ga + align256(static_cast<size_t>(P) * 4);
        counts = flags + align256(static_cast<size_t>(P));
        offsets = counts + align256(static_cast<size_t>(blocks) * NCOUNT * 4);
        total = offsets + align256(static_cast<size_t>(blocks) * NCOUNT * 4);
    }
};

// order-preserving key of a float (negative values included; -0 sorts below +0, which changes no result)
__device__ __forceinline__ uint32_t to_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_key(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__device__ __forceinline__ float nan_to_zero(float v) { return v != v ? 0.0f : v; }

// ---- phase 1 of the plan: ga = xyz_gradient_accum_abs / denom (NaN -> 0) into scratch, count(|g| >= max_grad) --------------------------
__global__ void __launch_bounds__(BLOCK) ga_kernel(uint32_t P, const float* __restrict__ xyz_grad, const float* __restrict__ denom,
                                                   const float* __restrict__ accum_abs, float max_grad, float* __restrict__ ga,
                                                   Header* __restrict__ hdr) {
    uint32_t hot = 0;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < P; i += gridDim.x * BLOCK) {
        const float d = denom[i];
        hot += fabsf(nan_to_zero(xyz_grad[i] / d)) >= max_grad;
        if (accum_abs) ga[i] = nan_to_zero(accum_abs[i] / d);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) hot += __shfl_down(hot, d, 64);
    if ((threadIdx.x & 63) == 0 && hot) atomicAdd(&hdr->sel.hot, hot);   // integer: the count is exact in any order
}

// ---- radix select: one histogram pass over the keys that share a prefix with either wanted rank ----------------------------------------
__global__ void __launch_bounds__(BLOCK) select_hist_kernel(uint32_t n, const float* __restrict__ v, SelState* __restrict__ st, int pass) {
    __shared__ uint32_t h[2][256];
    h[0][threadIdx.x] = 0;
    h[1][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass ? (0xffffffffu << (shift + 8)) : 0u;
    const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];   // equal prefixes: the pick step reads histogram 0 for both ranks
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t k = to_key(v[i]), d = (k >> shift) & 255u, hi = k & mask;
        if (hi == p0) atomicAdd(&h[0][d], 1u);
        else if (hi == p1) atomicAdd(&h[1][d], 1u);
    }
    __syncthreads();
    if (h[0][threadIdx.x]) atomicAdd(&st->hist[0][threadIdx.x], h[0][threadIdx.x]);
    if (h[1][threadIdx.x]) atomicAdd(&st->hist[1][threadIdx.x], h[1][threadIdx.x]);
}

__device__ __forceinline__ float lerp32(float a, float b, float w) {   // ATen's lerp
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}

// One workgroup: before pass 0 the ranks are formed (from q, or from the count of hot Gaussians); then the digit of each rank is picked
// and the histograms are cleared for the next pass; after pass 3 the two keys are complete and Q is interpolated.
__global__ void __launch_bounds__(BLOCK) select_pick_kernel(uint32_t n, Header* __restrict__ hdr, int pass, int from_count, double q_in,
                                                            float* __restrict__ result) {
#pragma clang fp contract(off)
    __shared__ uint32_t h[2][256];
    SelState* st = &hdr->sel;
    const bool same = st->prefix[0] == st->prefix[1];
    h[0][threadIdx.x] = st->hist[0][threadIdx.x];
    h[1][threadIdx.x] = same ? h[0][threadIdx.x] : st->hist[1][threadIdx.x];
    __syncthreads();
    st->hist[0][threadIdx.x] = 0;
    st->hist[1][threadIdx.x] = 0;
    if (threadIdx.x != 0) return;
    if (pass <= 0) {
        uint32_t lo, hi;
        if (n <= (1u << 24)) {
            float q = static_cast<float>(q_in);
            if (from_count) {
                st->ratio = static_cast<float>(st->hot) / static_cast<float>(n);
                q = 1.0f - st->ratio;
            }
            const float rank = q * static_cast<float>(n - 1);
            const float fl = floorf(rank);
            lo = static_cast<uint32_t>(fl);
            hi = static_cast<uint32_t>(ceilf(rank));
            st->w32 = rank - fl;
            st->w64 = static_cast<double>(st->w32);
        } else {
            double q = q_in;
            if (from_count) {
                const double ratio = static_cast<double>(st->hot) / static_cast<double>(n);
                st->ratio = static_cast<float>(ratio);
                q = 1.0 - ratio;
            }
            const double rank = q * static_cast<double>(n - 1);
            const double fl = floor(rank);
            lo = static_cast<uint32_t>(fl);
            hi = static_cast<uint32_t>(ceil(rank));
            st->w64 = rank - fl;
            st->w32 = static_cast<float>(st->w64);
        }
        st->rank[0] = min(lo, n - 1);
        st->rank[1] = min(hi, n - 1);
    }
    if (pass < 0) {   // no quantile is taken (use_abs_gradient off): the ratio alone
        st->Q = __uint_as_float(0x7fc00000u);
        return;
    }
    const int shift = 24 - 8 * pass;
    for (int r = 0; r < 2; r++) {
        uint32_t rank = st->rank[r], below = 0;
        int d = 0, last = 0;
        for (; d < 256; d++) {
            const uint32_t c = h[r][d];
            if (c) last = d;
            if (rank < below + c) break;
            below += c;
        }
        if (d == 256) {   // unreachable with consistent counts; stay inside the populated digits
            d = last;
            below -= h[r][last];
            rank = below + h[r][last] - 1;
        }
        st->prefix[r] |= static_cast<uint32_t>(d) << shift;
        st->rank[r] = rank - below;
    }
    if (pass == 3) {
        const float a = from_key(st->prefix[0]), b = from_key(st->prefix[1]);
        float Q;
        if (n <= (1u << 24)) {
            Q = lerp32(a, b, st->w32);
        } else {
            const double da = a, db = b, d = db - da, w = st->w64;
            Q = static_cast<float>(w < 0.5 ? da + w * d : db - d * (1.0 - w));
        }
        st->Q = Q;
        if (result) *result = Q;
    }
}

// ---- phase 2 of the plan: the decisions ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// exclusive prefix of NF flags over the workgroup (wave64 ballots, then the four waves through LDS); totals[f]: the workgroup's count
template <int NF>
__device__ __forceinline__ void block_prefix(const bool (&flag)[NF], uint32_t (&excl)[NF], uint32_t (&totals)[NF]) {
    __shared__ uint32_t wave_count[NF][BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < NF; f++) {
        const unsigned long long b = __ballot(flag[f]);
        excl[f] = static_cast<uint32_t>(__popcll(b & ((1ull << lane) - 1ull)));
        if (lane == 0) wave_count[f][wave] = static_cast<uint32_t>(__popcll(b));
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; f++) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < BLOCK / 64; w++) {
            const uint32_t c = wave_count[f][w];
            if (w < wave) excl[f] += c;
            t += c;
        }
        totals[f] = t;
    }
}

__global__ void __launch_bounds__(BLOCK) decide_kernel(uint32_t P, wg_densify_params prm, const float* __restrict__ xyz_grad,
                                                       const float* __restrict__ denom, const float* __restrict__ ga,
                                                       const float* __restrict__ scales, const float* __restrict__ opac,
                                                       const Header* __restrict__ hdr, uint8_t* __restrict__ flags,
                                                       uint32_t* __restrict__ counts, uint32_t blocks) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint8_t f = 0;
    if (i < P) {
        const float g = nan_to_zero(xyz_grad[i] / denom[i]);
        bool hot_clone = fabsf(g) >= prm.max_grad, hot_split = g >= prm.max_grad;
        if (prm.use_abs_gradient) {
            const float Q = hdr->sel.Q, a = ga[i];
            hot_clone |= fabsf(a) >= Q;
            hot_split |= a >= Q;
        }
        const ActFwd a = act_forward(make_float4(1.f, 0.f, 0.f, 0.f), scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], opac[i], 0.0f);
        const float m = max3(a.rs[0], a.rs[1], a.rs[2]);
        // a clone can never be split (its padded gradient is 0 in the reference and its m is on the clone side): one decision per input
        const bool clone = hot_clone && m <= prm.dense_threshold, split = hot_split && m > prm.dense_threshold;
        const bool faint = a.o < prm.min_opacity;
        const bool prune_self = faint || (prm.enable_size_pruning && m > prm.size_threshold);
        // the children's size test sees exp() of their NEW raw scales
        const float mc = max3(expf(logf(a.rs[0] / 1.6f)), expf(logf(a.rs[1] / 1.6f)), expf(logf(a.rs[2] / 1.6f)));
        const bool prune_child = faint || (prm.enable_size_pruning && mc > prm.size_threshold);
        if (!split && !prune_self) f |= F_ORIG;
        if (clone && !prune_self) f |= F_CLONE;
        if (split && !prune_child) f |= F_CHILD;
        if (split) f |= F_SPLIT;
        if (clone) f |= F_CLONED;
        flags[i] = f;
    }
    const bool fl[NCOUNT] = {(f & F_ORIG) != 0, (f & F_CLONE) != 0, (f & F_CHILD) != 0, (f & F_SPLIT) != 0, (f & F_CLONED) != 0};
    uint32_t excl[NCOUNT], tot[NCOUNT];
    block_prefix<NCOUNT>(fl, excl, tot);
#pragma unroll
    for (int k = 0; k < NCOUNT; k++)
        if (threadIdx.x == static_cast<uint32_t>(k)) counts[k * blocks + blockIdx.x] = tot[k];
}

// exclusive scan of the five rows of block counts (one workgroup; a row at a time, 1024 blocks per step), then the totals
__global__ void __launch_bounds__(1024) scan_kernel(uint32_t P, uint32_t blocks, const uint32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ offsets, Header* __restrict__ hdr) {
    __shared__ uint32_t wave_sum[16];
    __shared__ uint32_t totals[NCOUNT];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < NCOUNT; k++) {
        uint32_t running = 0;
        for (uint32_t base = 0; base < blocks; base += 1024) {
            const uint32_t idx = base + threadIdx.x;
            const uint32_t c = idx < blocks ? counts[k * blocks + idx] : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d, 64);
                if (lane >= static_cast<uint32_t>(d)) incl += o;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < 16; w++) {
                const uint32_t s = wave_sum[w];
                if (w < wave) before += s;
                all += s;
            }
            if (idx < blocks) offsets[k * blocks + idx] = running + before + incl - c;
            running += all;
            __syncthreads();
        }
        if (threadIdx.x == 0) totals[k] = running;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        wg_densify_counts& c = hdr->counts;
        c.n_out[0] = totals[0];
        c.n_out[1] = totals[1];
        c.n_out[2] = totals[2];
        c.n_out[3] = totals[2];
        c.n_cloned = totals[4];
        c.n_split = totals[3];
        // after clone and split the model holds P + clones + 2 S - S rows
        c.n_pruned = static_cast<int64_t>(P) + totals[4] + totals[3] - (static_cast<int64_t>(totals[0]) + totals[1] + 2ll * totals[2]);
        c.n_hot = hdr->sel.hot;
        c.ratio = hdr->sel.ratio;
        c.Q = hdr->sel.Q;
        c.reserved[0] = c.reserved[1] = 0;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------------
// origin[row] = (source index, kind) for every output row; split_rank[i] (in ga's place) = rank of split parent i among the split parents
__global__ void __launch_bounds__(BLOCK) origin_kernel(uint32_t P, uint32_t blocks, const uint8_t* __restrict__ flags,
                                                       const uint32_t* __restrict__ offsets, const Header* __restrict__ hdr,
                                                       int2* __restrict__ origin, uint32_t* __restrict__ split_rank) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint8_t f = i < P ? flags[i] : 0;
    const bool fl[4] = {(f & F_ORIG) != 0, (f & F_CLONE) != 0, (f & F_CHILD) != 0, (f & F_SPLIT) != 0};
    uint32_t excl[4], tot[4];
    block_prefix<4>(fl, excl, tot);
    const int64_t n0 = hdr->counts.n_out[0], n1 = hdr->counts.n_out[1], n2 = hdr->counts.n_out[2];
    const int src = static_cast<int>(i);
    if (fl[0]) origin[offsets[0 * blocks + blockIdx.x] + excl[0]] = make_int2(src, 0);
    if (fl[1]) origin[n0 + offsets[1 * blocks + blockIdx.x] + excl[1]] = make_int2(src, 1);
    if (fl[2]) {
        const int64_t r = offsets[2 * blocks + blockIdx.x] + excl[2];
        origin[n0 + n1 + r] = make_int2(src, 2);
        origin[n0 + n1 + n2 + r] = make_int2(src, 3);
    }
    if (fl[3]) split_rank[i] = offsets[3 * blocks + blockIdx.x] + excl[3];
}

struct GatherEntry {
    const float* src;
    float* dst;
    uint32_t row_floats;
    uint32_t role;
    uint32_t first_block;   // of this array in the launch
    uint32_t reserved;
};
struct GatherTable {
    GatherEntry e[WG_DENSIFY_MAX_ARRAYS];
    int n;
};
struct ChildInputs {
    const float* xyz;
    const float* scales;
    const float4* rot;
    const float* noise;
    const uint32_t* split_rank;
    uint32_t n_split;
};

__device__ __forceinline__ float load_src(const float* p) {
#if WG_DENSIFY_NT_LOADS
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// component c of a child's position: R(normalize(normalize(r))) . (z * exp(s)) + xyz  (method.py:1368-1372, build_rotation :619-640)
__device__ __forceinline__ float child_xyz(const ChildInputs& in, uint32_t s, int kind, uint32_t c) {
#pragma clang fp contract(off)
    const float* sc = in.scales + 3ull * s;
    const ActFwd a = act_forward(in.rot[s], sc[0], sc[1], sc[2], 0.0f, 0.0f);
    const float norm = sqrtf(a.q.x * a.q.x + a.q.y * a.q.y + a.q.z * a.q.z + a.q.w * a.q.w);   // build_rotation normalises once more
    const float r = a.q.x / norm, x = a.q.y / norm, y = a.q.z / norm, z = a.q.w / norm;
    const float* nz = in.noise + 3ull * (static_cast<uint64_t>(kind - 2) * in.n_split + in.split_rank[s]);
    const float s0 = nz[0] * a.rs[0], s1 = nz[1] * a.rs[1], s2 = nz[2] * a.rs[2];
    float R0, R1, R2;
    if (c == 0) {
        R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - r * z); R2 = 2.0f * (x * z + r * y);
    } else if (c == 1) {
        R0 = 2.0f * (x * y + r * z); R1 = 1.0f - 2.0f * (x * x + z * z); R2 = 2.0f * (y * z - r * x);
    } else {
        R0 = 2.0f * (x * z - r * y); R1 = 2.0f * (y * z + r * x); R2 = 1.0f - 2.0f * (x * x + y * y);
    }
    return (R0 * s0 + R1 * s1 + R2 * s2) + in.xyz[3ull * s + c];
}

__device__ __forceinline__ float gather_value(const GatherEntry& e, const ChildInputs& in, int2 o, uint32_t c) {
#pragma clang fp contract(off)
    const uint32_t s = static_cast<uint32_t>(o.x);
    const float* p = e.src + static_cast<uint64_t>(s) * e.row_floats + c;
    if (o.y == 0 || e.role == WG_DP_COPY) return load_src(p);
    if (e.role == WG_DP_ZERO_NEW) return 0.0f;
    if (o.y == 1) return load_src(p);
    if (e.role == WG_DP_XYZ) return child_xyz(in, s, o.y, c);
    return logf(expf(load_src(p)) / 1.6f);   // WG_DP_SCALES: scaling_inverse_activation(exp(s) / (0.8 N)), N = 2
}

// The destination of every array is a flat stream of floats; a lane owns 16 bytes of it (four floats, which may span rows) and finds each
// float's source through `origin`.  Stores are whole 16-byte words; a group that lies in one row whose source is 16-byte aligned is read as
// one word too, otherwise float by float (neighbouring lanes still read neighbouring addresses).  1024 groups per workgroup, 4 per lane.
constexpr uint32_t GROUPS_PER_BLOCK = 4 * BLOCK;

__global__ void __launch_bounds__(BLOCK) gather_kernel(GatherTable tab, ChildInputs in, const int2* __restrict__ origin, uint64_t n_new) {
    int a = 0;
    while (a + 1 < tab.n && blockIdx.x >= tab.e[a + 1].first_block) a++;   // wave-uniform: scalar loads of the table
    const GatherEntry e = tab.e[a];
    const uint32_t F = e.row_floats;
    const uint64_t total = n_new * F;
    const uint32_t block = blockIdx.x - e.first_block;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const uint32_t t = block * GROUPS_PER_BLOCK + it * BLOCK + threadIdx.x;   // group index: total / 4 < 2^32 (checked by the caller)
        const uint64_t e0 = 4ull * t;
        if (e0 >= total) break;
        // row and column of float e0 = 4 t = 4 (q F + r):  row 4 q + (4 r) / F, column (4 r) % F, the small quotient by comparison
        const uint32_t q = t / F, r4 = 4u * (t - q * F);
        const uint32_t k = (r4 >= F) + (r4 >= 2 * F) + (r4 >= 3 * F);
        uint64_t row = 4ull * q + k;
        uint32_t col = r4 - k * F;
        int2 o = origin[row];
        float v[4];
        if (col + 3 < F && e0 + 3 < total && (o.y == 0 || e.role == WG_DP_COPY || (o.y == 1 && e.role != WG_DP_ZERO_NEW))) {
            const float* p = e.src + static_cast<uint64_t>(static_cast<uint32_t>(o.x)) * F + col;
            if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#if WG_DENSIFY_NT_LOADS
                const float4 w = make_float4(__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1),
                                             __builtin_nontemporal_load(p + 2), __builtin_nontemporal_load(p + 3));
#else
                const float4 w = *reinterpret_cast<const float4*>(p);
#endif
                v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
            } else {
                v[0] = load_src(p); v[1] = load_src(p + 1); v[2] = load_src(p + 2); v[3] = load_src(p + 3);
            }
            *reinterpret_cast<float4*>(e.dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
            continue;
        }
        const uint32_t n = total - e0 < 4 ? static_cast<uint32_t>(total - e0) : 4u;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            v[j] = 0.0f;
            if (j < n) {
                v[j] = gather_value(e, in, o, col);
                if (++col == F && j + 1 < n) {
                    col = 0;
                    o = origin[++row];
                }
            }
        }
        if (n == 4) {
            *reinterpret_cast<float4*>(e.dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {   // the tail of an array whose length is not a multiple of four
#pragma unroll
            for (uint32_t j = 0; j < 3; j++)
                if (j < n) e.dst[e0 + j] = v[j];
        }
    }
}

// ---- reset_opacity (method.py:1252-1266) --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) reset_opacity_kernel(uint32_t P, const float* __restrict__ opac, const float* __restrict__ scales,
                                                              const float* __restrict__ filter, float* __restrict__ out,
                                                              float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const float f = filter[i];
    const ActFwd a = act_forward(make_float4(1.f, 0.f, 0.f, 0.f), scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], opac[i], f);
    const float o = fminf(a.o * a.coef, 0.01f);   // get_gaussians()["opacities"], capped
    // the coefficient the reference divides by is formed from the FILTERED scales (get_gaussians()["scales"]) and the filter again
    const float f2 = f * f;
    const float q0 = a.sc[0] * a.sc[0], q1 = a.sc[1] * a.sc[1], q2 = a.sc[2] * a.sc[2];
    const float det1 = q0 * q1 * q2, det2 = (q0 + f2) * (q1 + f2) * (q2 + f2);
    const float x = o / sqrtf(det1 / det2);
    out[i] = logf(x / (1.0f - x));   // torch.special.logit
    if (exp_avg) exp_avg[i] = 0.0f;
    if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
}

inline bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

inline uint32_t hist_grid(uint32_t n) {
    const uint32_t b = (n + BLOCK - 1) / BLOCK;
    return b < 2048u ? (b ? b : 1u) : 2048u;
}

// the four select passes over v[0..n); the state's prefixes, hot count and histograms must be zero (or hot already counted)
inline void run_select(uint32_t n, const float* v, Header* hdr, int from_count, double q, float* result, hipStream_t s) {
    for (int pass = 0; pass < 4; pass++) {
        select_hist_kernel<<<hist_grid(n), BLOCK, 0, s>>>(n, v, &hdr->sel, pass);
        select_pick_kernel<<<1, BLOCK, 0, s>>>(n, hdr, pass, from_count, q, pass == 3 ? result : nullptr);
    }
}

}  // namespace dp
}  // namespace wg

using namespace wg::dp;

static const int64_t kMaxP = 0x7fffffff / 4;   // as wg_densification_stats: per-Gaussian element indices (3 i, 4 i) are 32-bit

extern "C" size_t wg_densify_scratch_bytes(int64_t P) {
    if (P < 0 || P > kMaxP) return 0;
    return Layout(P).total;
}

extern "C" int wg_quantile(int64_t n, const float* values, double q, float* result, void* scratch, void* stream) {
    if (n <= 0 || n > 0x7fffffffll || !values || !result || !scratch || !(q >= 0.0 && q <= 1.0)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Header* hdr = static_cast<Header*>(scratch);
    if (hipMemsetAsync(hdr, 0, sizeof(Header), s) != hipSuccess) return WG_ERR_HIP;
    run_select(static_cast<uint32_t>(n), values, hdr, 0, q, result, s);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

extern "C" int wg_densify_plan(int64_t P, const wg_densify_params* prm, const float* xyz_grad, const float* denom, const float* accum_abs,
                               const float* scales_raw, const float* opacities_raw, void* scratch, wg_densify_counts* counts_host,
                               void* stream) {
    if (P < 0 || P > kMaxP || !prm || !counts_host) return WG_ERR_INVALID_ARGUMENT;
    if (P > 0 && (!xyz_grad || !denom || !scales_raw || !opacities_raw || !scratch)) return WG_ERR_INVALID_ARGUMENT;
    if (P > 0 && prm->use_abs_gradient && !accum_abs) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) {   // nothing to launch: the mailbox is plain host memory
        *counts_host = wg_densify_counts{};
        return WG_OK;
    }
    if (capturing(s)) return WG_ERR_INVALID_ARGUMENT;   // the output size is data-dependent
    const Layout L(P);
    char* base = static_cast<char*>(scratch);
    Header* hdr = reinterpret_cast<Header*>(base);
    float* ga = reinterpret_cast<float*>(base + L.ga);
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + L.flags);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base + L.counts);
    uint32_t* offsets = reinterpret_cast<uint32_t*>(base + L.offsets);
    const uint32_t n = static_cast<uint32_t>(P);
    if (hipMemsetAsync(hdr, 0, sizeof(Header), s) != hipSuccess) return WG_ERR_HIP;
    ga_kernel<<<hist_grid(n), BLOCK, 0, s>>>(n, xyz_grad, denom, prm->use_abs_gradient ? accum_abs : nullptr, prm->max_grad, ga, hdr);
    if (prm->use_abs_gradient) {
        run_select(n, ga, hdr, 1, 0.0, nullptr, s);
    } else {   // ratio is reported all the same; Q is NaN
        select_pick_kernel<<<1, BLOCK, 0, s>>>(n, hdr, -1, 1, 0.0, nullptr);
    }
    decide_kernel<<<L.blocks, BLOCK, 0, s>>>(n, *prm, xyz_grad, denom, ga, scales_raw, opacities_raw, hdr, flags, counts, L.blocks);
    scan_kernel<<<1, 1024, 0, s>>>(n, L.blocks, counts, offsets, hdr);
    if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    if (hipMemcpyAsync(counts_host, &hdr->counts, sizeof(wg_densify_counts), hipMemcpyDeviceToHost, s) != hipSuccess) return WG_ERR_HIP;
    return WG_OK;
}

extern "C" int wg_densify_apply(int64_t P, const wg_densify_counts* c, const void* scratch, int num_arrays, const wg_densify_array* arrays,
                                const float* xyz, const float* scales_raw, const float* rotations_raw, const float* noise, int32_t* origin,
                                void* stream) {
    if (P < 0 || P > kMaxP || !c || num_arrays < 0 || num_arrays > WG_DENSIFY_MAX_ARRAYS || (num_arrays && !arrays)) return WG_ERR_INVALID_ARGUMENT;
    int64_t n_new = 0;
    for (int k = 0; k < 4; k++) {
        if (c->n_out[k] < 0 || c->n_out[k] > P) return WG_ERR_INVALID_ARGUMENT;
        n_new += c->n_out[k];
    }
    if (c->n_split < 0 || c->n_split > P || c->n_out[2] != c->n_out[3] || c->n_out[2] > c->n_split || n_new > 0x7fffffffll) return WG_ERR_INVALID_ARGUMENT;
    if (P == 0 || n_new == 0) return WG_OK;
    if (!scratch || !origin) return WG_ERR_INVALID_ARGUMENT;
    if (c->n_out[2] > 0 && (!xyz || !scales_raw || !rotations_raw || !noise)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (capturing(s)) return WG_ERR_INVALID_ARGUMENT;
    GatherTable tab;
    tab.n = 0;
    uint64_t blocks = 0;
    for (int k = 0; k < num_arrays; k++) {
        const wg_densify_array& a = arrays[k];
        if (!a.src || !a.dst || a.row_floats <= 0 || a.role < WG_DP_COPY || a.role > WG_DP_SCALES) return WG_ERR_INVALID_ARGUMENT;
        if ((a.role == WG_DP_XYZ || a.role == WG_DP_SCALES) && a.row_floats != 3) return WG_ERR_INVALID_ARGUMENT;
        if (reinterpret_cast<uintptr_t>(a.dst) & 15) return WG_ERR_INVALID_ARGUMENT;
        const uint64_t groups = (static_cast<uint64_t>(n_new) * a.row_floats + 3) / 4;
        if (groups > 0xffffffffull) return WG_ERR_INVALID_ARGUMENT;
        GatherEntry& e = tab.e[tab.n++];
        e.src = a.src;
        e.dst = a.dst;
        e.row_floats = static_cast<uint32_t>(a.row_floats);
        e.role = static_cast<uint32_t>(a.role);
        e.first_block = static_cast<uint32_t>(blocks);
        e.reserved = 0;
        blocks += (groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK;
        if (blocks > 0x7fffffffull) return WG_ERR_INVALID_ARGUMENT;
    }
    const Layout L(P);
    const char* base = static_cast<const char*>(scratch);
    const Header* hdr = reinterpret_cast<const Header*>(base);
    // ga is dead once the decisions are taken: its place holds the split ranks
    uint32_t* split_rank = reinterpret_cast<uint32_t*>(const_cast<char*>(base) + L.ga);
    origin_kernel<<<L.blocks, BLOCK, 0, s>>>(static_cast<uint32_t>(P), L.blocks, reinterpret_cast<const uint8_t*>(base + L.flags),
                                             reinterpret_cast<const uint32_t*>(base + L.offsets), hdr, reinterpret_cast<int2*>(origin), split_rank);
    if (tab.n) {
        const ChildInputs in{xyz, scales_raw, reinterpret_cast<const float4*>(rotations_raw), noise, split_rank, static_cast<uint32_t>(c->n_split)};
        gather_kernel<<<static_cast<uint32_t>(blocks), BLOCK, 0, s>>>(tab, in, reinterpret_cast<const int2*>(origin), static_cast<uint64_t>(n_new));
    }
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

extern "C" int wg_reset_opacity(int64_t P, const float* opacities_raw, const float* scales_raw, const float* filter_3D, float* out,
                                float* exp_avg, float* exp_avg_sq, void* stream) {
    if (P < 0 || P > kMaxP) return WG_ERR_INVALID_ARGUMENT;
    if (P == 0) return WG_OK;
    if (!opacities_raw || !scales_raw || !filter_3D || !out) return WG_ERR_INVALID_ARGUMENT;
    reset_opacity_kernel<<<static_cast<uint32_t>((P + BLOCK - 1) / BLOCK), BLOCK, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<uint32_t>(P), opacities_raw, scales_raw, filter_3D, out, exp_avg, exp_avg_sq);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}
