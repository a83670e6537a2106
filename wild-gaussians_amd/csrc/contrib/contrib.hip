// The contribution pass (include/wg_rasterizer.h: wg_render_contributions): what each Gaussian contributed to a FINISHED frame.  Over the
// (pixel, Gaussian) pairs the frame's forward call blended, with w = alpha * T the forward's own blend weight,
//     max_weight[g]     = max w          (unsigned-integer atomic max on the bit pattern: w > 0, so the bit order is the value order)
//     hits[g]           = number of pairs                                   (64-bit integer atomic add)
//     weight_sum_q32[g] = sum of (uint64)(w * 2^32), truncated per term     (64-bit integer atomic add)
// Integer atomics commute exactly: two calls give the same bits whatever order the tiles run in.
//
// The walk is depth.hip's (the FORWARD walk run again over each tile's list up to tile_last: front to back, T carried per pixel, alpha from
// the forward kernel's evaluator, the same strip masks, a pixel taking part while the list position is below its stored n_contrib), built
// with render_fwd.hip's flags (build.py) so that w and T come out of the forward's instructions.  What replaces depth's per-pixel sum is a
// per-INSTANCE reduction over the wave's 256 pixels:
//   * the hit count is scalar arithmetic: the popcount of in_m & pass_m over the evaluated strips;
//   * a lane folds its (up to four) pixels into three 32-bit registers: the largest bit pattern, and the fixed-point term split into its
//     low and high 16 bits -- w <= 0.99, so a term is below 2^32 and 256 halves sum to less than 2^24: neither partial sum can carry out of
//     32 bits, and the 64-bit sum is lo + (hi << 16) formed once per instance;
//   * the three are reduced over the wave by a DPP butterfly (quad swaps, two row shifts, two row broadcasts: six steps each, the operand
//     fetched by the DPP modifier of the combining instruction).  The LDS tree of render_backward_colour_kernel's sibling kernels would park
//     3 x 64 words per instance and read them back; a full transposition (so that lane j reduces instance j alone) needs 64 x 64 x 3 words.
//     See EXPERIMENTS.md;
//   * the wave-uniform results are selected into lane j's registers, j the instance's place in the batch; behind the batch
//     lane j issues the atomics for the Gaussian whose record it loaded: at most three per (tile, Gaussian), none for an instance without a
//     hit, none for an output whose pointer is NULL.
// A NaN weight counts as a hit, adds 0 to the sum (selected explicitly) and wins the maximum (its bit pattern is above every finite weight's).
// pixel_mask: a pixel whose entry compares equal to 0.0f (so -0.0f too) takes no part: its n_contrib is read as 0.
// The pass only READS the frame: no order array is written (tiles launch in image order through xcd_tile), nothing of the gradient record or
// its clean mark is touched, no scratch, no host synchronisation.
#include "wg_common.h"
#include "wg_alpha.h"

namespace wg {

constexpr int CONTRIB_BATCH = 64;

// ---- wave64 reductions of 32-bit unsigned values on DPP; the result is valid in lane 63 and returned wave-uniform.
// `old` is what a lane without a source (a row shift's first lanes, a row outside the broadcast's row mask) combines with: the
// operation's neutral element.
#define WG_CONTRIB_DPP(v, ctrl, rmask) (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rmask, 0xF, false)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += WG_CONTRIB_DPP(v, 0xB1, 0xF);    // quad_perm [1,0,3,2]
    v += WG_CONTRIB_DPP(v, 0x4E, 0xF);    // quad_perm [2,3,0,1]
    v += WG_CONTRIB_DPP(v, 0x114, 0xF);   // row_shr:4
    v += WG_CONTRIB_DPP(v, 0x118, 0xF);   // row_shr:8   -> lane 15 of each row holds the row
    v += WG_CONTRIB_DPP(v, 0x142, 0xA);   // row_bcast:15 into rows 1 and 3
    v += WG_CONTRIB_DPP(v, 0x143, 0xC);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {   // (0 is neutral: the values are unsigned)
    v = max(v, WG_CONTRIB_DPP(v, 0xB1, 0xF));
    v = max(v, WG_CONTRIB_DPP(v, 0x4E, 0xF));
    v = max(v, WG_CONTRIB_DPP(v, 0x114, 0xF));
    v = max(v, WG_CONTRIB_DPP(v, 0x118, 0xF));
    v = max(v, WG_CONTRIB_DPP(v, 0x142, 0xA));
    v = max(v, WG_CONTRIB_DPP(v, 0x143, 0xC));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
#undef WG_CONTRIB_DPP

template <bool EXACT>
__global__ void __launch_bounds__(64) render_contrib_kernel(
    int W, int H, int gx, int tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ splats,
    const float2* __restrict__ subpixel_offset, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_last,
    const float* __restrict__ pixel_mask, uint32_t* __restrict__ max_weight, unsigned long long* __restrict__ hits,
    unsigned long long* __restrict__ weight_sum_q32) {
    __shared__ float4 lds[CONTRIB_BATCH * 2];   // r0 = (mx, my, conic terms), r1 = (conic term, opacity, -, -)

    const int tile = xcd_tile(blockIdx.x, tiles);
    const uint2 range = ranges[tile];
    const int n = min((int)tile_last[tile], (int)(range.y - range.x));   // (tile_last never exceeds the list: the min only guards the reads)
    if (n <= 0) return;   // wave-uniform: nothing was blended in this tile
    const int lane = threadIdx.x;
    const int tx = tile % gx, ty = tile / gx;

    float pfx[4], pfy[4], T[4];
    int last[4];
    StripBounds sb;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        const bool inside = px < W && py < H;
        float2 off = make_float2(0.f, 0.f);
        T[s] = 1.0f; last[s] = 0;
        if (inside) {
            const size_t pix = (size_t)W * py + px;
            if (subpixel_offset) off = subpixel_offset[pix];
            last[s] = (int)n_contrib[pix];
            if (pixel_mask && pixel_mask[pix] == 0.0f) last[s] = 0;   // a masked pixel takes no part; no other pixel needs its T
        }
        pfx[s] = (float)px + off.x;
        pfy[s] = (float)py + off.y;
        const float inf = __builtin_huge_valf();
        sb.x0[s] = wave_min_uniform(inside ? pfx[s] : inf);
        sb.x1[s] = wave_max_uniform(inside ? pfx[s] : -inf);
        sb.y0[s] = wave_min_uniform(inside ? pfy[s] : inf);
        sb.y1[s] = wave_max_uniform(inside ? pfy[s] : -inf);
    }
    // the last list position any (unmasked) pixel of a strip blended (wave-uniform): behind it the strip receives nothing
    int strip_last[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        int m = last[s];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
        strip_last[s] = __builtin_amdgcn_readfirstlane(m);
    }

    // Records travel list -> registers -> LDS one batch ahead of the walk, their ids two batches ahead, indices clamped to the walked part of
    // the list instead of predicated (render_fwd.hip: fwd_walk).  Nothing at or behind position n is read.
    const uint32_t* list = point_list + range.x;
    const int nl = n - 1;
    uint32_t id_cur = list[min(lane, nl)];
    float4 a0 = splats[3 * (size_t)id_cur], a1 = splats[3 * (size_t)id_cur + 1], a2 = splats[3 * (size_t)id_cur + 2];
    uint32_t id_next = list[min(CONTRIB_BATCH + lane, nl)];

    for (int base = 0; base < n; base += CONTRIB_BATCH) {
        const int cnt = min(CONTRIB_BATCH, n - base);
        float4 s0 = a0, s1 = a1;
        const uint32_t mymask = lane < cnt ? strip_mask(s0, s1, a2, sb) : 0u;
        __syncthreads();   // (the workgroup is the wave: no s_barrier; see fwd_walk on why it is kept)
        if (EXACT) halve_conic(s0, s1); else scale_conic(s0, s1);
        lds[2 * lane] = s0;
        lds[2 * lane + 1] = s1;
        __syncthreads();
        const uint32_t id_batch = id_cur;   // the Gaussian this lane staged: instance `lane` of the batch
        {
            id_cur = id_next;
            const size_t r = 3 * (size_t)id_next;
            a0 = splats[r];
            a1 = splats[r + 1];
            a2 = splats[r + 2];
            id_next = list[min(base + 2 * CONTRIB_BATCH + lane, nl)];
        }
        // instance j of the batch sits at position base + j: strip s can still receive from it while base + j < strip_last[s]
        uint64_t reach[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int live_n = strip_last[s] - base;   // wave-uniform
            const uint64_t live = live_n >= 64 ? ~0ull : (live_n <= 0 ? 0ull : ((1ull << live_n) - 1ull));
            reach[s] = __ballot((mymask >> s) & 1u) & live;
        }
        // lane j's results for instance j of this batch (hits 0: nothing to issue)
        uint32_t res_max = 0u, res_lo = 0u, res_hi = 0u, res_hits = 0u;
        uint64_t todo = reach[0] | reach[1] | reach[2] | reach[3];
        while (todo != 0ull) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r0 = lds[2 * j];
            const float4 r1 = lds[2 * j + 1];
            const SplatCoef sc = coef_of(r0, r1);
            const ExactCoef xc = exact_coef_of(r0, r1);
            const int pos = base + j;
            uint32_t nhit = 0u;                      // wave-uniform
            uint32_t vmax = 0u, vlo = 0u, vhi = 0u;  // this lane's pixels
#pragma unroll
            for (int s = 0; s < 4; s++) {
                if (((reach[s] >> j) & 1ull) == 0ull) continue;   // wave-uniform
                const uint64_t in_m = __builtin_amdgcn_ballot_w64(pos < last[s]);
                float alpha;
                uint64_t pass_m;
                if (EXACT) {
                    float dx, dy, G;
                    const float power = eval_alpha_exact_values(xc, pfx[s], pfy[s], dx, dy, G, alpha);
                    pass_m = __builtin_amdgcn_ballot_w64(!(power > 0.0f)) & __builtin_amdgcn_ballot_w64(!(alpha < (1.0f / 255.0f)));
                } else {
                    PairEval e;
                    const float p2 = eval_alpha_values(sc, pfx[s], pfy[s], e);
                    alpha = e.alpha;
                    pass_m = __builtin_amdgcn_ballot_w64(!(p2 > 0.0f)) & __builtin_amdgcn_ballot_w64(!(alpha < (1.0f / 255.0f)));
                }
                const float w = alpha * T[s];
                const float test_T = EXACT ? ref_test_T(T[s], alpha) : T[s] - w;   // as fwd_walk carries it
                const uint64_t go_m = in_m & pass_m;
                nhit += (uint32_t)__builtin_popcountll(go_m);
                if (__builtin_amdgcn_inverse_ballot_w64(go_m)) {
                    vmax = max(vmax, __float_as_uint(w));
                    const uint32_t q = (w == w) ? (uint32_t)(w * 4294967296.0f) : 0u;   // w * 2^32 is exact; the conversion truncates
                    vlo += q & 0xffffu;
                    vhi += q >> 16;
                    T[s] = test_T;
                }
            }
            if (nhit == 0u) continue;   // wave-uniform
            const uint32_t m = wave_max_u32(vmax), lo = wave_sum_u32(vlo), hi = wave_sum_u32(vhi);
            if (lane == j) { res_max = m; res_lo = lo; res_hi = hi; res_hits = nhit; }
        }
        if (res_hits != 0u) {   // (lanes at or behind cnt reached nothing: id_batch is a staged Gaussian's, below P)
            if (max_weight) atomicMax(max_weight + id_batch, res_max);
            if (hits) atomicAdd(hits + id_batch, (unsigned long long)res_hits);
            if (weight_sum_q32) atomicAdd(weight_sum_q32 + id_batch, (unsigned long long)res_lo + ((unsigned long long)res_hi << 16));
        }
    }
}

hipError_t launch_render_contrib(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                 const float* subpixel_offset, const float* pixel_mask, float* max_weight, unsigned long long* hits,
                                 unsigned long long* weight_sum_q32, bool exact, hipStream_t stream) {
    const int tiles = gx * gy;
    if (tiles <= 0) return hipSuccess;
#define WG_LAUNCH(EX)                                                                                                                    \
    hipLaunchKernelGGL((render_contrib_kernel<EX>), dim3(tiles), dim3(64), 0, stream, W, H, gx, tiles, img.ranges, b.point_list, g.splats, \
                       reinterpret_cast<const float2*>(subpixel_offset), img.n_contrib, img.tile_last, pixel_mask,                        \
                       reinterpret_cast<uint32_t*>(max_weight), hits, weight_sum_q32)
    if (exact) WG_LAUNCH(true); else WG_LAUNCH(false);
#undef WG_LAUNCH
    return hipGetLastError();
}

}  // namespace wg
