// The depth pass (include/wg_rasterizer.h: wg_render_depth): one per-Gaussian scalar composited over a FINISHED frame like a colour channel,
//     depth[pixel] = sum over the (pixel, Gaussian) pairs the forward pass blended of  v[Gaussian] * alpha * T
// -- no background term, no division by the accumulation: what the caller's three-channel "depth render" (a second rasterizer call with the
// distances as colours over an all-zero background, method.py:1621-1631) leaves in each of its three identical channels.
//
// Everything it needs lies in the frame's buffers: the per-tile lists up to tile_last, the splat records, n_contrib.  The walk is
// render_backward_colour_kernel's (render_bwd.hip, K9c), i.e. the FORWARD walk (render_fwd.hip: fwd_walk) run again -- front to back, T carried per
// pixel, alpha from the forward kernel's own evaluator, the same strip masks -- with that kernel's three per-Gaussian reductions replaced by one
// per-pixel sum:
//   * a pixel takes part while the list position is below its stored n_contrib.  Such a pixel was still accumulating in the forward pass and did
//     not stop there, so "blended" is exactly "passes the two skips" -- taken on eval_alpha_exact_values (EXACT) or eval_alpha_values: the
//     decisions are the forward's by construction and T is the forward's bit for bit;
//   * D[s] += v * w is the forward kernel's Cr[s] += r1.w * w: there one v_fma_f32 (render_fwd.hip is built with contraction on), here
//     __fmaf_rn over the same operands -- the Gaussian's scalar sits in the red channel's place of the parked record -- and the file is built
//     with render_fwd.hip's flags (build.py), so that w and T come out of the same instructions too: the sum has the forward's bits;
//   * the scalar travels with the record: the lane that loads an instance's record, one batch ahead of the walk, loads values[id] (or the
//     Gaussian's mean and takes its distance to the camera) with it.
// The pass only READS the frame: no order array is written (tiles launch in image order through xcd_tile), nothing of the gradient record or
// its clean mark is touched, no scratch, no atomics, no host synchronisation.  depth[H * W] is written in full -- 0 for a pixel without a
// contributor, for every pixel of a tile whose list is empty.
//
// What K9c keeps private to render_bwd.hip (the batch size) is restated here; the evaluators, strip masks and the lane -> pixel map come from
// wg_alpha.h.
#include "wg_common.h"
#include "wg_alpha.h"

namespace wg {

constexpr int DEPTH_BATCH = 64;

// DIST: the scalar is |means3D[id] - campos| (the caller's torch.norm(means3D - camera_center[None], dim=-1)); otherwise values[id].
template <bool DIST>
__device__ __forceinline__ float depth_scalar(uint32_t id, const float* __restrict__ values, const float* __restrict__ means3D, float cx, float cy, float cz) {
    if (DIST) {
        const float* m = means3D + 3 * (size_t)id;
        const float dx = m[0] - cx, dy = m[1] - cy, dz = m[2] - cz;
        return sqrtf(dx * dx + dy * dy + dz * dz);
    }
    return values[id];
}

template <bool EXACT, bool DIST = false>
__global__ void __launch_bounds__(64) render_depth_kernel(
    int W, int H, int gx, int tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ splats,
    const float2* __restrict__ subpixel_offset, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_last,
    const float* __restrict__ values, const float* __restrict__ means3D, const float* __restrict__ campos, float* __restrict__ depth) {
    __shared__ float4 lds[DEPTH_BATCH * 2];   // r0 = (mx, my, conic terms), r1 = (conic term, opacity, -, the Gaussian's scalar)

    const int tile = xcd_tile(blockIdx.x, tiles);
    const uint2 range = ranges[tile];
    const int n = min((int)tile_last[tile], (int)(range.y - range.x));   // (tile_last never exceeds the list: the min only guards the reads)
    const int lane = threadIdx.x;
    const int tx = tile % gx, ty = tile / gx;

    float pfx[4], pfy[4], T[4], D[4];
    int last[4];
    StripBounds sb;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        const bool inside = px < W && py < H;
        float2 off = make_float2(0.f, 0.f);
        T[s] = 1.0f; D[s] = 0.f; last[s] = 0;
        if (inside) {
            const size_t pix = (size_t)W * py + px;
            if (subpixel_offset) off = subpixel_offset[pix];
            if (n > 0) last[s] = (int)n_contrib[pix];
        }
        pfx[s] = (float)px + off.x;
        pfy[s] = (float)py + off.y;
        const float inf = __builtin_huge_valf();
        sb.x0[s] = wave_min_uniform(inside ? pfx[s] : inf);
        sb.x1[s] = wave_max_uniform(inside ? pfx[s] : -inf);
        sb.y0[s] = wave_min_uniform(inside ? pfy[s] : inf);
        sb.y1[s] = wave_max_uniform(inside ? pfy[s] : -inf);
    }
    if (n > 0) {   // wave-uniform
        // the last list position any pixel of a strip blended (wave-uniform): behind it the strip receives nothing
        int strip_last[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            int m = last[s];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
            strip_last[s] = __builtin_amdgcn_readfirstlane(m);
        }
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (DIST) { cx = campos[0]; cy = campos[1]; cz = campos[2]; }

        // Records travel list -> registers -> LDS one batch ahead of the walk, their ids two batches ahead, indices clamped to the walked part of
        // the list instead of predicated (render_fwd.hip: fwd_walk).  Nothing at or behind position n is read.
        const uint32_t* list = point_list + range.x;
        const int nl = n - 1;
        uint32_t id_cur = list[min(lane, nl)];
        float4 a0 = splats[3 * (size_t)id_cur], a1 = splats[3 * (size_t)id_cur + 1], a2 = splats[3 * (size_t)id_cur + 2];
        float av = depth_scalar<DIST>(id_cur, values, means3D, cx, cy, cz);
        uint32_t id_next = list[min(DEPTH_BATCH + lane, nl)];

        for (int base = 0; base < n; base += DEPTH_BATCH) {
            const int cnt = min(DEPTH_BATCH, n - base);
            float4 s0 = a0, s1 = a1;
            const uint32_t mymask = lane < cnt ? strip_mask(s0, s1, a2, sb) : 0u;
            __syncthreads();   // (the workgroup is the wave: no s_barrier; see fwd_walk on why it is kept)
            if (EXACT) halve_conic(s0, s1); else scale_conic(s0, s1);
            s1.w = av;   // the scalar where the forward walk finds the red channel
            lds[2 * lane] = s0;
            lds[2 * lane + 1] = s1;
            __syncthreads();
            {
                id_cur = id_next;
                const size_t r = 3 * (size_t)id_next;
                a0 = splats[r];
                a1 = splats[r + 1];
                a2 = splats[r + 2];
                av = depth_scalar<DIST>(id_next, values, means3D, cx, cy, cz);
                id_next = list[min(base + 2 * DEPTH_BATCH + lane, nl)];
            }
            // instance j of the batch sits at position base + j: strip s can still receive from it while base + j < strip_last[s]
            uint64_t reach[4];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int live_n = strip_last[s] - base;   // wave-uniform
                const uint64_t live = live_n >= 64 ? ~0ull : (live_n <= 0 ? 0ull : ((1ull << live_n) - 1ull));
                reach[s] = __ballot((mymask >> s) & 1u) & live;
            }
            uint64_t todo = reach[0] | reach[1] | reach[2] | reach[3];
            while (todo != 0ull) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1;
                const float4 r0 = lds[2 * j];
                const float4 r1 = lds[2 * j + 1];
                const SplatCoef sc = coef_of(r0, r1);
                const ExactCoef xc = exact_coef_of(r0, r1);
                const int pos = base + j;
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
                    if (__builtin_amdgcn_inverse_ballot_w64(in_m & pass_m)) {
                        D[s] = __fmaf_rn(r1.w, w, D[s]);   // Cr[s] += r1.w * w of fwd_walk, which compiles to one v_fma_f32 (its file contracts)
                        T[s] = test_T;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        if (px < W && py < H) depth[(size_t)W * py + px] = D[s];
    }
}

hipError_t launch_render_depth(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                               const float* subpixel_offset, const float* values, const float* means3D, const float* campos, float* depth,
                               bool exact, hipStream_t stream) {
    const int tiles = gx * gy;
    if (tiles <= 0) return hipSuccess;
#define WG_LAUNCH(EX, DI)                                                                                                                   \
    hipLaunchKernelGGL((render_depth_kernel<EX, DI>), dim3(tiles), dim3(64), 0, stream, W, H, gx, tiles, img.ranges, b.point_list, g.splats, \
                       reinterpret_cast<const float2*>(subpixel_offset), img.n_contrib, img.tile_last, values, means3D, campos, depth)
    if (values) { if (exact) WG_LAUNCH(true, false); else WG_LAUNCH(false, false); }
    else { if (exact) WG_LAUNCH(true, true); else WG_LAUNCH(false, true); }
#undef WG_LAUNCH
    return hipGetLastError();
}

}  // namespace wg
