// The distortion pass (include/wg_rasterizer.h: wg_render_distortion): the Mip-NeRF 360 / 2DGS distortion term of a FINISHED frame,
//     dist[pixel] = sum_{j < i} w_i w_j (v_i - v_j)^2,   w_i = alpha_i T_i over the (pixel, Gaussian) pairs the forward pass blended,
// as A Q' - D'^2 of the CENTRED moments  A = sum w,  D' = sum w u,  Q' = sum w u^2,  u_i = v_i - c,  c = the v of the pixel's first blended
// instance.  The term is invariant under a shift of v, so any pivot gives the same value in exact arithmetic; in float32 the uncentred
// A Q - D^2 cancels (a surface at distance 50 with a spread of 0.05: A Q ~ 2500 A^2 against a result of ~1e-3 A^2), the centred one does not:
// its moments have the magnitude of the spread.  A per-pixel pivot is what a colour channel cannot carry -- colours are per Gaussian.
//
// The walk is depth.hip's (render_depth_kernel), i.e. the forward walk run again over the frame's lists up to tile_last: front to back, T carried
// per pixel, alpha from the forward kernel's own evaluator, the same strip masks, a pixel taking part while the list position is below its stored
// n_contrib -- the decisions, alpha and T are the forward's bit for bit (the file is built with render_fwd.hip's flags).  Per pixel it carries
// T, A, D', Q', c in place of T, D:
//   * an instance is the pixel's first blended one exactly when A == 0 before the add (a blended w is > 0): it sets c = v, and its u is 0;
//   * u = v - c is ONE float32 subtraction; D' and Q' take one fused multiply-add each (u * u rounded on its own first);
//   * dist = fma(A, Q', -(D' * D')), not clamped: >= 0 in exact arithmetic, a last-bit negative value can come out.
// dist[H * W] and, when asked for, the four planes moments[4 * H * W] = (A, D', Q', c) for the backward pass are written in full -- zeros for a
// pixel without a contributor and for every pixel of a tile whose list is empty.  The pass only READS the frame: no order array, nothing of the
// gradient record or its clean mark, no scratch, no atomics, no host synchronisation.  Two calls give the same bits.
// What render_bwd.hip keeps private (K9c's batch size) is restated here, as depth.hip restates it; the evaluators, strip masks and the
// lane -> pixel map come from wg_alpha.h.
#include "wg_common.h"
#include "wg_alpha.h"
#include "distortion/distortion.h"

namespace wg {

constexpr int DIST_BATCH = 64;

// DIST: the scalar is |means3D[id] - campos| (depth.hip: depth_scalar); otherwise values[id].
template <bool DIST>
__device__ __forceinline__ float dist_scalar(uint32_t id, const float* __restrict__ values, const float* __restrict__ means3D, float cx, float cy, float cz) {
    if (DIST) {
        const float* m = means3D + 3 * (size_t)id;
        const float dx = m[0] - cx, dy = m[1] - cy, dz = m[2] - cz;
        return sqrtf(dx * dx + dy * dy + dz * dz);
    }
    return values[id];
}

template <bool EXACT, bool DIST = false>
__global__ void __launch_bounds__(64) render_distortion_kernel(
    int W, int H, int gx, int tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float4* __restrict__ splats,
    const float2* __restrict__ subpixel_offset, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_last,
    const float* __restrict__ values, const float* __restrict__ means3D, const float* __restrict__ campos, float* __restrict__ dist,
    float* __restrict__ moments) {
    __shared__ float4 lds[DIST_BATCH * 2];   // r0 = (mx, my, conic terms), r1 = (conic term, opacity, -, the Gaussian's scalar)

    const int tile = xcd_tile(blockIdx.x, tiles);
    const uint2 range = ranges[tile];
    const int n = min((int)tile_last[tile], (int)(range.y - range.x));   // (tile_last never exceeds the list: the min only guards the reads)
    const int lane = threadIdx.x;
    const int tx = tile % gx, ty = tile / gx;

    float pfx[4], pfy[4], T[4], A[4], D[4], Q[4], c[4];
    int last[4];
    StripBounds sb;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        const bool inside = px < W && py < H;
        float2 off = make_float2(0.f, 0.f);
        T[s] = 1.0f; A[s] = 0.f; D[s] = 0.f; Q[s] = 0.f; c[s] = 0.f; last[s] = 0;
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
        float av = dist_scalar<DIST>(id_cur, values, means3D, cx, cy, cz);
        uint32_t id_next = list[min(DIST_BATCH + lane, nl)];

        for (int base = 0; base < n; base += DIST_BATCH) {
            const int cnt = min(DIST_BATCH, n - base);
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
                av = dist_scalar<DIST>(id_next, values, means3D, cx, cy, cz);
                id_next = list[min(base + 2 * DIST_BATCH + lane, nl)];
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
                        if (A[s] == 0.0f) c[s] = r1.w;   // the pixel's first blended instance: the pivot (a blended w is > 0)
                        const float u = r1.w - c[s];      // one float32 subtraction; 0 for the first instance
                        A[s] += w;
                        D[s] = __fmaf_rn(u, w, D[s]);
                        Q[s] = __fmaf_rn(__fmul_rn(u, u), w, Q[s]);
                        T[s] = test_T;
                    }
                }
            }
        }
    }
    const size_t plane = (size_t)W * H;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        if (px < W && py < H) {
            const size_t pix = (size_t)W * py + px;
            dist[pix] = __fmaf_rn(A[s], Q[s], -__fmul_rn(D[s], D[s]));
            if (moments) {
                moments[pix] = A[s];
                moments[plane + pix] = D[s];
                moments[2 * plane + pix] = Q[s];
                moments[3 * plane + pix] = c[s];
            }
        }
    }
}

hipError_t launch_render_distortion(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                    const float* subpixel_offset, const float* values, const float* means3D, const float* campos, float* dist,
                                    float* moments, bool exact, hipStream_t stream) {
    const int tiles = gx * gy;
    if (tiles <= 0) return hipSuccess;
#define WG_LAUNCH(EX, DI)                                                                                                                        \
    hipLaunchKernelGGL((render_distortion_kernel<EX, DI>), dim3(tiles), dim3(64), 0, stream, W, H, gx, tiles, img.ranges, b.point_list, g.splats, \
                       reinterpret_cast<const float2*>(subpixel_offset), img.n_contrib, img.tile_last, values, means3D, campos, dist, moments)
    if (values) { if (exact) WG_LAUNCH(true, false); else WG_LAUNCH(false, false); }
    else { if (exact) WG_LAUNCH(true, true); else WG_LAUNCH(false, true); }
#undef WG_LAUNCH
    return hipGetLastError();
}

}  // namespace wg
