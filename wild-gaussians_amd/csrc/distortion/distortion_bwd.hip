// The gradient of the distortion pass (include/wg_rasterizer.h: wg_distortion_grad): what a cotangent g = dL/d dist[pixel] on distortion.hip's
//     dist = A Q' - D'^2,   A = sum w,  D' = sum w u,  Q' = sum w u^2,  u_i = v_i - c,  w_i = alpha_i T_i
// contributes to the frame's gradients, in ONE more per-tile walk that ADDS into the gradient record the image walk accumulates into, before the
// per-Gaussian kernel turns the record into the caller's arrays (depth_bwd.hip's place and manner).
//     d dist / d w_i = m_i = Q' + u_i (A u_i - 2 D')                 -- every factor but u_i a per-pixel constant of the forward pass (moments)
//     dL/dalpha_i = g T_i (m_i - R_i),  R_i = accum_rec for the "channel" m (backward.cu:555-561), back to front, no background term
//     dL/dv_g     = sum over g's pairs of 2 g w_i (A u_i - D')       -> dL_dvalues[g];  the pivot c takes none: d dist / d c = 0 (shift invariance)
//     from dL/dalpha on: the reference's chain (backward.cu:568-603) as the seven sums of record slots 3..9, in render_backward_kernel's conventions
// It is render_depth_backward_kernel's walk with the per-Gaussian scalar v dL_ddepth replaced by the per-(pixel, instance) value g m_i: back to
// front from tile_last, T rebuilt from final_T by T / (1 - alpha), the recursion carried as its product with g (recd), the same strip masks and
// blended set (a pixel takes part below its stored n_contrib; the two skips as the forward evaluator decides them, EXACT through the banded
// evaluation with the rare exact re-evaluation), the same arithmetic for q = G dL/dalpha.  Each lane holds g A, g D', g Q' and c for its four
// pixels (g folded in once: 2 g w (A u - D') = 2 w (gA u - gD')), and forms u from the instance's v exactly as the forward kernel did: one
// float32 subtraction.  The abs term (slot 5) accumulates |q_dist|, as depth_bwd.hip accumulates |q_depth|.
// The eight sums per instance go through depth_bwd.hip's LDS tree (render_backward_kernel's): seven float atomics into record slots 3..9 and one
// into dL_dvalues[id]; an instance without a contributing lane issues nothing.  No scratch, no host synchronisation: the launch captures.
// What render_bwd.hip keeps private (the batch size, the swap-and-add helpers) is restated here, as depth_bwd.hip restates its own.
#include "wg_common.h"
#include "wg_alpha.h"
#include "distortion/distortion.h"

namespace wg {

constexpr int DIST_BWD_BATCH = 64;
constexpr int DIST_BWD_RED_F4 = 64 + 8;   // float4 rows of the reduction: 32 + 8 unused + 32

template <int CTRL>
__device__ __forceinline__ float tbw_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// (a, b) -> one register: lanes 0-31 hold a[l] + a[l+32], lanes 32-63 hold b[l-32] + b[l].  The empty asm keeps the swap's two results
// apart (render_bwd.hip: pair_x32 on what hipcc 7.2 otherwise selects)
__device__ __forceinline__ float tbw_pair_x32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    unsigned x = r[0], y = r[1];
    asm volatile("" : "+v"(x), "+v"(y));
    return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
// DIST: the scalar is |means3D[id] - campos| (distortion.hip: dist_scalar); otherwise values[id].
template <bool DIST>
__device__ __forceinline__ float dist_bwd_scalar(uint32_t id, const float* __restrict__ values, const float* __restrict__ means3D, float cx, float cy, float cz) {
    if (DIST) {
        const float* m = means3D + 3 * (size_t)id;
        const float dx = m[0] - cx, dy = m[1] - cy, dz = m[2] - cz;
        return sqrtf(dx * dx + dy * dy + dz * dz);
    }
    return values[id];
}

template <bool EXACT, bool DIST>
__global__ void __launch_bounds__(64) render_distortion_backward_kernel(
    int W, int H, int gx, int tiles, const uint32_t* __restrict__ order, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ splats, const float2* __restrict__ subpixel_offset, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_last, const float* __restrict__ dL_ddist,
    const float* __restrict__ moments, const float* __restrict__ values, const float* __restrict__ means3D, const float* __restrict__ campos,
    float* __restrict__ grad_rec, float* __restrict__ dL_dvalues) {
    // the reduction's rows first (one float4 per lane; the upper half's 32 rows start 32 floats further on, so that the two halves' reads fall into
    // different banks), then the parked batch: r0 = (mx, my, ca, cb), r1 = (cc, opacity, the Gaussian's id, the Gaussian's scalar)
    __shared__ float4 smem[DIST_BWD_RED_F4 + DIST_BWD_BATCH * 2];
    float4* const lds = smem + DIST_BWD_RED_F4;
    float* const red = reinterpret_cast<float*>(smem);

    const int tile = (int)order[xcd_tile(blockIdx.x, tiles)];
    const uint2 range = ranges[tile];
    const int hi0 = min((int)tile_last[tile], (int)(range.y - range.x));   // (tile_last never exceeds the list: the min only guards the reads)
    if (hi0 <= 0) return;   // wave-uniform
    const int lane = threadIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;
    const size_t plane = (size_t)W * H;

    // which of the eight reduced values this lane holds after the reduction (lane 32 half + 4 m + h: value 2 (m & 3) + half), and where it adds
    // it: 0 -> dL_dvalues[id]; k = 1..7 -> record slot 2 + k
    const int red_m = (lane & 31) >> 2, red_half = lane >> 5;
    const int vidx = 2 * (red_m & 3) + red_half;
    const bool issue = (lane & 3) == 0 && red_m < 4;   // one lane per value
    // this lane's row (write) and its read base: row 32 half + h, column m & 3 of its half (lanes with m >= 4 repeat the columns: a broadcast)
    const int wr_row = lane + 8 * red_half;
    int rd0 = 4 * (40 * red_half + (lane & 3)) + (red_m & 3);
    asm volatile("" : "+v"(rd0));   // (kept in a register: render_bwd.hip)
    float* const abase = vidx == 0 ? dL_dvalues : grad_rec + 2 + vidx;
    const uint32_t astride = vidx == 0 ? 1u : (uint32_t)GRAD_REC_FLOATS;

    // per pixel: the cotangent times the forward pass's moments, the pivot, and the recursion's state
    float pfx[4], pfy[4], T[4], gA[4], gD[4], gQ[4], piv[4], recd[4];
    int last[4];
    StripBounds sb;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        const bool inside = px < W && py < H;
        float2 off = make_float2(0.f, 0.f);
        T[s] = 0.f; last[s] = 0; gA[s] = 0.f; gD[s] = 0.f; gQ[s] = 0.f; piv[s] = 0.f; recd[s] = 0.f;
        if (inside) {
            const size_t pix = (size_t)W * py + px;
            if (subpixel_offset) off = subpixel_offset[pix];
            T[s] = final_T[pix];
            last[s] = (int)n_contrib[pix];
            const float g = dL_ddist[pix];
            gA[s] = g * moments[pix];
            gD[s] = g * moments[plane + pix];
            gQ[s] = g * moments[2 * plane + pix];
            piv[s] = moments[3 * plane + pix];
        }
        pfx[s] = (float)px + off.x;
        pfy[s] = (float)py + off.y;
        const float inf = __builtin_huge_valf();
        sb.x0[s] = wave_min_uniform(inside ? pfx[s] : inf);
        sb.x1[s] = wave_max_uniform(inside ? pfx[s] : -inf);
        sb.y0[s] = wave_min_uniform(inside ? pfy[s] : inf);
        sb.y1[s] = wave_max_uniform(inside ? pfy[s] : -inf);
    }
    // the last list position any pixel of a strip blended (wave-uniform: the largest n_contrib of the strip)
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

    // the eight partial sums live across instances and are cleared after each reduction only
    float sv = 0.f, sx = 0.f, sy = 0.f, sab = 0.f, sxx = 0.f, sxy = 0.f, syy = 0.f, sq = 0.f;
    for (int hi = hi0; hi > 0; hi -= DIST_BWD_BATCH) {
        // lane l stages the instance at list position hi - 1 - l (back to front): positions 0 .. hi0 - 1 only, the walked part of the list
        const int posl = hi - 1 - lane;
        __syncthreads();   // (the workgroup is the wave)
        uint32_t mymask = 0;
        if (posl >= 0) {
            const uint32_t id = point_list[range.x + posl];
            float4 q0 = splats[3 * (size_t)id];
            float4 q1 = splats[3 * (size_t)id + 1];
            const float4 q2 = splats[3 * (size_t)id + 2];
            mymask = strip_mask(q0, q1, q2, sb);
            scale_conic(q0, q1);
            q1.z = __uint_as_float(id);
            q1.w = dist_bwd_scalar<DIST>(id, values, means3D, cx, cy, cz);   // the scalar where the image walk finds the red channel
            lds[2 * lane] = q0;
            lds[2 * lane + 1] = q1;
        }
        __syncthreads();
        // instance j of the batch sits at position hi - 1 - j: strip s can receive from it only while hi - 1 - j < strip_last[s]
        uint64_t reach[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int first = hi - strip_last[s];  // wave-uniform
            const uint64_t live = first <= 0 ? ~0ull : (first >= 64 ? 0ull : (~0ull << first));
            reach[s] = __ballot((mymask >> s) & 1u) & live;
        }
        uint64_t todo = reach[0] | reach[1] | reach[2] | reach[3];
        while (todo != 0ull) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r0 = lds[2 * j];
            const float4 r1 = lds[2 * j + 1];
            const SplatCoef sc = coef_of(r0, r1);
            const float val = r1.w;
            const float ca2 = 2.0f * r0.z, cc2 = 2.0f * r1.x;   // the gradient of the exponent, up to the factor 1 / log2(e) applied per Gaussian
            const int pos = hi - 1 - j;
            uint64_t any_m = 0ull;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                if (((reach[s] >> j) & 1ull) == 0ull) continue;  // wave-uniform
                const uint64_t before_last_m = __builtin_amdgcn_ballot_w64(pos < last[s]);
                PairEval e;
                uint64_t pass_m;
                if (EXACT) {
                    float margin, band;
                    eval_alpha_banded(sc, pfx[s], pfy[s], e, margin, band);
                    pass_m = __builtin_amdgcn_ballot_w64(margin >= 0.0f);
                    const uint64_t fragile_m = before_last_m & __builtin_amdgcn_ballot_w64(fabsf(margin) < band);
                    if (fragile_m != 0ull) {  // rare: the forward's arithmetic on the record as preprocess wrote it (pos < hi0: inside the walked part)
                        const size_t r = 3 * (size_t)point_list[range.x + pos];
                        float4 q0 = splats[r], q1 = splats[r + 1];
                        halve_conic(q0, q1);
                        float dx, dy, G, alpha;
                        const float power = eval_alpha_exact_values(exact_coef_of(q0, q1), pfx[s], pfy[s], dx, dy, G, alpha);
                        const uint64_t px_m = __builtin_amdgcn_ballot_w64(!(power > 0.0f)) & __builtin_amdgcn_ballot_w64(!(alpha < (1.0f / 255.0f)));
                        pass_m = (pass_m & ~fragile_m) | (px_m & fragile_m);
                        if (__builtin_amdgcn_inverse_ballot_w64(fragile_m)) { e.G = G; e.alpha = alpha; }
                    }
                } else {
                    const float p2 = eval_alpha_values(sc, pfx[s], pfy[s], e);
                    pass_m = __builtin_amdgcn_ballot_w64(!(p2 > 0.0f)) & __builtin_amdgcn_ballot_w64(!(e.alpha < (1.0f / 255.0f)));
                }
                const uint64_t go_m = before_last_m & pass_m;
                any_m |= go_m;
                if (__builtin_amdgcn_inverse_ballot_w64(go_m)) {
                    const float a = e.alpha;
                    const float inv = __builtin_amdgcn_rcpf(1.0f - a);
                    const float Tn = T[s] * inv;  // T / (1 - alpha), backward.cu:548
                    T[s] = Tn;
                    const float uc = val - piv[s];            // u, as the forward kernel formed it
                    const float t1 = gA[s] * uc - gD[s];      // g (A u - D')
                    sv += (a * Tn) * (2.0f * t1);             // 2 g w (A u - D')
                    const float gm = gQ[s] + uc * (t1 - gD[s]);   // g m = g (Q' + u (A u - 2 D'))
                    // (m - accum_rec) * g, accum_rec carried as its product with g: recd' = recd + alpha * (g m - recd)
                    const float diff = gm - recd[s];
                    recd[s] += a * diff;
                    const float q = e.G * (diff * Tn);   // no background term: the distortion has none
                    const float u = ca2 * e.dx + r0.w * e.dy;   // -log2(e) * (A dx + B dy)
                    const float v = cc2 * e.dy + r0.w * e.dx;   // -log2(e) * (C dy + B dx)
                    sq += q;
                    sx += q * u;
                    sy += q * v;
                    sab += fabsf(q) * (ddelx_dx * fabsf(u) + ddely_dy * fabsf(v));
                    sxx += q * e.xx;
                    sxy += q * e.xy;
                    syy += q * e.yy;
                }
            }
            if (any_m == 0ull) continue;
            float total;
            {
                reinterpret_cast<float4*>(red)[wr_row] = make_float4(tbw_pair_x32(sv, sx), tbw_pair_x32(sy, sab), tbw_pair_x32(sxx, sxy), tbw_pair_x32(syy, sq));
                asm volatile("" ::: "memory");   // (compiler order only: one wave's LDS operations execute in program order)
                float t[8];
#pragma unroll
                for (int i = 0; i < 8; i++) t[i] = red[rd0 + 16 * i];   // rows h, h + 4, ..., h + 28 of this lane's half
                asm volatile("" ::: "memory");
#pragma unroll
                for (int d = 1; d < 8; d <<= 1)
#pragma unroll
                    for (int i = 0; i < 8; i += 2 * d) t[i] += t[i + d];
                total = t[0];
                total += tbw_dpp<0xB1>(total);   // quad_perm [1,0,3,2]
                total += tbw_dpp<0x4E>(total);   // quad_perm [2,3,0,1]
            }
            if (issue) unsafeAtomicAdd(abase + (size_t)__float_as_uint(r1.z) * astride, total);
            sv = sx = sy = sab = sxx = sxy = syy = sq = 0.f;
        }
    }
}

hipError_t launch_render_distortion_backward(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                             const float* subpixel_offset, const float* dL_ddist, const float* moments, const float* values,
                                             const float* means3D, const float* campos, float* dL_dvalues, bool exact, hipStream_t stream) {
    const int tiles = gx * gy;
    if (tiles <= 0) return hipSuccess;
#define WG_LAUNCH(EX, DI)                                                                                                                              \
    hipLaunchKernelGGL((render_distortion_backward_kernel<EX, DI>), dim3(tiles), dim3(64), 0, stream, W, H, gx, tiles, img.order_bwd, img.ranges,       \
                       b.point_list, g.splats, reinterpret_cast<const float2*>(subpixel_offset), img.final_T, img.n_contrib, img.tile_last, dL_ddist, \
                       moments, values, means3D, campos, g.grad_rec, dL_dvalues)
    if (values) { if (exact) WG_LAUNCH(true, false); else WG_LAUNCH(false, false); }
    else { if (exact) WG_LAUNCH(true, true); else WG_LAUNCH(false, true); }
#undef WG_LAUNCH
    return hipGetLastError();
}

// Distance mode's direct term, one thread per Gaussian behind the per-Gaussian backward kernel (which WRITES dL_dmean3D) -- depth_bwd.hip's
// depth_distance_fold_kernel restated: v = |x - campos|  =>  dL/dx += dL/dv (x - campos) / v, and 0 at v == 0 (torch.norm's subgradient).  A Gaussian
// nothing was added to is left alone.
__global__ void __launch_bounds__(256) distortion_distance_fold_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ campos,
                                                                       const float* __restrict__ dL_dvalues, float* __restrict__ dL_dmean3D) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    const float dv = dL_dvalues[g];
    if (dv == 0.0f) return;   // (a NaN compares unequal and goes on)
    const float* m = means3D + 3 * (size_t)g;
    const float dx = m[0] - campos[0], dy = m[1] - campos[1], dz = m[2] - campos[2];
    const float v = sqrtf(dx * dx + dy * dy + dz * dz);
    if (v == 0.0f) return;
    const float s = dv / v;
    float* o = dL_dmean3D + 3 * (size_t)g;
    o[0] += s * dx;
    o[1] += s * dy;
    o[2] += s * dz;
}

hipError_t launch_distortion_distance_fold(int P, const float* means3D, const float* campos, const float* dL_dvalues, float* dL_dmean3D, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(distortion_distance_fold_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, campos, dL_dvalues, dL_dmean3D);
    return hipGetLastError();
}

}  // namespace wg
