// The colour-only backward pass in a FIXED summation order (wg_backward_args::colour_gradients_only = WG_COLOUR_GRADIENTS_FIXED_ORDER):
//     dL_dcolor[g, c] = sum over the (pixel, Gaussian) pairs the forward pass blended of  alpha * T * dL_dpixel[c]
// without a float atomic anywhere, so that two calls over one frame give the same bits whatever the tiles' launch order and timing.
//
// Two kernels, next to the machinery the full pass's deterministic mode already has (render_bwd.hip: render_backward_kernel<DET>,
// det_reduce_kernel; api.hip: run_scan, the leased scratch, the flag clear inside the tile-ordering launch):
//   * render_backward_colour_slots_kernel is render_backward_colour_kernel's walk (render_bwd.hip, K9c) statement for statement -- the tile's list up
//     to tile_last, a pixel takes part while pos < n_contrib, the forward kernel's own alpha evaluator and T, records one batch ahead and ids
//     two ahead with indices clamped to the walked part, tiles taken through order_bwd -- with two differences.  The staging lane puts the
//     instance's SLOT into the record's spare float instead of the byte offset 12 * id,
//         slot = offsets_incl[id] - tiles_touched[id] + (ty - rect.y) * (rect.z - rect.x) + (tx - rect.x)
//     (the exclusive prefix of tiles_touched + the tile's index inside the Gaussian's tile rectangle: what render_backward_kernel<DET> computes),
//     fetched with the record, one batch ahead, by the lane that stages it and not behind the butterfly by the lanes that store.  And behind
//     butterfly3 lanes 0 / 32 / 16 STORE red / green / blue to slots[4 * slot + c] and lane 0 sets flags[slot] = 1.  A slot is four floats
//     (16 bytes); the fourth is never written or read.  Only an instance with a contributing lane stores anything, as K9c adds only those.
//   * colour_slots_reduce_kernel, one Gaussian per lane, adds a Gaussian's flagged slots and WRITES dL_dcolor[3 id + c] for every id < P -- an
//     exact +0.0f for a Gaussian without a flagged slot -- so the array needs no clearing: the only clear of the call is the flag bytes.
//
// The order of the sums.  A (tile, Gaussian) term is one wave's butterfly over one tile's pixels: it does not depend on when the tile ran.
// The 64 Gaussians of a wave own one contiguous slot range; the wave walks its flag bytes in ascending slot order, appends the flagged slots'
// indices to a 64-entry batch and reduces a batch when the next group of 64 flags would not fit (and at the end).  Inside a batch a
// Gaussian's entries are consecutive lanes; a segmented Hillis-Steele scan adds them in a fixed tree, and the Gaussian's lane adds the batch's
// total to its accumulator (which starts at +0.0f), batch after batch in slot order.  Where the batches are cut and what the trees look like
// follows from tiles_touched, the rectangles and which slots were flagged -- the frame -- and from nothing else.
//
// What K9c and det_reduce_kernel keep private to render_bwd.hip (the batch size, the three-value butterfly, the compaction) is restated here, so that
// render_bwd.hip compiles to the instructions and registers it had; the evaluators, strip masks and the lane -> pixel map come from wg_alpha.h.
// The file is built with render_bwd.hip's flags less -munsafe-fp-atomics: there is no atomic in it.
#include "wg_common.h"
#include "wg_alpha.h"

namespace wg {

constexpr int FO_BATCH = 64;

template <int CTRL>
__device__ __forceinline__ float fo_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// (a, b) -> one register: lanes 0-31 hold a[l] + a[l+32], lanes 32-63 hold b[l-32] + b[l]   (render_bwd.hip: pair_x32, with its note on
// why the swap's two results pass through an empty asm)
__device__ __forceinline__ float fo_pair_x32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    unsigned x = r[0], y = r[1];
    asm volatile("" : "+v"(x), "+v"(y));
    return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
// (a, b) -> one register: even 16-lane rows hold a summed over the row pair, odd rows hold b likewise
__device__ __forceinline__ float fo_pair_x16(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    unsigned x = r[0], y = r[1];
    asm volatile("" : "+v"(x), "+v"(y));
    return __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
}
// Three per-lane values summed over the wave: on return every lane of row 0 (lanes 0 - 15) holds the total of v0, of row 2 that of v1, of
// rows 1 and 3 that of v2   (render_bwd.hip: butterfly3, operation for operation: a tile's term has K9c's bits)
__device__ __forceinline__ float fo_butterfly3(float v0, float v1, float v2) {
    const float w0 = fo_pair_x32(v0, v1), w1 = fo_pair_x32(v2, v2);
    float y = fo_pair_x16(w0, w1);
    y += fo_dpp<0xB1>(y);    // quad_perm [1,0,3,2]
    y += fo_dpp<0x4E>(y);    // quad_perm [2,3,0,1]
    y += fo_dpp<0x124>(y);   // row_ror 4
    y += fo_dpp<0x128>(y);   // row_ror 8
    return y;
}

// the instance's slot: exclusive prefix of tiles_touched + the tile's index inside the Gaussian's rectangle (render_bwd.hip:336-340)
__device__ __forceinline__ uint32_t fo_slot_of(uint32_t id, int tx, int ty, const ushort4* __restrict__ rects, const uint32_t* __restrict__ offsets_incl,
                                               const uint32_t* __restrict__ tiles_touched) {
    const ushort4 rc = rects[id];
    return offsets_incl[id] - tiles_touched[id] + (uint32_t)((ty - rc.y) * (rc.z - rc.x) + (tx - rc.x));
}

template <bool EXACT>
__global__ void __launch_bounds__(64) render_backward_colour_slots_kernel(
    int W, int H, int gx, int tiles, const uint32_t* __restrict__ order, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
    const float4* __restrict__ splats, const float2* __restrict__ subpixel_offset, const uint32_t* __restrict__ n_contrib,
    const uint32_t* __restrict__ tile_last, const float* __restrict__ dL_dpix, const ushort4* __restrict__ rects,
    const uint32_t* __restrict__ offsets_incl, const uint32_t* __restrict__ tiles_touched, float* __restrict__ slots,
    unsigned char* __restrict__ flags, uint32_t slot_capacity) {
    __shared__ float4 lds[FO_BATCH * 2];   // r0 = (mx, my, conic terms), r1 = (conic term, opacity, the instance's slot, -)

    const int tile = (int)order[xcd_tile(blockIdx.x, tiles)];
    const uint2 range = ranges[tile];
    const int n = min((int)tile_last[tile], (int)(range.y - range.x));   // (tile_last never exceeds the list: the min only guards the reads)
    if (n <= 0) return;
    const int lane = threadIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const size_t plane = (size_t)W * H;

    float pfx[4], pfy[4], T[4], dLr[4], dLg[4], dLb[4];
    int last[4];
    StripBounds sb;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int px = tx * TILE_X + strip_x(lane, s), py = ty * TILE_Y + strip_y(lane, s);
        const bool inside = px < W && py < H;
        float2 off = make_float2(0.f, 0.f);
        T[s] = 1.0f; last[s] = 0; dLr[s] = dLg[s] = dLb[s] = 0.f;
        if (inside) {
            const size_t pix = (size_t)W * py + px;
            if (subpixel_offset) off = subpixel_offset[pix];
            last[s] = (int)n_contrib[pix];
            dLr[s] = dL_dpix[pix];
            dLg[s] = dL_dpix[plane + pix];
            dLb[s] = dL_dpix[2 * plane + pix];
        }
        pfx[s] = (float)px + off.x;
        pfy[s] = (float)py + off.y;
        const float inf = __builtin_huge_valf();
        sb.x0[s] = wave_min_uniform(inside ? pfx[s] : inf);
        sb.x1[s] = wave_max_uniform(inside ? pfx[s] : -inf);
        sb.y0[s] = wave_min_uniform(inside ? pfy[s] : inf);
        sb.y1[s] = wave_max_uniform(inside ? pfy[s] : -inf);
    }
    // the last list position any pixel of a strip blended (wave-uniform): behind it the strip receives nothing
    int strip_last[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        int m = last[s];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
        strip_last[s] = __builtin_amdgcn_readfirstlane(m);
    }

    // after fo_butterfly3(): lane 0 holds red, lane 32 green, lane 16 blue (lane 48: a copy of blue, not stored)
    const bool issue = (lane & 15) == 0 && lane != 48;
    const uint32_t chan = lane == 0 ? 0u : (lane == 32 ? 1u : 2u);

    // Records travel list -> registers -> LDS one batch ahead of the walk, their ids two batches ahead, indices clamped to the walked part of
    // the list instead of predicated (render_fwd.hip: fwd_walk).  Nothing at or behind position n is read.  The slot's three gathers go with
    // the record.
    const uint32_t* list = point_list + range.x;
    const int nl = n - 1;
    uint32_t id_cur = list[min(lane, nl)];
    float4 a0 = splats[3 * (size_t)id_cur], a1 = splats[3 * (size_t)id_cur + 1], a2 = splats[3 * (size_t)id_cur + 2];
    uint32_t slot_cur = fo_slot_of(id_cur, tx, ty, rects, offsets_incl, tiles_touched);
    uint32_t id_next = list[min(FO_BATCH + lane, nl)];
    float acr = 0.f, acg = 0.f, acb = 0.f;   // cleared after each reduction only: an instance nobody contributed to leaves them at zero

    for (int base = 0; base < n; base += FO_BATCH) {
        const int cnt = min(FO_BATCH, n - base);
        float4 s0 = a0, s1 = a1;
        const uint32_t mymask = lane < cnt ? strip_mask(s0, s1, a2, sb) : 0u;
        __syncthreads();   // (the workgroup is the wave: no s_barrier; see fwd_walk on why it is kept)
        if (EXACT) halve_conic(s0, s1); else scale_conic(s0, s1);
        s1.z = __uint_as_float(slot_cur);
        lds[2 * lane] = s0;
        lds[2 * lane + 1] = s1;
        __syncthreads();
        {
            id_cur = id_next;
            const size_t r = 3 * (size_t)id_next;
            a0 = splats[r];
            a1 = splats[r + 1];
            a2 = splats[r + 2];
            slot_cur = fo_slot_of(id_next, tx, ty, rects, offsets_incl, tiles_touched);
            id_next = list[min(base + 2 * FO_BATCH + lane, nl)];
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
            uint64_t any_m = 0ull;
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
                const uint64_t go_m = in_m & pass_m;
                any_m |= go_m;
                if (__builtin_amdgcn_inverse_ballot_w64(go_m)) {
                    const float w = alpha * T[s];
                    acr += w * dLr[s];
                    acg += w * dLg[s];
                    acb += w * dLb[s];
                    T[s] = EXACT ? ref_test_T(T[s], alpha) : T[s] - w;   // as fwd_walk carries it
                }
            }
            if (any_m == 0ull) continue;
            const float total = fo_butterfly3(acr, acg, acb);
            const uint32_t slot = __float_as_uint(r1.z);
            // (slot < the instance count for every listed instance: a Gaussian is listed only by tiles of its rectangle.  The compare keeps a
            //  frame whose buffers do not belong together from writing outside the lease.)
            if (issue && slot < slot_capacity) {
                slots[4 * (size_t)slot + chan] = total;
                if (lane == 0) flags[slot] = 1;   // only flagged slots hold sums: the slot array itself is never cleared
            }
            acr = acg = acb = 0.f;
        }
    }
}

// Per-Gaussian sum of the slots, in a fixed order: det_reduce_kernel (render_bwd.hip) restated for three floats per slot and the caller's array as the
// target.  The wave's Gaussians own the contiguous slot range [prefix(first) .. prefix(last) + tiles_touched(last)); its flag bytes are
// fetched 4 x 64 at a time (coalesced, one memory round trip per 256 slots), the flagged slots' indices appended in slot order to a 64-entry
// batch in LDS.  A batch is reduced with every lane busy: lane l loads entry l's three floats, finds its owner among the wave's Gaussians (a
// 6-step search over their end offsets), a segmented inclusive scan adds each Gaussian's entries in a fixed tree, the last lane of each
// segment hands the total to its owner's lane through LDS, which adds it to its accumulator.
// LDS banks: ends[] / batch[] / s_touch[] are accessed at the lane's own index (or, the search's first step, at one address: a broadcast).
// s_out rows are three floats: 3 is coprime with the 32 banks, so the owners' reads (row = lane) are conflict-free.  Two kinds of access can
// conflict, neither by more than data allows: the search's later steps read ends[] at data-dependent indices (up to 2^step distinct
// addresses, at most 32-way in its last step when every lane of a half lands on an index of one bank -- consecutive indices lie on
// consecutive banks, so owners that differ by less than 32 never collide), and a segment's last lane writes row `owner`: two owners 32
// apart in one 32-lane half share a bank (2-way).
__global__ void __launch_bounds__(256) colour_slots_reduce_kernel(int P, const uint32_t* __restrict__ offsets_incl, const uint32_t* __restrict__ tiles_touched,
                                                                  const float* __restrict__ slots, const unsigned char* __restrict__ flags,
                                                                  float* __restrict__ dL_dcolor, size_t slot_capacity) {
    __shared__ uint32_t s_ends[4][64];
    __shared__ uint32_t s_batch[4][64];
    __shared__ float s_out[4][64][3];
    __shared__ unsigned char s_touch[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < P;
    const uint32_t n = valid ? tiles_touched[g] : 0u;
    const uint32_t end = valid ? offsets_incl[g] : 0u;
    const uint32_t base = end - n;
    const int g0 = blockIdx.x * blockDim.x + wave * 64;
    if (g0 >= P) return;  // wave-uniform
    const int last_lane = min(63, P - 1 - g0);
    const uint32_t wlo = (uint32_t)__builtin_amdgcn_readlane((int)base, 0);
    const uint32_t whi = (uint32_t)__builtin_amdgcn_readlane((int)end, last_lane);
    uint32_t* ends = s_ends[wave];
    uint32_t* batch = s_batch[wave];
    ends[lane] = valid ? end : 0xffffffffu;   // nondecreasing over the lanes (inclusive prefix sums); lanes past P: beyond every slot
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;

    auto reduce_batch = [&](uint32_t cnt) {   // cnt (wave-uniform, 1..64) slot indices in batch[], in slot order
        __builtin_amdgcn_wave_barrier();
        const bool act = (uint32_t)lane < cnt;
        const uint32_t k = act ? batch[lane] : 0u;
        float x0 = 0.f, x1 = 0.f, x2 = 0.f;
        if (act) {
            const float* sl = slots + 4 * (size_t)k;   // 16-byte slots; the fourth float is not read
            x0 = sl[0]; x1 = sl[1]; x2 = sl[2];
        }
        // owner = the wave's Gaussian whose slot range holds k = the number of end offsets <= k
        int owner = 0;
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1)
            if (ends[owner + st - 1] <= k) owner += st;
        if (!act) owner = 64 + lane;   // idle lanes: segments of their own
        // (the two shuffles stand alone, outside any short-circuit: a ds_bpermute returns 0 for a source lane that is not executing)
        const int owner_left = __shfl_up(owner, 1), owner_right = __shfl_down(owner, 1);
        int head = (lane == 0 || owner_left != owner) ? 1 : 0;
        const bool seg_last = act && (lane == 63 || owner_right != owner);
        // segmented inclusive scan over the 64 lanes (Hillis-Steele; a lane stops taking once a head lies in its window)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int hup = __shfl_up(head, d);
            const float u0 = __shfl_up(x0, d), u1 = __shfl_up(x1, d), u2 = __shfl_up(x2, d);
            if (lane >= d && head == 0) {
                x0 += u0; x1 += u1; x2 += u2;
                head = hup;
            }
        }
        s_touch[wave][lane] = 0;
        __builtin_amdgcn_wave_barrier();
        if (seg_last) {
            s_out[wave][owner][0] = x0; s_out[wave][owner][1] = x1; s_out[wave][owner][2] = x2;
            s_touch[wave][owner] = 1;
        }
        __builtin_amdgcn_wave_barrier();
        if (s_touch[wave][lane]) {
            acc0 += s_out[wave][lane][0]; acc1 += s_out[wave][lane][1]; acc2 += s_out[wave][lane][2];
        }
        __builtin_amdgcn_wave_barrier();
    };

    uint32_t nb = 0;   // slots in the batch (wave-uniform)
    constexpr int G = 4;   // flag bytes of G x 64 slots are fetched together
    for (uint64_t glo = wlo; glo < whi; glo += 64u * G) {  // wave-uniform trip count (64-bit: whi may lie within 256 of 2^32)
        bool flagged[G];
#pragma unroll
        for (int u = 0; u < G; u++) {
            const uint64_t k = glo + 64u * u + (uint32_t)lane;
            flagged[u] = k < whi && k < slot_capacity && flags[k] != 0;
        }
#pragma unroll
        for (int u = 0; u < G; u++) {
            const uint64_t m = __ballot(flagged[u]);
            const uint32_t c = (uint32_t)__popcll(m);
            if (c == 0u) continue;   // wave-uniform
            if (nb + c > 64u) { reduce_batch(nb); nb = 0u; }
            if (flagged[u]) batch[nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)(glo + 64u * u + (uint32_t)lane);
            nb += c;
        }
    }
    if (nb != 0u) reduce_batch(nb);
    if (valid) {
        float* out = dL_dcolor + 3 * (size_t)g;   // (3 P floats at any 4-byte alignment: three dword stores, the wave's 768 bytes contiguous)
        out[0] = acc0; out[1] = acc1; out[2] = acc2;
    }
}

hipError_t launch_render_backward_colour_fixed(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                               const float* subpixel_offset, const float* dL_dpix, float* dL_dcolor, bool exact, float* slots,
                                               unsigned char* flags, size_t slot_capacity, int P, hipStream_t stream) {
    const int tiles = gx * gy;
    if (tiles <= 0 || P <= 0) return hipSuccess;
#define WG_LAUNCH(EX)                                                                                                                               \
    hipLaunchKernelGGL(render_backward_colour_slots_kernel<EX>, dim3(tiles), dim3(64), 0, stream, W, H, gx, tiles, img.order_bwd, img.ranges,         \
                       b.point_list, g.splats, reinterpret_cast<const float2*>(subpixel_offset), img.n_contrib, img.tile_last, dL_dpix, g.rects,     \
                       g.point_offsets, g.tiles_touched, slots, flags, (uint32_t)slot_capacity)
    if (exact) WG_LAUNCH(true); else WG_LAUNCH(false);
#undef WG_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(colour_slots_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, g.point_offsets, g.tiles_touched, slots, flags,
                       dL_dcolor, slot_capacity);
    return hipGetLastError();
}

}  // namespace wg
