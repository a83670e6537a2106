// Device-resident training frames for gfx950 (include/wg_frames.h): float32 frames whose every value is exactly k / 255 are kept as uint8
// (pack) and turned back into planar float32, bit for bit, at each access (unpack).
//
// Both kernels are pure streaming work: pack reads 4 B and writes 1 B per element, unpack reads 1 B and writes 4 B.  A thread takes FOUR
// consecutive elements (pack) or pixels (unpack): one 16-byte load and one dword store in pack; in unpack C dwords of a pixel-major frame
// (four pixels of C bytes are exactly C dwords) or one dword per plane, and one 16-byte store into each plane.  Planes start at HW * 4 bytes,
// so the 16-byte store needs HW % 4 == 0; the wide forms are template parameters chosen per launch from the addresses (as run-time flags
// the compiler folds the two store forms into the narrow one), bytes and single floats are used elsewhere, and the HW % 4 (n % 4) tail goes
// element by element through the thread that owns the last, partial group.
// A workgroup is ONE wave of 64 threads, 256 elements: the kernels have no reuse and no LDS, and small workgroups keep the ragged end short.
// The grid is capped and strided with 64-bit indices.
//
// The conversion is (float)byte / 255.0f with the compiler's correctly rounded float32 division (no reciprocal, no fast-math flag on this
// file): tests/test_frame_store.py holds all 256 values to NumPy's division.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wg_frames.h"
#include "wg_rasterizer.h"

namespace wgf {

constexpr int TPB = 64;                // one wave
constexpr int PER = 4;                 // elements (pixels) per thread and step
constexpr unsigned MAX_BLOCKS = 8192;  // 256 CUs x 32 one-wave workgroups; larger frames stride
constexpr int FINISH_TPB = 256;

__device__ inline float byte_to_float(uint32_t b) { return (float)b / 255.0f; }

// -> 1 for a mismatch.  `b` is the stored byte (0 for a mismatch).
__device__ inline uint32_t pack_one(float v, uint32_t& b) {
    const float q = rintf(v * 255.0f);
    bool ok = q >= 0.f && q <= 255.f;   // false for NaN
    b = ok ? (uint32_t)q : 0u;          // -0.0 becomes byte 0, whose float is +0.0: the bits below differ
    ok = ok && __float_as_uint(byte_to_float(b)) == __float_as_uint(v);
    b = ok ? b : 0u;
    return ok ? 0u : 1u;
}

template <bool WIDE>
__global__ void __launch_bounds__(TPB) pack_kernel(size_t n, const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                   uint32_t* __restrict__ partials) {
    const size_t full = n / PER, groups = (n + PER - 1) / PER, step = (size_t)gridDim.x * TPB;
    uint32_t bad = 0;
    for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < groups; g += step) {
        if (g < full) {
            float v[PER];
            if (WIDE) {
                const float4 t = *reinterpret_cast<const float4*>(src + PER * g);
                v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
            } else {
#pragma unroll
                for (int p = 0; p < PER; ++p) v[p] = src[PER * g + p];
            }
            uint32_t w = 0;
#pragma unroll
            for (int p = 0; p < PER; ++p) {
                uint32_t b;
                bad += pack_one(v[p], b);
                w |= b << (8 * p);
            }
            if (WIDE) {
                *reinterpret_cast<uint32_t*>(dst + PER * g) = w;
            } else {
#pragma unroll
                for (int p = 0; p < PER; ++p) dst[PER * g + p] = (uint8_t)(w >> (8 * p));
            }
        } else {
            for (size_t i = PER * full; i < n; ++i) {
                uint32_t b;
                bad += pack_one(src[i], b);
                dst[i] = (uint8_t)b;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d);
    if (threadIdx.x == 0) partials[1 + blockIdx.x] = bad;
}

// partials[1 .. nb] added in workgroup order into partials[0] (integers: any order gives the same word; this one is fixed anyway)
__global__ void __launch_bounds__(FINISH_TPB) pack_finish_kernel(unsigned nb, uint32_t* __restrict__ partials) {
    __shared__ uint32_t red[FINISH_TPB / 64];
    uint32_t s = 0;
    for (unsigned i = threadIdx.x; i < nb; i += FINISH_TPB) s += partials[1 + i];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool WIDE>
__device__ inline uint32_t load_word(const uint8_t* __restrict__ s) {
    if (WIDE) return *reinterpret_cast<const uint32_t*>(s);
    return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}

// MODE 0: byte loads, single-float stores (any address).  1: dword loads, single-float stores (a pixel-major frame with HW % 4 != 0).
// 2: dword loads, 16-byte stores (HW % 4 == 0, or one channel).
template <int C, bool INTER, int MODE>
__global__ void __launch_bounds__(TPB) unpack_kernel(size_t HW, const uint8_t* __restrict__ src, float* __restrict__ dst) {
    constexpr bool WIDE_LOAD = MODE >= 1, WIDE_STORE = MODE == 2;
    const size_t full = HW / PER, groups = (HW + PER - 1) / PER, step = (size_t)gridDim.x * TPB;
    for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < groups; g += step) {
        if (g < full) {
            uint32_t b[C][PER];
            if (INTER) {
                uint32_t w[C];   // pixels 4 g .. 4 g + 3: 4 C bytes
#pragma unroll
                for (int k = 0; k < C; ++k) w[k] = load_word<WIDE_LOAD>(src + (PER * g) * C + 4 * k);
#pragma unroll
                for (int p = 0; p < PER; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c) b[c][p] = (w[(p * C + c) >> 2] >> (8 * ((p * C + c) & 3))) & 0xffu;
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t w = load_word<WIDE_LOAD>(src + (size_t)c * HW + PER * g);
#pragma unroll
                    for (int p = 0; p < PER; ++p) b[c][p] = (w >> (8 * p)) & 0xffu;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float* d = dst + (size_t)c * HW + PER * g;
                const float4 f = make_float4(byte_to_float(b[c][0]), byte_to_float(b[c][1]), byte_to_float(b[c][2]), byte_to_float(b[c][3]));
                if (WIDE_STORE) {
                    *reinterpret_cast<float4*>(d) = f;
                } else {
                    d[0] = f.x, d[1] = f.y, d[2] = f.z, d[3] = f.w;
                }
            }
        } else {
            for (size_t i = PER * full; i < HW; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) dst[(size_t)c * HW + i] = byte_to_float(INTER ? src[i * C + c] : src[(size_t)c * HW + i]);
        }
    }
}

inline unsigned blocks_for(size_t elements) {
    const size_t groups = (elements + PER - 1) / PER, blocks = (groups + TPB - 1) / TPB;
    return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int done() { return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP; }

constexpr size_t MAX_ELEMENTS = 0xffffffffUL;   // the mismatch count is one 32-bit word

template <int C, bool INTER>
inline void launch_unpack(int mode, unsigned blocks, hipStream_t stream, size_t HW, const uint8_t* src, float* dst) {
    if (mode == 2)
        hipLaunchKernelGGL((unpack_kernel<C, INTER, 2>), dim3(blocks), dim3(TPB), 0, stream, HW, src, dst);
    else if (mode == 1)
        hipLaunchKernelGGL((unpack_kernel<C, INTER, 1>), dim3(blocks), dim3(TPB), 0, stream, HW, src, dst);
    else
        hipLaunchKernelGGL((unpack_kernel<C, INTER, 0>), dim3(blocks), dim3(TPB), 0, stream, HW, src, dst);
}

template <int C>
inline void launch_unpack(bool inter, int mode, unsigned blocks, hipStream_t stream, size_t HW, const uint8_t* src, float* dst) {
    if (inter)
        launch_unpack<C, true>(mode, blocks, stream, HW, src, dst);
    else
        launch_unpack<C, false>(mode, blocks, stream, HW, src, dst);
}

}  // namespace wgf

using namespace wgf;

extern "C" {

size_t wg_frames_pack_scratch_words(size_t n) {
    if (n < 1 || n > MAX_ELEMENTS) return 0;
    return 1 + (size_t)blocks_for(n);
}

int wg_frames_pack(size_t n, const float* src, uint8_t* dst, uint32_t* mismatch_partials, void* stream) {
    if (n < 1 || n > MAX_ELEMENTS || !src || !dst || !mismatch_partials || !aligned(src, 4) || !aligned(mismatch_partials, 4))
        return WG_ERR_INVALID_ARGUMENT;
    const unsigned blocks = blocks_for(n);
    if (aligned(src, 16) && aligned(dst, 4))
        hipLaunchKernelGGL(pack_kernel<true>, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, n, src, dst, mismatch_partials);
    else
        hipLaunchKernelGGL(pack_kernel<false>, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, n, src, dst, mismatch_partials);
    if (hipGetLastError() != hipSuccess) return WG_ERR_HIP;
    hipLaunchKernelGGL(pack_finish_kernel, dim3(1), dim3(FINISH_TPB), 0, (hipStream_t)stream, blocks, mismatch_partials);
    return done();
}

int wg_frames_unpack(int C, size_t HW, int interleaved, const uint8_t* src, float* dst, void* stream) {
    if (C < 1 || C > 4 || HW < 1 || HW > MAX_ELEMENTS / 4 || !src || !dst || !aligned(dst, 4)) return WG_ERR_INVALID_ARGUMENT;
    const bool inter = interleaved != 0 && C > 1;   // one channel: both layouts are the same bytes
    const bool planes_on_4 = HW % 4 == 0 || C == 1;
    const bool wide_load = aligned(src, 4) && (inter || planes_on_4), wide_store = aligned(dst, 16) && planes_on_4;
    const int mode = !wide_load ? 0 : wide_store ? 2 : 1;
    const unsigned blocks = blocks_for(HW);
    const hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: launch_unpack<1>(inter, mode, blocks, s, HW, src, dst); break;
        case 2: launch_unpack<2>(inter, mode, blocks, s, HW, src, dst); break;
        case 3: launch_unpack<3>(inter, mode, blocks, s, HW, src, dst); break;
        default: launch_unpack<4>(inter, mode, blocks, s, HW, src, dst); break;
    }
    return done();
}

}  // extern "C"
