// Fused Gaussian activations + 3-D filter, forward and backward (include/wg_activations.h).
// Reference semantics: wildgaussians/method.py:1060-1086 with scaling_activation = exp, opacity_activation = sigmoid,
// rotation_activation = F.normalize.  Streaming kernels, one Gaussian per lane: 36 B in / 32 B out forward, 68 B in / 32 B
// out backward; everything is recomputed from the raw parameters in the backward pass (nothing is saved).
#include <hip/hip_runtime.h>
#include "wg_activations.h"
#include "wg_rasterizer.h"
#include "wg_act.h"
#include "wg_filter3d.h"

namespace wg {

__global__ void __launch_bounds__(256) activations_forward_kernel(int P, const float4* __restrict__ raw_rot, const float* __restrict__ raw_scale,
                                                                  const float* __restrict__ raw_opac, const float* __restrict__ filter,
                                                                  float4* __restrict__ rot, float* __restrict__ scale, float* __restrict__ opac) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const ActFwd a = act_forward(raw_rot[i], raw_scale[3 * i], raw_scale[3 * i + 1], raw_scale[3 * i + 2], raw_opac[i], filter[i]);
    rot[i] = a.q;
    scale[3 * i] = a.sc[0]; scale[3 * i + 1] = a.sc[1]; scale[3 * i + 2] = a.sc[2];
    opac[i] = a.o * a.coef;
}

__global__ void __launch_bounds__(256) activations_backward_kernel(int P, const float4* __restrict__ raw_rot, const float* __restrict__ raw_scale,
                                                                   const float* __restrict__ raw_opac, const float* __restrict__ filter,
                                                                   const float4* __restrict__ d_rot, const float* __restrict__ d_scale,
                                                                   const float* __restrict__ d_opac, float4* __restrict__ g_rot,
                                                                   float* __restrict__ g_scale, float* __restrict__ g_opac) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float4 r = raw_rot[i];
    const ActFwd a = act_forward(r, raw_scale[3 * i], raw_scale[3 * i + 1], raw_scale[3 * i + 2], raw_opac[i], filter[i]);
    const float4 dq = d_rot ? d_rot[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float dsc[3] = {d_scale ? d_scale[3 * i] : 0.f, d_scale ? d_scale[3 * i + 1] : 0.f, d_scale ? d_scale[3 * i + 2] : 0.f};
    float4 gr;
    float gs[3], go;
    act_backward(a, dq, dsc, d_opac ? d_opac[i] : 0.f, gr, gs, go);
    g_rot[i] = gr;
    g_opac[i] = go;
    g_scale[3 * i] = gs[0]; g_scale[3 * i + 1] = gs[1]; g_scale[3 * i + 2] = gs[2];
}

// ---- computation of filter_3D (include/wg_filter3d.h; wildgaussians/method.py:1140-1190) --------------------------------------------
// One Gaussian per lane, its position in three VGPRs for the whole camera loop.  The loop counter is wave-uniform, so the 64-byte
// camera record arrives by scalar loads and is used as SGPR operands.  Depth first: the screen test of a camera can only change a lane
// whose depth passes the near test AND is below the lane's minimum so far (or the lane has not been seen yet); when no lane of the wave
// is in that state the x / y arithmetic, the two divisions and the rest of the record are skipped behind a wave-uniform branch.
// Cameras are taken four at a time so that the four depth rows are in flight together.

__device__ __forceinline__ float filter3d_depth(const wg_filter3d_camera& k, float x, float y, float z) {
    return fmaf(k.w2c[8], x, fmaf(k.w2c[9], y, fmaf(k.w2c[10], z, k.w2c[11])));
}

// `best`: the smallest depth over the cameras that have seen the lane's point so far, NaN while none has (every comparison with it is false,
// so !(pz >= best) lets the first candidate through and afterwards means pz < best).
__device__ __forceinline__ void filter3d_camera_step(const wg_filter3d_camera& k, float x, float y, float z, float pz, bool live, float& best) {
    const bool need = live & (pz > 0.2f) & !(pz >= best);
    if (__builtin_amdgcn_ballot_w64(need) == 0) return;   // wave-uniform: a scalar compare of the mask
    const float px = fmaf(k.w2c[0], x, fmaf(k.w2c[1], y, fmaf(k.w2c[2], z, k.w2c[3])));
    const float py = fmaf(k.w2c[4], x, fmaf(k.w2c[5], y, fmaf(k.w2c[6], z, k.w2c[7])));
    const float zc = fmaxf(pz, 0.001f);
    const float u = px / zc * k.fx + k.width * 0.5f;    // width / 2, not cx (method.py:1172); this file is built without contraction
    const float v = py / zc * k.fy + k.height * 0.5f;
    // the limits as the reference forms them: a double product (numpy), rounded to float32 where it meets the float32 tensor
    const float u_lo = static_cast<float>(-0.15 * static_cast<double>(k.width)), u_hi = static_cast<float>(static_cast<double>(k.width) * 1.15);
    const float v_lo = static_cast<float>(-0.15 * static_cast<double>(k.height)), v_hi = static_cast<float>(1.15 * static_cast<double>(k.height));
    if (need & (u >= u_lo) & (u <= u_hi) & (v >= v_lo) & (v <= v_hi)) best = pz;   // `need` says pz is the new minimum
}

// distance[i] = min(100000, min over the cameras that see i of depth) for seen points, -1 for unseen ones; *seen_max (cleared by the
// entry point) = bit pattern of the largest distance of a seen point (positive floats order like their bit patterns), 0 if none.
__global__ void __launch_bounds__(256) filter3d_distance_kernel(int P, const float* __restrict__ xyz, int C,
                                                                const wg_filter3d_camera* __restrict__ cams, float* __restrict__ distance,
                                                                unsigned int* __restrict__ seen_max) {
    __shared__ float wave_max[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < P;
    const float x = live ? xyz[3 * i] : 0.f, y = live ? xyz[3 * i + 1] : 0.f, z = live ? xyz[3 * i + 2] : 0.f;
    float best = __builtin_nanf("");
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float pz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pz[j] = filter3d_depth(cams[c + j], x, y, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) filter3d_camera_step(cams[c + j], x, y, z, pz[j], live, best);
    }
    for (; c < C; ++c) filter3d_camera_step(cams[c], x, y, z, filter3d_depth(cams[c], x, y, z), live, best);
    const bool seen = best == best;
    const float dist = fminf(best, 100000.0f);   // a point whose only views are farther than that counts as seen, at 100000
    if (live) distance[i] = seen ? dist : -1.0f;
    float m = seen ? dist : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
        if (m > 0.f) atomicMax(seen_max, __float_as_uint(m));   // max is order-independent: the result does not depend on block order
    }
}

// unseen points take the largest distance of a seen one (100000 when nothing was seen); then distance / focal_length * float32(0.2 ** 0.5),
// a true division, so that equal distances give equal bits.
__global__ void __launch_bounds__(256) filter3d_finish_kernel(int P, float* __restrict__ filter, const unsigned int* __restrict__ seen_max,
                                                              float focal_length) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const unsigned int bits = *seen_max;
    const float fill = bits ? __uint_as_float(bits) : 100000.0f;
    const float d = filter[i];
    filter[i] = (d < 0.f ? fill : d) / focal_length * static_cast<float>(0.4472135954999579);
}

}  // namespace wg

extern "C" {

int wg_activations_forward(int P, const float* raw_rotations, const float* raw_scales, const float* raw_opacities,
                           const float* filter_3D, float* rotations, float* scales, float* opacities, void* stream) {
    if (P < 0 || P > 0x7fffffff / 4) return WG_ERR_INVALID_ARGUMENT;  // per-Gaussian element indices (3 i, 4 i) are 32-bit
    if (P == 0) return WG_OK;
    if (!raw_rotations || !raw_scales || !raw_opacities || !filter_3D || !rotations || !scales || !opacities) return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(wg::activations_forward_kernel, dim3((P + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), P,
                       reinterpret_cast<const float4*>(raw_rotations), raw_scales, raw_opacities, filter_3D,
                       reinterpret_cast<float4*>(rotations), scales, opacities);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

int wg_activations_backward(int P, const float* raw_rotations, const float* raw_scales, const float* raw_opacities,
                            const float* filter_3D, const float* dL_drotations, const float* dL_dscales, const float* dL_dopacities,
                            float* dL_draw_rotations, float* dL_draw_scales, float* dL_draw_opacities, void* stream) {
    if (P < 0 || P > 0x7fffffff / 4) return WG_ERR_INVALID_ARGUMENT;  // per-Gaussian element indices (3 i, 4 i) are 32-bit
    if (P == 0) return WG_OK;
    if (!raw_rotations || !raw_scales || !raw_opacities || !filter_3D || !dL_draw_rotations || !dL_draw_scales || !dL_draw_opacities)
        return WG_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(wg::activations_backward_kernel, dim3((P + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), P,
                       reinterpret_cast<const float4*>(raw_rotations), raw_scales, raw_opacities, filter_3D,
                       reinterpret_cast<const float4*>(dL_drotations), dL_dscales, dL_dopacities,
                       reinterpret_cast<float4*>(dL_draw_rotations), dL_draw_scales, dL_draw_opacities);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

int wg_compute_3d_filter(int P, const float* xyz, int num_cameras, const wg_filter3d_camera* cameras, float focal_length, float* filter_3D,
                         void* workspace, void* stream) {
    if (P < 0 || P > 0x7fffffff / 4 || num_cameras < 0) return WG_ERR_INVALID_ARGUMENT;  // the element index 3 i is 32-bit
    if (!(focal_length > 0.f) || !(focal_length <= 3.402823466e+38f)) return WG_ERR_INVALID_ARGUMENT;   // also NaN and infinity
    if (P == 0) return WG_OK;
    if (!xyz || !filter_3D || !workspace || (num_cameras > 0 && !cameras)) return WG_ERR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(workspace, 0, 8, s) != hipSuccess) return WG_ERR_HIP;
    hipLaunchKernelGGL(wg::filter3d_distance_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, xyz, num_cameras, cameras, filter_3D,
                       reinterpret_cast<unsigned int*>(workspace));
    hipLaunchKernelGGL(wg::filter3d_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, filter_3D,
                       reinterpret_cast<const unsigned int*>(workspace), focal_length);
    return hipGetLastError() == hipSuccess ? WG_OK : WG_ERR_HIP;
}

}  // extern "C"
