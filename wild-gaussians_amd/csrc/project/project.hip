// The projection-only pass (include/wg_rasterizer.h: wg_project_radii): a frame's cull decisions -- radii[i], so also radii[i] > 0 -- without
// rendering it.  radii depends on the geometry inputs and the camera only, and is decided in the first part of preprocess_kernel
// (preprocess.hip).  project_kernel restates that part statement for statement and in the same order: the optional raw-parameter activation, the
// near cull, the homogeneous projection, the 3-D covariance, the clamped EWA Jacobian, the 2-D covariance with the mip filter, the eigenvalue
// radius, the double-precision ndc2Pix and getRect against the tile grid.  This file is built with preprocess.hip's flags (build.py:
// -ffp-contract=off, -fno-slp-vectorize), every operation is a correctly rounded float32 / float64 one, and the shared device functions
// (cov3d_from_scale_rot, act_forward) switch contraction off for themselves: the same statements give the same bits, so radii equals what the
// forward call writes for the same inputs and camera.  The device code is duplicated from preprocess.hip on purpose: that kernel's code and
// resource usage stay untouched.
//
// A streaming kernel: 40 bytes read per Gaussian (12 mean + 12 scale + 16 rotation; 36 with cov3D_precomp; + 4 filter value in raw-parameter
// mode), 4 written, nothing else touched.  The raw opacity is NOT read: of act_forward's outputs only the normalised rotation and the filtered
// scales reach the radius, and those depend on the raw rotation, the raw scales and the filter value alone (wg_act.h).  No colour, no SH block,
// no scratch buffer, no atomics, no host synchronisation, no allocation: the launch can be captured in a stream.  Indices are size_t (P up to
// 2^31 - 1); a lane at or past P returns before it loads or stores anything; every element of radii[0 .. P) is written (0 = culled).
#include "wg_common.h"
#include "wg_act.h"

#pragma clang fp contract(off)

namespace wg {

template <bool PRECOMP, bool RAW>
__global__ void __launch_bounds__(256) project_kernel(const ProjectParams p) {
    static_assert(!(PRECOMP && RAW), "raw parameters are scale / rotation pairs");
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.P) return;

    float vm[16], pm[16];   // wave-uniform: scalar loads
#pragma unroll
    for (int i = 0; i < 16; i++) {
        vm[i] = p.viewmatrix[i];
        pm[i] = p.projmatrix[i];
    }
    const float px = p.means3D[3 * idx], py = p.means3D[3 * idx + 1], pz = p.means3D[3 * idx + 2];
    float sc0 = 0.f, sc1 = 0.f, sc2 = 0.f;
    float4 quat = make_float4(0.f, 0.f, 0.f, 0.f);
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f, c5 = 0.f;
    if (!PRECOMP) {
        sc0 = p.scales[3 * idx]; sc1 = p.scales[3 * idx + 1]; sc2 = p.scales[3 * idx + 2];
        if (p.rot_vec) {   // kernel argument: the rotations are 16-byte aligned (they always are from a tensor of whole rows)
            quat = reinterpret_cast<const float4*>(p.rotations)[idx];
        } else {
            const float* r = p.rotations + 4 * idx;
            quat = make_float4(r[0], r[1], r[2], r[3]);
        }
    } else {
        const float* c = p.cov3D_precomp + 6 * idx;
        c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3]; c4 = c[4]; c5 = c[5];
    }
    if (RAW) {   // get_gaussians() on the raw parameters; the opacity argument only reaches a.o, which nothing here reads
        const ActFwd a = act_forward(quat, sc0, sc1, sc2, 0.0f, p.filter_3D[idx]);
        quat = a.q;
        sc0 = a.sc[0]; sc1 = a.sc[1]; sc2 = a.sc[2];
    }

    int radius_i = 0;

    // in_frustum (near cull only)
    const float vx = vm[0] * px + vm[4] * py + vm[8] * pz + vm[12];
    const float vy = vm[1] * px + vm[5] * py + vm[9] * pz + vm[13];
    const float vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
    const bool alive = !(vz <= 0.2f);

    if (alive) {
        const float hx = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12];
        const float hy = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13];
        const float hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15];
        const float p_w = 1.0f / (hw + 0.0000001f);
        const float projx = hx * p_w, projy = hy * p_w;

        // ---- 3D covariance ----
        if (!PRECOMP) {
            float cv[6];
            cov3d_from_scale_rot(p.scale_modifier, sc0, sc1, sc2, quat, cv);
            c0 = cv[0]; c1 = cv[1]; c2 = cv[2]; c3 = cv[3]; c4 = cv[4]; c5 = cv[5];
        }

        // ---- EWA 2D covariance + mip filter ----
        const float limx = 1.3f * p.tan_fovx, limy = 1.3f * p.tan_fovy;
        const float txtz = vx / vz, tytz = vy / vz;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * vz;
        const float ty = fminf(limy, fmaxf(-limy, tytz)) * vz;
        const float j00 = p.focal_x / vz, j02 = -(p.focal_x * tx) / (vz * vz);
        const float j11 = p.focal_y / vz, j12 = -(p.focal_y * ty) / (vz * vz);
        // T = W*J with W[c][r] = vm[c + 4r]
        const float T00 = vm[0] * j00 + vm[2] * j02, T01 = vm[4] * j00 + vm[6] * j02, T02 = vm[8] * j00 + vm[10] * j02;
        const float T10 = vm[1] * j11 + vm[2] * j12, T11 = vm[5] * j11 + vm[6] * j12, T12 = vm[9] * j11 + vm[10] * j12;
        const float A00 = T00 * c0 + T01 * c1 + T02 * c2, A10 = T00 * c1 + T01 * c3 + T02 * c4, A20 = T00 * c2 + T01 * c4 + T02 * c5;
        const float A01 = T10 * c0 + T11 * c1 + T12 * c2, A11 = T10 * c1 + T11 * c3 + T12 * c4, A21 = T10 * c2 + T11 * c4 + T12 * c5;
        float cov00 = A00 * T00 + A10 * T01 + A20 * T02;
        const float cov01 = A01 * T00 + A11 * T01 + A21 * T02;
        float cov11 = A01 * T10 + A11 * T11 + A21 * T12;
        cov00 += p.kernel_size;
        cov11 += p.kernel_size;

        const float det = cov00 * cov11 - cov01 * cov01;
        if (det != 0.0f) {
            const float mid = 0.5f * (cov00 + cov11);
            const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
            const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
            const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
            // ndc2Pix (double)
            const float pixx = (float)((((double)projx + 1.0) * (double)p.W - 1.0) * 0.5);
            const float pixy = (float)((((double)projy + 1.0) * (double)p.H - 1.0) * 0.5);
            // getRect
            const int mr = (int)my_radius;
            const int rminx = min(p.gx, max(0, (int)((pixx - mr) / TILE_X)));
            const int rminy = min(p.gy, max(0, (int)((pixy - mr) / TILE_Y)));
            const int rmaxx = min(p.gx, max(0, (int)((pixx + mr + TILE_X - 1) / TILE_X)));
            const int rmaxy = min(p.gy, max(0, (int)((pixy + mr + TILE_Y - 1) / TILE_Y)));
            const int ntiles = (rmaxx - rminx) * (rmaxy - rminy);
            if (ntiles != 0) radius_i = mr;
        }
    }
    p.radii[idx] = radius_i;
}

hipError_t launch_project_radii(const ProjectParams& p, hipStream_t stream) {
    if (p.P <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((size_t)p.P + 255) / 256)), block(256);
    if (p.cov3D_precomp != nullptr) hipLaunchKernelGGL((project_kernel<true, false>), grid, block, 0, stream, p);
    else if (p.filter_3D != nullptr) hipLaunchKernelGGL((project_kernel<false, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((project_kernel<false, false>), grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace wg
