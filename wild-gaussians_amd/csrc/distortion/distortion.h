// Launchers of the distortion pass (distortion/distortion.hip, distortion/distortion_bwd.hip), declared here instead of in wg_common.h so that the
// operator's own files compile as before.
#pragma once
#include "wg_common.h"

namespace wg {

// the distortion pass (distortion/distortion.hip: render_distortion_kernel): per pixel A Q' - D'^2 of the blend weights' centred moments over each
// tile's first tile_last entries; values = nullptr: the scalar is |means3D[id] - campos|.  dist[H*W] is written in full, and so are the four
// planes moments[4*H*W] = (A, D', Q', c) when the pointer is given; only reads the frame
hipError_t launch_render_distortion(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                    const float* subpixel_offset, const float* values, const float* means3D, const float* campos, float* dist,
                                    float* moments, bool exact, hipStream_t stream);
// its gradient (distortion/distortion_bwd.hip: render_distortion_backward_kernel): per (tile, Gaussian) instance the seven geometry sums of
// record slots 3..9 ADDED into g.grad_rec and sum 2 g w (A u - D') ADDED into dL_dvalues (both float atomics); walks img.order_bwd, which the
// frame's backward call has written by then
hipError_t launch_render_distortion_backward(int W, int H, int gx, int gy, const ImageState& img, const BinningState& b, const GeometryState& g,
                                             const float* subpixel_offset, const float* dL_ddist, const float* moments, const float* values,
                                             const float* means3D, const float* campos, float* dL_dvalues, bool exact, hipStream_t stream);
// distance mode, behind the per-Gaussian backward kernel: dL_dmean3D[g] += dL_dvalues[g] * (means3D[g] - campos) / |means3D[g] - campos| (0 at distance 0)
hipError_t launch_distortion_distance_fold(int P, const float* means3D, const float* campos, const float* dL_dvalues, float* dL_dmean3D, hipStream_t stream);

}  // namespace wg
