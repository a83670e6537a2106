/* wg_filter3d.h -- C-ABI of the fused computation of filter_3D ("fused activations / 3-D filter").
 *
 * Replaces, as an opt-in for callers, GaussianModel.compute_3D_filter (wildgaussians/method.py:1140-1190), which the training loop
 * runs at set-up, after every densify_and_prune and every 100 steps afterwards.  The reference loops in Python over all training
 * cameras; per camera, with (R, T) the world-to-camera transform (the inverse of the pose, taken on the host):
 *
 *     p = R xyz + T;  valid_depth = p.z > 0.2;  z = max(p.z, 0.001)
 *     u = p.x / z * fx + width / 2;  v = p.y / z * fy + height / 2                (width / 2, not cx)
 *     valid = valid_depth and -0.15 width <= u <= 1.15 width and -0.15 height <= v <= 1.15 height
 *     distance[valid] = min(distance[valid], z[valid])                            (distance starts at 100000)
 *
 * and then: points no camera sees get the largest distance of a seen point; filter_3D = distance / focal_length * float32(0.2 ** 0.5)
 * with focal_length the largest fx of ALL cameras (the caller passes it).  Here: one kernel over all (Gaussian, camera) pairs with
 * the camera record in scalar registers, and one small kernel for the fill and the scale; the largest seen distance travels through
 * `workspace`.  The three products of a row and the translation are summed with fused multiply-adds, the divisions are IEEE.
 *
 * The case the reference leaves undefined (it raises) -- NO point is seen by any camera, which includes num_cameras == 0 -- is
 * defined here: every value is 100000 / focal_length * float32(0.2 ** 0.5), what the reference's `distance` holds at that moment.
 *
 * Stream-ordered on `stream`: no allocation, no synchronisation, no read-back.  Results are bit-identical from run to run.
 * float32 device pointers: xyz [P, 3], filter_3D [P] (written whole); `cameras` may be NULL when num_cameras == 0.  Two calls
 * that may overlap (different streams) need a workspace each.
 * Returns 0 or a negative wg_status (wg_rasterizer.h): P < 0, num_cameras < 0, a null pointer with P > 0, focal_length <= 0 or
 * not finite -> WG_ERR_INVALID_ARGUMENT; P == 0 -> WG_OK, nothing launched.
 */
#ifndef WG_FILTER3D_H
#define WG_FILTER3D_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct wg_filter3d_camera {   /* 64 bytes, device memory, one per camera */
    float w2c[12];                    /* rows of [R | T], world -> camera */
    float fx, fy, width, height;
} wg_filter3d_camera;

/* xyz[P,3] -> filter_3D[P]; workspace: 8 bytes of device memory owned by the caller, contents irrelevant on entry */
int wg_compute_3d_filter(int P, const float* xyz, int num_cameras, const wg_filter3d_camera* cameras, float focal_length,
                         float* filter_3D, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
