/* wg_frames.h -- C-ABI of the device-resident frame store: a trainer's ground-truth images and masks kept on the device as uint8 and turned
 * back into the planar float32 tensors the training step reads (wildgaussians/method.py:1716-1723 builds them, :1917-1918 fetches them),
 * bit for bit.
 *
 *   pack     q = rintf(src * 255); dst = q where 0 <= q <= 255 AND the bits of (float)q / 255.0f equal the bits of src; any other element
 *            (-0.0, NaN, 0.5, 1.0000001, a 16-bit source's value) is a MISMATCH: dst receives 0 and the element is counted.  One count per
 *            workgroup, added in workgroup order by a finishing launch: integers only, no atomics.  A frame with a count of 0 is exactly 8-bit
 *   unpack   dst [C, HW] planar float32 = (float)byte / 255.0f, one correctly rounded float32 division per element: what NumPy's
 *            astype(np.float32) / 255.0 gives for every one of the 256 byte values (a multiplication by 1.0f / 255.0f differs for 126 of them)
 *
 * Device pointers, an explicit HIP stream, no allocation.  Returns 0 or a negative wg_status (wg_rasterizer.h); invalid arguments (a null
 * pointer, a size of 0, C outside 1..4, a float pointer that is not 4-byte aligned, more elements than 32 bits count) are refused before any
 * device work.  Any other alignment is accepted: dword loads and 16-byte stores are used where the addresses allow them, bytes and single
 * floats elsewhere (HW % 4 != 0 leaves plane starts off a 16-byte boundary, and a tail of HW % 4 pixels).
 */
#ifndef WG_FRAMES_H
#define WG_FRAMES_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Words `mismatch_partials` of wg_frames_pack must hold (0 for an invalid n): word 0 receives the total, the per-workgroup counts follow. */
size_t wg_frames_pack_scratch_words(size_t n);

/* src [n] float32 -> dst [n] uint8; mismatch_partials[0] = the number of elements that are not exactly k / 255. */
int wg_frames_pack(size_t n, const float* src, uint8_t* dst, uint32_t* mismatch_partials, void* stream);

/* src: C * HW bytes, pixel-major (HW pixels of C bytes each) when interleaved != 0, planar [C, HW] otherwise -> dst [C, HW] float32. */
int wg_frames_unpack(int C, size_t HW, int interleaved, const uint8_t* src, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
