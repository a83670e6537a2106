/* wg_dino.h -- C-ABI of the fused frozen DINOv2 ViT-S/14 feature extractor: what `UncertaintyModel._get_dino_cached` asks of its backbone,
 * `get_intermediate_layers(x, n=[k], reshape=True)[-1]` (wildgaussians/dinov2.py:789-813), forward only, float32 throughout, stopping at
 * block k, with no tensor of size N x N anywhere.
 *
 * Covered model (exactly what `dinov2_vits14_reg` builds; both ways of preparing the position embedding, which is the caller's): patch 14,
 * embed 384, 6 heads x 64, an `Mlp` FFN 384 -> 1536 -> 384 with the exact (erf) GELU, every bias on, LayerScale on both branches, LayerNorm with
 * the caller's eps, 1 class token and 4 register tokens put in front AFTER the position embedding is added (dinov2.py:704-723).
 *
 *   tokens     x[b, 0] = cls + pos[0];  x[b, 1..4] = the register tokens;  x[b, 5 + p] = patch_w . patch(p) + patch_b + pos[1 + p]
 *   block i    x += ls1 * (proj . attention(qkv . LN1(x) + qkv_b) + proj_b);   x += ls2 * (fc2 . gelu(fc1 . LN2(x) + fc1_b) + fc2_b)
 *   output     out[b, c, p] = LN(x[b, 5 + p])[c] after the last block that is run: [B, 384, h, w]
 *
 * N = 5 + h w tokens per image, h = H / 14, w = W / 14.  `pos` [1 + h w, 384] is the position embedding PREPARED for this grid: row 0 the class
 * token's, rows 1.. the patch rows of `interpolate_pos_encoding` (dinov2.py:670-702), which stays the caller's (bicubic F.interpolate, once per
 * grid size).  Weights are in nn.Linear layout, row-major [out, in]; patch_w is the convolution's [384, 3, 14, 14] read as [384, 588].
 *
 * Arithmetic: every product (the five linear shapes, q k^T and p v) is a float32-input, float32-accumulate MFMA (v_mfma_f32_32x32x2_f32),
 * i.e. k-ordered fmaf chains.  Attention is softmax(q k^T / 8) v per head with an online softmax over tiles of 64 keys; q is scaled by 1/8
 * (exactly) before the product, as the reference does.  There is no reduced-precision path and there are no atomics: two calls give the same
 * bits, and image b of a batch gives the bits of the single-image call (no value depends on where its row lies in a tile).
 *
 * Host contract: device pointers, explicit HIP stream, no host synchronisation, no allocation, nothing that prevents stream capture.
 * `scratch` holds at least wg_dino_scratch_floats(B, h, w) floats.  Every call returns 0 or a negative wg_status (wg_rasterizer.h); a malformed
 * call -- a struct_size that does not cover the fields, a NULL required pointer, H or W not a positive multiple of 14, a block count outside
 * 1..12, an unknown tiling, B < 1, a scratch that is too small, sizes whose index arithmetic would leave 31 bits -- is refused with
 * WG_ERR_INVALID_ARGUMENT before any device work.
 */
#ifndef WG_DINO_H
#define WG_DINO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WG_DINO_PATCH 14
#define WG_DINO_EMBED 384
#define WG_DINO_HEADS 6
#define WG_DINO_HEAD_DIM 64
#define WG_DINO_HIDDEN 1536
#define WG_DINO_LEAD_TOKENS 5        /* the class token and 4 register tokens */
#define WG_DINO_MAX_BLOCKS 12
#define WG_DINO_TILING_AUTO 0         /* 128 x 128 output tiles where that gives at least 128 workgroups, else 64 x 64 */
#define WG_DINO_TILING_64 1
#define WG_DINO_TILING_128 2
/* floats of scratch per token: the residual stream [384], one LayerNorm / attention output [384], and the packed QKV [1152] or the FFN's
 * hidden layer [1536], which share one buffer */
#define WG_DINO_SCRATCH_FLOATS_PER_TOKEN (WG_DINO_EMBED + WG_DINO_EMBED + WG_DINO_HIDDEN)

typedef struct wg_dino_block {
    const float* norm1_w; const float* norm1_b;     /* [384] */
    const float* qkv_w; const float* qkv_b;         /* [1152, 384], [1152]: rows q (6 heads x 64), then k, then v */
    const float* proj_w; const float* proj_b;       /* [384, 384], [384] */
    const float* ls1;                               /* [384] LayerScale gamma of the attention branch */
    const float* norm2_w; const float* norm2_b;     /* [384] */
    const float* fc1_w; const float* fc1_b;         /* [1536, 384], [1536] */
    const float* fc2_w; const float* fc2_b;         /* [384, 1536], [384] */
    const float* ls2;                               /* [384] LayerScale gamma of the FFN branch */
} wg_dino_block;

typedef struct wg_dino_args {
    size_t struct_size;      /* the caller's sizeof(wg_dino_args) */
    int32_t B, H, W;         /* image [B, 3, H, W]; H and W positive multiples of 14 */
    int32_t num_blocks;      /* blocks 0 .. num_blocks - 1 are run: 1..12 (the caller's k + 1) */
    float eps;               /* of every LayerNorm (> 0) */
    int32_t gemm_tiling;     /* WG_DINO_TILING_AUTO, or one of the two tilings for every product (tests reach both at small sizes); no bit depends on it */
    const float* image;
    const float* patch_w; const float* patch_b;     /* [384, 588], [384] */
    const float* pos;        /* [1 + h w, 384], prepared for this grid */
    const float* cls_token;  /* [384] */
    const float* reg_tokens; /* [4, 384] */
    wg_dino_block blocks[WG_DINO_MAX_BLOCKS];        /* the first num_blocks are read */
    const float* norm_w; const float* norm_b;       /* [384] the final norm */
    float* scratch;
    int64_t scratch_floats;  /* what `scratch` holds */
    float* out;              /* [B, 384, h, w] */
    void* stream;
} wg_dino_args;

/* = B * (5 + h * w) * WG_DINO_SCRATCH_FLOATS_PER_TOKEN.  Host arithmetic only; WG_ERR_INVALID_ARGUMENT for a negative argument,
 * WG_ERR_OVERFLOW when the count leaves 31 bits (such a call is refused by wg_dino_features too). */
int64_t wg_dino_scratch_floats(int32_t B, int32_t h, int32_t w);

int wg_dino_features(const wg_dino_args* args);

/* The attention stage alone: qkv [B, N, 3, 6, 64] packed as the QKV linear layer writes it -> out [B, N, 384] (head-major columns, as the
 * projection reads them).  B, N >= 1; no row past N is read, of either buffer. */
int wg_dino_attention(const float* qkv, int32_t B, int32_t N, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
