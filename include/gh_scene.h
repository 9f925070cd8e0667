/*
 * gh_scene.h — C-ABI of the texture scene code: the statements that turn the backbone's tokens into `scene_codes_texture`
 * (infer_one_shot.py:266-271): the sum of two token tensors, TriplaneLearnablePositionalEmbedding.detokenize
 * (tgs/models/tokenizers/triplane_texture.py:45-57), TriplaneUpsampleNetwork (tgs/models/networks_texture.py:30-54: a
 * ConvTranspose2d with kernel 2 and stride 2 per plane), the planes joined side by side, and the `map_bias` add.
 *
 * A transposed convolution with kernel 2 and stride 2 has no overlap: every output texel is one dot product over the input channels.
 * With x = tok_a + tok_b of shape (B, Ci, T), T = Np S^2, token t = p S^2 + y S + x_; W = upsample.weight (Ci, Co, 2, 2) read as
 * (Ci, 4 Co), column j = 4 o + 2 dy + dx; b = upsample.bias (Co,); pb = the first 2 S columns of a (Co, 2 S, Wb >= 2 S) parameter:
 *
 *     out[b, 0, o, 2y+dy, p 2S + 2x_+dx] = ( sum_c x[b,c,t] W[c,j]  +  b[o] )  +  pb[o, 2y+dy, 2x_+dx]
 *     d_tok[b, c, t]                     = sum_j W[c,j] dout[b, 0, o, 2y+dy, p 2S + 2x_+dx]
 *     d_plane_bias[o, Y, X]              = sum_b sum_p dout[b, 0, o, Y, p 2S + X]                        for X < 2 S
 *
 * Layouts. `out` and `dout` are contiguous: the joined form (B, 1, Co, 2S, Np 2S) by default, and with GH_SCENE_PER_PLANE in
 * GhSceneDims.flags the same values as (B, Np, Co, 2S, 2S), which is what TriplaneUpsampleNetwork.forward returns. Tokens are read
 * through a batch stride and a channel stride (in elements) with unit token stride; the plane bias through a channel stride and a row
 * stride with unit column stride, so that `map_bias` (80, 64, 128) is read in place through its first 64 columns.
 *
 * Arithmetic contract (the library is built with -ffp-contract=off; float32 throughout):
 *   x          one float add tok_a + tok_b (tok_a alone when tok_b is NULL).
 *   out        ONE chain of fmaf from 0 over c ascending, acc = fmaf(W[c,j], x[c], acc); then one add of b[o] (skipped when conv_bias
 *              is NULL); then one add of pb (skipped when plane_bias is NULL).
 *   d_tok      ONE chain of fmaf from 0 over j = 4 o + 2 dy + dx ascending, acc = fmaf(W[c,j], dout[..], acc).
 *   d_plane_bias  ONE chain of float adds from 0 over b ascending and, inside it, p ascending.
 * The products run on v_mfma_f32_32x32x2_f32, which is such a chain bit for bit. No atomics, and no sum is split across workgroups:
 * every result is bitwise reproducible. An element's value depends on its own token column (or its own texels) and the weights alone:
 * not on B, not on the tile it falls in, not on the strides and not on the output layout.
 *
 * Kernel shape. One wave works on a 32 x 32 tile with the token on the lane. Forward: D[j][t] = sum_c W[c][j] x[c][t]; both operands
 * are K-major in memory as they stand, so each lane's loads are coalesced without a transpose, and a lane's result registers r .. r+3
 * (r a multiple of 4) are one output channel's (dy, dx) quad: two 8-byte stores. Backward: D[c][t] = sum_j W[c][j] dout[j][t]; the
 * two lane halves read dx = 0 and dx = 1 of the same row, and the weight — the strided operand here — crosses LDS in slabs of
 * 32 x 32 with pitch 33. d_plane_bias is an elementwise kernel of its own.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. Gradients of the weight
 * and of the convolution's bias are not produced. 4-byte alignment suffices everywhere.
 *
 * Status, judged in this order, before any launch:
 *   GH_ERR_INVALID_ARG   dims is NULL; B < 0; Ci, Co, Np or S < 1; a flag other than GH_SCENE_PER_PLANE
 *   GH_ERR_UNSUPPORTED   Ci > GH_SCENE_MAX_CI; Co > GH_SCENE_MAX_CO; more than GH_SCENE_MAX_TILES wave tiles in one launch
 *   GH_ERR_INVALID_ARG   a required pointer is NULL or any pointer is not 4-byte aligned; a negative stride; plane_bias (or
 *                        d_plane_bias) together with GH_SCENE_PER_PLANE
 *   GH_OK                B = 0 (nothing is launched); a backward with d_tok and d_plane_bias both NULL (nothing is launched)
 *   GH_ERR_LAUNCH        the runtime refused a launch
 */
#ifndef GH_SCENE_H
#define GH_SCENE_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_SCENE_PER_PLANE 1      /* GhSceneDims.flags: out / dout are (B, Np, Co, 2S, 2S) */
#define GH_SCENE_MAX_CI 1024      /* 1 <= Ci <= 1024 */
#define GH_SCENE_MAX_CO 128       /* 1 <= Co <= 128 */
#define GH_SCENE_MAX_TILES 2147483647 /* 32 x 32 wave tiles of one launch: B ceil(T / 32) ceil(4 Co / 32) forward, ... ceil(Ci / 32) backward */

typedef struct GhSceneDims {
  int32_t B, Ci, Co, Np, S;
  uint32_t flags;
} GhSceneDims;

/*
 * tok_a (required), tok_b (or NULL): (B, Ci, T) through their strides. weight: (Ci, 4 Co) contiguous (required). conv_bias: (Co,) or
 * NULL. plane_bias: (Co, 2S, >= 2S) through pb_stride_c, pb_stride_r, or NULL (required NULL with GH_SCENE_PER_PLANE).
 * out (required): every element is written. One launch.
 */
int gh_scene_code_forward(const GhSceneDims* dims, const float* tok_a, int64_t a_stride_b, int64_t a_stride_c, const float* tok_b,
                          int64_t b_stride_b, int64_t b_stride_c, const float* weight, const float* conv_bias, const float* plane_bias,
                          int64_t pb_stride_c, int64_t pb_stride_r, float* out, void* hip_stream);

/*
 * weight, dout (required): as above, dout contiguous in the layout `dims->flags` names. d_tok: (B, Ci, T) contiguous, every element
 * written, or NULL to skip the product (the fit that trains the plane bias only). d_plane_bias: written (not added into) over its
 * first 2 S columns only, through dpb_stride_c, dpb_stride_r, or NULL (required NULL with GH_SCENE_PER_PLANE). One launch each.
 */
int gh_scene_code_backward(const GhSceneDims* dims, const float* weight, const float* dout, float* d_tok, float* d_plane_bias,
                           int64_t dpb_stride_c, int64_t dpb_stride_r, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_SCENE_H */
