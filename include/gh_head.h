/*
 * gh_head.h — C-ABI of the fused Gaussian head: what the reference's GSLayer.forward (tgs/models/renderer_one_shot.py:156-214)
 * does with five nn.Linear calls and eight to ten elementwise launches, as one pass over the feature rows.
 *
 * Every point p carries a row x[p, :] of Cin float32 features and a position pts[p, :]. The five heads' weights are handed in
 * concatenated in the order of the reference's `feature_channels`: W (O, Cin) and b (O) with the rows
 *
 *     [0, 3) xyz    [3, 6) scaling    [6, 10) rotation    [10, 11) opacity    [11, 11 + shs_width) shs        O = 11 + shs_width
 *
 * raw[p, o] = b[o] + sum_k x[p, k] * W[o, k], and the activations are GSLayer.forward's with tgs/utils/ops.py:37-53 (trunc_exp):
 *
 *   xyz       (sigmoid(v) - 0.5) * (1.2 / 32) under GH_HEAD_RESTRICT_OFFSET, else v; then + pts under GH_HEAD_XYZ_OFFSET. Without
 *             GH_HEAD_XYZ_OFFSET the output is pts itself and no gradient reaches v.
 *   scaling   exp(v); backward g * exp(min(v, 15)). Under GH_HEAD_CLIP_SCALING clamped to [0, clip_scaling], the gradient passing
 *             only where exp(v) lies inside the closed interval.
 *   rotation  v / max(|v|_2, 1e-12); backward (g - n (n . g)) / |v|_2 with n = v / |v|_2 where |v|_2 >= 1e-12, g / 1e-12 below.
 *   opacity   sigmoid(v).
 *   shs       sigmoid(v) under GH_HEAD_USE_RGB, else v.
 *
 * Summation. A dot product of the forward runs over k in four interleaved partial sums (k mod 4), each in ascending k with one
 * fmaf per term, added as ((s0 + s1) + (s2 + s3)) + b[o]. A grad_x element is one chain of fmaf over o = 0 .. O-1. Both orders
 * depend on (Cin, O) alone: a row's outputs and its grad_x are bitwise the same whether it is computed alone or among 100,000
 * rows, at any row stride. grad_W and grad_b are summed without atomics: one partial per workgroup (GH_HEAD_ROWS rows in ascending
 * row order) in the workspace, then the partials in workgroup order, cut into GH_HEAD_SEGMENTS contiguous runs whose sums are added
 * in run order. They are bitwise reproducible run to run for a given P.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, no global state, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or a short
 * workspace. Row strides are in float elements. x and grad_x need 4-byte alignment only (a column window of a wider tensor is read
 * in place); the other arrays are contiguous, and are written 16 bytes at a time where their base is 16-byte aligned.
 */
#ifndef GH_HEAD_H
#define GH_HEAD_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_HEAD_USE_RGB 1u         /* shs = sigmoid(raw); shs_width must be 3 */
#define GH_HEAD_XYZ_OFFSET 2u      /* xyz = offset + pts (else pts) */
#define GH_HEAD_RESTRICT_OFFSET 4u /* offset = (sigmoid(raw) - 0.5) * (1.2 / 32) (else raw) */
#define GH_HEAD_CLIP_SCALING 8u    /* clip_scaling is set */

#define GH_HEAD_ROWS 64     /* rows per workgroup: one partial of grad_W / grad_b per GH_HEAD_ROWS rows */
#define GH_HEAD_SEGMENTS 16 /* runs of partials in the fixed-order sum */
#define GH_HEAD_MAX_O 59    /* 11 + 3 * 16 */

typedef struct GhHeadDesc {
  int32_t shs_width;  /* 3, or 3 * M with M in {1, 4, 9, 16} */
  uint32_t flags;     /* GH_HEAD_* */
  float clip_scaling; /* read under GH_HEAD_CLIP_SCALING; >= 0 */
} GhHeadDesc;

/* Bytes of workspace gh_head_backward needs to produce grad_W / grad_b (0 for invalid sizes: P < 1, Cin < 1, O not 11 + a valid
 * shs width). Pure host arithmetic. A backward without grad_W and grad_b needs none. */
size_t gh_head_workspace_bytes(int P, int Cin, int O);

/*
 * x: (P, Cin), row stride x_stride >= Cin. pts: (P, 3). W: (O, Cin), b: (O), contiguous. Outputs, contiguous, every element written:
 * xyz (P, 3), scaling (P, 3), rotation (P, 4), opacity (P, 1), shs (P, shs_width); raw (P, O) or NULL: the pre-activations the
 * backward reads. One launch. P >= 1, Cin >= 1.
 */
int gh_head_forward(const float* x, int64_t x_stride, int P, int Cin, const float* pts, const float* W, const float* b,
                    const GhHeadDesc* desc, float* xyz, float* scaling, float* rotation, float* opacity, float* shs, float* raw,
                    void* hip_stream);

/*
 * raw: what the forward wrote. g_*: the gradients of the five outputs, shaped like them; any may be NULL, which means zero.
 * grad_x: (P, Cin) with row stride gx_stride >= Cin, every element written. grad_pts: (P, 3) or NULL. grad_W (O, Cin) and grad_b (O):
 * both or neither; when NULL none of the reduction work is done, x is not read and no workspace is needed. Otherwise workspace holds
 * >= gh_head_workspace_bytes(P, Cin, O) bytes, 16-byte aligned. One launch, two with grad_W / grad_b.
 */
int gh_head_backward(const float* raw, const float* x, int64_t x_stride, int P, int Cin, const float* W, const GhHeadDesc* desc,
                     const float* g_xyz, const float* g_scaling, const float* g_rotation, const float* g_opacity, const float* g_shs,
                     float* grad_x, int64_t gx_stride, float* grad_pts, float* grad_W, float* grad_b, void* workspace,
                     size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_HEAD_H */
