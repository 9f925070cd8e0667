/*
 * gh_vert.h — C-ABI of the fused vertex MLP block: what the reference's vert_valid and vert_pos_refinement
 * (tgs/models/verts_refinement.py:35-83) do with a materialised concatenation, a LayerNorm, three nn.Linear calls and their
 * elementwise launches, as one pass over the feature rows.
 *
 * Every point p carries a row x[p, :] of Cf float32 features and a position pts[p, :]. With D = Cf + 3 and Hd = D / 4 (integer
 * division), per row:
 *
 *     z    = (x[p, 0..Cf), pts[p, 0..3))                                         never written anywhere
 *     zn   = LayerNorm(z) * ln_weight + ln_bias     mean (corrected by the mean of the deviations from it), then the CENTRED sum of squares; biased variance; rstd = 1 / sqrt(var + eps)
 *     h1   = relu(fc1_weight (Hd, D) . zn + fc1_bias)
 *     h2   = fc2_weight (Hd, Hd) . h1 + fc2_bias
 *     o    = fc_weight (K, Hd) . h2 + fc_bias
 *     out  = sigmoid(o)                             GH_VERT_ACT_SIGMOID       (vert_valid, K = 1)
 *          = pts + tanh(o) * radius                 GH_VERT_ACT_TANH_OFFSET   (vert_pos_refinement, K = 3)
 *
 * The three layers run in this order; nothing is folded on the host. The backward recomputes the row's forward from x and pts:
 * nothing else is saved. The position enters through the MLP only: the `pts +` of GH_VERT_ACT_TANH_OFFSET is the reference's
 * `verts_position.detach()` and carries no gradient. The ReLU passes a gradient where its input is > 0.
 *
 * Summation. One 4-wave workgroup works on GH_VERT_ROWS rows, lane = row. The LayerNorm's two sums run over k in four interleaved
 * partial sums (k mod 4), each in ascending k, added as (s0 + s1) + (s2 + s3). A dot product of the forward likewise: four partial
 * sums (k mod 4) with one fmaf per term, ((s0 + s1) + (s2 + s3)) + bias. A gradient with respect to a layer's input is one chain of
 * fmaf over that layer's outputs in ascending order; the two means of the LayerNorm's backward are four partial sums over the
 * columns 16t + 4w .. 16t + 4w + 3 (w = 0..3), each ascending, added as (s0 + s1) + (s2 + s3). All of these orders depend on (Cf, K)
 * alone: a row's output, its grad_x and its grad_pts are bitwise the same whether it is computed alone or among 100,000 rows, at any
 * row stride. Parameter gradients are summed without atomics: one partial per workgroup (its GH_VERT_ROWS rows in ascending order) in
 * the workspace, then the partials in workgroup order, cut into GH_VERT_SEGMENTS contiguous runs whose sums are added in run order.
 * They are bitwise reproducible run to run for a given P.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or a short workspace. Row
 * strides are in float elements. x and grad_x need 4-byte alignment only (a column window of a wider tensor is read in place); the
 * other arrays are contiguous.
 *
 * Supported: 1 <= Cf <= GH_VERT_MAX_CF, K in {1, 3}, GH_VERT_ACT_TANH_OFFSET with K = 3 only; anything else is GH_ERR_INVALID_ARG.
 * P = 0 returns GH_OK without a launch.
 */
#ifndef GH_VERT_H
#define GH_VERT_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_VERT_ACT_SIGMOID 0u     /* out = sigmoid(o) */
#define GH_VERT_ACT_TANH_OFFSET 1u /* out = pts + tanh(o) * radius; K must be 3 */

#define GH_VERT_ROWS 64     /* rows per workgroup: one partial of every parameter gradient per GH_VERT_ROWS rows */
#define GH_VERT_SEGMENTS 16 /* runs of partials in the fixed-order sum */
#define GH_VERT_MAX_CF 256

typedef struct GhVertDesc {
  int32_t K;    /* outputs per row: 1 or 3 */
  uint32_t act; /* GH_VERT_ACT_* */
  float radius; /* read under GH_VERT_ACT_TANH_OFFSET */
  float eps;    /* the LayerNorm's; >= 0 */
} GhVertDesc;

/* The block's parameters, contiguous float32: ln_* (D), fc1_weight (Hd, D), fc1_bias (Hd), fc2_weight (Hd, Hd), fc2_bias (Hd),
 * fc_weight (K, Hd), fc_bias (K). GhVertGrads has the same shapes; every element is written. */
typedef struct GhVertParams {
  const float *ln_weight, *ln_bias, *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias, *fc_weight, *fc_bias;
} GhVertParams;

typedef struct GhVertGrads {
  float *ln_weight, *ln_bias, *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias, *fc_weight, *fc_bias;
} GhVertGrads;

/* Bytes of workspace gh_vert_backward needs to produce parameter gradients (0 for invalid sizes: P < 1, D outside
 * [4, GH_VERT_MAX_CF + 3], Hd != D / 4, K not 1 or 3). Pure host arithmetic. A backward without parameter gradients needs none. */
size_t gh_vert_workspace_bytes(int P, int D, int Hd, int K);

/* x: (P, Cf), row stride x_stride >= Cf. pts: (P, 3). out: (P, K), every element written. One launch. */
int gh_vert_forward(const float* x, int64_t x_stride, const float* pts, int P, int Cf, const GhVertParams* params,
                    const GhVertDesc* desc, float* out, void* hip_stream);

/*
 * g_out: the gradient of out, (P, K), or NULL, which means zero. grad_x: (P, Cf) with row stride gx_stride >= Cf, every element
 * written. grad_pts: (P, 3), every element written, or NULL. grads: NULL for frozen parameters — one launch, no workspace; otherwise
 * all eight pointers set, workspace >= gh_vert_workspace_bytes(P, Cf + 3, (Cf + 3) / 4, K) bytes, 16-byte aligned — two launches.
 */
int gh_vert_backward(const float* x, int64_t x_stride, const float* pts, int P, int Cf, const GhVertParams* params,
                     const GhVertDesc* desc, const float* g_out, float* grad_x, int64_t gx_stride, float* grad_pts,
                     const GhVertGrads* grads, void* workspace, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_VERT_H */
