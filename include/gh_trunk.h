/*
 * gh_trunk.h — C-ABI of the fused Gaussian trunk: what the reference's forward_gs (tgs/models/renderer_one_shot.py:254-257) does with
 * its trunk MLP (tgs/models/networks.py:57-105: Linear, activation, Linear, activation, Linear) followed by GSLayer.forward, as one
 * pass over the feature rows each way.
 *
 * Every point p carries a row x[p, :] of Cin float32 features and a position pts[p, :]. With act the activation selected,
 *
 *     v1[p] = b1 + W1 . x[p]              W1 (H, Cin)
 *     v2[p] = b2 + W2 . act(v1[p])        W2 (H, H)
 *     y[p]  = b3 + W3 . act(v2[p])        W3 (Cout, H)
 *     raw[p] = bh + Wh . y[p]             Wh (O, Cout): the five heads concatenated in gh_head.h's order, O = 11 + shs_width
 *
 * and the five outputs are gh_head.h's activations of raw[p] and pts[p], formula for formula (the GhHeadDesc is gh_head.h's).
 *   GH_TRUNK_SILU   act(v) = v / (1 + exp(-v));    act'(v) = s (1 + v (1 - s)) with s = 1 / (1 + exp(-v))
 *   GH_TRUNK_RELU   act(v) = 0 for v < 0, else v (a NaN passes);    act'(v) = 1 for v > 0, else 0 (a NaN v makes the
 *                   gradient NaN, as it makes the output)
 *
 * Backward, for frozen weights: with graw the gradient of raw under gh_head.h's backward formulas (trunc_exp's clamp at 15, the clip
 * gate, F.normalize's floor, sigmoid), read from the forward's `raw`,
 *
 *     dy = Wh^T . graw      dv2 = act'(v2) * (W3^T . dy)      dv1 = act'(v1) * (W2^T . dv2)      grad_x = W1^T . dv1
 *
 * v1 and v2 are recomputed from x, bit for bit as the forward computed them; nothing of the hidden layers is stored. grad_pts is the
 * cotangent of xyz (zeros where it is NULL). No gradient of a weight is produced.
 *
 * Summation. Every element is ONE chain of fmaf — the products run on v_mfma_f32_32x32x2_f32, which is such a chain bit for bit — whose
 * accumulator starts at the bias for the hidden layers and y, and at 0 for raw and in the backward:
 *   v1      over k = 0 .. Cin-1 ascending.
 *   v2, y   over the input channel j = 32 t + 8 q + 4 e + i, the loops nested t (0 .. H/32-1), q (0 .. 3), i (0 .. 3), e (0, 1) from the
 *           outside in: the order in which the matrix instruction's result registers hold the previous layer (gh_res.h's order).
 *   raw     over y's channels in that same order (t up to Cout/32-1), from 0; bh[o] is added to the finished sum, as gh_head.h adds
 *           its bias (a scaling bias of -5 at the start of the chain would put every one of its roundings at that magnitude).
 *   dy      over o = 0 .. O-1 ascending.
 *   W3^T . dy, W2^T . dv2, W1^T . dv1    over the rows of W3, W2, W1 in that register order.
 * The orders depend on (Cin, H, Cout, O) alone: a row's outputs, its raw and its grad_x are bitwise the same whether the row is
 * alone, in a tail tile or among 100,000 rows, at any row stride. No atomics: results are bitwise reproducible run to run.
 *
 * One 4-wave workgroup works on GH_TRUNK_ROWS rows, 32 per wave with the point on the lane; the weights cross LDS in slabs shared by
 * the waves, the hidden rows stay in the accumulators from one product to the next.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, no global state, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. P = 0
 * returns GH_OK without a launch. Row strides are in float elements; everything but x and grad_x is contiguous. 4-byte alignment
 * suffices everywhere (16-byte aligned arrays are moved four floats at a time). Sizes outside
 *
 *     1 <= Cin <= GH_TRUNK_MAX_CIN,    H and Cout each one of 32, 64, 96, 128,    shs_width one of gh_head.h's
 *
 * are refused with GH_ERR_UNSUPPORTED.
 */
#ifndef GH_TRUNK_H
#define GH_TRUNK_H

#include "gh_head.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_TRUNK_SILU 0
#define GH_TRUNK_RELU 1

#define GH_TRUNK_ROWS 128    /* rows per workgroup */
#define GH_TRUNK_MAX_CIN 192 /* six slabs of 32 columns */

/*
 * x: (P, Cin), row stride x_stride >= Cin. pts: (P, 3). Outputs, every element written: xyz (P, 3), scaling (P, 3), rotation (P, 4),
 * opacity (P, 1), shs (P, shs_width); raw (P, O) or NULL: the head's pre-activations, which the backward reads. One launch.
 */
int gh_trunk_forward(const float* x, int64_t x_stride, int P, int Cin, int H, int Cout, const float* pts, const float* W1,
                     const float* b1, const float* W2, const float* b2, const float* W3, const float* b3, const float* Wh,
                     const float* bh, const GhHeadDesc* desc, int activation, float* xyz, float* scaling, float* rotation,
                     float* opacity, float* shs, float* raw, void* hip_stream);

/*
 * raw: what the forward wrote. g_*: the gradients of the five outputs, shaped like them; any may be NULL, which means zero.
 * grad_x: (P, Cin) with row stride gx_stride >= Cin, every element written. grad_pts: (P, 3) or NULL. One launch. (b3 and bh do not
 * enter a gradient, and pts enters none but its own, which is g_xyz.)
 */
int gh_trunk_backward(const float* raw, const float* x, int64_t x_stride, int P, int Cin, int H, int Cout, const float* W1,
                      const float* b1, const float* W2, const float* b2, const float* W3, const float* Wh, const GhHeadDesc* desc,
                      int activation, const float* g_xyz, const float* g_scaling, const float* g_rotation, const float* g_opacity,
                      const float* g_shs, float* grad_x, int64_t gx_stride, float* grad_pts, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_TRUNK_H */
