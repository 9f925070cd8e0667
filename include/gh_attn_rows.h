/*
 * gh_attn_rows.h — C-ABI of the row work around the interaction attention's core (gh_attn.h): what the reference's SelfAttn.forward
 * (tgs/models/self_attn.py:78-85) and the loop that calls it (renderer_one_shot.py:554-574) ask of a boolean gather, two LayerNorms,
 * six nn.Linear calls, a ReLU, two residual adds and a masked scatter, as one launch ahead of the core and one behind it, each way.
 * Network parameters are frozen: the backward produces the gradient of the features and nothing else.
 *
 * Rows. V rows are listed: row i of the launch is row r = idx[i] of X (idx == NULL: r = i). idx is int32 with entries in [0, rows of
 * X) that are DISTINCT — the caller guarantees it; two entries naming one row would race on Out and dX. X, Out, dOut and dX have F
 * columns of unit stride and the row strides of GhAttnRowsDims; everything else is contiguous. HD = H * 32. Per listed row:
 *
 *     pre_forward    xn = LayerNorm1(x);  qkv[i] = (Wq xn + bq, Wk xn + bk, Wv xn + bv)          (V, 3 * HD): the core reads it in place
 *                    stats1[i] = (mean, rstd)                                                    through stride_v = 3 * HD, stride_h = 32
 *     post_forward   y = x + (Wfc a[i] + bfc);  yn = LayerNorm2(y);  h = relu(W1 yn + b1);  Out[r] = y + (W2 h + b2)
 *                    saved: y[i] (F), stats2[i] = (mean, rstd), relu_mask[i]: bit j of word j / 32 is h[j] > 0
 *     post_backward  dz = dOut[r];  dh = (W2^T dz) where the mask has a bit;  dyn = W1^T dh;  dy = dz + LayerNorm2'(dyn)
 *                    da[i] = Wfc^T dy (V, HD): gh_attn_backward's dout;  dy[i] -> workspace (V, F)
 *     pre_backward   dxn = (Wq^T dq[i] + Wk^T dk[i]) + Wv^T dv[i];  dX[r] = dy[i] + LayerNorm1'(dxn)
 *
 * The ReLU is saved, not recomputed: with frozen weights the backward needs of relu(fc1(...)) only where it is positive, (hid + 31) / 32
 * words per row, which spares the backward the fc1 product (F x hid fmaf per row) for 4 to 24 bytes per row. The mask passes a gradient
 * where the ReLU's input is > 0, as torch does.
 *
 * Supported sizes. The head width is GH_ATTN_D (32) as the core's; 1 <= H <= GH_ATTN_ROWS_MAX_H, 1 <= F, hid <= GH_ATTN_ROWS_MAX_F,
 * 0 <= V <= GH_ATTN_MAX_V; anything else is GH_ERR_UNSUPPORTED before any launch (V < 0, a null pointer, a stride < F, an eps that is
 * not >= 0, a misaligned or short workspace: GH_ERR_INVALID_ARG / GH_ERR_WORKSPACE_SMALL). V = 0 launches nothing.
 *
 * Arithmetic (float32 throughout, -ffp-contract=off: FMAs only where stated). One 4-wave workgroup works on 64 rows, lane = row,
 * weights wave-uniform (32 rows, every row on two lanes, where the tile of 64 would not fit 128 KiB of LDS; the values are the same).
 *   moments    both LayerNorms: the mean, then the deviations' sum and the centred sum of squares (one fmaf per term), each as four
 *              partial sums over the columns k mod 4 in ascending k, added as (s0 + s1) + (s2 + s3); the mean is corrected by the
 *              deviations' mean c (mean + c, m2 = sum d^2 - c sum d, not below 0); biased variance; rstd = 1 / sqrtf(m2 / F + eps);
 *              xhat = (x - mean) * rstd, xn = fmaf(xhat, weight, bias). The backward recomputes xhat from the saved mean and rstd.
 *   forward    a dot product W[j, :] . in is four partial sums (k mod 4), one fmaf per term in ascending k, ((s0 + s1) + (s2 + s3)) +
 *              bias. The residuals add as written above: x + (dot + bias), y + (dot + bias).
 *   backward   a product W^T g is per input column one chain of fmaf over the layer's outputs in ascending order, from 0. The two
 *              means of a LayerNorm's backward (of g = weight * dxn and of g * xhat) are four partial sums over the columns
 *              16t + 4w .. 16t + 4w + 3 (w = 0..3), each ascending, added as (s0 + s1) + (s2 + s3), divided by F;
 *              pre_backward: dX[k] = dy[k] + fmaf(-xhat[k], m2, g[k] - m1) * rstd. post_backward folds the same expression into dz,
 *              which spares its tile a buffer: t = fmaf(g[k], rstd, dz[k]), dy[k] = fmaf(-rstd, fmaf(xhat[k], m2, m1), t).
 *              dxn = (Wq^T dq + Wk^T dk) + Wv^T dv.
 * Every order depends on (F, H, hid) alone: a row's qkv, Out, da and dX are bitwise the same whatever V, the row's place in the
 * launch, idx or the row strides. No atomics, nothing to zero: every element of a listed row of Out and dX is written, no other row
 * is touched.
 *
 * Conventions are those of gh_pool.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. All pointers 4-byte aligned,
 * the workspace 16-byte aligned.
 */
#ifndef GH_ATTN_ROWS_H
#define GH_ATTN_ROWS_H

#include "gh_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_ATTN_ROWS_MAX_H 8
#define GH_ATTN_ROWS_MAX_F 192 /* of F and of hid */

typedef struct GhAttnRowsDims {
  int32_t V, F, H, hid;
  float eps1, eps2; /* of the first LayerNorm and of the feed-forward block's; >= 0 */
  int64_t x_stride, out_stride, dout_stride, dx_stride; /* row strides in elements, each >= F; an entry point reads the ones it uses */
} GhAttnRowsDims;

/* The module's sixteen tensors in state-dict order, contiguous float32: w_* (HD, F) and (HD), ln* (F), fc (F, HD) and (F), fc1 (hid, F)
 * and (hid), fc2 (F, hid) and (F). */
typedef struct GhAttnRowsParams {
  const float *wq_weight, *wq_bias, *wk_weight, *wk_bias, *wv_weight, *wv_bias, *ln1_weight, *ln1_bias, *fc_weight, *fc_bias,
      *ln2_weight, *ln2_bias, *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias;
} GhAttnRowsParams;

/* Bytes of the workspace that carries dy from post_backward to pre_backward, (V, F) floats; 0 for unsupported or empty sizes. */
size_t gh_attn_rows_workspace_bytes(const GhAttnRowsDims* dims);

/* qkv: (V, 3 * HD), stats1: (V, 2); every element written. Reads x_stride. */
int gh_attn_rows_pre_forward(const GhAttnRowsDims* dims, const GhAttnRowsParams* params, const float* X, const int32_t* idx, float* qkv,
                             float* stats1, void* hip_stream);

/* a: the core's output, (V, HD). Out: the listed rows are written (it must not overlap X). y: (V, F), stats2: (V, 2), relu_mask:
 * (V, (hid + 31) / 32); every element written. Reads x_stride and out_stride. */
int gh_attn_rows_post_forward(const GhAttnRowsDims* dims, const GhAttnRowsParams* params, const float* X, const int32_t* idx,
                              const float* a, float* Out, float* y, float* stats2, uint32_t* relu_mask, void* hip_stream);

/* y, stats2, relu_mask: what post_forward saved. da: (V, HD), every element written. workspace: >= gh_attn_rows_workspace_bytes(dims)
 * bytes; it receives dy. Reads dout_stride. */
int gh_attn_rows_post_backward(const GhAttnRowsDims* dims, const GhAttnRowsParams* params, const float* dOut, const int32_t* idx,
                               const float* y, const float* stats2, const uint32_t* relu_mask, float* da, void* workspace,
                               size_t ws_bytes, void* hip_stream);

/* stats1: what pre_forward saved. dq, dk, dv: the core's, (V, HD) each. workspace: as post_backward left it. dX: the listed rows are
 * written. Reads x_stride and dx_stride. */
int gh_attn_rows_pre_backward(const GhAttnRowsDims* dims, const GhAttnRowsParams* params, const float* X, const int32_t* idx,
                              const float* stats1, const float* dq, const float* dk, const float* dv, const void* workspace,
                              size_t ws_bytes, float* dX, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_ATTN_ROWS_H */
