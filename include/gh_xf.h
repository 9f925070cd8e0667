/*
 * gh_xf.h — C-ABI of the Transformer1D backbones' forward for frozen inference: what the reference's two backbones
 * (tgs/models/transformers.py:673-908, called at infer_one_shot.py:256-264) ask of a GroupNorm, about 85 library launches of
 * dense float32 GEMMs, LayerNorms, SDPA and a GEGLU per forward. Forward only: there is no backward here, and the Python layer
 * falls back to torch wherever a gradient is wanted.
 *
 * The module's mathematics, written from transformers.py and the attribute layout of diffusers' Attention (not pinned against
 * a recorded run of the reference):
 *   input     x (B, C, N) channel first. GroupNorm with G groups, eps gn_eps, affine; read as (B N, C) rows; proj_in (C -> M,
 *             bias), M = heads * D.
 *   block     h += to_out0(attn(LN1(h)));  h += to_out0'(attn'(LN2(h))) where attn2 exists (it attends to h itself);
 *             h += W2 (a * gelu(g)) + b2 with [a | g] = W1 LN3(h) + b1, W1 (8M, M), gelu(g) = 0.5 g (1 + erf(g / sqrt 2)).
 *             to_q, to_k, to_v carry no bias, to_out[0] one. Scores are (q.k) * D^-0.5, softmax over all N keys of the same
 *             batch element and head. LayerNorm eps ln_eps, affine.
 *   output    proj_out (M -> C, bias), written back channel first, plus the input x.
 *
 * Entry points.
 *   gh_xf_linear         Y = epilogue(prologue(X) W^T) over T rows, K a multiple of 32, 1 <= N_out <= GH_XF_MAX_N_OUT.
 *                          prologues   NONE; LN (LayerNorm over the row's K columns); GN (GroupNorm from the per-(batch, group)
 *                                      moments gh_xf_group_moments wrote, X read channel first: element (t, c) of the rows is
 *                                      x[b * x_stride_b + c * x_stride + n], t = b * rows_per_batch + n).
 *                          epilogues   PLAIN (with [Wq; Wk; Wv] stacked this writes (T, 3M) in one launch); BIAS_RES
 *                                      (+ bias + residual; res == NULL is the bias alone; res may be y itself); GEGLU (W has
 *                                      2 N_out rows, value rows first: a workgroup forms the value and the gate column tile
 *                                      together and writes a * gelu(g), so the (T, 8M) array never exists); BIAS_RES_CF
 *                                      (+ bias + residual, y and res channel first: element (t, j) at
 *                                      [b * stride_b + j * stride + n]).
 *                        The LayerNorm's row moments are formed by a row launch ahead of the product (one wave per row) into
 *                        the workspace, not inside the product kernel: a row's moments would otherwise be formed again by
 *                        every column tile. So an LN call is two launches and needs gh_xf_linear_workspace_bytes.
 *   gh_xf_group_moments  mean and sum of squared deviations per (batch, group), two launches.
 *   gh_xf_attention      softmax(q k^T D^-0.5) v per (batch, head), D in {32, 64}: q, k and v are read in place from one
 *                        (T, 3M) buffer (q at column h D, k at M + h D, v at 2M + h D of a row), out is (T, M). No score
 *                        matrix is written and there is no lse output.
 *   gh_xf_forward        the whole stack, enqueued from C++ in one host call: 4 + 11 launches per layer (7 where attn2 is
 *                        absent).
 *
 * Supported sizes. D in {32, 64}; M = heads * D <= GH_XF_MAX_M; C a multiple of G and of 32, C <= GH_XF_MAX_C; K a multiple
 * of 32 and <= GH_XF_MAX_K and N_out <= GH_XF_MAX_N_OUT in gh_xf_linear; any N >= 1 and B >= 1 with B * N <= GH_XF_MAX_T and every launch's workgroup count
 * within int32. Anything else is GH_ERR_UNSUPPORTED before any launch. B = 0 or N = 0 (T = 0) launches nothing: GH_OK.
 *
 * Arithmetic (float32 throughout, no reduced precision, -ffp-contract=off: FMAs only where stated; no atomics, no workgroup
 * waits for another, every result bitwise reproducible).
 *   product    a workgroup of 4 waves owns GH_XF_ROWS x GH_XF_COLS outputs, a wave 32 x 32 (two such tiles for GEGLU). X and W
 *              cross LDS in slabs of 32 columns; the products are v_mfma_f32_32x32x2_f32, exact float32. Each output is one
 *              ascending fmaf chain over k = 0 .. K - 1 that starts from the bias (BIAS_RES, BIAS_RES_CF, GEGLU) or from zero
 *              (PLAIN); the residual is added to the finished chain. gelu(g) = (0.5 g) * (1 + erff(g * 0.70710678f)).
 *   LayerNorm  two passes per row by one wave: lane l sums the columns l, l + 64, ... in ascending order, the 64 shares are
 *              added by the butterfly xor 32, 16, 8, 4, 2, 1; mean = sum / K; then the squared deviations fmaf(d, d, .) in the
 *              same order; rstd = 1 / sqrtf(m2 / K + eps). The row enters the product as ((x - mean) * rstd) * gamma + beta.
 *   GroupNorm  stage one: a workgroup per (batch, group, chunk of GH_XF_GN_CHUNK positions) — thread i owns position n0 + i and
 *              sums its group's channels in ascending order, the wave's shares are added by the same butterfly and the four
 *              waves as (s0 + s1) + (s2 + s3); the chunk's mean, then its squared deviations the same way. Stage two: one
 *              thread per (batch, group) joins the chunks in ascending order by the pairwise update delta = mean_c - mean,
 *              mean += delta * n_c / n, m2 += m2_c + delta^2 * n_a * n_c / n. The moments written are {mean, m2}; the
 *              prologue forms rstd = 1 / sqrtf(m2 / (cpg N) + eps) and ((x - mean) * rstd) * gamma + beta.
 *   attention  a workgroup owns GH_XF_ATTN_ROWS = 64 queries of one (batch, head): waves 0, 1 the first 32, waves 2, 3 the
 *              second. K and V cross LDS 64 keys at a time; of each such stage the even wave of a pair folds keys 0 .. 31, the
 *              odd wave keys 32 .. 63, each with a running maximum m and sum l of its own: s = (q.k) * scale with q.k one
 *              ascending fmaf chain over d from 0 and scale = float32(D^-0.5); a key past N scores -inf and contributes
 *              exactly 0; m' = max(m, max of the tile), p = expf(s - m'), l = l * expf(m - m') + (sum of p), acc = acc *
 *              expf(m - m') then acc = fmaf(p, v, acc) key by key. Inside a tile the 32 keys enter the sum of p as two
 *              ascending chains of 16 (keys with bit 2 clear, keys with bit 2 set) added at the end, and enter acc in the
 *              order 0 4 1 5 2 6 3 7 8 12 9 13 ... (gh_attn.h's order). At the end the pair is joined in a fixed order:
 *              mm = max(m0, m1), l = l0 * expf(m0 - mm) + l1 * expf(m1 - mm), acc = acc0 * expf(m0 - mm) + acc1 * expf(m1 -
 *              mm), out = acc / l. An odd wave that met no key has m1 = -inf, l1 = 0 and contributes exactly 0.
 *   A row's result in gh_xf_linear is a function of that row (and, under GN, of its batch element's moments) alone, and a
 *   query's attention of its q and the batch element's K and V alone: not of the row's place in the launch, of B, or of whether
 *   16-byte loads were used.
 *
 * Conventions are those of gh_pool.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, nothing thrown, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or a
 * short workspace. Strides are in float elements. All pointers 4-byte aligned, a workspace 16-byte aligned. An input whose
 * pointer is 16-byte aligned and whose row stride is a multiple of 4 is staged with 16-byte loads; the values do not depend on
 * it.
 */
#ifndef GH_XF_H
#define GH_XF_H

#include "gh_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_XF_ROWS 64      /* rows of X per workgroup of the product */
#define GH_XF_COLS 64      /* output columns per workgroup of the product */
#define GH_XF_ATTN_ROWS 64 /* queries per workgroup of the attention */
#define GH_XF_ATTN_KEYS 64 /* keys per LDS stage of the attention */
#define GH_XF_GN_CHUNK 256 /* positions per stage-one workgroup of the group moments */
#define GH_XF_MAX_M 1024
#define GH_XF_MAX_C 1024
#define GH_XF_MAX_K 4096   /* 4 GH_XF_MAX_M: the feed-forward's inner width */
#define GH_XF_MAX_N_OUT 8192 /* the widest output of gh_xf_linear: 8 GH_XF_MAX_M */
#define GH_XF_MAX_T (1 << 30)

#define GH_XF_PRO_NONE 0
#define GH_XF_PRO_LN 1
#define GH_XF_PRO_GN 2

#define GH_XF_EPI_PLAIN 0
#define GH_XF_EPI_BIAS_RES 1
#define GH_XF_EPI_GEGLU 2
#define GH_XF_EPI_BIAS_RES_CF 3

typedef struct GhXfLinear {
  int32_t T, K, N_out;      /* rows, inner width, width written (GEGLU: w has 2 N_out rows and bias 2 N_out entries) */
  int32_t prologue, epilogue;
  int32_t rows_per_batch;   /* N: PRO_GN and EPI_BIAS_RES_CF (T a multiple of it); ignored otherwise */
  int32_t groups;           /* PRO_GN: K a multiple of it */
  float eps;                /* PRO_LN, PRO_GN */
  const float* x;           /* PRO_NONE, PRO_LN: (T, K), row stride x_stride >= K. PRO_GN: see above */
  int64_t x_stride, x_stride_b;
  const float* w;           /* (N_out, K) contiguous; GEGLU (2 N_out, K) */
  const float* bias;        /* N_out (GEGLU 2 N_out); ignored by EPI_PLAIN */
  const float* gamma;       /* K: PRO_LN, PRO_GN */
  const float* beta;
  const float* moments;     /* PRO_GN: (T / rows_per_batch, groups, 2) from gh_xf_group_moments */
  const float* res;         /* EPI_BIAS_RES: (T, N_out) with row stride res_stride, or NULL. EPI_BIAS_RES_CF: channel first */
  int64_t res_stride, res_stride_b;
  float* y;                 /* (T, N_out) with row stride y_stride; EPI_BIAS_RES_CF: channel first. res may be y (same strides) */
  int64_t y_stride, y_stride_b;
} GhXfLinear;

typedef struct GhXfDims {
  int32_t B, C, N, G, heads, D, layers;
  float gn_eps, ln_eps;
} GhXfDims;

typedef struct GhXfStem {
  const float *gn_w, *gn_b; /* C */
  const float *in_w, *in_b; /* (M, C), M */
  const float *out_w, *out_b; /* (C, M), C */
} GhXfStem;

typedef struct GhXfLayer {
  const float *ln1_w, *ln1_b; /* M */
  const float* qkv1;          /* (3M, M): [Wq; Wk; Wv] of attn1 */
  const float *o1_w, *o1_b;   /* (M, M), M */
  const float *ln2_w, *ln2_b;
  const float* qkv2;          /* NULL where the block has no attn2: ln2 and o2 are then ignored */
  const float *o2_w, *o2_b;
  const float *ln3_w, *ln3_b;
  const float *ff1_w, *ff1_b; /* (8M, M), 8M: value rows first, then the gate's */
  const float *ff2_w, *ff2_b; /* (M, 4M), M */
} GhXfLayer;

/* Bytes of workspace gh_xf_linear needs: the row moments under PRO_LN, else 0 (also for invalid sizes). */
size_t gh_xf_linear_workspace_bytes(int T, int prologue);
int gh_xf_linear(const GhXfLinear* args, void* workspace, size_t ws_bytes, void* hip_stream);

/* x: element (b, c, n) at x[b * stride_b + c * stride_c + n]. moments: (B, G, 2) {mean, m2}, every element written. */
size_t gh_xf_group_moments_workspace_bytes(int B, int C, int N, int G);
int gh_xf_group_moments(const float* x, int64_t stride_b, int64_t stride_c, int B, int C, int N, int G, float* moments,
                        void* workspace, size_t ws_bytes, void* hip_stream);

/* qkv: (B N, 3 heads D) with row stride qkv_stride; out: (B N, heads D) with row stride out_stride, every element written. */
int gh_xf_attention(const float* qkv, int64_t qkv_stride, int B, int N, int heads, int D, float* out, int64_t out_stride,
                    void* hip_stream);

/* x, out: (B, C, N) contiguous; out may not alias x. layers: dims->layers structs in host memory, read during the call. */
size_t gh_xf_workspace_bytes(const GhXfDims* dims);
int gh_xf_forward(const GhXfDims* dims, const GhXfStem* stem, const GhXfLayer* layers, const float* x, float* out,
                  void* workspace, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_XF_H */
