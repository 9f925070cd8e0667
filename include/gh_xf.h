/*
 * gh_xf.h — C-ABI of the Transformer1D backbones' forward for frozen inference: what the reference's two backbones
 * (tgs/models/transformers.py:673-908, called at infer_one_shot.py:256-264) ask of a GroupNorm, about 85 library launches of
 * dense float32 GEMMs, LayerNorms, SDPA and a GEGLU per forward. The forward serves frozen inference; a second, opt-in path keeps
 * a tape and backpropagates to the input x alone, every weight frozen (the one-shot fit's identity code reaches the loss through
 * the texture backbone). A third path, opt-in as well, reads the same tape and also returns the gradient of every parameter that
 * wants one (gh_xf_backward_params): fine-tuning a few layers, or training the prior.
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
 *                          prologues   NONE; CF (the GN read without the norm); LN (LayerNorm over the row's K columns); GN (GroupNorm from the per-(batch, group)
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
 *                        matrix is written and there is no lse output (gh_xf_attention_lse has one).
 *   gh_xf_forward        the whole stack, enqueued from C++ in one host call: 4 + 11 launches per layer (7 where attn2 is
 *                        absent).
 *   gh_xf_backward_params  gh_xf_backward plus the gradients of the parameters that want one ("The parameters' gradients" below);
 *                        gh_xf_linear_wgrad, gh_xf_layernorm_param_grads and gh_xf_group_norm_param_grads are its single launches.
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
 * The backward to x (frozen weights). gh_xf_forward_tape is gh_xf_forward — the same kernels in the same order, `out` bitwise
 * the same — with the arrays the backward reads written into a caller's tape instead of the workspace, and the attention in
 * its gh_xf_attention_lse form. gh_xf_backward runs the chain in reverse from one host call: 5 + 13 launches per layer (8 where
 * attn2 is absent). Sizes are the forward's with M <= 512, because the product dn = [da | dg] W1 has inner width 8M <=
 * GH_XF_MAX_K; anything larger is GH_ERR_UNSUPPORTED before any launch.
 *   tape       parts in this order, each starting on 256 bytes (sizes in floats; T = B N, M = heads D):
 *                the GroupNorm's moments (B, G, 2);
 *                per layer three slots, laid out whether or not the layer has an attn2 (an absent one stays unwritten):
 *                  attn1, attn2:  h (T, M) the stream at the sub-block's input | LN moments (T, 2) {mean, rstd} | qkv (T, 3M) |
 *                                 the attention's output (T, M) | lse (B, heads, N)
 *                  feed-forward:  h (T, M) | LN moments (T, 2)
 *              about 11 M T floats a layer. The (T, 8M) pre-activation of the GEGLU is not kept: the backward forms it again.
 *   data       dX = dY W is gh_xf_linear over a transposed copy of W (Y = X (W^T)^T, EPI_PLAIN): each dX element is one ascending
 *              fmaf chain over the output-channel index from zero. GhXfStemT and GhXfLayerT hold those copies. PRO_CF reads X
 *              channel first as PRO_GN does, without a norm (dh = dout_rows W_out reads dout (B, C, N) in place).
 *   attention  p = expf(s - lse) with s = (q.k) * scale formed exactly as the forward forms it, lse = mm + logf(l) of the forward's
 *              pair join; delta = dot(dout, out) per (row, head), one ascending fmaf chain over d from 0; ds = (p * (dot(dout, v)
 *              - delta)) * scale, dot(dout, v) one ascending fmaf chain over d from 0. The key-block kernel: a workgroup owns
 *              GH_XF_ATTN_BWD_ROWS = 128 keys of one (batch, head), a wave 32, and sweeps the query tiles in ascending order, 64
 *              queries per LDS stage as two tiles of 32; dv = sum p dout and dk = sum ds q are each one fmaf chain from 0 over
 *              the queries, inside a tile of 32 in the order 0 4 1 5 2 6 3 7 8 12 ... A query past N contributes exactly 0 (p
 *              and ds are masked, lse is not consulted). The query-block kernel: a workgroup owns 128 queries, a wave 32, and
 *              sweeps the key tiles in ascending order the same way; dq = sum ds k. A key past N contributes exactly 0 to dq,
 *              and its dk and dv rows are not written. Both kinds of workgroup are enqueued by one launch (the key blocks first);
 *              neither reads what the other writes.
 *   GEGLU      one kernel, two X slabs (the cotangent gh and LN3(h)) and three accumulators for the same 64 x 64 tile of the 4M
 *              inner columns: du = gh W2 (from zero, over W2^T), a and g exactly as the forward's GEGLU epilogue forms them
 *              (from b1). da = du * gelu(g), dg = (du * a) * gelu'(g), gelu'(g) = 0.5 (1 + erff(g * 0.70710678f)) + (g *
 *              0.39894228f) * expf((-0.5 g) * g). Neither du nor [a | g] is written.
 *   LayerNorm  one wave per row, w = dn * gamma, xh = (x - mean) * rstd; s1 = sum w and s2 = sum fmaf(w, xh, .) in the forward's
 *              lane order and butterfly, each divided by K; g += rstd * ((w - s1) - xh * s2), in place.
 *   GroupNorm  the same two sums per (batch, group): stage one per chunk of GH_XF_GN_CHUNK positions as gh_xf_group_moments
 *              (thread = position, channels ascending, the butterfly, (s0 + s1) + (s2 + s3)), stage two adds the chunks in
 *              ascending order; rstd = 1 / sqrtf(m2 / (cpg N) + eps) as the prologue forms it. Then one element-wise channel-first
 *              pass: dx = dout + rstd * ((w - s1 / (cpg N)) - xh * (s2 / (cpg N))); the + dout is the residual + x of the output.
 *
 * The parameters' gradients. gh_xf_backward_params is gh_xf_backward — the same launches in the same order on the same buffers, dx
 * bitwise the same — with the parameter-gradient launches enqueued beside each step. Two activations are not on the tape and are formed
 * again with the forward's own launches: a * gelu(g) (T, 4M) by gh_xf_linear LN + GEGLU over the feed-forward slot's h, and for the last
 * layer the final stream by one BIAS_RES launch on top of it (with no layer: the proj_in launch). A NULL gradient pointer is "not
 * wanted": its launches are skipped and nothing is written; a gradient's bits do not depend on which others are asked for. Layers below
 * the lowest one that wants anything are not visited when neither dx nor a stem gradient below them is wanted.
 *   product    gh_xf_linear_wgrad: dW[j][k] = sum over t of dY[t][j] * P(X)[t][k], db[j] = sum over t of dY[t][j]. P is a forward
 *              prologue re-applied from stored moments (LN: rows {mean, rstd}; GN: (B, G, 2) {mean, m2}, rstd = 1 / sqrtf(m2 / (cpg N) +
 *              eps)) exactly as the forward's product forms it; dY is rows or channel first. A workgroup of 4 waves owns 64 (j) x 64
 *              (k) outputs of one chunk of rows, a wave 32 x 32; dY and P(X) cross LDS in slabs of 32 rows; the products are
 *              v_mfma_f32_32x32x2_f32. The rows are split into chunks of R = gh_xf_linear_wgrad_chunk(T, K, N_out): R =
 *              GH_XF_WGRAD_CHUNK, doubled while R < T and (number of 64 x 64 output tiles) * ceil(T / R) > GH_XF_WGRAD_MAX_BLOCKS — a
 *              function of T, K and N_out alone, the same whether dW, db or both are asked for. Within chunk c each dW element is one
 *              ascending fmaf chain over t = c R .. min(T, (c + 1) R) - 1 from zero, each db element one ascending chain of
 *              additions over the same t from zero (formed by the workgroups of the first k tile). Rows past T enter as zeros on both
 *              sides and are never read. With one chunk the results go straight to dW and db; otherwise the partials land in the
 *              workspace, (chunks, N_out, K) and (chunks, N_out), and a second launch joins them per element in ascending chunk order,
 *              ((p0 + p1) + p2) + ...
 *   LayerNorm  gh_xf_layernorm_param_grads: dgamma[k] = sum dn[t][k] * xh[t][k], dbeta[k] = sum dn[t][k], xh = (x - mean) * rstd from
 *              the taped row moments. Stage one: a workgroup per (chunk of GH_XF_LNP_ROWS rows, 64 columns), lane = column; wave w
 *              takes the chunk's rows w, w + 4, ... in ascending order, dgamma by fmaf(dn, xh, .) from zero, dbeta by addition from
 *              zero; the four waves are added as (s0 + s1) + (s2 + s3). Stage two: one thread per column adds the chunks in ascending
 *              order from chunk 0's partial.
 *   GroupNorm  gh_xf_group_norm_param_grads: the same two sums per channel over (b, n), xh = (x - mean) * rstd with rstd = 1 / sqrtf(m2 /
 *              (cpg N) + eps) as the prologue forms it. Stage one: a workgroup per (batch, channel, chunk of GH_XF_GN_CHUNK positions),
 *              thread = position with the one term dy * xh (and dy), the wave butterfly, (s0 + s1) + (s2 + s3). Stage two: one thread
 *              per channel adds the partials in ascending (batch, chunk) order from the first.
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
#define GH_XF_ATTN_BWD_ROWS 128 /* queries (dq) or keys (dk, dv) per workgroup of the attention's backward: 32 per wave */
#define GH_XF_ATTN_BWD_STAGE 64 /* rows of the swept operand per LDS stage of the attention's backward */
#define GH_XF_GRAD_MAX_M 512    /* the backward to x: 8 M <= GH_XF_MAX_K */
#define GH_XF_WGRAD_ROWS 32     /* rows of dY and X per LDS slab of the backward-weight product */
#define GH_XF_WGRAD_CHUNK 256   /* the smallest chunk of rows the backward-weight product splits T into */
#define GH_XF_WGRAD_MAX_BLOCKS 1024 /* the chunk doubles while tiles * chunks exceeds this */
#define GH_XF_LNP_ROWS 64       /* rows per stage-one workgroup of the LayerNorm's parameter gradients */

#define GH_XF_PRO_NONE 0
#define GH_XF_PRO_LN 1
#define GH_XF_PRO_GN 2
#define GH_XF_PRO_CF 3     /* X channel first as under PRO_GN, no norm: x_stride, x_stride_b and rows_per_batch as there */

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

/* ---- the backward to x, every weight frozen ---- */

/* What the backward reads of the frozen weights: transposed copies for the backward-data products, the norms' scales, and the
 * feed-forward's first layer as the forward reads it (the GEGLU's pre-activation is formed again). */
typedef struct GhXfStemT {
  const float* gn_w;          /* C */
  const float* in_t;          /* (C, M): proj_in's weight transposed */
  const float* out_t;         /* (M, C): proj_out's weight transposed */
} GhXfStemT;

typedef struct GhXfLayerT {
  const float* ln1_w;         /* M */
  const float* qkv1_t;        /* (M, 3M): [Wq; Wk; Wv] of attn1 transposed */
  const float* o1_t;          /* (M, M): to_out[0]'s weight transposed */
  const float* ln2_w;
  const float* qkv2_t;        /* NULL where the block has no attn2: ln2_w and o2_t are then ignored */
  const float* o2_t;
  const float *ln3_w, *ln3_b; /* M */
  const float *ff1_w, *ff1_b; /* (8M, M), 8M: as GhXfLayer's */
  const float* ff1_t;         /* (M, 8M): ff1_w transposed */
  const float* ff2_t;         /* (4M, M): ff2_w transposed */
} GhXfLayerT;

/* gh_xf_attention that also writes lse (B, heads, N) = mm + logf(l) of the pair join; out is bitwise gh_xf_attention's. */
int gh_xf_attention_lse(const float* qkv, int64_t qkv_stride, int B, int N, int heads, int D, float* out, int64_t out_stride,
                        float* lse, void* hip_stream);

/* dqkv (B N, 3 heads D) with row stride dqkv_stride: [dq | dk | dv] in the columns of qkv, every element written. out and dout are
 * (B N, heads D) rows, lse (B, heads, N) contiguous. The workspace holds delta, one float per (batch, head, row). */
size_t gh_xf_attention_backward_workspace_bytes(int B, int N, int heads);
int gh_xf_attention_backward(const float* qkv, int64_t qkv_stride, const float* out, int64_t out_stride, const float* lse,
                             const float* dout, int64_t dout_stride, int B, int N, int heads, int D, float* dqkv,
                             int64_t dqkv_stride, void* workspace, size_t ws_bytes, void* hip_stream);

/* y (T, 8M) = [da | dg] of the feed-forward: g (T, M) the cotangent of its output, h (T, M) its input with the LayerNorm's row
 * moments (T, 2) {mean, rstd}, gamma and beta (M), w1 (8M, M), b1 (8M), w2t (4M, M) = W2 transposed. M a multiple of 32. */
int gh_xf_geglu_backward(const float* g, int64_t g_stride, const float* h, int64_t h_stride, const float* moments,
                         const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2t, int T, int M,
                         float* y, int64_t y_stride, void* hip_stream);

/* g (T, K) += the LayerNorm's backward of dn (T, K) at x (T, K) with moments (T, 2) {mean, rstd}; any K >= 1. */
int gh_xf_layernorm_backward(const float* dn, int64_t dn_stride, const float* x, int64_t x_stride, const float* moments,
                             const float* gamma, int T, int K, float* g, int64_t g_stride, void* hip_stream);

/* dx = dout + the GroupNorm's backward of dy at x; dy, x, dout, dx (B, C, N) contiguous, moments (B, G, 2) {mean, m2} of
 * gh_xf_group_moments. dx may not alias dy, x or dout. */
size_t gh_xf_group_norm_backward_workspace_bytes(int B, int C, int N, int G);
int gh_xf_group_norm_backward(const float* dy, const float* x, const float* moments, const float* gamma, const float* dout,
                              float* dx, int B, int C, int N, int G, float eps, void* workspace, size_t ws_bytes,
                              void* hip_stream);

/* gh_xf_forward that keeps the tape (layout above); workspace as gh_xf_workspace_bytes. 0 bytes for unsupported or empty sizes. */
size_t gh_xf_tape_bytes(const GhXfDims* dims);
int gh_xf_forward_tape(const GhXfDims* dims, const GhXfStem* stem, const GhXfLayer* layers, const float* x, float* out,
                       void* tape, size_t tape_bytes, void* workspace, size_t ws_bytes, void* hip_stream);

/* dx (B, C, N) = the gradient of sum(out * dout) with respect to x, from the tape gh_xf_forward_tape wrote for the same dims, x
 * and weights. x, dout, dx contiguous; dx may not alias x or dout. layers: dims->layers structs in host memory. */
size_t gh_xf_backward_workspace_bytes(const GhXfDims* dims);
int gh_xf_backward(const GhXfDims* dims, const GhXfStemT* stem, const GhXfLayerT* layers, const float* x, const void* tape,
                   const float* dout, float* dx, void* workspace, size_t ws_bytes, void* hip_stream);

/* ---- the parameters' gradients ---- */

typedef struct GhXfWgrad {
  int32_t T, K, N_out;      /* rows summed over, width of X (a multiple of 32), width of dY */
  int32_t prologue;         /* of X: GH_XF_PRO_* */
  int32_t dy_cf;            /* 0: dY is (T, N_out) rows. 1: channel first, element (t, j) at dy[b * dy_stride_b + j * dy_stride + n] */
  int32_t rows_per_batch;   /* N: PRO_GN, PRO_CF and dy_cf (T a multiple of it); ignored otherwise */
  int32_t groups;           /* PRO_GN: K a multiple of it */
  float eps;                /* PRO_GN */
  const float* x;           /* as GhXfLinear's x; may be NULL where dw is */
  int64_t x_stride, x_stride_b;
  const float* dy;
  int64_t dy_stride, dy_stride_b;
  const float* gamma;       /* K: PRO_LN, PRO_GN */
  const float* beta;
  const float* moments;     /* PRO_LN: (T, 2) {mean, rstd}. PRO_GN: (T / rows_per_batch, groups, 2) {mean, m2} */
  float* dw;                /* (N_out, K) contiguous, every element written; NULL: not wanted */
  float* db;                /* N_out, every element written; NULL: not wanted */
} GhXfWgrad;

/* The gradients' buffers: GhXfStem's and GhXfLayer's fields, each NULL (not wanted, never written) or a contiguous buffer of the
 * parameter's shape; qkv1 and qkv2 are the stacked (3M, M) gradients of [Wq; Wk; Wv]. */
typedef struct GhXfStemG {
  float *gn_w, *gn_b;
  float *in_w, *in_b;
  float *out_w, *out_b;
} GhXfStemG;

typedef struct GhXfLayerG {
  float *ln1_w, *ln1_b;
  float* qkv1;
  float *o1_w, *o1_b;
  float *ln2_w, *ln2_b;
  float* qkv2;
  float *o2_w, *o2_b;
  float *ln3_w, *ln3_b;
  float *ff1_w, *ff1_b;
  float *ff2_w, *ff2_b;
} GhXfLayerG;

/* Rows per chunk of the backward-weight product (0 for invalid sizes), and the bytes of its partials (0 with one chunk). */
int gh_xf_linear_wgrad_chunk(int T, int K, int N_out);
size_t gh_xf_linear_wgrad_workspace_bytes(int T, int K, int N_out);
int gh_xf_linear_wgrad(const GhXfWgrad* args, void* workspace, size_t ws_bytes, void* hip_stream);

/* dgamma, dbeta (K) of a LayerNorm whose output's cotangent is dn (T, K), at x (T, K) with moments (T, 2) {mean, rstd}; either may be
 * NULL; any K >= 1. */
size_t gh_xf_layernorm_param_grads_workspace_bytes(int T, int K);
int gh_xf_layernorm_param_grads(const float* dn, int64_t dn_stride, const float* x, int64_t x_stride, const float* moments, int T, int K,
                                float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* hip_stream);

/* dgamma, dbeta (C) of the GroupNorm whose output's cotangent is dy; dy, x (B, C, N) contiguous, moments (B, G, 2) {mean, m2}. */
size_t gh_xf_group_norm_param_grads_workspace_bytes(int B, int C, int N, int G);
int gh_xf_group_norm_param_grads(const float* dy, const float* x, const float* moments, int B, int C, int N, int G, float eps,
                                 float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* hip_stream);

/* gh_xf_backward plus the gradient of every parameter gstem / glayers name. fstem / flayers: the weights as gh_xf_forward_tape read
 * them. dx may be NULL. Sizes are gh_xf_backward's. */
size_t gh_xf_backward_params_workspace_bytes(const GhXfDims* dims);
int gh_xf_backward_params(const GhXfDims* dims, const GhXfStemT* stem, const GhXfLayerT* layers, const GhXfStem* fstem,
                          const GhXfLayer* flayers, const GhXfStemG* gstem, const GhXfLayerG* glayers, const float* x, const void* tape,
                          const float* dout, float* dx, void* workspace, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_XF_H */
