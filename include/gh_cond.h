/*
 * gh_cond.h — C-ABI of the point conditioning: the rows the reference's TGS._forward concatenates per point (infer_one_shot.py:244,
 * :251, :273) and the LayerNorm + MLP that reads the widest of them (additional_features_fc, tgs/models/verts_refinement.py:119-131),
 * without the columns that are the same in every row of a batch element.
 *
 * The varying row. Per point, from optional segments in this fixed order (an absent segment is a NULL pointer and is skipped), with
 * L = levels in [1, GH_COND_MAX_LEVELS] and f_l = float32(pi) * 2^l — the float32 value of pi * 2^l, as SpatialEncoder.pe_vector
 * builds it (spatial.py:42-48):
 *
 *     uv   (P,2)   u, v, u, v, then for l = 0..L-1: sin(f_l u), sin(f_l v), cos(f_l u), cos(f_l v)            4 + 4L columns
 *     xyz  (P,3)   x, y, z, x, y, z, then for l = 0..L-1: sin(f_l x), .., sin(f_l z), cos(f_l x), .., cos(f_l z)  6 + 6L columns
 *     flag (P,)    one column
 *     code (P,Cc)  0 <= Cc <= GH_COND_MAX_CODE columns, read in place through code_stride (float elements)
 *
 * Dv is the sum of those widths (gh_cond_width). The product f_l * x is rounded to float32 before sinf / cosf (the library is built
 * with -ffp-contract=off), and sinf / cosf are the accurate ones. gh_cond_rows writes the (P,Dv) rows; the MLP entry points build the
 * same rows in LDS with the same routine and never write them.
 *
 * The LayerNorm + MLP. A full row is (v, e): the Dv varying columns and De >= 0 columns e[b, :] shared by the N rows of batch
 * element b = row / N. With D = Dv + De, parameters gamma, beta (D), W1 (Hd,D), b1, W2 (Hd,Hd), b2, Hd <= GH_COND_MAX_HD, suffix v
 * the first Dv and suffix e the last De columns:
 *
 *   gh_cond_fold, one workgroup per batch element, float64 accumulation, float32 stores, into `fold`:
 *     once      c0 = W1 . beta + b1 (Hd)           W1g = W1_v * gamma_v, column-wise (Hd,Dv)
 *     per b     m_e = mean(e)    M_e = sum (e - m_e)^2    c1 = W1_e . gamma_e (Hd)    c2 = W1_e . (gamma_e * (e - m_e)) (Hd)
 *     (m_e is rounded to float32 first and that value is what M_e and c2 are centred on.) De = 0: every per-b constant is 0.
 *     Layout in floats: c0 at 0, W1g at Hd, batch element b at Hd + Hd*Dv + b*(2 + 2*Hd) as m_e, M_e, c1[Hd], c2[Hd].
 *
 *   forward, per row:
 *     m_v = mean(v), M_v = sum (v - m_v)^2          two passes over the row, m_v corrected by the mean of the second pass's deviations
 *     delta = m_e - m_v      mu = fmaf(delta, De/D, m_v)      M = (M_v + M_e) + (delta * delta) * (Dv*De/D)     (the pairwise form)
 *     rstd = 1 / sqrt(M / D + eps)                  correctly rounded division and square root
 *     pre1 = fmaf(rstd, (W1g . (v - mu) + c2) + (m_e - mu) * c1, c0)         h1 = relu(pre1), a NaN passes
 *     out  = W2 . h1 + b2
 *
 *   backward with respect to code (the only differentiable input), recomputing the forward from the inputs and `fold`:
 *     d1 = (W2^T . g) where pre1 > 0, else 0        a = W1g^T . d1 (Dv)        xhat = rstd * (v - mu)
 *     s1 = sum a + d1 . c1                          s2 = sum a * xhat + rstd * (d1 . (c2 + (m_e - mu) * c1))
 *     dcode_j = rstd * fmaf(-xhat_j, s2 / D, a_j - s1 / D)                    over the code columns
 *
 * Summation. One 4-wave workgroup works on GH_COND_ROWS rows, lane = row; a tile may hold rows of several batch elements (the per-b
 * constants are per-lane loads, every weight is wave-uniform). m_v and M_v: four interleaved partial sums (k mod 4), ascending k,
 * added as (s0 + s1) + (s2 + s3). A forward dot product: four partial sums (k mod 4) with one fmaf per term, (s0 + s1) + (s2 + s3),
 * then the terms in the order written above. W2^T . g and W1g^T . d1: one chain of fmaf over the layer's outputs in ascending order.
 * s1 and s2: wave w sums a over the columns 16t + 4w .. + 3 in ascending order, adds its share of the d1 dot products (j = w mod 4,
 * ascending; for s2 multiplied by rstd), and the four shares are added as (s0 + s1) + (s2 + s3). All of these orders depend on the
 * layout (segments, L, Cc, Hd) alone: a row's output and dcode are bitwise the same alone or among 100,000 rows, at any code stride.
 * No atomics; the backward is one launch.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. uv, xyz, flag, out of the
 * MLP, g_out and fold are contiguous; code, dcode and the rows of gh_cond_rows have row strides in float elements. 4-byte alignment
 * suffices everywhere. P = 0 returns GH_OK without a launch.
 */
#ifndef GH_COND_H
#define GH_COND_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_COND_ROWS 64       /* rows per workgroup */
#define GH_COND_MAX_LEVELS 8  /* L */
#define GH_COND_MAX_CODE 64   /* Cc */
#define GH_COND_MAX_HD 64     /* Hd */

typedef struct GhCondRows {
  const float *uv, *xyz, *flag, *code; /* (P,2), (P,3), (P,), (P,Cc); each may be NULL (code: with Cc = 0) */
  int64_t code_stride;                  /* >= Cc */
  int32_t Cc;
  int32_t levels;
} GhCondRows;

/* contiguous float32: ln_* (D), fc1_weight (Hd,D), fc1_bias (Hd), fc2_weight (Hd,Hd), fc2_bias (Hd) */
typedef struct GhCondParams {
  const float *ln_weight, *ln_bias, *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias;
} GhCondParams;

/* Dv of the layout, or GH_ERR_INVALID_ARG (levels or Cc out of range, code and Cc disagreeing, code_stride < Cc, no segment). */
int gh_cond_width(const GhCondRows* in);

/* Bytes of `fold` for B batch elements; 0 for B < 1, Dv < 1, Hd outside [1, GH_COND_MAX_HD]. Pure host arithmetic. */
size_t gh_cond_fold_bytes(int B, int Dv, int Hd);

/* out: (P,Dv) with row stride out_stride >= Dv, every element written. One launch. */
int gh_cond_rows(const GhCondRows* in, int P, float* out, int64_t out_stride, void* hip_stream);

/* e: (B,De), NULL allowed when De = 0. fold: gh_cond_fold_bytes(B, Dv, Hd) bytes, every element written. One launch of B workgroups. */
int gh_cond_fold(const float* e, int B, int De, int Dv, int Hd, const GhCondParams* params, float* fold, size_t fold_bytes,
                 void* hip_stream);

/* P = B * N rows, N >= 1 rows per batch element; fold as gh_cond_fold left it for (B, Dv = gh_cond_width(in), Hd). out: (P,Hd). Reads
 * fc2_weight and fc2_bias of params (the other four reach it through fold). One launch. */
int gh_cond_mlp_forward(const GhCondRows* in, int P, int N, int De, int Hd, const GhCondParams* params, const float* fold, float eps,
                        float* out, void* hip_stream);

/* g_out: the gradient of out, (P,Hd), or NULL, which means zero. dcode: (P,Cc) with row stride dcode_stride >= Cc, every element
 * written; Cc >= 1. One launch. */
int gh_cond_mlp_backward(const GhCondRows* in, int P, int N, int De, int Hd, const GhCondParams* params, const float* fold, float eps,
                         const float* g_out, float* dcode, int64_t dcode_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_COND_H */
