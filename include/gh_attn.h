/*
 * gh_attn.h — C-ABI of the interaction attention's core: softmax((q k^T) / norm) v per (batch, head), forward and backward,
 * without the V x V score matrix. What the reference's SelfAttn.self_attn (tgs/models/self_attn.py:70-74) asks of two
 * torch.matmul calls and an F.softmax for the points `mink_idxs_inter` flags (renderer_one_shot.py:554-574): 4 heads of
 * D = 32, float32. The projections, the LayerNorm and the feed-forward block around it stay the module's own.
 *
 * Tensors. q, k, v and the cotangent of the output are given as GhAttnTensor: a pointer and the strides, in elements, of
 * the batch, row and head dimensions of a logical (BS, V, H, D) array whose last dimension has unit stride. So
 * `w_qs(x).view(BS, V, H, D)` is read in place, and so is a (BS, V, 3 * H * D) block of one concatenated projection. out, dq,
 * dk and dv are (BS, V, H * D) contiguous (the form `:74` produces); lse is (BS, H, V): ln sum_j exp(score[i, j]) of row i.
 *
 * Supported shapes. D == GH_ATTN_D (32) only; BS * H <= GH_ATTN_MAX_BH (one grid row per (batch, head)); V <= GH_ATTN_MAX_V
 * (row and key counters are int32 and leave room for a tile; every address is formed in 64 bits). Anything else is
 * GH_ERR_UNSUPPORTED before any launch. V = 0 or BS = 0 launches nothing and returns GH_OK.
 *
 * Arithmetic (float32 throughout, no reduced precision, -ffp-contract=off: FMAs only where stated).
 *   tile       a wave owns 32 rows, a workgroup of 4 waves 128; the other operand crosses LDS 64 rows at a time and is
 *              folded 32 rows (one tile) at a time. Products are v_mfma_f32_32x32x2_f32: exact float32, each dot product one
 *              fmaf chain.
 *   dot        a dot product over d = 0 .. 31 (q.k, dout.v, dout.out) is one ascending fmaf chain starting from 0.
 *   score      s = (q.k) / norm, a division by the float32 `norm`, as `:70` divides. A key past V in a partial tile scores
 *              -inf and contributes exactly 0.
 *   forward    key tiles are folded in ascending order with a running maximum m and sum l per row: m' = max(m, max of the
 *              tile), p = expf(s - m'), l = l * expf(m - m') + (sum of p), acc = acc * expf(m - m') then acc = fmaf(p, v,
 *              acc) key by key; out = acc / l, lse = m + logf(l). Inside a tile the 32 keys enter the sum of p as two
 *              ascending chains of 16 (keys with bit 2 clear, keys with bit 2 set) added at the end, and enter acc in the
 *              order 0 4 1 5 2 6 3 7 8 12 9 13 ... (the order in which the first product's accumulator feeds the second).
 *   backward   p = expf(s - lse), delta = dot(dout, out), ds = (p * (dot(dout, v) - delta)) / norm.
 *              dv[j] = sum_i p[i, j] dout[i], dk[j] = sum_i ds[i, j] q[i]: one workgroup per 128 keys sweeps the query tiles
 *              in ascending order and owns its dk and dv. dq[i] = sum_j ds[i, j] k[j]: one workgroup per 128 queries sweeps
 *              the key tiles in ascending order and owns its dq. Each sum is one fmaf chain from 0; inside a tile of 32 its
 *              terms come in the order 0 4 1 5 2 6 3 7 8 12 ... as above. delta is written once per (batch, head, row) by a
 *              row kernel ahead of the two. No atomics of any kind, no workgroup waits for another: seven tile products
 *              instead of five, and every result is bitwise reproducible.
 *   A row's out and lse are a function of that row's q, of K and of V alone: not of the row's place in the launch, of BS, of
 *   the head index or of the strides. The same holds for dq, and for a key's dk and dv.
 *
 * Conventions are those of gh_pool.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation,
 * no allocation, nothing thrown, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or
 * a short workspace. All pointers 4-byte aligned, the workspace 16-byte aligned. An input whose pointer is 16-byte aligned
 * and whose strides are multiples of 4 is staged with 16-byte loads; the values do not depend on it.
 */
#ifndef GH_ATTN_H
#define GH_ATTN_H

#include "gh_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_ATTN_D 32
#define GH_ATTN_MAX_BH 65535
#define GH_ATTN_MAX_V (1 << 30)

typedef struct GhAttnDims {
  int32_t BS, V, H, D;
  float norm; /* the divisor of the scores: float32(sqrt(D)) in the reference; finite and > 0 */
} GhAttnDims;

typedef struct GhAttnTensor {
  const float* p;
  int64_t stride_b, stride_v, stride_h; /* elements; the last dimension has unit stride */
} GhAttnTensor;

/* Bytes of workspace gh_attn_backward needs (delta, one float per (batch, head, row)); 0 for unsupported or empty sizes. */
size_t gh_attn_workspace_bytes(const GhAttnDims* dims);

/* out: (BS, V, H * D), lse: (BS, H, V); every element of both is written. Three inputs may alias each other, not an output. */
int gh_attn_forward(const GhAttnDims* dims, const GhAttnTensor* q, const GhAttnTensor* k, const GhAttnTensor* v, float* out,
                    float* lse, void* hip_stream);

/*
 * out, lse: what gh_attn_forward wrote for the same q, k, v. dout: the cotangent of out through its strides. dq, dk, dv:
 * (BS, V, H * D) contiguous, every element written, nothing to zero. dq == NULL skips the query-block kernel; dk == NULL and
 * dv == NULL skip the key-block kernel (one of the two alone is allowed and then the only one written).
 * workspace: >= gh_attn_workspace_bytes(dims) bytes.
 */
int gh_attn_backward(const GhAttnDims* dims, const GhAttnTensor* q, const GhAttnTensor* k, const GhAttnTensor* v, const float* out,
                     const float* lse, const GhAttnTensor* dout, float* dq, float* dk, float* dv, void* workspace, size_t ws_bytes,
                     void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_ATTN_H */
