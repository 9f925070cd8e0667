/*
 * gh_res.h — C-ABI of the point encoders' ResNet blocks: ResnetBlockFC (tgs/models/networks.py:162-204) as LocalPoolPointnet applies it
 * to torch.cat([net, pooled], dim=2) (tgs/models/pointclouds/pointnet_texture.py:102-112), with the pooled half folded per cell.
 *
 * Every point of a cell carries the same pooled row, so with W0 = [W0a | W0b] and Ws = [Wsa | Wsb] split at column H the pooled
 * half's share of fc_0 and of the shortcut is one row per cell. The caller computes those rows (GEMMs over the cells) and hands them
 * in as two tables u, s of R rows; the row kernel does what is left per point.
 *
 * Row kernel, forward. x (T,Cin), tables u, s (R,H), r(p) = row_of[p] (NULL: row 0 for every point), W0, Ws (H,Cin), W1 (H,H):
 *
 *     h[p]   = u[r(p)] + W0 . relu(x[p])
 *     out[p] = s[r(p)] + Ws . x[p] + W1 . relu(h[p])
 *     mask[p, t] bit b = h[p, 32 t + b] > 0                                   (optional output, uint32[T, H/32])
 *
 * relu(v) is 0 for v < 0 and v otherwise (a NaN passes). Summation: every element is ONE chain of fmaf whose accumulator starts at the
 * table's element: h adds W0's terms in ascending k; out adds Ws's terms in ascending k and then W1's terms in the order
 * j = 32 t + 8 q + 4 e + i, the loops nested t (0 .. H/32-1), q (0 .. 3), i (0 .. 3), e (0, 1) from the outside in — the order in which
 * the matrix instruction's result registers hold h, so that h never leaves the registers. The products run on v_mfma_f32_32x32x2_f32,
 * which is such a chain bit for bit.
 *
 * Row kernel, backward, for frozen weights. The backward reads the forward's `mask` (h is not recomputed), g (T,H) and x:
 *
 *     dh[p] = mask[p] ? W1^T . g[p] : 0                    a chain from 0 over W1's rows in ascending order
 *     dx[p] = (x[p] > 0 ? W0^T . dh[p] : 0) + Ws^T . g[p]  a chain from 0 over W0's rows in the order j above; where x <= 0 (or NaN)
 *                                                          the chain restarts from 0; then Ws's rows in ascending order
 *
 * Every element of dx (T,Cin) is written; dh (T,H) is written when given (the tables' gradients are its per-cell sums:
 * du = cell_sum(dh), ds = cell_sum(g)). Gradients of the weights are not produced.
 *
 * A row's out, mask, dx and dh depend on that row's data, its table rows and the weights alone: they are bitwise the same whether
 * the row is alone, in a tail tile or among 100,000 rows, at any stride. One 4-wave workgroup works on GH_RES_ROWS rows, 32 per
 * wave with the point on the lane; the weights cross LDS in slabs of 32 columns (forward) or 32 rows (backward) shared by the waves.
 *
 * Cell kernels, over a plan of gh_pool.h (cell_start[n_cells + 1], order[T]):
 *   gh_res_cell_sum           y[c, ch] = sum of x[p, ch] over the points of cell c: the list cut into 4 contiguous parts (part w is
 *                             [n w / 4, n (w + 1) / 4) of the cell's n points), each summed in ascending point index from 0, the
 *                             parts added as ((s0 + s1) + s2) + s3 — gh_pool.h's rule. 0 for an empty cell. With tail != 0, y
 *                             has a row n_cells: the same sum over the points without a cell, order[cell_start[n_cells] .. T).
 *   gh_res_cell_max           vals[c, ch], argmax[c, ch]: the maximum over the cell's points and the lowest point index attaining it,
 *                             under gh_pool.h's rules to the letter (a NaN never wins; a cell of NaNs alone or an empty cell gives
 *                             value 0, argmax T; -inf is an ordinary value). No (T,C) array is written.
 *   gh_res_cell_max_backward  grad_x[argmax[c, ch], ch] += gm[c, ch] for every argmax in [0, T): one thread per (cell, channel); a
 *                             (row, channel) is hit by at most one cell, so plain loads and stores suffice.
 * No atomics anywhere: every result is bitwise reproducible run to run.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. T = 0 returns GH_OK without a
 * launch. Strides are in float elements; u, s, W1, mask, dh, y, vals, argmax and gm are contiguous. 4-byte alignment suffices
 * everywhere (16-byte aligned rows are moved four floats at a time). The caller keeps row_of within [0, R); the kernels clamp it.
 */
#ifndef GH_RES_H
#define GH_RES_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_RES_ROWS 128  /* rows per workgroup */
#define GH_RES_MAX_H 128 /* H is 32, 64, 96 or 128 */

/*
 * x: (T,Cin), row stride x_stride >= Cin. Cin is H or 2H. W0, Ws: (H,Cin) with row strides >= Cin. out: (T,H), row stride
 * out_stride >= H, every element written. mask: uint32[T * H/32] or NULL. R >= 1. One launch.
 */
int gh_res_forward(const float* x, int64_t x_stride, int T, int Cin, int H, const float* u, const float* s, int R,
                   const int32_t* row_of, const float* W0, int64_t w0_stride, const float* Ws, int64_t ws_stride, const float* W1,
                   float* out, int64_t out_stride, uint32_t* mask, void* hip_stream);

/*
 * g: (T,H), row stride g_stride >= H. mask: as the forward over the same x, tables and weights wrote it (required).
 * dx: (T,Cin), row stride dx_stride >= Cin. dh: (T,H) contiguous, or NULL. One launch.
 */
int gh_res_backward(const float* g, int64_t g_stride, const float* x, int64_t x_stride, int T, int Cin, int H, const uint32_t* mask,
                    const float* W0, int64_t w0_stride, const float* Ws, int64_t ws_stride, const float* W1, float* dx,
                    int64_t dx_stride, float* dh, void* hip_stream);

/* x: (T,C), row stride x_stride >= C. y: (n_cells + (tail != 0), C), every element written. 1 <= n_cells <= GH_POOL_MAX_CELLS. */
int gh_res_cell_sum(const float* x, int64_t x_stride, int T, int C, int n_cells, const int32_t* cell_start, const int32_t* order,
                    int tail, float* y, void* hip_stream);

/* vals: (n_cells,C) float32, argmax: (n_cells,C) int32, every element written. */
int gh_res_cell_max(const float* x, int64_t x_stride, int T, int C, int n_cells, const int32_t* cell_start, const int32_t* order,
                    float* vals, int32_t* argmax, void* hip_stream);

/* gm: (n_cells,C). grad_x: (T,C), row stride gx_stride >= C, added into. */
int gh_res_cell_max_backward(const float* gm, const int32_t* argmax, int T, int C, int n_cells, float* grad_x, int64_t gx_stride,
                             void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_RES_H */
