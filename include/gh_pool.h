/*
 * gh_pool.h — C-ABI of the per-cell pooling of point features: what the reference's LocalPoolPointnet
 * (tgs/models/pointclouds/pointnet_texture.py) does through torch_scatter's scatter_max / scatter_mean.
 *
 * Every point p of a cloud carries a cell index in [0, n_cells) (its UV cell, fixed for a whole encoder forward) and
 * a row of C float32 features. Three operations share one grouping of the points by cell (the "plan"):
 *
 *   plan          index[T] -> cell_start[n_cells + 1], order[T]: a counting sort. order[cell_start[c] .. cell_start[c+1])
 *                 are the points of cell c in ascending point index. A point whose index is outside [0, n_cells) belongs to
 *                 no cell: such points follow the last cell, order[cell_start[n_cells] .. T), and *flag is set to 1 (else
 *                 0). The reference asserts on that condition with a host synchronisation; here the host reads the flag when
 *                 it wants to. Every operation below skips those points: they contribute to nothing and receive zeros.
 *   pool          out[p, :] = the per-channel reduction of x over the points of p's cell (pool_local's scatter + gather,
 *                 pointnet_texture.py:68-81), for GH_POOL_MAX or GH_POOL_MEAN (sum / count).
 *   plane mean    plane[ch, c] = sum over the points of cell c of x[p, ch] / max(count, 1), 0 for an empty cell
 *                 (generate_plane_features, :55-66), channel-first as the reference returns it.
 *
 * Ties of the maximum go to the LOWEST point index: argmax[c, ch] is the first point of cell c that attains the maximum
 * of channel ch, and the backward sends the cell's whole gradient there. torch_scatter's GPU scatter_max leaves the
 * choice between tied points to a race between atomics. An empty cell has argmax T.
 *
 * NaN and infinities. A NaN never wins a maximum, wherever it sits in its cell (torch_scatter's rule: it compares val > current
 * from the lowest value). A cell whose rows are all NaN in a channel behaves like an empty cell for that channel: value 0,
 * argmax T, gradient nowhere. -inf and +inf are ordinary values: a cell that is all -inf in a channel returns -inf with its
 * first point as argmax. The means (GH_POOL_MEAN, plane mean) propagate NaN and infinities as float arithmetic does, within
 * the cell that holds them. A NaN or infinity in a point without a cell is read by nothing.
 *
 * Sums run over a cell's points in ascending point index, the list cut into at most 4 contiguous parts that are added
 * in part order: no atomics anywhere, so values and gradients are bitwise reproducible run to run.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host
 * synchronisation, no allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad
 * arguments or a short workspace. Row strides and column offsets are in float elements. All pointers 4-byte aligned.
 */
#ifndef GH_POOL_H
#define GH_POOL_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_POOL_MAX 0
#define GH_POOL_MEAN 1
#define GH_POOL_MAX_CELLS 8192 /* the plan's histogram lives in LDS */

/* Bytes of workspace gh_pool_plan needs (0 for invalid sizes). Pure host arithmetic. */
size_t gh_pool_plan_workspace(int T, int n_cells);

/*
 * index: T entries, int32 (index_is_int64 == 0) or int64 (!= 0). cell_start: int32[n_cells + 1]; order: int32[T];
 * flag: uint32[1]. workspace: >= gh_pool_plan_workspace(T, n_cells) bytes. Three launches.
 * 1 <= n_cells <= GH_POOL_MAX_CELLS (GH_ERR_UNSUPPORTED above), T >= 1.
 */
int gh_pool_plan(const void* index, int index_is_int64, int T, int n_cells, int32_t* cell_start, int32_t* order,
                 uint32_t* flag, void* workspace, size_t ws_bytes, void* hip_stream);

/*
 * x: (T, C) with row stride x_stride >= C. out: element (p, ch) at out[p * out_stride + out_col + ch], every row written.
 * out may be the right half of the (T, 2C) buffer whose left half is x (the reference's torch.cat([net, pooled], dim=2),
 * :107): x and out may share memory only with equal row strides and disjoint column windows, any other overlap is
 * GH_ERR_INVALID_ARG. argmax: int32[n_cells * C], written for GH_POOL_MAX (required), ignored for GH_POOL_MEAN.
 */
int gh_pool_forward(const float* x, int x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                    const int32_t* order, int reduce, float* out, int out_stride, int out_col, int32_t* argmax,
                    void* hip_stream);

/*
 * grad_out: element (p, ch) at grad_out[p * g_stride + g_col + ch]. grad_x: (T, C) with row stride gx_stride.
 *   GH_POOL_MAX:  grad_x[argmax[c, ch], ch] = sum over p in cell c of grad_out[p, ch], 0 elsewhere
 *   GH_POOL_MEAN: grad_x[p, ch] = (sum over q in cell(p) of grad_out[q, ch]) / count
 * accumulate == 0: every element of grad_x is written. accumulate != 0: the values are added into grad_x (the gradient
 * of the left half of the cat buffer is already there). The same overlap rule as the forward holds for grad_out, grad_x.
 */
int gh_pool_backward(const float* grad_out, int g_stride, int g_col, int T, int C, int n_cells,
                     const int32_t* cell_start, const int32_t* order, int reduce, const int32_t* argmax, float* grad_x,
                     int gx_stride, int accumulate, void* hip_stream);

/* x: (T, C), row stride x_stride. plane: (C, n_cells) contiguous, every element written. No overlap allowed. */
int gh_plane_mean_forward(const float* x, int x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                          const int32_t* order, float* plane, void* hip_stream);

/* grad_x[p, ch] = grad_plane[ch, cell(p)] / count; every element of grad_x (T, C; row stride gx_stride) is written. */
int gh_plane_mean_backward(const float* grad_plane, int T, int C, int n_cells, const int32_t* cell_start,
                           const int32_t* order, float* grad_x, int gx_stride, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_POOL_H */
