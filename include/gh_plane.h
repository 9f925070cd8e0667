/*
 * gh_plane.h — C-ABI of the plane fetch: bilinear sampling of a CHANNEL-FIRST feature plane at per-point UVs, and its
 * ordered backward. What the reference's query_triplane_texture (tgs/models/renderer_one_shot.py:420-446) asks of
 * F.grid_sample(mode="bilinear", align_corners=True, zeros padding) for the (B,1,80,64,128) texture code at all N points.
 *
 * All maps keep the reference's layout: (C, Hp, Wp) contiguous. uv is (N, 2) in [-1, 1] and finite (u addresses x / Wp,
 * v addresses y / Hp, as grid_sample's grid does). Every buffer is float32 or int32.
 *
 *   forward    out[n, :] = the four corner texels times their weights, added nw, ne, sw, se, corners outside the map skipped:
 *              the values of gh_uv_sample_forward (gh_raster.h) on the channel-last copy of the plane, bit for bit. The copy
 *              is made in the workspace by a tiled transpose and that entry point is then called on it: two launches.
 *   index      the incidence of points and texels, inverted on the device. Pair e = 4 * n + corner (corner 0..3 = nw, ne,
 *              sw, se) has the weight w[e] (wx0*wy0, wx1*wy0, wx0*wy1, wx1*wy1, the forward's own arithmetic) and the linear
 *              texel y * Wp + x, or none when the corner lies outside the map. gh_pool_plan (gh_pool.h) sorts the 4N pairs by
 *              texel: pairs[texel_start[t] .. texel_start[t + 1]) are the pairs of texel t in ascending e. Pairs without a
 *              texel follow the last one, pairs[texel_start[Hp * Wp] .. 4N), and are read by nothing. One launch plus the
 *              plan's three. Hp * Wp <= GH_POOL_MAX_CELLS.
 *   backward   grad_plane[c, t] = the chain acc = 0; acc = acc + grad_out[e >> 2, c] * w[e] over texel t's pairs in list
 *              order (a multiply, then an add; never fused). Every element of grad_plane is written, 0 for a texel without
 *              pairs. This is the sum gh_uv_scatter_sorted forms over host-built lists, so both give the same bits. No
 *              atomics of any kind: the gradient is bitwise reproducible run to run. One launch.
 *
 * Conventions are those of gh_pool.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation,
 * no allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or a short
 * workspace. All pointers 4-byte aligned, the workspace 16-byte aligned.
 */
#ifndef GH_PLANE_H
#define GH_PLANE_H

#include "gh_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of workspace that serve gh_plane_sample_forward and gh_plane_index for these sizes (0 for invalid sizes: N < 0,
 * C, Hp or Wp < 1, or counts beyond int32). Pure host arithmetic. Both calls lay their data out from the first byte, so one
 * buffer serves either call, and both only when they are ordered on one stream. N = 0, or Hp * Wp > GH_POOL_MAX_CELLS,
 * gives the forward's part alone.
 */
size_t gh_plane_workspace(int N, int C, int Hp, int Wp);

/* plane: (C, Hp, Wp); uv: (N, 2); out: (N, C), every element written. N = 0 launches nothing. Any plane size. */
int gh_plane_sample_forward(const float* plane, const float* uv, float* out, int N, int C, int Hp, int Wp, void* workspace,
                            size_t ws_bytes, void* hip_stream);

/*
 * uv: (N, 2). texel_start: int32[Hp * Wp + 1]; pairs: int32[4N]; w: float[4N]. workspace: >= gh_plane_workspace(N, 1, Hp, Wp)
 * bytes. N = 0 writes texel_start = 0 (one launch). Hp * Wp > GH_POOL_MAX_CELLS is GH_ERR_UNSUPPORTED.
 */
int gh_plane_index(const float* uv, int N, int Hp, int Wp, int32_t* texel_start, int32_t* pairs, float* w, void* workspace,
                   size_t ws_bytes, void* hip_stream);

/*
 * grad_out: (N, C) contiguous; texel_start, pairs, w: as gh_plane_index wrote them for the same N, Hp, Wp; grad_plane:
 * (C, Hp, Wp), every element written. A list entry outside [0, 4N) is skipped. grad_plane overlaps no input.
 */
int gh_plane_sample_backward(const float* grad_out, const int32_t* texel_start, const int32_t* pairs, const float* w,
                             float* grad_plane, int N, int C, int Hp, int Wp, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_PLANE_H */
