/*
 * gh_uvd.h — C-ABI of the UV search: for every point, its closest point on a triangle mesh that carries per-corner UVs, and that
 * point's UV, distance, face and barycentrics. What the reference asks of livehand.input_encoder.get_uvd (infer_one_shot.py:229,
 * tgs/models/renderer_one_shot.py:481) on the UV-topology hand mesh. The block is specified by the mathematics below; it is NOT
 * pinned against livehand's implementation ("The UV search").
 *
 * Inputs   points (N,3) float32, verts (V,3) float32, faces (F,3) int32, face_uv (F,3,2) float32; all contiguous.
 *
 * Valid    A face is valid when its three indices lie in [0, V) and its nine coordinates are finite. An invalid face never wins and
 *          its vertices are never read out of range. The check runs on the device; nothing is read back.
 *
 * Distance For a valid face f with corners a, b, c, c_f(p) is the closest point of the closed triangle to p, and s_f = |p - c_f|^2 in
 *          float32. It is the smallest of up to four candidates, each a squared length of a residual vector formed with fmaf:
 *            interior  v, w from the 2 x 2 normal equations of (ab, ac), taken when v >= 0, w >= 0 and (1 - v) - w >= 0;
 *            ab, ac, bc  the parameter of p's projection on the edge, clamped to [0, 1].
 *          A triangle of zero area has no interior candidate and acts as the union of its three edges; an edge of zero length acts as
 *          its first vertex, so three coincident vertices act as that vertex. "Zero area" in float32 means
 *          |ab|^2 |ac|^2 - (ab.ac)^2 <= 2^-15 |ab|^2 |ac|^2 (the sine of the angle at a is below 2^-7.5): below that the normal
 *          equations lose more than the sliver's height. Among equal candidates of one face the order interior, ab, ac, bc decides.
 *
 * Winner   The lexicographic minimum of (s_f, f): the smallest squared distance as computed, and among equal values the lowest face
 *          index. A point with a non-finite coordinate, a mesh without a valid face, or a point so far away that every s_f overflows
 *          has no winner: face = -1 and uv, dist, bary are NaN. Nothing faults.
 *
 * Outputs  face int32; bary (3) with every b_i >= 0 exactly (the interior's b0 = max((1 - v) - w, 0), an edge's 1 - t with t in
 *          [0, 1]); uv = fmaf(b2, uv2, fmaf(b1, uv1, b0 * uv0)) per component; dist = sqrtf(s). b_i >= 0 keeps every UV inside the
 *          hull of its face's corner UVs: the grid_sample that consumes it pads with zeros outside the map.
 *
 * Independence  A point's four outputs are a function of that point and the mesh alone: bitwise independent of N, of the point's
 *          place in the launch and of `split`. The library is built with -ffp-contract=off: FMAs only where the source says fmaf.
 *
 * Launches face records (one thread per face: validity, a, ab, ac, bc, their dot products and reciprocals; GH_UVD_REC_BYTES each, in
 *          the workspace) -> search (lane = point, 256-thread workgroups, blockIdx.y = one of `split` contiguous face chunks, the
 *          running best replaced on a strict < walking ascending f) -> finish (split > 1 only: one thread per point, the minimum over
 *          chunks in ascending chunk order, then the winner recomputed by the search's own device function). No atomics, and no
 *          workgroup waits for another. A chunk past the last face (split > F) is not launched.
 *
 * split = 0 lets the library choose: gh_uvd_auto_split(N, F) = clamp(min(GH_UVD_TARGET_WGS / ceil(N / 256), F / GH_UVD_MIN_CHUNK),
 *          1, GH_UVD_MAX_SPLIT), integer divisions. Pure host arithmetic. GH_UVD_TARGET_WGS workgroups are four rounds of the eight
 *          that fit a CU of an MI355X at once: at the workload's shape (N = 98,562, F = 3,076) the measured time falls with every
 *          finer split up to GH_UVD_MAX_SPLIT (profiles/uvd_timing.txt), the last workgroups of a coarse grid leaving CUs idle. A
 *          chunk keeps at least GH_UVD_MIN_CHUNK faces, so a small mesh is searched in one launch less.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments or a short workspace. All
 * pointers 4-byte aligned, the workspace 16-byte aligned.
 */
#ifndef GH_UVD_H
#define GH_UVD_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_UVD_MAX_SPLIT 16
#define GH_UVD_REC_BYTES 80
#define GH_UVD_TARGET_WGS 8192
#define GH_UVD_MIN_CHUNK 128

/* Bytes of workspace gh_uvd_forward needs for these sizes; split = 0 sizes it for gh_uvd_auto_split(N, F). 0 for invalid sizes:
 * N < 0, F < 1, split outside [0, GH_UVD_MAX_SPLIT]. Pure host arithmetic. */
size_t gh_uvd_workspace_bytes(int N, int F, int split);

/* The split that split = 0 stands for (the rule above); 1 for N < 1 or F < 1. Pure host arithmetic. */
int gh_uvd_auto_split(int N, int F);

/*
 * uv: (N,2), every element written. dist (N,), face (N,) and bary (N,3) may each be NULL: not wanted. N = 0 returns GH_OK without a
 * launch. N < 0, F < 1, V < 1, split outside [0, GH_UVD_MAX_SPLIT], a null or misaligned pointer: GH_ERR_INVALID_ARG. ws_bytes below
 * gh_uvd_workspace_bytes(N, F, split): GH_ERR_WORKSPACE_SMALL.
 */
int gh_uvd_forward(const float* points, int N, const float* verts, int V, const int32_t* faces, const float* face_uv, int F,
                   int split, float* uv, float* dist, int32_t* face, float* bary,
                   void* workspace, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_UVD_H */
