// gh_uvd.hip — the UV search (include/gh_uvd.h): every point's closest point on a triangle mesh with per-corner UVs.
//   records (1 launch)  one thread per face: the validity flag and what the inner loop needs (a, ab, ac, bc, |ab|^2, ab.ac, |ac|^2 and
//                       the reciprocals the loop multiplies by), 20 words per face in the workspace
//   search  (1 launch)  lane = point, 4 waves per workgroup, blockIdx.y = a contiguous chunk of faces. The face index is wave-uniform,
//                       so a record arrives through scalar loads (a dwordx16, a dwordx2 and a dword) and sits in SGPRs: no LDS, no
//                       barrier. GHU_UNROLL records are fetched at a time, so that their loads are in flight under the arithmetic of
//                       the ones before. ghu_closest is written with selects only, and the loop has no branch but its own: an invalid
//                       face's record carries a = NaN, every candidate of it is NaN and loses the strict <. The running best is
//                       replaced on a strict < in ascending f. One chunk: the lane finishes its point (ghu_finish); otherwise it
//                       stores its (s, f) at [chunk * N + point].
//   finish  (split > 1) one thread per point: the minimum over chunks in ascending chunk order on a strict <, then ghu_finish.
// ghu_finish recomputes the winner with ghu_closest, the function the search ran: s has the same bits whatever the split.
// No atomics, and no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_uvd.h"
#include "../csrc_rows/gh_rows.h"

#define GHU_BLOCK 256
#define GHU_UNROLL 4      // records the search loop fetches at a time (20 SGPRs each)
#define GHU_DEGENERATE 0x1p-15f   // |ab|^2 |ac|^2 - (ab.ac)^2 at or below this share of |ab|^2 |ac|^2: no interior candidate

struct GhuRec {
  float ax, ay, az, abx, aby, abz, acx, acy, acz, bcx, bcy, bcz;
  float d00, d01, d11;          // |ab|^2, ab.ac, |ac|^2
  float i00, i11, ibc, iden;    // 1 / |ab|^2, 1 / |ac|^2, 1 / |bc|^2, 1 / (d00 d11 - d01^2); 0 where the quotient does not exist
  int valid;
};
static_assert(sizeof(GhuRec) == GH_UVD_REC_BYTES, "the header states the record's size");

__device__ __forceinline__ float ghu_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ float ghu_recip(float d) {   // 0 for a zero length, and for one so small that 1 / d is not finite
  const float r = 1.0f / d;
  return (d > 0.0f && r <= FLT_MAX) ? r : 0.0f;
}

__device__ __forceinline__ float ghu_clamp01(float t) { return fminf(fmaxf(t, 0.0f), 1.0f); }   // NaN -> 0

// The squared distance of p to the closed triangle of r and the barycentrics of the closest point. Selects only.
__device__ __forceinline__ float ghu_closest(const GhuRec& r, float px, float py, float pz, float& b0, float& b1, float& b2) {
  const float apx = px - r.ax, apy = py - r.ay, apz = pz - r.az;
  const float d1 = ghu_dot(r.abx, r.aby, r.abz, apx, apy, apz);
  const float d2 = ghu_dot(r.acx, r.acy, r.acz, apx, apy, apz);
  // interior: the normal equations of (ab, ac)
  const float v = (r.d11 * d1 - r.d01 * d2) * r.iden;
  const float w = (r.d00 * d2 - r.d01 * d1) * r.iden;
  const float u = (1.0f - v) - w;
  const bool inside = r.iden > 0.0f && v >= 0.0f && w >= 0.0f && u >= 0.0f;
  const float ix = fmaf(-w, r.acx, fmaf(-v, r.abx, apx)), iy = fmaf(-w, r.acy, fmaf(-v, r.aby, apy)), iz = fmaf(-w, r.acz, fmaf(-v, r.abz, apz));
  const float s_in = ghu_dot(ix, iy, iz, ix, iy, iz);
  // the three edges
  const float t1 = ghu_clamp01(d1 * r.i00);
  const float ex = fmaf(-t1, r.abx, apx), ey = fmaf(-t1, r.aby, apy), ez = fmaf(-t1, r.abz, apz);
  const float s_ab = ghu_dot(ex, ey, ez, ex, ey, ez);
  const float t2 = ghu_clamp01(d2 * r.i11);
  const float fx = fmaf(-t2, r.acx, apx), fy = fmaf(-t2, r.acy, apy), fz = fmaf(-t2, r.acz, apz);
  const float s_ac = ghu_dot(fx, fy, fz, fx, fy, fz);
  const float bpx = apx - r.abx, bpy = apy - r.aby, bpz = apz - r.abz;
  const float t3 = ghu_clamp01(ghu_dot(r.bcx, r.bcy, r.bcz, bpx, bpy, bpz) * r.ibc);
  const float gx = fmaf(-t3, r.bcx, bpx), gy = fmaf(-t3, r.bcy, bpy), gz = fmaf(-t3, r.bcz, bpz);
  const float s_bc = ghu_dot(gx, gy, gz, gx, gy, gz);
  float s = inside ? s_in : INFINITY;
  b0 = fmaxf(u, 0.0f); b1 = v; b2 = w;
  bool lt = s_ab < s;
  s = lt ? s_ab : s; b0 = lt ? 1.0f - t1 : b0; b1 = lt ? t1 : b1; b2 = lt ? 0.0f : b2;
  lt = s_ac < s;
  s = lt ? s_ac : s; b0 = lt ? 1.0f - t2 : b0; b1 = lt ? 0.0f : b1; b2 = lt ? t2 : b2;
  lt = s_bc < s;
  s = lt ? s_bc : s; b0 = lt ? 0.0f : b0; b1 = lt ? 1.0f - t3 : b1; b2 = lt ? t3 : b2;
  return s;
}

// ---- face records -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHU_BLOCK) void ghu_records_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                 GhuRec* __restrict__ recs) {
  const int f = blockIdx.x * GHU_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  GhuRec r = {};
  r.ax = r.ay = r.az = __int_as_float(0x7fc00000);          // an invalid face: every candidate is NaN and never wins
  if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {     // integers, before anything is addressed by them
    const float* a = verts + 3 * (size_t)i0;
    const float* b = verts + 3 * (size_t)i1;
    const float* c = verts + 3 * (size_t)i2;
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && fabsf(a[k]) <= FLT_MAX && fabsf(b[k]) <= FLT_MAX && fabsf(c[k]) <= FLT_MAX;
    if (finite) {
      r.ax = a[0]; r.ay = a[1]; r.az = a[2];
      r.abx = b[0] - a[0]; r.aby = b[1] - a[1]; r.abz = b[2] - a[2];
      r.acx = c[0] - a[0]; r.acy = c[1] - a[1]; r.acz = c[2] - a[2];
      r.bcx = c[0] - b[0]; r.bcy = c[1] - b[1]; r.bcz = c[2] - b[2];
      r.d00 = ghu_dot(r.abx, r.aby, r.abz, r.abx, r.aby, r.abz);
      r.d01 = ghu_dot(r.abx, r.aby, r.abz, r.acx, r.acy, r.acz);
      r.d11 = ghu_dot(r.acx, r.acy, r.acz, r.acx, r.acy, r.acz);
      r.i00 = ghu_recip(r.d00);
      r.i11 = ghu_recip(r.d11);
      r.ibc = ghu_recip(ghu_dot(r.bcx, r.bcy, r.bcz, r.bcx, r.bcy, r.bcz));
      const float den = r.d00 * r.d11 - r.d01 * r.d01;
      r.iden = den > GHU_DEGENERATE * (r.d00 * r.d11) ? ghu_recip(den) : 0.0f;
      r.valid = 1;
    }
  }
  recs[f] = r;
}

// ---- the winner's outputs -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ghu_finish(int n, int best_f, float px, float py, float pz, const GhuRec* __restrict__ recs,
                                           const float* __restrict__ face_uv, float* __restrict__ uv, float* __restrict__ dist,
                                           int* __restrict__ face, float* __restrict__ bary) {
  const float nan = __int_as_float(0x7fc00000);
  float b0 = nan, b1 = nan, b2 = nan, u = nan, v = nan, d = nan;
  if (best_f >= 0) {
    const GhuRec r = recs[best_f];
    d = sqrtf(ghu_closest(r, px, py, pz, b0, b1, b2));
    const float* t = face_uv + 6 * (size_t)best_f;
    u = fmaf(b2, t[4], fmaf(b1, t[2], b0 * t[0]));
    v = fmaf(b2, t[5], fmaf(b1, t[3], b0 * t[1]));
  }
  uv[2 * (size_t)n] = u;
  uv[2 * (size_t)n + 1] = v;
  if (dist) dist[n] = d;
  if (face) face[n] = best_f;
  if (bary) { bary[3 * (size_t)n] = b0; bary[3 * (size_t)n + 1] = b1; bary[3 * (size_t)n + 2] = b2; }
}

// ---- search -------------------------------------------------------------------------------------------------------------------------
// per: faces per chunk. part_s / part_f: (chunks, N) when the grid has more than one chunk, unused otherwise.
__global__ __launch_bounds__(GHU_BLOCK) void ghu_search_kernel(const float* __restrict__ points, int N, const GhuRec* __restrict__ recs, int F,
                                                                int per, const float* __restrict__ face_uv, float* __restrict__ part_s,
                                                                int* __restrict__ part_f, float* __restrict__ uv, float* __restrict__ dist,
                                                                int* __restrict__ face, float* __restrict__ bary) {
  const int n = blockIdx.x * GHU_BLOCK + threadIdx.x;
  const int m = n < N ? n : N - 1;                      // lanes past the end search the last point and store nothing
  const float px = points[3 * (size_t)m], py = points[3 * (size_t)m + 1], pz = points[3 * (size_t)m + 2];
  const int f0 = blockIdx.y * per, f1 = min(F, f0 + per);
  float best_s = INFINITY;
  int best_f = -1;
  auto step = [&](const GhuRec& r, int f) {
    float b0, b1, b2;
    const float s = ghu_closest(r, px, py, pz, b0, b1, b2);   // NaN for an invalid face (its record's a is NaN)
    const bool lt = s < best_s;                         // false for a NaN: an invalid face and a non-finite point never win
    best_s = lt ? s : best_s;
    best_f = lt ? f : best_f;
  };
  int f = f0;                                           // f is wave-uniform: scalar loads, GHU_UNROLL records in flight
  for (; f + GHU_UNROLL <= f1; f += GHU_UNROLL) {
    GhuRec r[GHU_UNROLL];
#pragma unroll
    for (int k = 0; k < GHU_UNROLL; ++k) r[k] = recs[f + k];
#pragma unroll
    for (int k = 0; k < GHU_UNROLL; ++k) step(r[k], f + k);
  }
  for (; f < f1; ++f) step(recs[f], f);
  if (n >= N) return;
  if (gridDim.y == 1) {
    ghu_finish(n, best_f, px, py, pz, recs, face_uv, uv, dist, face, bary);
  } else {
    const size_t at = (size_t)blockIdx.y * (size_t)N + (size_t)n;
    part_s[at] = best_s;
    part_f[at] = best_f;
  }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHU_BLOCK) void ghu_finish_kernel(const float* __restrict__ points, int N, const GhuRec* __restrict__ recs,
                                                                int chunks, const float* __restrict__ face_uv,
                                                                const float* __restrict__ part_s, const int* __restrict__ part_f,
                                                                float* __restrict__ uv, float* __restrict__ dist, int* __restrict__ face,
                                                                float* __restrict__ bary) {
  const int n = blockIdx.x * GHU_BLOCK + threadIdx.x;
  if (n >= N) return;
  float best_s = INFINITY;
  int best_f = -1;
  for (int c = 0; c < chunks; ++c) {
    const size_t at = (size_t)c * (size_t)N + (size_t)n;
    const float s = part_s[at];
    const int f = part_f[at];
    const bool lt = s < best_s;                         // ascending chunks are ascending faces: equal s keeps the lower f
    best_s = lt ? s : best_s;
    best_f = lt ? f : best_f;
  }
  ghu_finish(n, best_f, points[3 * (size_t)n], points[3 * (size_t)n + 1], points[3 * (size_t)n + 2], recs, face_uv, uv, dist, face, bary);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct GhuLayout {
  size_t recs, part_s, part_f, total;
  int split;
};

extern "C" int gh_uvd_auto_split(int N, int F) {
  if (N < 1 || F < 1) return 1;
  const int blocks = (int)(((long long)N + GHU_BLOCK - 1) / GHU_BLOCK);
  int s = GH_UVD_TARGET_WGS / blocks;
  if (s > F / GH_UVD_MIN_CHUNK) s = F / GH_UVD_MIN_CHUNK;
  if (s > GH_UVD_MAX_SPLIT) s = GH_UVD_MAX_SPLIT;
  return s < 1 ? 1 : s;
}

static bool ghu_layout(int N, int F, int split, GhuLayout* L) {
  if (N < 0 || F < 1 || split < 0 || split > GH_UVD_MAX_SPLIT) return false;
  L->split = split == 0 ? gh_uvd_auto_split(N, F) : split;
  L->recs = 0;
  L->part_s = ghr_align((size_t)F * sizeof(GhuRec));
  const size_t part = L->split > 1 ? ghr_align((size_t)L->split * (size_t)N * sizeof(float)) : 0;
  L->part_f = L->part_s + part;
  L->total = L->part_f + part;
  return true;
}

extern "C" size_t gh_uvd_workspace_bytes(int N, int F, int split) {
  GhuLayout L;
  return ghu_layout(N, F, split, &L) ? L.total : 0;
}

extern "C" int gh_uvd_forward(const float* points, int N, const float* verts, int V, const int32_t* faces, const float* face_uv, int F,
                              int split, float* uv, float* dist, int32_t* face, float* bary, void* workspace, size_t ws_bytes,
                              void* hip_stream) {
  GhuLayout L;
  if (V < 1 || !ghu_layout(N, F, split, &L)) return GH_ERR_INVALID_ARG;
  if (N == 0) return GH_OK;
  if (!points || !verts || !faces || !face_uv || !uv || !workspace) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(points) || !ghr_al4(verts) || !ghr_al4(faces) || !ghr_al4(face_uv) || !ghr_al4(uv) ||
      !ghr_al4(dist) || !ghr_al4(face) || !ghr_al4(bary) || !ghr_al16(workspace))
    return GH_ERR_INVALID_ARG;
  if (ws_bytes < L.total) return GH_ERR_WORKSPACE_SMALL;
  hipStream_t s = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  GhuRec* recs = (GhuRec*)(ws + L.recs);
  float* part_s = (float*)(ws + L.part_s);
  int* part_f = (int*)(ws + L.part_f);
  const int per = (F + L.split - 1) / L.split;          // faces per chunk
  const int chunks = (F + per - 1) / per;               // <= split: a chunk past the last face is not launched
  const unsigned pblocks = (unsigned)(((long long)N + GHU_BLOCK - 1) / GHU_BLOCK);
  (void)hipGetLastError();
  hipLaunchKernelGGL(ghu_records_kernel, dim3((unsigned)((F + GHU_BLOCK - 1) / GHU_BLOCK)), dim3(GHU_BLOCK), 0, s, verts, V, faces, F, recs);
  if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(ghu_search_kernel, dim3(pblocks, (unsigned)chunks), dim3(GHU_BLOCK), 0, s, points, N, recs, F, per, face_uv, part_s,
                     part_f, uv, dist, face, bary);
  if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  if (chunks > 1) {
    hipLaunchKernelGGL(ghu_finish_kernel, dim3(pblocks), dim3(GHU_BLOCK), 0, s, points, N, recs, chunks, face_uv, part_s, part_f, uv, dist,
                       face, bary);
    if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  }
  return GH_OK;
}
