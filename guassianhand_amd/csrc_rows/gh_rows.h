// gh_rows.h — what the row-tile blocks (csrc_head/gh_head.hip, csrc_vert/gh_vert.hip) share. Internal: not part of the C-ABI.
//   tile      one 4-wave workgroup per 64 rows; the rows' feature columns cross LDS at an odd pitch, so that lane = row reads its own
//             row without a bank conflict (ghr_stage).
//   reduce    the per-workgroup partials of a backward are summed by a second launch, GHR_RED_EL elements x GHR_SEGMENTS runs per
//             workgroup: a run is summed in workgroup order, then the runs in run order (ghr_reduce).
// gh_pool.hip and gh_metrics.hip take ghr_align from here.
#ifndef GH_ROWS_H
#define GH_ROWS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define GHR_BLOCK 256
#define GHR_SEGMENTS 16  // runs of partials (GH_HEAD_SEGMENTS, GH_VERT_SEGMENTS)
#define GHR_RED_EL 16    // elements per workgroup of the reduction

static_assert(GHR_SEGMENTS * GHR_RED_EL == GHR_BLOCK, "one thread per (run, element) of the reduction");

static inline size_t ghr_align(size_t x) { return (x + 255) & ~(size_t)255; }  // workspace parts start on 256 bytes
static inline bool ghr_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ float ghr_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// columns [k0, k0 + kc) of the tile's R rows -> s[row * pitch + col]; rows past the end of x are zeros.
// vec: x is 16-byte aligned and its width and x_stride are multiples of 4 — so is every row, and so are k0 and kc.
__device__ __forceinline__ void ghr_stage(float* s, int pitch, const float* __restrict__ x, long long x_stride, long long row0, int R,
                                          int nrows, int k0, int kc, int vec, int tid) {
  if (vec) {
    const int q = kc >> 2;
    for (int i = tid; i < R * q; i += GHR_BLOCK) {
      const int r = i / q, c = 4 * (i - r * q);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nrows) v = *(const float4*)(x + (row0 + r) * x_stride + k0 + c);
      float* d = s + r * pitch + c;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = tid; i < R * kc; i += GHR_BLOCK) {
      const int r = i / kc, c = i - r * kc;
      s[r * pitch + c] = r < nrows ? x[(row0 + r) * x_stride + k0 + c] : 0.f;
    }
  }
}

// The body of a reduce kernel (GHR_BLOCK threads). Element el of n is store(el, t), t the sum of load(i, el) over the nblk
// workgroups' partials i: GHR_SEGMENTS contiguous runs of i, each summed in ascending i, then the runs in run order.
template <class Load, class Store>
__device__ __forceinline__ void ghr_reduce(int nblk, int n, Load load, Store store) {
  __shared__ float s_red[GHR_SEGMENTS][GHR_RED_EL];
  const int tid = threadIdx.x, el = blockIdx.x * GHR_RED_EL + (tid & (GHR_RED_EL - 1)), seg = tid / GHR_RED_EL;
  const int per = (nblk + GHR_SEGMENTS - 1) / GHR_SEGMENTS;
  const int lo = seg * per, hi = lo + per < nblk ? lo + per : nblk;
  float s = 0.f;
  if (el < n) {
    for (int i = lo; i < hi; ++i) s += load(i, el);
  }
  s_red[seg][tid & (GHR_RED_EL - 1)] = s;
  __syncthreads();
  if (tid < GHR_RED_EL && el < n) {
    float t = 0.f;
    for (int q = 0; q < GHR_SEGMENTS; ++q) t += s_red[q][tid];
    store(el, t);
  }
}

static inline unsigned ghr_reduce_blocks(int n) { return (unsigned)((n + GHR_RED_EL - 1) / GHR_RED_EL); }

#endif
