// gh_pool.hip — per-cell pooling of point features (include/gh_pool.h): what LocalPoolPointnet asks of torch_scatter.
//   plan (3 launches)  hist:    one point per thread; a histogram of the workgroup's 256 points in LDS -> its row of block_hist
//                      scan:    one workgroup; per bin the exclusive prefix over the workgroups, then over the bins -> cell_start
//                      scatter: the same 256 points again; a point's slot is cell_start[bin] + its workgroup's prefix + its rank
//                               among the workgroup's earlier points of the bin, so a cell keeps ascending point order
//   pool fwd / bwd     one 4-wave workgroup per (cell, 64-channel slab), lanes are channels: each wave reduces a contiguous quarter
//                      of the cell's list (every load a coalesced 256-byte row segment, 4 rows in flight), the quarters are combined
//                      through LDS in quarter order, and each wave walks its quarter again to write the rows.
//   plane mean         one workgroup per (8 consecutive cells, 64-channel slab): the 8 lists are contiguous in `order`, each wave
//                      takes a quarter of that range; the (8 x 64) tile crosses LDS so that the channel-first plane is read and
//                      written in 32-byte runs while the point rows stay 256-byte runs.
// The bin after the last cell collects points whose index is out of range; they are written zeros and counted nowhere.
// Maximum (gh_pool.h): ties go to the lowest point index (strict > in the walk and in the quarter combine); a NaN never wins,
// and a cell whose rows are all NaN in a channel is empty for that channel (value 0, argmax T, no gradient); -inf is an ordinary
// value, so a cell of -inf alone returns -inf with its first point as argmax. Means propagate NaN and inf as arithmetic does.
// Only integer LDS atomics (the histogram); every float sum has a fixed order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_pool.h"
#include "../csrc_rows/gh_rows.h"

#define GHP_BLOCK 256
#define GHP_WAVES (GHP_BLOCK / 64)
#define GHP_SCAN_BLOCK 1024
#define GHP_PLANE_CELLS 8

static inline int ghp_blocks(int T) { return (T + GHP_BLOCK - 1) / GHP_BLOCK; }

__device__ __forceinline__ int ghp_bin(const void* __restrict__ index, int is64, int p, int n_cells) {
  const long long v = is64 ? ((const long long*)index)[p] : (long long)((const int*)index)[p];
  return (v >= 0 && v < n_cells) ? (int)v : n_cells;
}

// ---- plan ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHP_BLOCK) void ghp_hist_kernel(const void* __restrict__ index, int is64, int T, int n_cells,
                                                             int* __restrict__ block_hist, unsigned* __restrict__ block_bad) {
  extern __shared__ int s_hist[];                    // n_cells + 1 bins
  __shared__ unsigned s_bad;
  const int bins = n_cells + 1, p = blockIdx.x * GHP_BLOCK + threadIdx.x;
  for (int i = threadIdx.x; i < bins; i += GHP_BLOCK) s_hist[i] = 0;
  if (threadIdx.x == 0) s_bad = 0u;
  __syncthreads();
  if (p < T) {
    const int bin = ghp_bin(index, is64, p, n_cells);
    atomicAdd(&s_hist[bin], 1);
    if (bin == n_cells) s_bad = 1u;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += GHP_BLOCK) block_hist[(size_t)blockIdx.x * bins + i] = s_hist[i];
  if (threadIdx.x == 0) block_bad[blockIdx.x] = s_bad;
}

__global__ __launch_bounds__(GHP_SCAN_BLOCK) void ghp_scan_kernel(int nb, int n_cells, int* __restrict__ block_hist,
                                                                  const unsigned* __restrict__ block_bad,
                                                                  int* __restrict__ cell_start, unsigned* __restrict__ flag) {
  __shared__ int s_scan[GHP_SCAN_BLOCK];
  __shared__ int s_carry;
  __shared__ unsigned s_any;
  const int bins = n_cells + 1, t = threadIdx.x;
  if (t == 0) { s_carry = 0; s_any = 0u; }
  __syncthreads();
  unsigned bad = 0u;
  for (int b = t; b < nb; b += GHP_SCAN_BLOCK) bad |= block_bad[b];
  if (bad) s_any = 1u;
  for (int base = 0; base < bins; base += GHP_SCAN_BLOCK) {
    const int c = base + t;
    int run = 0;
    if (c < bins) {
      for (int b = 0; b < nb; ++b) {                 // exclusive prefix of this bin over the workgroups (coalesced over the bins)
        const size_t i = (size_t)b * bins + c;
        const int v = block_hist[i];
        block_hist[i] = run;
        run += v;
      }
    }
    s_scan[t] = run;
    __syncthreads();
    for (int o = 1; o < GHP_SCAN_BLOCK; o <<= 1) {   // inclusive scan over the bins of this pass
      const int v = t >= o ? s_scan[t - o] : 0;
      __syncthreads();
      s_scan[t] += v;
      __syncthreads();
    }
    const int carry = s_carry;
    if (c < bins) cell_start[c] = carry + s_scan[t] - run;     // bins - 1 == n_cells: the number of points that have a cell
    __syncthreads();
    if (t == GHP_SCAN_BLOCK - 1) s_carry = carry + s_scan[t];
    __syncthreads();
  }
  if (t == 0) *flag = s_any;
}

__global__ __launch_bounds__(GHP_BLOCK) void ghp_scatter_kernel(const void* __restrict__ index, int is64, int T, int n_cells,
                                                                const int* __restrict__ block_hist,
                                                                const int* __restrict__ cell_start, int* __restrict__ order) {
  __shared__ int s_bin[GHP_BLOCK];
  const int bins = n_cells + 1, p = blockIdx.x * GHP_BLOCK + threadIdx.x;
  const int bin = p < T ? ghp_bin(index, is64, p, n_cells) : -1;
  s_bin[threadIdx.x] = bin;
  __syncthreads();
  if (p >= T) return;
  int rank = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) rank += s_bin[j] == bin;
  const int pos = cell_start[bin] + block_hist[(size_t)blockIdx.x * bins + bin] + rank;
  if (pos >= 0 && pos < T) order[pos] = p;
}

// ---- pool forward ---------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(GHP_BLOCK) void ghp_pool_fwd_kernel(const float* __restrict__ x, int xs, int T, int C, int n_cells,
                                                                 const int* __restrict__ cell_start, const int* __restrict__ order,
                                                                 float* __restrict__ out, int os, int* __restrict__ argmax) {
  __shared__ float s_val[GHP_WAVES][64];
  __shared__ int s_arg[GHP_WAVES][64];
  const int cell = blockIdx.x, lane = threadIdx.x & 63, ch = blockIdx.y * 64 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  const int a = cell_start[cell], b = cell == n_cells ? T : cell_start[cell + 1], n = b - a;
  if (cell == n_cells) {                             // points without a cell: zeros
    ghr_walk_store(order, ghr_part(a, n, w), ghr_part(a, n, w + 1), [&](int p) { if (on) out[(size_t)p * os + ch] = 0.0f; });
    return;
  }
  if (n <= 0) {
    if (MODE == GH_POOL_MAX && w == 0 && on) argmax[(size_t)cell * C + ch] = T;
    return;
  }
  const int lo = ghr_part(a, n, w), hi = ghr_part(a, n, w + 1);
  float acc = 0.0f;
  int arg = T;
  ghr_walk(order, lo, hi, [&](int p) { return on ? x[(size_t)p * xs + ch] : 0.0f; },
           [&](int p, float v) {
             if (MODE == GH_POOL_MAX) {
               // strict: the first of equal values stays. v == v: a NaN is never taken, wherever it sits, so a quarter (and a
               // cell) of NaNs alone keeps arg == T and counts as empty; -inf is a value like any other and is taken when first.
               if (v == v && (arg == T || v > acc)) { acc = v; arg = p; }
             } else {
               acc += v;
             }
           });
  s_val[w][lane] = acc;
  s_arg[w][lane] = arg;
  __syncthreads();
  float r = s_val[0][lane];
  int ra = s_arg[0][lane];
#pragma unroll
  for (int q = 1; q < GHP_WAVES; ++q) {                                // quarter order = ascending point order
    const float v = s_val[q][lane];
    const int va = s_arg[q][lane];
    if (MODE == GH_POOL_MAX) {
      if (va != T && (ra == T || v > r)) { r = v; ra = va; }
    } else {
      r += v;
    }
  }
  if (MODE == GH_POOL_MEAN) r = r / (float)n;
  if (MODE == GH_POOL_MAX && w == 0 && on) argmax[(size_t)cell * C + ch] = ra;
  ghr_walk_store(order, lo, hi, [&](int p) { if (on) out[(size_t)p * os + ch] = r; });
}

// ---- pool backward --------------------------------------------------------------------------------------------------------
template <int MODE, int ACC>
__global__ __launch_bounds__(GHP_BLOCK) void ghp_pool_bwd_kernel(const float* __restrict__ g, int gs, int T, int C, int n_cells,
                                                                 const int* __restrict__ cell_start, const int* __restrict__ order,
                                                                 const int* __restrict__ argmax, float* __restrict__ gx, int gxs) {
  __shared__ float s_val[GHP_WAVES][64];
  const int cell = blockIdx.x, lane = threadIdx.x & 63, ch = blockIdx.y * 64 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  const int a = cell_start[cell], b = cell == n_cells ? T : cell_start[cell + 1], n = b - a;
  if (cell == n_cells) {
    if (!ACC) ghr_walk_store(order, ghr_part(a, n, w), ghr_part(a, n, w + 1), [&](int p) { if (on) gx[(size_t)p * gxs + ch] = 0.0f; });
    return;
  }
  if (n <= 0) return;
  const int lo = ghr_part(a, n, w), hi = ghr_part(a, n, w + 1);
  float acc = 0.0f;
  ghr_walk(order, lo, hi, [&](int p) { return on ? g[(size_t)p * gs + ch] : 0.0f; }, [&](int, float v) { acc += v; });
  s_val[w][lane] = acc;
  __syncthreads();
  const float total = ((s_val[0][lane] + s_val[1][lane]) + s_val[2][lane]) + s_val[3][lane];
  if (MODE == GH_POOL_MEAN) {
    const float v = total / (float)n;
    ghr_walk_store(order, lo, hi, [&](int p) {
      if (on) { float* d = gx + (size_t)p * gxs + ch; *d = ACC ? *d + v : v; }
    });
  } else {
    const int am = on ? argmax[(size_t)cell * C + ch] : -1;
    if (ACC) {
      if (w == 0 && am >= 0 && am < T) gx[(size_t)am * gxs + ch] += total;     // one (row, channel) per lane: nothing collides
    } else {
      ghr_walk_store(order, lo, hi, [&](int p) { if (on) gx[(size_t)p * gxs + ch] = p == am ? total : 0.0f; });
    }
  }
}

// ---- plane mean -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHP_BLOCK) void ghp_plane_fwd_kernel(const float* __restrict__ x, int xs, int C, int n_cells,
                                                                  const int* __restrict__ cell_start, const int* __restrict__ order,
                                                                  float* __restrict__ plane) {
  __shared__ float s_part[GHP_WAVES][GHP_PLANE_CELLS][65];
  __shared__ int s_cs[GHP_PLANE_CELLS + 1];
  const int c0 = blockIdx.x * GHP_PLANE_CELLS, ch0 = blockIdx.y * 64, lane = threadIdx.x & 63, ch = ch0 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  if (threadIdx.x <= GHP_PLANE_CELLS) s_cs[threadIdx.x] = cell_start[min(c0 + (int)threadIdx.x, n_cells)];
  __syncthreads();
  const int A = s_cs[0], n = s_cs[GHP_PLANE_CELLS] - A;
  const int lo = ghr_part(A, n, w), hi = ghr_part(A, n, w + 1);
  for (int cl = 0; cl < GHP_PLANE_CELLS; ++cl) {
    const int l = max(s_cs[cl], lo), h = min(s_cs[cl + 1], hi);
    float acc = 0.0f;
    ghr_walk(order, l, h, [&](int p) { return on ? x[(size_t)p * xs + ch] : 0.0f; }, [&](int, float v) { acc += v; });
    s_part[w][cl][lane] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GHP_PLANE_CELLS * 64; i += GHP_BLOCK) {
    const int chl = i / GHP_PLANE_CELLS, cl = i % GHP_PLANE_CELLS;
    if (ch0 + chl >= C || c0 + cl >= n_cells) continue;
    const float total = ((s_part[0][cl][chl] + s_part[1][cl][chl]) + s_part[2][cl][chl]) + s_part[3][cl][chl];
    const int cnt = s_cs[cl + 1] - s_cs[cl];
    plane[(size_t)(ch0 + chl) * n_cells + c0 + cl] = total / (float)max(cnt, 1);
  }
}

__global__ __launch_bounds__(GHP_BLOCK) void ghp_plane_bwd_kernel(const float* __restrict__ gp, int T, int C, int n_cells,
                                                                  const int* __restrict__ cell_start, const int* __restrict__ order,
                                                                  float* __restrict__ gx, int gxs) {
  __shared__ float s_t[GHP_PLANE_CELLS][65];
  __shared__ int s_cs[GHP_PLANE_CELLS + 1];
  const int c0 = blockIdx.x * GHP_PLANE_CELLS, ch0 = blockIdx.y * 64, lane = threadIdx.x & 63, ch = ch0 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  if (c0 >= n_cells) {                               // the workgroup after the last cells: points without a cell get zeros
    const int a = cell_start[n_cells], n = T - a;
    ghr_walk_store(order, ghr_part(a, n, w), ghr_part(a, n, w + 1), [&](int p) { if (on) gx[(size_t)p * gxs + ch] = 0.0f; });
    return;
  }
  if (threadIdx.x <= GHP_PLANE_CELLS) s_cs[threadIdx.x] = cell_start[min(c0 + (int)threadIdx.x, n_cells)];
  __syncthreads();
  for (int i = threadIdx.x; i < GHP_PLANE_CELLS * 64; i += GHP_BLOCK) {
    const int chl = i / GHP_PLANE_CELLS, cl = i % GHP_PLANE_CELLS;
    float v = 0.0f;
    if (ch0 + chl < C && c0 + cl < n_cells) {
      const int cnt = s_cs[cl + 1] - s_cs[cl];
      v = gp[(size_t)(ch0 + chl) * n_cells + c0 + cl] / (float)max(cnt, 1);
    }
    s_t[cl][chl] = v;
  }
  __syncthreads();
  const int A = s_cs[0], n = s_cs[GHP_PLANE_CELLS] - A;
  const int lo = ghr_part(A, n, w), hi = ghr_part(A, n, w + 1);
  for (int cl = 0; cl < GHP_PLANE_CELLS; ++cl) {
    const float v = s_t[cl][lane];
    ghr_walk_store(order, max(s_cs[cl], lo), min(s_cs[cl + 1], hi), [&](int p) { if (on) gx[(size_t)p * gxs + ch] = v; });
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct GhpPlanLayout {
  size_t hist, bad, total;
  int nb;
};

static bool ghp_plan_layout(int T, int n_cells, GhpPlanLayout* L) {
  if (T < 1 || n_cells < 1 || n_cells > GH_POOL_MAX_CELLS) return false;
  L->nb = ghp_blocks(T);
  L->hist = 0;
  L->bad = ghr_align((size_t)L->nb * (n_cells + 1) * sizeof(int));
  L->total = ghr_align(L->bad + (size_t)L->nb * sizeof(unsigned));
  return true;
}

// Two (T x width) windows of float rows: apart, or interleaved columns of rows of one stride (the halves of a cat buffer).
static bool ghp_windows_ok(const float* a, int as, int aw, const float* b, int bs, int bw, int T) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((size_t)(T - 1) * as + aw) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((size_t)(T - 1) * bs + bw) * sizeof(float);
  if (a1 <= b0 || b1 <= a0) return true;
  if (as != bs) return false;
  const long long d = ((long long)b0 - (long long)a0) / (long long)sizeof(float);
  const long long r = ((d % as) + as) % as;          // b's first column counted from a's first column, modulo the row
  return r >= aw && r + bw <= as;
}

static bool ghp_common_ok(int T, int C, int n_cells, const void* cell_start, const void* order) {
  return T >= 1 && C >= 1 && n_cells >= 1 && cell_start && order && ghr_al4(cell_start) && ghr_al4(order);
}

extern "C" size_t gh_pool_plan_workspace(int T, int n_cells) {
  GhpPlanLayout L;
  return ghp_plan_layout(T, n_cells, &L) ? L.total : 0;
}

extern "C" int gh_pool_plan(const void* index, int index_is_int64, int T, int n_cells, int32_t* cell_start, int32_t* order,
                            uint32_t* flag, void* workspace, size_t ws_bytes, void* hip_stream) {
  if (T < 1 || n_cells < 1 || !index || !cell_start || !order || !flag || !workspace) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(cell_start) || !ghr_al4(order) || !ghr_al4(flag) || ((uintptr_t)workspace & 15) != 0 ||
      ((uintptr_t)index & (index_is_int64 ? 7 : 3)) != 0)
    return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS) return GH_ERR_UNSUPPORTED;
  GhpPlanLayout L;
  if (!ghp_plan_layout(T, n_cells, &L)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < L.total) return GH_ERR_WORKSPACE_SMALL;
  (void)hipGetLastError();
  char* ws = (char*)workspace;
  int* block_hist = (int*)(ws + L.hist);
  unsigned* block_bad = (unsigned*)(ws + L.bad);
  hipStream_t s = (hipStream_t)hip_stream;
  const int is64 = index_is_int64 != 0;
  hipLaunchKernelGGL(ghp_hist_kernel, dim3((unsigned)L.nb), dim3(GHP_BLOCK), (size_t)(n_cells + 1) * sizeof(int), s, index, is64, T,
                     n_cells, block_hist, block_bad);
  hipLaunchKernelGGL(ghp_scan_kernel, dim3(1), dim3(GHP_SCAN_BLOCK), 0, s, L.nb, n_cells, block_hist, (const unsigned*)block_bad,
                     cell_start, flag);
  hipLaunchKernelGGL(ghp_scatter_kernel, dim3((unsigned)L.nb), dim3(GHP_BLOCK), 0, s, index, is64, T, n_cells,
                     (const int*)block_hist, (const int*)cell_start, order);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

static inline dim3 ghp_cell_grid(int n_cells, int C) { return dim3((unsigned)(n_cells + 1), (unsigned)((C + 63) / 64)); }

extern "C" int gh_pool_forward(const float* x, int x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                               const int32_t* order, int reduce, float* out, int out_stride, int out_col, int32_t* argmax,
                               void* hip_stream) {
  if (!ghp_common_ok(T, C, n_cells, cell_start, order) || !x || !out || !ghr_al4(x) || !ghr_al4(out))
    return GH_ERR_INVALID_ARG;
  if (reduce != GH_POOL_MAX && reduce != GH_POOL_MEAN) return GH_ERR_INVALID_ARG;
  if (reduce == GH_POOL_MAX && (!argmax || !ghr_al4(argmax))) return GH_ERR_INVALID_ARG;
  if (x_stride < C || out_col < 0 || (long long)out_stride < (long long)out_col + C) return GH_ERR_INVALID_ARG;
  if (!ghp_windows_ok(x, x_stride, C, out + out_col, out_stride, C, T)) return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS || (C + 63) / 64 > 65535) return GH_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  hipStream_t s = (hipStream_t)hip_stream;
  const dim3 grid = ghp_cell_grid(n_cells, C);
  if (reduce == GH_POOL_MAX)
    hipLaunchKernelGGL(ghp_pool_fwd_kernel<GH_POOL_MAX>, grid, dim3(GHP_BLOCK), 0, s, x, x_stride, T, C, n_cells, cell_start, order,
                       out + out_col, out_stride, argmax);
  else
    hipLaunchKernelGGL(ghp_pool_fwd_kernel<GH_POOL_MEAN>, grid, dim3(GHP_BLOCK), 0, s, x, x_stride, T, C, n_cells, cell_start, order,
                       out + out_col, out_stride, argmax);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_pool_backward(const float* grad_out, int g_stride, int g_col, int T, int C, int n_cells,
                                const int32_t* cell_start, const int32_t* order, int reduce, const int32_t* argmax, float* grad_x,
                                int gx_stride, int accumulate, void* hip_stream) {
  if (!ghp_common_ok(T, C, n_cells, cell_start, order) || !grad_out || !grad_x || !ghr_al4(grad_out) || !ghr_al4(grad_x))
    return GH_ERR_INVALID_ARG;
  if (reduce != GH_POOL_MAX && reduce != GH_POOL_MEAN) return GH_ERR_INVALID_ARG;
  if (reduce == GH_POOL_MAX && (!argmax || !ghr_al4(argmax))) return GH_ERR_INVALID_ARG;
  if (gx_stride < C || g_col < 0 || (long long)g_stride < (long long)g_col + C) return GH_ERR_INVALID_ARG;
  if (!ghp_windows_ok(grad_x, gx_stride, C, grad_out + g_col, g_stride, C, T)) return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS || (C + 63) / 64 > 65535) return GH_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  hipStream_t s = (hipStream_t)hip_stream;
  const dim3 grid = ghp_cell_grid(n_cells, C);
  const float* g = grad_out + g_col;
#define GHP_BWD(MODE, ACC)                                                                                                      \
  hipLaunchKernelGGL((ghp_pool_bwd_kernel<MODE, ACC>), grid, dim3(GHP_BLOCK), 0, s, g, g_stride, T, C, n_cells, cell_start, order, \
                     argmax, grad_x, gx_stride)
  if (reduce == GH_POOL_MAX) {
    if (accumulate) GHP_BWD(GH_POOL_MAX, 1); else GHP_BWD(GH_POOL_MAX, 0);
  } else {
    if (accumulate) GHP_BWD(GH_POOL_MEAN, 1); else GHP_BWD(GH_POOL_MEAN, 0);
  }
#undef GHP_BWD
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_plane_mean_forward(const float* x, int x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                                     const int32_t* order, float* plane, void* hip_stream) {
  if (!ghp_common_ok(T, C, n_cells, cell_start, order) || !x || !plane || !ghr_al4(x) || !ghr_al4(plane))
    return GH_ERR_INVALID_ARG;
  if (x_stride < C) return GH_ERR_INVALID_ARG;
  const uintptr_t p0 = (uintptr_t)plane, p1 = (uintptr_t)(plane + (size_t)C * n_cells);
  const uintptr_t x0 = (uintptr_t)x, x1 = (uintptr_t)(x + (size_t)(T - 1) * x_stride + C);
  if (p0 < x1 && x0 < p1) return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS || (C + 63) / 64 > 65535) return GH_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  const dim3 grid((unsigned)((n_cells + GHP_PLANE_CELLS - 1) / GHP_PLANE_CELLS), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(ghp_plane_fwd_kernel, grid, dim3(GHP_BLOCK), 0, (hipStream_t)hip_stream, x, x_stride, C, n_cells, cell_start,
                     order, plane);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_plane_mean_backward(const float* grad_plane, int T, int C, int n_cells, const int32_t* cell_start,
                                      const int32_t* order, float* grad_x, int gx_stride, void* hip_stream) {
  if (!ghp_common_ok(T, C, n_cells, cell_start, order) || !grad_plane || !grad_x || !ghr_al4(grad_plane) || !ghr_al4(grad_x))
    return GH_ERR_INVALID_ARG;
  if (gx_stride < C) return GH_ERR_INVALID_ARG;
  const uintptr_t p0 = (uintptr_t)grad_plane, p1 = (uintptr_t)(grad_plane + (size_t)C * n_cells);
  const uintptr_t g0 = (uintptr_t)grad_x, g1 = (uintptr_t)(grad_x + (size_t)(T - 1) * gx_stride + C);
  if (p0 < g1 && g0 < p1) return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS || (C + 63) / 64 > 65535) return GH_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  const dim3 grid((unsigned)((n_cells + GHP_PLANE_CELLS - 1) / GHP_PLANE_CELLS + 1), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(ghp_plane_bwd_kernel, grid, dim3(GHP_BLOCK), 0, (hipStream_t)hip_stream, grad_plane, T, C, n_cells, cell_start,
                     order, grad_x, gx_stride);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
