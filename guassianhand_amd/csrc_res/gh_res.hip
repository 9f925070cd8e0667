// gh_res.hip — the point encoders' ResNet blocks with the pooled half folded per cell (include/gh_res.h).
//
// Row kernels. One product shape, gh_rows.h's "columns": v_mfma_f32_32x32x2_f32, D[i][j] = fma chain over k of A[i][k] * B[k][j],
// exact float32, with the point as the column: a wave owns 32 rows of x, lane l the point l & 31, and every product is
// [channel][point]. The weights are the A operand and come from LDS, where the four waves of a workgroup share one slab: 32 columns
// of all H rows in the forward (read along the row, pitch 33), 32 rows of up to 128 columns in the backward (read along the column:
// the product is with W^T); every window lies inside its matrix (ghr_fetch, unchecked). h and dh stay in the accumulators and are the
// B operand of the next product register by register, so the sum over them runs in the order the registers hold their rows
// (gh_res.h). 32 rows x 128 channels are four accumulators; the forward keeps two such sets (h, out). The forward's first loop runs
// two chains from one pass over x's slabs and is written out here; the other products are gh_rows.h's (ghr_mm, ghr_mm_t, ghr_mm_tg).
//
// Cell kernels: gh_pool.hip's walk (gh_rows.h) with one 4-wave workgroup per (cell, 64-channel slab), lanes are channels; the
// quarters are combined through LDS in quarter order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_pool.h"
#include "../../include/gh_res.h"
#include "../csrc_rows/gh_rows.h"

#define GR_BLOCK GHR_BLOCK
#define GR_WAVE_ROWS 32
#define GR_SLAB 32   // columns (forward) or rows (backward) of a weight slab

static_assert(GH_RES_ROWS == (GR_BLOCK / 64) * GR_WAVE_ROWS, "four waves of 32 rows");
static_assert(GH_RES_MAX_H == 4 * 32, "four accumulators of 32 channels");

__device__ __forceinline__ float gr_relu(float v) { return v < 0.f ? 0.f : v; }  // a NaN passes

struct GrFwd {
  const float *x, *u, *s, *W0, *Ws, *W1;
  const int32_t* row_of;
  float* out;
  uint32_t* mask;
  long long x_stride, w0_stride, ws_stride, out_stride;
  int T, Cin, R, vec_w0, vec_ws, vec_w1, vec_out;
};

template <int NT>
__global__ __launch_bounds__(GR_BLOCK, 2) void gr_forward_kernel(GrFwd a) {
  constexpr int H = 32 * NT;
  __shared__ float s_w[2 * H * GHR_WP];
  float* s_a = s_w;
  float* s_b = s_w + H * GHR_WP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const long long p = (long long)blockIdx.x * GH_RES_ROWS + wave * GR_WAVE_ROWS + col;
  const bool live = p < a.T;
  int r = (live && a.row_of) ? a.row_of[p] : 0;
  r = r < 0 ? 0 : (r >= a.R ? a.R - 1 : r);
  const float* ur = a.u + (long long)r * H;
  const float* sr = a.s + (long long)r * H;
  ghr_acc h[NT], o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      h[t][k] = ur[32 * t + ghr_acc_row(k, half)];
      o[t][k] = sr[32 * t + ghr_acc_row(k, half)];
    }
  }
  const float* xp = a.x + (live ? p : 0) * a.x_stride;
  for (int k0 = 0; k0 < a.Cin; k0 += GR_SLAB) {
    GhrSlab<NT, GR_SLAB / 4> wa, wb;                            // H rows x 32 columns each
    ghr_fetch(wa, a.W0, a.w0_stride, 0, k0, a.vec_w0, tid);
    ghr_fetch(wb, a.Ws, a.ws_stride, 0, k0, a.vec_ws, tid);
    float xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) xv[s] = live ? xp[k0 + 2 * s + half] : 0.f;
    __syncthreads();                                           // the previous slab has been read by every wave
    ghr_put(wa, s_a, GHR_WP, tid);
    ghr_put(wb, s_b, GHR_WP, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float xr = gr_relu(xv[s]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int w = (32 * t + col) * GHR_WP + 2 * s + half;
        h[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[w], xr, h[t], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_b[w], xv[s], o[t], 0, 0, 0);
      }
    }
  }
  if (a.mask) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      unsigned m = 0u;
#pragma unroll
      for (int k = 0; k < 16; ++k) m |= (h[t][k] > 0.f ? 1u : 0u) << ghr_acc_row(k, half);
      m |= (unsigned)__shfl_xor((int)m, 32);
      if (half == 0 && live) a.mask[p * NT + t] = m;
    }
  }
  ghr_mm<true, NT, NT>(o, NT, h, [](float v) { return gr_relu(v); }, s_a, a.W1, H, a.vec_w1, tid, col, half);
  ghr_store_tiles<NT>(o, a.out + (live ? p : 0) * a.out_stride, half, live, a.vec_out);
}

struct GrBwd {
  const float *g, *x, *W0, *Ws, *W1;
  const uint32_t* mask;
  float *dx, *dh;
  long long g_stride, x_stride, w0_stride, ws_stride, dx_stride;
  int T, Cin, vec_w0, vec_ws, vec_w1, vec_dx, vec_dh;
};

template <int NT>
__global__ __launch_bounds__(GR_BLOCK, 2) void gr_backward_kernel(GrBwd a) {  // two waves per SIMD: 256 registers
  constexpr int H = 32 * NT;
  __shared__ float s_w[GR_SLAB * H];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const long long p = (long long)blockIdx.x * GH_RES_ROWS + wave * GR_WAVE_ROWS + col;
  const bool live = p < a.T;
  const long long pl = live ? p : 0;
  const float* gp = a.g + pl * a.g_stride;
  const float* xp = a.x + pl * a.x_stride;

  ghr_acc dh[NT];
  ghr_fill<NT>(dh, nullptr, half);
  ghr_mm_tg<true, NT>(dh, s_w, a.W1, H, 0, H, H, a.vec_w1, gp, live, tid, col, half);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const unsigned m = live ? a.mask[p * NT + t] : 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) dh[t][k] = ((m >> ghr_acc_row(k, half)) & 1u) ? dh[t][k] : 0.f;
  }
  if (a.dh) ghr_store_tiles<NT>(dh, a.dh + pl * H, half, live, a.vec_dh);

  for (int k0 = 0; k0 < a.Cin; k0 += H) {
    ghr_acc d[NT];
    ghr_fill<NT>(d, nullptr, half);
    ghr_mm_t<true, NT, NT>(d, NT, dh, s_w, a.W0, a.w0_stride, k0, a.Cin, a.vec_w0, tid, col, half);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float xv = live ? xp[k0 + 32 * t + ghr_acc_row(k, half)] : 0.f;
        d[t][k] = xv > 0.f ? d[t][k] : 0.f;
      }
    }
    ghr_mm_tg<true, NT>(d, s_w, a.Ws, a.ws_stride, k0, H, a.Cin, a.vec_ws, gp, live, tid, col, half);
    ghr_store_tiles<NT>(d, a.dx + pl * a.dx_stride + k0, half, live, a.vec_dx);
  }
}

// ---- cell kernels ----------------------------------------------------------------------------------------------------------------------
// [a, b) of `order` for cell c; c == n_cells: the points without a cell
__device__ __forceinline__ void gr_cell_range(const int* __restrict__ cell_start, int cell, int n_cells, int T, int* a, int* b) {
  *a = cell_start[cell];
  *b = cell == n_cells ? T : cell_start[cell + 1];
}

__global__ __launch_bounds__(GR_BLOCK) void gr_cell_sum_kernel(const float* __restrict__ x, long long xs, int T, int C, int n_cells,
                                                               const int* __restrict__ cell_start, const int* __restrict__ order,
                                                               float* __restrict__ y) {
  __shared__ float s_val[GR_BLOCK / 64][64];
  const int cell = blockIdx.x, lane = threadIdx.x & 63, ch = blockIdx.y * 64 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  int a, b;
  gr_cell_range(cell_start, cell, n_cells, T, &a, &b);
  const int n = b - a;
  float acc = 0.0f;
  if (n > 0) ghr_walk(order, ghr_part(a, n, w), ghr_part(a, n, w + 1), [&](int p) { return on ? x[(size_t)p * xs + ch] : 0.0f; },
                      [&](int, float v) { acc += v; });
  s_val[w][lane] = acc;
  __syncthreads();
  if (w == 0 && on) y[(size_t)cell * C + ch] = ((s_val[0][lane] + s_val[1][lane]) + s_val[2][lane]) + s_val[3][lane];
}

__global__ __launch_bounds__(GR_BLOCK) void gr_cell_max_kernel(const float* __restrict__ x, long long xs, int T, int C,
                                                               const int* __restrict__ cell_start, const int* __restrict__ order,
                                                               float* __restrict__ vals, int* __restrict__ argmax) {
  __shared__ float s_val[GR_BLOCK / 64][64];
  __shared__ int s_arg[GR_BLOCK / 64][64];
  const int cell = blockIdx.x, lane = threadIdx.x & 63, ch = blockIdx.y * 64 + lane;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  const int a = cell_start[cell], n = cell_start[cell + 1] - a;
  float acc = 0.0f;
  int arg = T;
  // strict >: the first of equal values stays; v == v: a NaN is never taken, so a quarter of NaNs alone keeps arg == T (gh_pool.hip)
  if (n > 0) ghr_walk(order, ghr_part(a, n, w), ghr_part(a, n, w + 1), [&](int p) { return on ? x[(size_t)p * xs + ch] : 0.0f; },
                      [&](int p, float v) { if (v == v && (arg == T || v > acc)) { acc = v; arg = p; } });
  s_val[w][lane] = acc;
  s_arg[w][lane] = arg;
  __syncthreads();
  if (w != 0 || !on) return;
  float r = s_val[0][lane];
  int ra = s_arg[0][lane];
#pragma unroll
  for (int q = 1; q < GR_BLOCK / 64; ++q) {
    const float v = s_val[q][lane];
    const int va = s_arg[q][lane];
    if (va != T && (ra == T || v > r)) { r = v; ra = va; }
  }
  vals[(size_t)cell * C + ch] = ra == T ? 0.0f : r;
  argmax[(size_t)cell * C + ch] = ra;
}

__global__ __launch_bounds__(GR_BLOCK) void gr_cell_max_bwd_kernel(const float* __restrict__ gm, const int* __restrict__ argmax, int T, int C,
                                                                   long long total, float* __restrict__ gx, long long gxs) {
  const long long i = (long long)blockIdx.x * GR_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int am = argmax[i], ch = (int)(i % C);
  if (am >= 0 && am < T) gx[(size_t)am * gxs + ch] += gm[i];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static inline int gr_vec(const void* p, long long stride) { return ghr_al16(p) && stride % 4 == 0; }

static bool gr_dims_ok(int T, int Cin, int H) {
  return T >= 0 && (H == 32 || H == 64 || H == 96 || H == 128) && (Cin == H || Cin == 2 * H);
}

extern "C" int gh_res_forward(const float* x, int64_t x_stride, int T, int Cin, int H, const float* u, const float* s, int R,
                              const int32_t* row_of, const float* W0, int64_t w0_stride, const float* Ws, int64_t ws_stride,
                              const float* W1, float* out, int64_t out_stride, uint32_t* mask, void* hip_stream) {
  if (!gr_dims_ok(T, Cin, H) || R < 1) return GH_ERR_INVALID_ARG;
  if (!x || !u || !s || !W0 || !Ws || !W1 || !out) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(x) || !ghr_al4(u) || !ghr_al4(s) || !ghr_al4(W0) || !ghr_al4(Ws) || !ghr_al4(W1) || !ghr_al4(out) || !ghr_al4(row_of) ||
      !ghr_al4(mask))
    return GH_ERR_INVALID_ARG;
  if (x_stride < Cin || w0_stride < Cin || ws_stride < Cin || out_stride < H) return GH_ERR_INVALID_ARG;
  if (T == 0) return GH_OK;
  GrFwd a;
  a.x = x; a.u = u; a.s = s; a.W0 = W0; a.Ws = Ws; a.W1 = W1; a.row_of = row_of; a.out = out; a.mask = mask;
  a.x_stride = x_stride; a.w0_stride = w0_stride; a.ws_stride = ws_stride; a.out_stride = out_stride;
  a.T = T; a.Cin = Cin; a.R = R;
  a.vec_w0 = gr_vec(W0, w0_stride); a.vec_ws = gr_vec(Ws, ws_stride); a.vec_w1 = gr_vec(W1, H); a.vec_out = gr_vec(out, out_stride);
  const dim3 grid((unsigned)(((long long)T + GH_RES_ROWS - 1) / GH_RES_ROWS));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  ghr_tiles(H / 32, [&](auto nt) { hipLaunchKernelGGL(gr_forward_kernel<nt()>, grid, dim3(GR_BLOCK), 0, st, a); });
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_res_backward(const float* g, int64_t g_stride, const float* x, int64_t x_stride, int T, int Cin, int H,
                               const uint32_t* mask, const float* W0, int64_t w0_stride, const float* Ws, int64_t ws_stride,
                               const float* W1, float* dx, int64_t dx_stride, float* dh, void* hip_stream) {
  if (!gr_dims_ok(T, Cin, H)) return GH_ERR_INVALID_ARG;
  if (!g || !x || !mask || !W0 || !Ws || !W1 || !dx) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(g) || !ghr_al4(x) || !ghr_al4(mask) || !ghr_al4(W0) || !ghr_al4(Ws) || !ghr_al4(W1) || !ghr_al4(dx) || !ghr_al4(dh))
    return GH_ERR_INVALID_ARG;
  if (g_stride < H || x_stride < Cin || w0_stride < Cin || ws_stride < Cin || dx_stride < Cin) return GH_ERR_INVALID_ARG;
  if (T == 0) return GH_OK;
  GrBwd a;
  a.g = g; a.x = x; a.W0 = W0; a.Ws = Ws; a.W1 = W1; a.mask = mask; a.dx = dx; a.dh = dh;
  a.g_stride = g_stride; a.x_stride = x_stride; a.w0_stride = w0_stride; a.ws_stride = ws_stride; a.dx_stride = dx_stride;
  a.T = T; a.Cin = Cin;
  a.vec_w0 = gr_vec(W0, w0_stride); a.vec_ws = gr_vec(Ws, ws_stride); a.vec_w1 = gr_vec(W1, H); a.vec_dx = gr_vec(dx, dx_stride);
  a.vec_dh = dh ? gr_vec(dh, H) : 0;
  const dim3 grid((unsigned)(((long long)T + GH_RES_ROWS - 1) / GH_RES_ROWS));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  ghr_tiles(H / 32, [&](auto nt) { hipLaunchKernelGGL(gr_backward_kernel<nt()>, grid, dim3(GR_BLOCK), 0, st, a); });
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

static int gr_cells_ok(int T, int C, int n_cells, const void* cell_start, const void* order) {
  if (T < 0 || C < 1 || n_cells < 1 || !cell_start || !order || !ghr_al4(cell_start) || !ghr_al4(order)) return GH_ERR_INVALID_ARG;
  if (n_cells > GH_POOL_MAX_CELLS || (C + 63) / 64 > 65535) return GH_ERR_UNSUPPORTED;
  return GH_OK;
}

extern "C" int gh_res_cell_sum(const float* x, int64_t x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                               const int32_t* order, int tail, float* y, void* hip_stream) {
  const int rc = gr_cells_ok(T, C, n_cells, cell_start, order);
  if (rc != GH_OK) return rc;
  if (!x || !y || !ghr_al4(x) || !ghr_al4(y) || x_stride < C) return GH_ERR_INVALID_ARG;
  if (T == 0) return GH_OK;
  (void)hipGetLastError();
  const dim3 grid((unsigned)(n_cells + (tail ? 1 : 0)), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(gr_cell_sum_kernel, grid, dim3(GR_BLOCK), 0, (hipStream_t)hip_stream, x, (long long)x_stride, T, C, n_cells, cell_start,
                     order, y);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_res_cell_max(const float* x, int64_t x_stride, int T, int C, int n_cells, const int32_t* cell_start,
                               const int32_t* order, float* vals, int32_t* argmax, void* hip_stream) {
  const int rc = gr_cells_ok(T, C, n_cells, cell_start, order);
  if (rc != GH_OK) return rc;
  if (!x || !vals || !argmax || !ghr_al4(x) || !ghr_al4(vals) || !ghr_al4(argmax) || x_stride < C) return GH_ERR_INVALID_ARG;
  if (T == 0) return GH_OK;
  (void)hipGetLastError();
  const dim3 grid((unsigned)n_cells, (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(gr_cell_max_kernel, grid, dim3(GR_BLOCK), 0, (hipStream_t)hip_stream, x, (long long)x_stride, T, C, cell_start, order,
                     vals, argmax);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_res_cell_max_backward(const float* gm, const int32_t* argmax, int T, int C, int n_cells, float* grad_x,
                                        int64_t gx_stride, void* hip_stream) {
  if (T < 0 || C < 1 || n_cells < 1 || !gm || !argmax || !grad_x || !ghr_al4(gm) || !ghr_al4(argmax) || !ghr_al4(grad_x) || gx_stride < C)
    return GH_ERR_INVALID_ARG;
  if (T == 0) return GH_OK;
  const long long total = (long long)n_cells * C;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gr_cell_max_bwd_kernel, dim3((unsigned)((total + GR_BLOCK - 1) / GR_BLOCK)), dim3(GR_BLOCK), 0, (hipStream_t)hip_stream,
                     gm, argmax, T, C, total, grad_x, (long long)gx_stride);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
