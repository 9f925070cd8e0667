// gh_attn.hip — the interaction attention's core (include/gh_attn.h): streaming softmax over key tiles, forward and backward, on the
// exact float32 MFMA. No V x V array, no atomics, no workgroup that waits for another.
//
// One product shape serves every kernel: v_mfma_f32_32x32x2_f32, D[i][j] = fma chain over k of A[i][k] * B[k][j].
//   operands   lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: one float each.
//   result     lane l holds column j = l & 31; its register r holds row ghr_acc_row(r, l >> 5) (gh_rows.h's "columns").
// So a result X is the B operand of a product that sums over X's rows with no lane movement: step r of that product takes register r
// and the A operand's k is row ghr_acc_row(r, l >> 5). The owner of a workgroup's rows (queries in the forward and the dq kernel,
// keys in the dk/dv kernel) is therefore kept on the lane in every first product, and the swept rows come from LDS.
//   forward    S^T = K Q^T  (keys x queries), P^T = softmax part, O^T += V^T P^T
//   dk, dv     S = Q K^T, dP = dO V^T (queries x keys), dV^T += dO^T P, dK^T += Q^T dS
//   dq         S^T = K Q^T, dP^T = V dO^T (keys x queries), dQ^T += K^T dS^T
// LDS tiles have the odd pitch 33: a column read (lane = row) is conflict free, a row read (lane = column, the two lane halves four
// rows apart) is two-way at worst. Results leave through LDS transposed, so that every store instruction writes whole 128-byte runs.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_attn.h"
#include "../csrc_rows/gh_rows.h"

#define GA_D GH_ATTN_D
#define GA_ROWS 32                 // rows per wave: the MFMA's 32 columns
#define GA_BLOCK_ROWS 128          // rows per workgroup (4 waves)
#define GA_STAGE 64                // rows of the swept operand staged per barrier pair (forward, dq)
#define GA_PITCH 33

static_assert(GHR_BLOCK == 256 && GA_BLOCK_ROWS == (GHR_BLOCK / 64) * GA_ROWS, "four waves of 32 rows; ghr_stage strides by GHR_BLOCK");
static_assert(GA_D == 32, "one 32x32 tile holds a head");
static_assert(2 * GA_STAGE * GA_PITCH >= 4 * GA_ROWS * GA_PITCH, "the stage doubles as the four waves' transpose tiles");

__device__ __forceinline__ ghr_acc ga_zero() {
  ghr_acc z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// reg[s] = x[row][2 s + half], s = 0 .. 15: the lane's share of its own row as the B operand of a product over d. Zeros past nrows.
__device__ __forceinline__ void ga_load_own(float (&reg)[16], const float* __restrict__ x, long long stride, long long row, int nrows,
                                            int half) {
#pragma unroll
  for (int s = 0; s < 16; ++s) reg[s] = row < nrows ? x[row * stride + 2 * s + half] : 0.f;
}

// X = T Own^T: rows of the LDS tile t (from local row r0) against the lane's own row. X[tile row][own row on the lane].
__device__ __forceinline__ ghr_acc ga_tile_times_own(const float* t, int r0, const float (&own)[16], int col, int half) {
  ghr_acc x = ga_zero();
  const float* a = t + (r0 + col) * GA_PITCH + half;
#pragma unroll
  for (int s = 0; s < 16; ++s) x = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], own[s], x, 0, 0, 0);
  return x;
}

// Y += T^T X: X's rows (register r = tile row ghr_acc_row(r, half)) are summed against the tile's rows read along d. Y[d][own row on the lane].
__device__ __forceinline__ ghr_acc ga_tile_t_times(ghr_acc y, const float* t, int r0, const float (&x)[16], int col, int half) {
#pragma unroll
  for (int r = 0; r < 16; ++r) y = __builtin_amdgcn_mfma_f32_32x32x2f32(t[(r0 + ghr_acc_row(r, half)) * GA_PITCH + col], x[r], y, 0, 0, 0);
  return y;
}

// y holds [d][own row on the lane] of the wave's 32 rows from row0; dst is (.., V, H * 32) contiguous at this (batch, head). The tile
// crosses the wave's LDS region so that each half-wave stores one row of 32 floats. Every thread of the workgroup calls this.
__device__ __forceinline__ void ga_store_rows(float* region, const ghr_acc& y, float* __restrict__ dst, long long dst_stride, long long row0,
                                              int V, int col, int half) {
  __syncthreads();                                             // the stage this region overlays has been read by every wave
#pragma unroll
  for (int r = 0; r < 16; ++r) region[col * GA_PITCH + ghr_acc_row(r, half)] = y[r];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int row = 2 * it + half;
    if (row0 + row < V) dst[(row0 + row) * dst_stride + col] = region[row * GA_PITCH + col];
  }
}

struct GaView {                                                // one (batch, head) of a GhAttnTensor
  const float* p;
  long long stride;
  int vec;
};

__device__ __forceinline__ GaView ga_view(const GhAttnTensor& t, int vec, int b, int h) {
  GaView w;
  w.p = t.p + (long long)b * t.stride_b + (long long)h * t.stride_h;
  w.stride = t.stride_v;
  w.vec = vec;
  return w;
}

__device__ __forceinline__ void ga_stage(float* s, const GaView& x, int row0, int R, int V, int tid) {
  ghr_stage(s, GA_PITCH, x.p, x.stride, row0, R, V - row0, 0, GA_D, x.vec, tid);
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void ga_forward_kernel(GhAttnTensor q, GhAttnTensor k, GhAttnTensor v, int vec_k, int vec_v,
                                                                float* __restrict__ out, float* __restrict__ lse, int V, int H, float norm) {
  __shared__ float s_stage[2 * GA_STAGE * GA_PITCH];
  float* s_k = s_stage;
  float* s_v = s_stage + GA_STAGE * GA_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long long row0 = (long long)blockIdx.x * GA_BLOCK_ROWS + wave * GA_ROWS, row = row0 + col;
  const GaView qv = ga_view(q, 0, b, h), kv = ga_view(k, vec_k, b, h), vv = ga_view(v, vec_v, b, h);

  float qr[16];
  ga_load_own(qr, qv.p, qv.stride, row, V, half);
  ghr_acc o = ga_zero();
  float m = -INFINITY, l = 0.f;

  for (int kt = 0; kt < V; kt += GA_STAGE) {
    __syncthreads();
    ga_stage(s_k, kv, kt, GA_STAGE, V, tid);
    ga_stage(s_v, vv, kt, GA_STAGE, V, tid);
    __syncthreads();
    for (int sub = 0; sub < GA_STAGE && kt + sub < V; sub += GA_ROWS) {
      const ghr_acc st = ga_tile_times_own(s_k, sub, qr, col, half);
      float p[16];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = kt + sub + ghr_acc_row(r, half) < V ? st[r] / norm : -INFINITY;
        mx = fmaxf(mx, p[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m, mx);                        // finite: the tile holds at least one key
      const float alpha = expf(m - m_new);
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = expf(p[r] - m_new);
        sum += p[r];
      }
      sum += __shfl_xor(sum, 32);
      l = l * alpha + sum;
      m = m_new;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
      o = ga_tile_t_times(o, s_v, sub, p, col, half);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = o[r] / l;
  if (half == 0 && row < V) lse[(long long)bh * V + row] = m + logf(l);
  ga_store_rows(s_stage + wave * GA_ROWS * GA_PITCH, o, out + (long long)b * V * H * GA_D + h * GA_D, (long long)H * GA_D, row0, V, col, half);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// delta[bh][row] = dot(dout[row], out[row]): one thread per row, one ascending fmaf chain.
__global__ __launch_bounds__(GHR_BLOCK) void ga_delta_kernel(GhAttnTensor dout, const float* __restrict__ out, float* __restrict__ delta,
                                                              int V, int H) {
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long long row = (long long)blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (row >= V) return;
  const float* g = dout.p + (long long)b * dout.stride_b + (long long)h * dout.stride_h + row * dout.stride_v;
  const float* o = out + ((long long)b * V + row) * H * GA_D + h * GA_D;
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < GA_D; ++d) acc = fmaf(g[d], o[d], acc);
  delta[(long long)bh * V + row] = acc;
}

// One workgroup per 128 keys: sweeps the query tiles in ascending order, owns dk and dv of its keys.
__global__ __launch_bounds__(GHR_BLOCK) void ga_backward_kv_kernel(GhAttnTensor q, GhAttnTensor k, GhAttnTensor v, GhAttnTensor dout,
                                                                    int vec_q, int vec_g, const float* __restrict__ lse,
                                                                    const float* __restrict__ delta, float* __restrict__ dk,
                                                                    float* __restrict__ dv, int V, int H, float norm) {
  __shared__ float s_stage[2 * GA_STAGE * GA_PITCH];
  __shared__ float s_lse[GA_ROWS], s_delta[GA_ROWS];
  float* s_q = s_stage;
  float* s_g = s_stage + GA_STAGE * GA_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long long row0 = (long long)blockIdx.x * GA_BLOCK_ROWS + wave * GA_ROWS, row = row0 + col;   // the lane's key
  const GaView qv = ga_view(q, vec_q, b, h), kv = ga_view(k, 0, b, h), vv = ga_view(v, 0, b, h), gv = ga_view(dout, vec_g, b, h);

  float kr[16], vr[16];
  ga_load_own(kr, kv.p, kv.stride, row, V, half);
  ga_load_own(vr, vv.p, vv.stride, row, V, half);
  ghr_acc dkt = ga_zero(), dvt = ga_zero();

  for (int qt = 0; qt < V; qt += GA_ROWS) {
    __syncthreads();
    ga_stage(s_q, qv, qt, GA_ROWS, V, tid);
    ga_stage(s_g, gv, qt, GA_ROWS, V, tid);
    if (tid < GA_ROWS) {
      const bool in = qt + tid < V;
      s_lse[tid] = in ? lse[(long long)bh * V + qt + tid] : 0.f;
      s_delta[tid] = in ? delta[(long long)bh * V + qt + tid] : 0.f;
    }
    __syncthreads();
    const ghr_acc s = ga_tile_times_own(s_q, 0, kr, col, half);   // [query][key on the lane]
    const ghr_acc dp = ga_tile_times_own(s_g, 0, vr, col, half);
    float p[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ghr_acc_row(r, half);
      p[r] = (qt + i < V && row < V) ? expf(s[r] / norm - s_lse[i]) : 0.f;
      ds[r] = (p[r] * (dp[r] - s_delta[i])) / norm;
    }
    dvt = ga_tile_t_times(dvt, s_g, 0, p, col, half);
    dkt = ga_tile_t_times(dkt, s_q, 0, ds, col, half);
  }
  float* region = s_stage + wave * GA_ROWS * GA_PITCH;
  const long long base = (long long)b * V * H * GA_D + h * GA_D;
  if (dk) ga_store_rows(region, dkt, dk + base, (long long)H * GA_D, row0, V, col, half);
  if (dv) ga_store_rows(region, dvt, dv + base, (long long)H * GA_D, row0, V, col, half);
}

// One workgroup per 128 queries: sweeps the key tiles in ascending order, owns dq of its queries.
__global__ __launch_bounds__(GHR_BLOCK) void ga_backward_q_kernel(GhAttnTensor q, GhAttnTensor k, GhAttnTensor v, GhAttnTensor dout,
                                                                   int vec_k, int vec_v, const float* __restrict__ lse,
                                                                   const float* __restrict__ delta, float* __restrict__ dq, int V, int H,
                                                                   float norm) {
  __shared__ float s_stage[2 * GA_STAGE * GA_PITCH];
  float* s_k = s_stage;
  float* s_v = s_stage + GA_STAGE * GA_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long long row0 = (long long)blockIdx.x * GA_BLOCK_ROWS + wave * GA_ROWS, row = row0 + col;   // the lane's query
  const GaView qv = ga_view(q, 0, b, h), kv = ga_view(k, vec_k, b, h), vv = ga_view(v, vec_v, b, h), gv = ga_view(dout, 0, b, h);

  float qr[16], gr[16];
  ga_load_own(qr, qv.p, qv.stride, row, V, half);
  ga_load_own(gr, gv.p, gv.stride, row, V, half);
  const float lse_q = row < V ? lse[(long long)bh * V + row] : 0.f;
  const float delta_q = row < V ? delta[(long long)bh * V + row] : 0.f;
  ghr_acc dqt = ga_zero();

  for (int kt = 0; kt < V; kt += GA_STAGE) {
    __syncthreads();
    ga_stage(s_k, kv, kt, GA_STAGE, V, tid);
    ga_stage(s_v, vv, kt, GA_STAGE, V, tid);
    __syncthreads();
    for (int sub = 0; sub < GA_STAGE && kt + sub < V; sub += GA_ROWS) {
      const ghr_acc st = ga_tile_times_own(s_k, sub, qr, col, half);   // [key][query on the lane]
      const ghr_acc dpt = ga_tile_times_own(s_v, sub, gr, col, half);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = kt + sub + ghr_acc_row(r, half) < V ? expf(st[r] / norm - lse_q) : 0.f;
        ds[r] = (p * (dpt[r] - delta_q)) / norm;
      }
      dqt = ga_tile_t_times(dqt, s_k, sub, ds, col, half);
    }
  }
  ga_store_rows(s_stage + wave * GA_ROWS * GA_PITCH, dqt, dq + (long long)b * V * H * GA_D + h * GA_D, (long long)H * GA_D, row0, V, col, half);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// GH_OK with *empty set when there is nothing to launch.
static int ga_check_dims(const GhAttnDims* d, bool* empty) {
  *empty = true;
  if (!d || d->BS < 0 || d->V < 0 || d->H < 1 || d->D < 1) return GH_ERR_INVALID_ARG;
  if (!(d->norm > 0.f) || !isfinite(d->norm)) return GH_ERR_INVALID_ARG;
  if (d->D != GH_ATTN_D) return GH_ERR_UNSUPPORTED;
  if ((long long)d->BS * d->H > GH_ATTN_MAX_BH || d->V > GH_ATTN_MAX_V) return GH_ERR_UNSUPPORTED;
  *empty = d->BS == 0 || d->V == 0;
  return GH_OK;
}

static int ga_check_tensor(const GhAttnTensor* t) {
  if (!t || !t->p || !ghr_al4(t->p)) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

static int ga_vec(const GhAttnTensor* t) {
  return ghr_al16(t->p) && t->stride_b % 4 == 0 && t->stride_v % 4 == 0 && t->stride_h % 4 == 0;
}

extern "C" size_t gh_attn_workspace_bytes(const GhAttnDims* dims) {
  bool empty;
  if (ga_check_dims(dims, &empty) != GH_OK || empty) return 0;
  return ghr_align((size_t)dims->BS * dims->H * (size_t)dims->V * sizeof(float));
}

extern "C" int gh_attn_forward(const GhAttnDims* dims, const GhAttnTensor* q, const GhAttnTensor* k, const GhAttnTensor* v, float* out,
                               float* lse, void* hip_stream) {
  bool empty;
  const int rc = ga_check_dims(dims, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  if (ga_check_tensor(q) || ga_check_tensor(k) || ga_check_tensor(v) || !out || !lse || !ghr_al4(out) || !ghr_al4(lse)) return GH_ERR_INVALID_ARG;
  const dim3 grid((unsigned)((dims->V + GA_BLOCK_ROWS - 1) / GA_BLOCK_ROWS), (unsigned)(dims->BS * dims->H));
  (void)hipGetLastError();
  hipLaunchKernelGGL(ga_forward_kernel, grid, dim3(GHR_BLOCK), 0, (hipStream_t)hip_stream, *q, *k, *v, ga_vec(k), ga_vec(v), out, lse,
                     dims->V, dims->H, dims->norm);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_attn_backward(const GhAttnDims* dims, const GhAttnTensor* q, const GhAttnTensor* k, const GhAttnTensor* v,
                                const float* out, const float* lse, const GhAttnTensor* dout, float* dq, float* dk, float* dv,
                                void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = ga_check_dims(dims, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  if (ga_check_tensor(q) || ga_check_tensor(k) || ga_check_tensor(v) || ga_check_tensor(dout)) return GH_ERR_INVALID_ARG;
  if (!out || !lse || !ghr_al4(out) || !ghr_al4(lse) || !ghr_al4(dq) || !ghr_al4(dk) || !ghr_al4(dv)) return GH_ERR_INVALID_ARG;
  if (!dq && !dk && !dv) return GH_OK;
  if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_attn_workspace_bytes(dims)) return GH_ERR_WORKSPACE_SMALL;
  float* delta = (float*)workspace;
  hipStream_t s = (hipStream_t)hip_stream;
  const int V = dims->V, H = dims->H;
  const unsigned bh = (unsigned)(dims->BS * H);
  (void)hipGetLastError();
  hipLaunchKernelGGL(ga_delta_kernel, dim3((unsigned)((V + GHR_BLOCK - 1) / GHR_BLOCK), bh), dim3(GHR_BLOCK), 0, s, *dout, out, delta, V, H);
  if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  const dim3 grid((unsigned)((V + GA_BLOCK_ROWS - 1) / GA_BLOCK_ROWS), bh);
  if (dk || dv) {
    hipLaunchKernelGGL(ga_backward_kv_kernel, grid, dim3(GHR_BLOCK), 0, s, *q, *k, *v, *dout, ga_vec(q), ga_vec(dout), lse, delta, dk, dv, V,
                       H, dims->norm);
    if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  }
  if (dq) {
    hipLaunchKernelGGL(ga_backward_q_kernel, grid, dim3(GHR_BLOCK), 0, s, *q, *k, *v, *dout, ga_vec(k), ga_vec(v), lse, delta, dq, V, H,
                       dims->norm);
    if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  }
  return GH_OK;
}
