// gh_xf.hip — the Transformer1D backbones' forward (include/gh_xf.h): the LDS-tiled product with its prologues and epilogues, the
// LayerNorm and GroupNorm moments, the streaming-softmax attention for D = 32 and 64, and the host loop that enqueues a whole
// backbone; behind them the backward to the input for frozen weights (the taped forward is the same host loop with other pointers;
// the attention's, the GEGLU's and the norms' backward kernels, the host loop in reverse), and behind that the parameters' gradients
// (the backward-weight product with its join, the norms' two-stage column sums; the same host loop enqueues them beside each step).
// Exact float32 MFMA, no atomics, no workgroup that waits for another.
//
// The product shape is gh_rows.h's "columns" turned round: v_mfma_f32_32x32x2_f32 with the ROW of X as the A operand's i and the
// output channel as the B operand's j, so that lane l holds channel j = l & 31 of the rows ghr_acc_row(r, l >> 5) and a register's
// store is a 128-byte run of one output row per half wave. Both operands cross LDS at the odd pitch 33: lane = row of the tile
// reads without a bank conflict. The attention keeps gh_attn.hip's shape (the query on the lane, keys and values from LDS).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_xf.h"
#include "../csrc_rows/gh_rows.h"

#define GX_TR GH_XF_ROWS
#define GX_TC GH_XF_COLS
#define GX_KS 32                   // columns of X and W per slab
#define GX_P 33                    // LDS pitch of a slab
#define GX_LN_ROWS (GHR_BLOCK / 64)  // rows per workgroup of the LayerNorm moments: one wave each

static_assert(GHR_BLOCK == 256 && GX_TR == 64 && GX_TC == 64, "four waves, 2 x 2 tiles of 32 x 32; GhrSlab<2, 8> is 64 rows x 32 columns");
static_assert(GH_XF_GN_CHUNK == GHR_BLOCK, "one position per thread in stage one of the group moments");
static_assert(GH_XF_ATTN_ROWS == 64 && GH_XF_ATTN_KEYS == 64, "two waves per 32 queries, one per 32 keys of a stage");

__device__ __forceinline__ ghr_acc gx_splat(float v) {
  ghr_acc z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = v;
  return z;
}

// the 64 lanes' shares in the fixed order xor 32, 16, 8, 4, 2, 1: every lane ends with the same sum
__device__ __forceinline__ float gx_wave_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  return s;
}

// ---- LayerNorm moments: one wave per row -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_row_moments_kernel(const float* __restrict__ x, long long stride, int T, int K, float eps,
                                                                    float* __restrict__ mom) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * GX_LN_ROWS + wave;
  if (row >= T) return;                                        // wave-uniform; the kernel has no barrier
  const float* xr = x + row * stride;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += xr[k];
  const float mean = gx_wave_sum(s) / (float)K;
  float q = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float d = xr[k] - mean;
    q = fmaf(d, d, q);
  }
  const float m2 = gx_wave_sum(q);
  if (lane == 0) {
    mom[2 * row] = mean;
    mom[2 * row + 1] = 1.0f / sqrtf(m2 / (float)K + eps);
  }
}

// ---- GroupNorm moments -----------------------------------------------------------------------------------------------------------
// the workgroup's sum of one value per thread: the wave butterfly, then (s0 + s1) + (s2 + s3). Two barriers; every thread calls it.
__device__ __forceinline__ float gx_block_sum(float v, float* s_red) {
  const float w = gx_wave_sum(v);
  __syncthreads();                                             // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = w;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_group_part_kernel(const float* __restrict__ x, long long stride_b, long long stride_c, int N,
                                                                   int G, int cpg, int nchunks, float* __restrict__ part) {
  __shared__ float s_red[4];
  const int chunk = blockIdx.x % nchunks, bg = blockIdx.x / nchunks, b = bg / G, g = bg - b * G;
  const int n = chunk * GH_XF_GN_CHUNK + threadIdx.x;
  const int len = N - chunk * GH_XF_GN_CHUNK < GH_XF_GN_CHUNK ? N - chunk * GH_XF_GN_CHUNK : GH_XF_GN_CHUNK;
  const float* xp = x + (long long)b * stride_b + (long long)g * cpg * stride_c + n;
  const bool live = n < N;
  float s = 0.f;
  if (live) {
    for (int c = 0; c < cpg; ++c) s += xp[c * stride_c];
  }
  const float mean = gx_block_sum(s, s_red) / ((float)cpg * (float)len);
  float q = 0.f;
  if (live) {
    for (int c = 0; c < cpg; ++c) {
      const float d = xp[c * stride_c] - mean;
      q = fmaf(d, d, q);
    }
  }
  const float m2 = gx_block_sum(q, s_red);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = mean;
    part[2 * (long long)blockIdx.x + 1] = m2;
  }
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_group_join_kernel(const float* __restrict__ part, int BG, int N, int cpg, int nchunks,
                                                                   float* __restrict__ mom) {
  const int bg = blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (bg >= BG) return;
  const float* p = part + 2 * (long long)bg * nchunks;
  float mean = p[0], m2 = p[1];
  float na = (float)cpg * (float)(N < GH_XF_GN_CHUNK ? N : GH_XF_GN_CHUNK);
  for (int c = 1; c < nchunks; ++c) {
    const int len = N - c * GH_XF_GN_CHUNK < GH_XF_GN_CHUNK ? N - c * GH_XF_GN_CHUNK : GH_XF_GN_CHUNK;
    const float nc = (float)cpg * (float)len, n = na + nc, delta = p[2 * c] - mean;
    mean = mean + (delta * nc) / n;
    m2 = (m2 + p[2 * c + 1]) + ((delta * delta) * na) * nc / n;
    na = n;
  }
  mom[2 * bg] = mean;
  mom[2 * bg + 1] = m2;
}

// ---- the product ---------------------------------------------------------------------------------------------------------------------
// One slab of X on its way into LDS. PRO_NONE and PRO_LN: gh_rows.h's window, element (r, c) = X[row0 + r][k0 + c], thread i moves
// rows i / 8 and (i + 256) / 8. PRO_GN: X is channel first, so consecutive threads take consecutive rows: thread i owns tile row
// i & 63 and the wave-uniform columns (i >> 6) + 4 it. PRO_CF: the same read, no norm.
template <int PRO>
constexpr bool gx_cf = PRO == GH_XF_PRO_GN || PRO == GH_XF_PRO_CF;

template <int PRO>
struct GxSlabX {
  GhrSlab<2, 8> w;
  float g[8];
};

template <int PRO>
__device__ __forceinline__ void gx_fetch_x(GxSlabX<PRO>& t, const GhXfLinear& a, int row0, int k0, int vec, long long gn_base, bool gn_live,
                                           int tid) {
  if constexpr (gx_cf<PRO>) {
#pragma unroll
    for (int it = 0; it < 8; ++it) t.g[it] = gn_live ? a.x[gn_base + (long long)(k0 + (tid >> 6) + 4 * it) * a.x_stride] : 0.f;
  } else {
    ghr_fetch_in(t.w, a.x, a.x_stride, row0, k0, a.T, a.K, vec, tid);
  }
}

// what gx_fetch_x brought, through the prologue, into s_x. ln: {mean, rstd} of the thread's two rows; gn_mom: the thread's batch
// element's moments.
template <int PRO>
__device__ __forceinline__ void gx_put_x(const GxSlabX<PRO>& t, float* s_x, const GhXfLinear& a, int k0, const float (&ln)[2][2],
                                         const float* __restrict__ gn_mom, int cpg, float gn_cnt, int tid) {
  if constexpr (PRO == GH_XF_PRO_CF) {
#pragma unroll
    for (int it = 0; it < 8; ++it) s_x[(tid & 63) * GX_P + (tid >> 6) + 4 * it] = t.g[it];
  } else if constexpr (PRO == GH_XF_PRO_GN) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int kk = (tid >> 6) + 4 * it, c = k0 + kk, g = c / cpg;
      const float mean = gn_mom ? gn_mom[2 * g] : 0.f, m2 = gn_mom ? gn_mom[2 * g + 1] : 0.f;
      const float rstd = 1.0f / sqrtf(m2 / gn_cnt + a.eps);
      s_x[(tid & 63) * GX_P + kk] = ((t.g[it] - mean) * rstd) * a.gamma[c] + a.beta[c];
    }
  } else {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + it * GHR_BLOCK, r = i / 8, c = 4 * (i % 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = t.w.v[it][j];
        if constexpr (PRO == GH_XF_PRO_LN) v = ((v - ln[it][0]) * ln[it][1]) * a.gamma[k0 + c + j] + a.beta[k0 + c + j];
        s_x[r * GX_P + c + j] = v;
      }
    }
  }
}

template <int PRO, int EPI>
__global__ __launch_bounds__(GHR_BLOCK) void gx_linear_kernel(GhXfLinear a, const float* __restrict__ ln_mom, int vec_x, int vec_w,
                                                               int ncol_tiles) {
  constexpr int NB = EPI == GH_XF_EPI_GEGLU ? 2 : 1;
  __shared__ float s_all[GX_TR * GX_P + NB * GX_TC * GX_P];    // X slab, NB W slabs; the channel-first epilogue's four 32 x 33 tiles
  static_assert(GX_TR * GX_P + GX_TC * GX_P >= 4 * 32 * GX_P, "the slabs double as the four waves' transpose tiles");
  float* s_x = s_all;
  float* s_w = s_all + GX_TR * GX_P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int tc = blockIdx.x % ncol_tiles, tr = blockIdx.x / ncol_tiles;
  const int row0 = tr * GX_TR, c0 = tc * GX_TC;
  const int N = a.rows_per_batch;

  float ln[2][2] = {{0.f, 1.f}, {0.f, 1.f}};
  if constexpr (PRO == GH_XF_PRO_LN) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r = row0 + (tid + it * GHR_BLOCK) / 8;
      if (r < a.T) {
        ln[it][0] = ln_mom[2 * (long long)r];
        ln[it][1] = ln_mom[2 * (long long)r + 1];
      }
    }
  }
  long long gn_base = 0;
  bool gn_live = false;
  const float* gn_mom = nullptr;
  int cpg = 1;
  float gn_cnt = 1.f;
  if constexpr (gx_cf<PRO>) {
    const int t = row0 + (tid & 63);
    gn_live = t < a.T;
    const int b = gn_live ? t / N : 0, n = gn_live ? t - b * N : 0;
    gn_base = (long long)b * a.x_stride_b + n;
    if constexpr (PRO == GH_XF_PRO_GN) {
      cpg = a.K / a.groups;
      gn_cnt = (float)cpg * (float)N;
      gn_mom = gn_live ? a.moments + 2 * (long long)b * a.groups : nullptr;
    }
  }

  const int j = c0 + 32 * wc + col;                            // the lane's output channel
  ghr_acc acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float bv = 0.f;
    if (EPI != GH_XF_EPI_PLAIN && a.bias && j < a.N_out) bv = a.bias[(long long)b * a.N_out + j];
    acc[b] = gx_splat(bv);
  }

  GxSlabX<PRO> xs;
  GhrSlab<2, 8> ws[NB];
  gx_fetch_x<PRO>(xs, a, row0, 0, vec_x, gn_base, gn_live, tid);
#pragma unroll
  for (int b = 0; b < NB; ++b) ghr_fetch_in(ws[b], a.w + (long long)b * a.N_out * a.K, a.K, c0, 0, a.N_out, a.K, vec_w, tid);
  for (int k0 = 0; k0 < a.K; k0 += GX_KS) {
    __syncthreads();                                           // the previous slab has been read by every wave
    gx_put_x<PRO>(xs, s_x, a, k0, ln, gn_mom, cpg, gn_cnt, tid);
#pragma unroll
    for (int b = 0; b < NB; ++b) ghr_put(ws[b], s_w + b * GX_TC * GX_P, GX_P, tid);
    __syncthreads();
    if (k0 + GX_KS < a.K) {                                    // the next slab's loads fly under this slab's products
      gx_fetch_x<PRO>(xs, a, row0, k0 + GX_KS, vec_x, gn_base, gn_live, tid);
#pragma unroll
      for (int b = 0; b < NB; ++b) ghr_fetch_in(ws[b], a.w + (long long)b * a.N_out * a.K, a.K, c0, k0 + GX_KS, a.N_out, a.K, vec_w, tid);
    }
    const float* ap = s_x + (32 * wr + col) * GX_P + half;
    const float* bp = s_w + (32 * wc + col) * GX_P + half;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float av = ap[2 * s];
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[b * GX_TC * GX_P + 2 * s], acc[b], 0, 0, 0);
    }
  }

  if constexpr (EPI == GH_XF_EPI_BIAS_RES_CF) {
    // the wave's tile crosses LDS so that the lane becomes the row: a channel's store is then a run along n
    float* region = s_all + wave * 32 * GX_P;
    __syncthreads();                                           // the slabs this region overlays have been read by every wave
#pragma unroll
    for (int r = 0; r < 16; ++r) region[ghr_acc_row(r, half) * GX_P + col] = acc[0][r];
    __syncthreads();
    const int t = row0 + 32 * wr + col;
    if (t < a.T) {
      const int b = t / N, n = t - b * N;
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int ch = 2 * it + half, jj = c0 + 32 * wc + ch;
        if (jj < a.N_out) {
          float v = region[col * GX_P + ch];
          if (a.res) v = v + a.res[(long long)b * a.res_stride_b + (long long)jj * a.res_stride + n];
          a.y[(long long)b * a.y_stride_b + (long long)jj * a.y_stride + n] = v;
        }
      }
    }
  } else {
    if (j < a.N_out) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long t = row0 + 32 * wr + ghr_acc_row(r, half);
        if (t < a.T) {
          float v = acc[0][r];
          if constexpr (EPI == GH_XF_EPI_BIAS_RES) {
            if (a.res) v = v + a.res[t * a.res_stride + j];
          }
          if constexpr (EPI == GH_XF_EPI_GEGLU) {
            const float g = acc[NB - 1][r];
            v = v * ((0.5f * g) * (1.0f + erff(g * 0.70710678118654752440f)));
          }
          a.y[t * a.y_stride + j] = v;
        }
      }
    }
  }
}

// ---- attention -------------------------------------------------------------------------------------------------------------------------
template <int ND, bool LSE>
__global__ __launch_bounds__(GHR_BLOCK) void gx_attn_kernel(const float* __restrict__ qkv, long long stride, float* __restrict__ out,
                                                             long long out_stride, int N, int H, float scale, int vec, int nq_tiles,
                                                             float* __restrict__ lse) {
  constexpr int D = 32 * ND, P = D + 1;
  constexpr int SLOT = 16 * ND + 2;                            // floats a lane hands to its partner wave
  __shared__ float s_stage[2 * GH_XF_ATTN_KEYS * P];
  static_assert(2 * GH_XF_ATTN_KEYS * P >= 2 * 64 * SLOT && 2 * GH_XF_ATTN_KEYS * P >= 2 * 32 * P, "the stage doubles as the join and the transpose");
  float* s_k = s_stage;
  float* s_v = s_stage + GH_XF_ATTN_KEYS * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int qi = wave >> 1, kh = wave & 1;
  const int qt = blockIdx.x % nq_tiles, bh = blockIdx.x / nq_tiles, b = bh / H, h = bh - b * H;
  const int M = H * D;
  const float* q = qkv + (long long)b * N * stride + h * D;
  const float* k = q + M;
  const float* v = q + 2 * M;
  const int row0 = qt * GH_XF_ATTN_ROWS + qi * 32, row = row0 + col;

  float qr[16 * ND];
#pragma unroll
  for (int s = 0; s < 16 * ND; ++s) qr[s] = row < N ? q[(long long)row * stride + 2 * s + half] : 0.f;
  ghr_acc o[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) o[t] = gx_splat(0.f);
  float m = -INFINITY, l = 0.f;

  const int sub = 32 * kh;
  GhrSlab<2 * ND, 8 * ND> ks, vs;                              // 64 keys x D columns each; rows past N arrive as zeros
  ghr_fetch_in(ks, k, stride, 0, 0, N, D, vec, tid);
  ghr_fetch_in(vs, v, stride, 0, 0, N, D, vec, tid);
  for (int kt = 0; kt < N; kt += GH_XF_ATTN_KEYS) {
    __syncthreads();                                           // the previous stage has been read by every wave
    ghr_put(ks, s_k, P, tid);
    ghr_put(vs, s_v, P, tid);
    __syncthreads();
    if (kt + GH_XF_ATTN_KEYS < N) {                            // the next stage's loads fly under this stage's products
      ghr_fetch_in(ks, k, stride, kt + GH_XF_ATTN_KEYS, 0, N, D, vec, tid);
      ghr_fetch_in(vs, v, stride, kt + GH_XF_ATTN_KEYS, 0, N, D, vec, tid);
    }
    if (kt + sub < N) {                                        // wave-uniform: the tile holds at least one key
      ghr_acc st = gx_splat(0.f);
      const float* ap = s_k + (sub + col) * P + half;
#pragma unroll
      for (int s = 0; s < 16 * ND; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], qr[s], st, 0, 0, 0);
      float p[16];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = kt + sub + ghr_acc_row(r, half) < N ? st[r] * scale : -INFINITY;
        mx = fmaxf(mx, p[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m, mx);
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
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_v[(sub + ghr_acc_row(r, half)) * P + 32 * t + col], p[r], o[t], 0, 0, 0);
      }
    }
  }

  // the pair's join: the odd wave hands over through LDS, element e of lane l at [e * 64 + l]
  float* join = s_stage + qi * 64 * SLOT;
  __syncthreads();                                             // the last stage has been read by every wave
  if (kh == 1) {
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) join[(16 * t + r) * 64 + lane] = o[t][r];
    }
    join[(16 * ND) * 64 + lane] = m;
    join[(16 * ND + 1) * 64 + lane] = l;
  }
  __syncthreads();
  if (kh == 0) {
    const float m1 = join[(16 * ND) * 64 + lane], l1 = join[(16 * ND + 1) * 64 + lane];
    const float mm = fmaxf(m, m1);                             // finite: the even wave met key 0
    const float a0 = expf(m - mm), a1 = expf(m1 - mm);
    l = l * a0 + l1 * a1;
    if constexpr (LSE) {                                       // both halves of a lane pair hold the query's mm and l
      if (half == 0 && row < N) lse[(long long)bh * N + row] = mm + logf(l);
    }
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] = (o[t][r] * a0 + join[(16 * t + r) * 64 + lane] * a1) / l;
    }
  }
  __syncthreads();                                             // the join has been read: the transpose overlays it
  float* region = s_stage + qi * 32 * P;                       // [query][d]
  if (kh == 0) {
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) region[col * P + 32 * t + ghr_acc_row(r, half)] = o[t][r];
    }
  }
  __syncthreads();
  // both waves of the pair store: wave kh the queries 16 kh .. 16 kh + 15, a half wave one run of 32 floats
  float* dst = out + (long long)b * N * out_stride + h * D;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int rq = 16 * kh + 2 * it + half;
    if (row0 + rq < N) {
#pragma unroll
      for (int t = 0; t < ND; ++t) dst[(long long)(row0 + rq) * out_stride + 32 * t + col] = region[rq * P + 32 * t + col];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static bool gx_launched() { return hipGetLastError() == hipSuccess; }

static int gx_tiles(long long a, long long b, int* out) {      // a * b workgroups within int32
  if (a * b > INT_MAX) return GH_ERR_UNSUPPORTED;
  *out = (int)(a * b);
  return GH_OK;
}

// need_bias: the C-ABI's rule that a biased epilogue has a bias; the backward's proj_in product runs BIAS_RES_CF with neither bias nor
// residual (the chain then starts from zero, as under PLAIN)
static int gx_check_linear(const GhXfLinear* a, bool* empty, bool need_bias) {
  *empty = true;
  if (!a || a->T < 0 || a->K < 1 || a->N_out < 1) return GH_ERR_INVALID_ARG;
  if (a->prologue < GH_XF_PRO_NONE || a->prologue > GH_XF_PRO_CF || a->epilogue < GH_XF_EPI_PLAIN || a->epilogue > GH_XF_EPI_BIAS_RES_CF)
    return GH_ERR_INVALID_ARG;
  if (a->K % 32 != 0 || a->K > GH_XF_MAX_K || a->T > GH_XF_MAX_T || a->N_out > GH_XF_MAX_N_OUT) return GH_ERR_UNSUPPORTED;
  const bool normed = a->prologue == GH_XF_PRO_LN || a->prologue == GH_XF_PRO_GN;
  const bool cf = a->prologue == GH_XF_PRO_GN || a->prologue == GH_XF_PRO_CF;
  const bool batched = cf || a->epilogue == GH_XF_EPI_BIAS_RES_CF;
  if (batched && a->T > 0 && (a->rows_per_batch < 1 || a->T % a->rows_per_batch != 0)) return GH_ERR_INVALID_ARG;
  if (a->prologue == GH_XF_PRO_GN && (a->groups < 1 || a->K % a->groups != 0)) return GH_ERR_INVALID_ARG;
  if (normed && !(a->eps >= 0.f && isfinite(a->eps))) return GH_ERR_INVALID_ARG;
  *empty = a->T == 0;
  if (*empty) return GH_OK;
  if (!a->x || !a->w || !a->y || !ghr_al4(a->x) || !ghr_al4(a->w) || !ghr_al4(a->y) || !ghr_al4(a->bias) || !ghr_al4(a->res)) return GH_ERR_INVALID_ARG;
  if (normed && (!a->gamma || !a->beta || !ghr_al4(a->gamma) || !ghr_al4(a->beta))) return GH_ERR_INVALID_ARG;
  if (a->prologue == GH_XF_PRO_GN && (!a->moments || !ghr_al4(a->moments))) return GH_ERR_INVALID_ARG;
  if (!cf && a->x_stride < a->K) return GH_ERR_INVALID_ARG;
  if (need_bias && a->epilogue != GH_XF_EPI_PLAIN && !a->bias) return GH_ERR_INVALID_ARG;
  if (a->epilogue != GH_XF_EPI_BIAS_RES_CF && a->y_stride < a->N_out) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

extern "C" size_t gh_xf_linear_workspace_bytes(int T, int prologue) {
  if (T <= 0 || T > GH_XF_MAX_T || prologue != GH_XF_PRO_LN) return 0;
  return ghr_align((size_t)T * 2 * sizeof(float));
}

template <int PRO>
static void gx_launch_linear(const GhXfLinear& a, const float* ln_mom, int vec_x, int vec_w, int ncol, int grid, hipStream_t s) {
  const dim3 g((unsigned)grid), blk(GHR_BLOCK);
  switch (a.epilogue) {
    case GH_XF_EPI_PLAIN: hipLaunchKernelGGL((gx_linear_kernel<PRO, GH_XF_EPI_PLAIN>), g, blk, 0, s, a, ln_mom, vec_x, vec_w, ncol); break;
    case GH_XF_EPI_BIAS_RES: hipLaunchKernelGGL((gx_linear_kernel<PRO, GH_XF_EPI_BIAS_RES>), g, blk, 0, s, a, ln_mom, vec_x, vec_w, ncol); break;
    case GH_XF_EPI_GEGLU: hipLaunchKernelGGL((gx_linear_kernel<PRO, GH_XF_EPI_GEGLU>), g, blk, 0, s, a, ln_mom, vec_x, vec_w, ncol); break;
    default: hipLaunchKernelGGL((gx_linear_kernel<PRO, GH_XF_EPI_BIAS_RES_CF>), g, blk, 0, s, a, ln_mom, vec_x, vec_w, ncol); break;
  }
}

static int gx_linear(const GhXfLinear* a, void* workspace, size_t ws_bytes, void* hip_stream, bool need_bias) {
  bool empty;
  const int rc = gx_check_linear(a, &empty, need_bias);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  const int ncol = (a->N_out + GX_TC - 1) / GX_TC, nrow = (a->T + GX_TR - 1) / GX_TR;
  int grid;
  if (gx_tiles(ncol, nrow, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;
  float* ln_mom = nullptr;
  if (a->prologue == GH_XF_PRO_LN) {
    if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
    if (ws_bytes < gh_xf_linear_workspace_bytes(a->T, a->prologue)) return GH_ERR_WORKSPACE_SMALL;
    ln_mom = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  if (ln_mom) {
    hipLaunchKernelGGL(gx_row_moments_kernel, dim3((unsigned)((a->T + GX_LN_ROWS - 1) / GX_LN_ROWS)), dim3(GHR_BLOCK), 0, s, a->x,
                       (long long)a->x_stride, a->T, a->K, a->eps, ln_mom);
    if (!gx_launched()) return GH_ERR_LAUNCH;
  }
  const int vec_x = (a->prologue == GH_XF_PRO_NONE || a->prologue == GH_XF_PRO_LN) && ghr_al16(a->x) && a->x_stride % 4 == 0, vec_w = ghr_al16(a->w);
  switch (a->prologue) {
    case GH_XF_PRO_NONE: gx_launch_linear<GH_XF_PRO_NONE>(*a, ln_mom, vec_x, vec_w, ncol, grid, s); break;
    case GH_XF_PRO_LN: gx_launch_linear<GH_XF_PRO_LN>(*a, ln_mom, vec_x, vec_w, ncol, grid, s); break;
    case GH_XF_PRO_CF: gx_launch_linear<GH_XF_PRO_CF>(*a, ln_mom, vec_x, vec_w, ncol, grid, s); break;
    default: gx_launch_linear<GH_XF_PRO_GN>(*a, ln_mom, vec_x, vec_w, ncol, grid, s); break;
  }
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_xf_linear(const GhXfLinear* a, void* workspace, size_t ws_bytes, void* hip_stream) {
  return gx_linear(a, workspace, ws_bytes, hip_stream, true);
}

static int gx_check_groups(int B, int C, int N, int G, bool* empty) {
  *empty = true;
  if (B < 0 || N < 0 || C < 1 || G < 1 || C % G != 0) return GH_ERR_INVALID_ARG;
  if (C > GH_XF_MAX_C || (long long)B * N > GH_XF_MAX_T) return GH_ERR_UNSUPPORTED;
  *empty = B == 0 || N == 0;
  if (*empty) return GH_OK;
  int grid;
  return gx_tiles((long long)B * G, (N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, &grid);
}

extern "C" size_t gh_xf_group_moments_workspace_bytes(int B, int C, int N, int G) {
  bool empty;
  if (gx_check_groups(B, C, N, G, &empty) != GH_OK || empty) return 0;
  return ghr_align((size_t)B * G * ((N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK) * 2 * sizeof(float));
}

extern "C" int gh_xf_group_moments(const float* x, int64_t stride_b, int64_t stride_c, int B, int C, int N, int G, float* moments,
                                   void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_groups(B, C, N, G, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  if (!x || !moments || !ghr_al4(x) || !ghr_al4(moments) || !workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_xf_group_moments_workspace_bytes(B, C, N, G)) return GH_ERR_WORKSPACE_SMALL;
  const int nchunks = (N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, BG = B * G;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_group_part_kernel, dim3((unsigned)(BG * nchunks)), dim3(GHR_BLOCK), 0, s, x, (long long)stride_b, (long long)stride_c, N,
                     G, C / G, nchunks, (float*)workspace);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(gx_group_join_kernel, dim3((unsigned)((BG + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, (const float*)workspace,
                     BG, N, C / G, nchunks, moments);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

static int gx_check_attn(int B, int N, int heads, int D, int* grid, bool* empty) {
  *empty = true;
  if (B < 0 || N < 0 || heads < 1 || D < 1) return GH_ERR_INVALID_ARG;
  if ((D != 32 && D != 64) || (long long)heads * D > GH_XF_MAX_M || (long long)B * N > GH_XF_MAX_T) return GH_ERR_UNSUPPORTED;
  *empty = B == 0 || N == 0;
  if (*empty) return GH_OK;
  return gx_tiles((long long)B * heads, (N + GH_XF_ATTN_ROWS - 1) / GH_XF_ATTN_ROWS, grid);
}

template <bool LSE>
static int gx_attention(const float* qkv, int64_t qkv_stride, int B, int N, int heads, int D, float* out, int64_t out_stride, float* lse,
                        void* hip_stream) {
  bool empty;
  int grid = 0;
  const int rc = gx_check_attn(B, N, heads, D, &grid, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  const int M = heads * D;
  if (!qkv || !out || !ghr_al4(qkv) || !ghr_al4(out) || qkv_stride < 3 * M || out_stride < M) return GH_ERR_INVALID_ARG;
  if (LSE && (!lse || !ghr_al4(lse))) return GH_ERR_INVALID_ARG;
  const int vec = ghr_al16(qkv) && qkv_stride % 4 == 0, nq = (N + GH_XF_ATTN_ROWS - 1) / GH_XF_ATTN_ROWS;
  const float scale = (float)(1.0 / sqrt((double)D));
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  if (D == 32) {
    hipLaunchKernelGGL((gx_attn_kernel<1, LSE>), dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, qkv, (long long)qkv_stride, out,
                       (long long)out_stride, N, heads, scale, vec, nq, lse);
  } else {
    hipLaunchKernelGGL((gx_attn_kernel<2, LSE>), dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, qkv, (long long)qkv_stride, out,
                       (long long)out_stride, N, heads, scale, vec, nq, lse);
  }
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_xf_attention(const float* qkv, int64_t qkv_stride, int B, int N, int heads, int D, float* out, int64_t out_stride,
                               void* hip_stream) {
  return gx_attention<false>(qkv, qkv_stride, B, N, heads, D, out, out_stride, nullptr, hip_stream);
}

extern "C" int gh_xf_attention_lse(const float* qkv, int64_t qkv_stride, int B, int N, int heads, int D, float* out, int64_t out_stride,
                                   float* lse, void* hip_stream) {
  return gx_attention<true>(qkv, qkv_stride, B, N, heads, D, out, out_stride, lse, hip_stream);
}

// the workspace of a whole forward: h (T, M), qkv (T, 3M), att (T, M), ff (T, 4M), the LayerNorm's row moments, the GroupNorm's
// moments and their partials
struct GxPlan {
  size_t h, qkv, att, ff, ln, gn, gnp, total;
};

static int gx_check_dims(const GhXfDims* d, bool* empty) {
  *empty = true;
  if (!d || d->B < 0 || d->N < 0 || d->C < 1 || d->G < 1 || d->heads < 1 || d->D < 1 || d->layers < 0 || d->C % d->G != 0) return GH_ERR_INVALID_ARG;
  if (!(d->gn_eps >= 0.f && isfinite(d->gn_eps)) || !(d->ln_eps >= 0.f && isfinite(d->ln_eps))) return GH_ERR_INVALID_ARG;
  if ((d->D != 32 && d->D != 64) || (long long)d->heads * d->D > GH_XF_MAX_M || d->C > GH_XF_MAX_C || d->C % 32 != 0) return GH_ERR_UNSUPPORTED;
  if ((long long)d->B * d->N > GH_XF_MAX_T) return GH_ERR_UNSUPPORTED;
  *empty = d->B == 0 || d->N == 0;
  if (*empty) return GH_OK;
  const long long T = (long long)d->B * d->N, rows = (T + GX_TR - 1) / GX_TR, M = (long long)d->heads * d->D;
  int grid;
  if (gx_tiles(rows, (4 * M + GX_TC - 1) / GX_TC, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;   // the widest product
  if (gx_tiles((long long)d->B * d->heads, (d->N + GH_XF_ATTN_ROWS - 1) / GH_XF_ATTN_ROWS, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;
  return gx_tiles((long long)d->B * d->G, (d->N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, &grid);
}

static GxPlan gx_plan(const GhXfDims* d) {
  const size_t T = (size_t)d->B * d->N, M = (size_t)d->heads * d->D, f = sizeof(float);
  GxPlan p;
  size_t at = 0;
  p.h = at; at += ghr_align(T * M * f);
  p.qkv = at; at += ghr_align(T * 3 * M * f);
  p.att = at; at += ghr_align(T * M * f);
  p.ff = at; at += ghr_align(T * 4 * M * f);
  p.ln = at; at += gh_xf_linear_workspace_bytes((int)T, GH_XF_PRO_LN);
  p.gn = at; at += ghr_align((size_t)d->B * d->G * 2 * f);
  p.gnp = at; at += gh_xf_group_moments_workspace_bytes(d->B, d->C, d->N, d->G);
  p.total = at;
  return p;
}

extern "C" size_t gh_xf_workspace_bytes(const GhXfDims* dims) {
  bool empty;
  if (gx_check_dims(dims, &empty) != GH_OK || empty) return 0;
  return gx_plan(dims).total;
}

// ---- the tape of gh_xf_forward_tape (include/gh_xf.h): byte offsets; a slot's parts are relative to the slot ----------------------------
struct GxTape {
  size_t gn, layer0, layer_stride, total;
  size_t a_ln, a_qkv, a_att, a_lse, a_size;                    // an attention slot: h at 0
  size_t f_ln, f_size;                                         // the feed-forward's slot: h at 0
};

static GxTape gx_tape(const GhXfDims* d) {
  const size_t T = (size_t)d->B * d->N, M = (size_t)d->heads * d->D, f = sizeof(float);
  GxTape t;
  size_t at = ghr_align(T * M * f);
  t.a_ln = at; at += ghr_align(T * 2 * f);
  t.a_qkv = at; at += ghr_align(T * 3 * M * f);
  t.a_att = at; at += ghr_align(T * M * f);
  t.a_lse = at; at += ghr_align(T * d->heads * f);
  t.a_size = at;
  t.f_ln = ghr_align(T * M * f);
  t.f_size = t.f_ln + ghr_align(T * 2 * f);
  t.gn = 0;
  t.layer0 = ghr_align((size_t)d->B * d->G * 2 * f);
  t.layer_stride = 2 * t.a_size + t.f_size;
  t.total = t.layer0 + (size_t)d->layers * t.layer_stride;
  return t;
}

static char* gx_slot(const GxTape& t, char* tape, int layer, int which) {   // which: 0 attn1, 1 attn2, 2 the feed-forward
  return tape + t.layer0 + (size_t)layer * t.layer_stride + (size_t)which * t.a_size;
}

static int gx_check_grad_dims(const GhXfDims* d, bool* empty) {
  const int rc = gx_check_dims(d, empty);
  if (rc != GH_OK) return rc;
  if ((long long)d->heads * d->D > GH_XF_GRAD_MAX_M) { *empty = true; return GH_ERR_UNSUPPORTED; }
  if (*empty) return GH_OK;
  int grid;
  const long long T = (long long)d->B * d->N, M = (long long)d->heads * d->D;
  if (gx_tiles((T + GX_TR - 1) / GX_TR, (8 * M + GX_TC - 1) / GX_TC, &grid) != GH_OK) { *empty = true; return GH_ERR_UNSUPPORTED; }
  if (gx_tiles((long long)d->B * d->C, (d->N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, &grid) != GH_OK) { *empty = true; return GH_ERR_UNSUPPORTED; }
  return GH_OK;
}

// the forward's host loop. tape == nullptr: every intermediate lives in the workspace and the stream h is updated in place. Otherwise
// what the backward reads goes to the tape: each sub-block reads h from its own slot and writes the next sub-block's.
static int gx_forward(const GhXfDims* d, const GhXfStem* stem, const GhXfLayer* layers, const float* x, float* out, char* tape,
                      void* workspace, size_t ws_bytes, void* hip_stream) {
  if (!stem || (d->layers > 0 && !layers) || !x || !out || x == out || !ghr_al4(x) || !ghr_al4(out)) return GH_ERR_INVALID_ARG;
  const float* sp[] = {stem->gn_w, stem->gn_b, stem->in_w, stem->in_b, stem->out_w, stem->out_b};
  for (const float* p : sp) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  for (int i = 0; i < d->layers; ++i) {
    const GhXfLayer& L = layers[i];
    const float* need[] = {L.ln1_w, L.ln1_b, L.qkv1, L.o1_w, L.o1_b, L.ln3_w, L.ln3_b, L.ff1_w, L.ff1_b, L.ff2_w, L.ff2_b};
    for (const float* p : need) {
      if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
    }
    if (L.qkv2) {
      const float* second[] = {L.qkv2, L.ln2_w, L.ln2_b, L.o2_w, L.o2_b};
      for (const float* p : second) {
        if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
      }
    }
  }
  if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  const GxPlan p = gx_plan(d);
  if (ws_bytes < p.total) return GH_ERR_WORKSPACE_SMALL;
  const GxTape tp = gx_tape(d);

  char* ws = (char*)workspace;
  float* h = (float*)(ws + p.h);
  float* ff = (float*)(ws + p.ff);
  float* gn = tape ? (float*)(tape + tp.gn) : (float*)(ws + p.gn);
  const size_t ln_bytes = p.gn - p.ln;
  const int T = d->B * d->N, M = d->heads * d->D, C = d->C, N = d->N;
  int rc;

  // where the stream goes after sub-block `which` of layer i: the next sub-block's slot, the workspace behind the last
  auto next = [&](int i, int which) -> float* {
    if (!tape) return h;
    if (which == 0 && layers[i].qkv2) return (float*)gx_slot(tp, tape, i, 1);
    if (which < 2) return (float*)gx_slot(tp, tape, i, 2);
    return i + 1 < d->layers ? (float*)gx_slot(tp, tape, i + 1, 0) : h;
  };
  float* hin = tape && d->layers > 0 ? (float*)gx_slot(tp, tape, 0, 0) : h;

  rc = gh_xf_group_moments(x, (int64_t)C * N, N, d->B, C, N, d->G, gn, ws + p.gnp, p.total - p.gnp, hip_stream);
  if (rc != GH_OK) return rc;

  GhXfLinear a = {};
  a.T = T; a.K = C; a.N_out = M; a.prologue = GH_XF_PRO_GN; a.epilogue = GH_XF_EPI_BIAS_RES; a.rows_per_batch = N; a.groups = d->G;
  a.eps = d->gn_eps; a.x = x; a.x_stride = N; a.x_stride_b = (int64_t)C * N; a.w = stem->in_w; a.bias = stem->in_b; a.gamma = stem->gn_w;
  a.beta = stem->gn_b; a.moments = gn; a.y = hin; a.y_stride = M;
  rc = gh_xf_linear(&a, nullptr, 0, hip_stream);
  if (rc != GH_OK) return rc;

  // y = epilogue(LN(src) w^T) or epilogue(src w^T); ln: where the LayerNorm's row moments go
  auto product = [&](int pro, int epi, const float* src, int K, const float* gamma, const float* beta, const float* w, const float* bias,
                     int n_out, const float* res, float* y, void* ln) {
    GhXfLinear l = {};
    l.T = T; l.K = K; l.N_out = n_out; l.prologue = pro; l.epilogue = epi; l.eps = d->ln_eps; l.x = src; l.x_stride = K; l.w = w; l.bias = bias;
    l.gamma = gamma; l.beta = beta; l.res = res; l.res_stride = n_out; l.y = y; l.y_stride = n_out;
    return gh_xf_linear(&l, ln, ln_bytes, hip_stream);
  };
  for (int i = 0; i < d->layers; ++i) {
    const GhXfLayer& L = layers[i];
    for (int which = 0; which < 2; ++which) {
      const float* wqkv = which ? L.qkv2 : L.qkv1;
      if (!wqkv) continue;
      char* slot = tape ? gx_slot(tp, tape, i, which) : nullptr;
      float* qkv = slot ? (float*)(slot + tp.a_qkv) : (float*)(ws + p.qkv);
      float* att = slot ? (float*)(slot + tp.a_att) : (float*)(ws + p.att);
      void* ln = slot ? (void*)(slot + tp.a_ln) : (void*)(ws + p.ln);
      rc = product(GH_XF_PRO_LN, GH_XF_EPI_PLAIN, hin, M, which ? L.ln2_w : L.ln1_w, which ? L.ln2_b : L.ln1_b, wqkv, nullptr, 3 * M, nullptr, qkv, ln);
      if (rc != GH_OK) return rc;
      rc = slot ? gh_xf_attention_lse(qkv, 3 * M, d->B, N, d->heads, d->D, att, M, (float*)(slot + tp.a_lse), hip_stream)
                : gh_xf_attention(qkv, 3 * M, d->B, N, d->heads, d->D, att, M, hip_stream);
      if (rc != GH_OK) return rc;
      float* hout = next(i, which);
      rc = product(GH_XF_PRO_NONE, GH_XF_EPI_BIAS_RES, att, M, nullptr, nullptr, which ? L.o2_w : L.o1_w, which ? L.o2_b : L.o1_b, M, hin, hout, nullptr);
      if (rc != GH_OK) return rc;
      hin = hout;
    }
    void* ln = tape ? (void*)(gx_slot(tp, tape, i, 2) + tp.f_ln) : (void*)(ws + p.ln);
    rc = product(GH_XF_PRO_LN, GH_XF_EPI_GEGLU, hin, M, L.ln3_w, L.ln3_b, L.ff1_w, L.ff1_b, 4 * M, nullptr, ff, ln);
    if (rc != GH_OK) return rc;
    float* hout = next(i, 2);
    rc = product(GH_XF_PRO_NONE, GH_XF_EPI_BIAS_RES, ff, 4 * M, nullptr, nullptr, L.ff2_w, L.ff2_b, M, hin, hout, nullptr);
    if (rc != GH_OK) return rc;
    hin = hout;
  }

  GhXfLinear z = {};
  z.T = T; z.K = M; z.N_out = C; z.prologue = GH_XF_PRO_NONE; z.epilogue = GH_XF_EPI_BIAS_RES_CF; z.rows_per_batch = N; z.x = hin; z.x_stride = M;
  z.w = stem->out_w; z.bias = stem->out_b; z.res = x; z.res_stride = N; z.res_stride_b = (int64_t)C * N; z.y = out; z.y_stride = N;
  z.y_stride_b = (int64_t)C * N;
  return gh_xf_linear(&z, nullptr, 0, hip_stream);
}

extern "C" int gh_xf_forward(const GhXfDims* d, const GhXfStem* stem, const GhXfLayer* layers, const float* x, float* out, void* workspace,
                             size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_dims(d, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  return gx_forward(d, stem, layers, x, out, nullptr, workspace, ws_bytes, hip_stream);
}

extern "C" size_t gh_xf_tape_bytes(const GhXfDims* dims) {
  bool empty;
  if (gx_check_grad_dims(dims, &empty) != GH_OK || empty) return 0;
  return gx_tape(dims).total;
}

extern "C" int gh_xf_forward_tape(const GhXfDims* d, const GhXfStem* stem, const GhXfLayer* layers, const float* x, float* out, void* tape,
                                  size_t tape_bytes, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_grad_dims(d, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  if (!tape || !ghr_al16(tape)) return GH_ERR_INVALID_ARG;
  if (tape_bytes < gx_tape(d).total) return GH_ERR_WORKSPACE_SMALL;
  return gx_forward(d, stem, layers, x, out, (char*)tape, workspace, ws_bytes, hip_stream);
}

// ==== the backward to x, every weight frozen ============================================================================================
static_assert(GH_XF_ATTN_BWD_ROWS == 32 * (GHR_BLOCK / 64) && GH_XF_ATTN_BWD_STAGE == 64, "a wave owns 32 rows; GhrSlab<2 ND, 8 ND> is 64 rows x D columns");
static_assert(8 * GH_XF_GRAD_MAX_M <= GH_XF_MAX_K, "dn = [da | dg] W1 is a product of inner width 8M");

// ---- attention: delta = dot(dout, out) per (row, head), one ascending chain -------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_attn_delta_kernel(const float* __restrict__ dout, long long dstride, const float* __restrict__ out,
                                                                   long long ostride, long long T, int N, int H, int D, float* __restrict__ delta) {
  const long long i = (long long)blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (i >= T * H) return;
  const long long t = i / H, b = t / N, n = t - b * N;
  const int h = (int)(i - t * H);
  const float* a = dout + t * dstride + h * D;
  const float* o = out + t * ostride + h * D;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s = fmaf(a[d], o[d], s);
  delta[(b * H + h) * N + n] = s;
}

// ---- attention: the query-block kernel owns dq -----------------------------------------------------------------------------------------
// The forward's shape: the query on the lane, K and V from LDS 64 keys a stage; every wave folds both tiles of 32 keys of a stage, in
// ascending order, so a query's dq is one chain over all keys. `block` is the workgroup's index among the query blocks.
template <int ND>
__device__ __forceinline__ void gx_attn_dq(int block, float* s_stage, const float* __restrict__ qkv, long long stride, const float* __restrict__ dout,
                                           long long dstride, const float* __restrict__ lse, const float* __restrict__ delta,
                                           float* __restrict__ dqkv, long long gstride, int N, int H, float scale, int vec, int ntiles) {
  constexpr int D = 32 * ND, P = D + 1;
  float* s_k = s_stage;
  float* s_v = s_stage + GH_XF_ATTN_BWD_STAGE * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int qt = block % ntiles, bh = block / ntiles, b = bh / H, h = bh - b * H;
  const int M = H * D;
  const float* q = qkv + (long long)b * N * stride + h * D;
  const float* k = q + M;
  const float* v = q + 2 * M;
  const float* go = dout + (long long)b * N * dstride + h * D;
  const int row = qt * GH_XF_ATTN_BWD_ROWS + 32 * wave + col;
  const bool live = row < N, wave_live = qt * GH_XF_ATTN_BWD_ROWS + 32 * wave < N;

  float qr[16 * ND], gr[16 * ND];
#pragma unroll
  for (int s = 0; s < 16 * ND; ++s) {
    qr[s] = live ? q[(long long)row * stride + 2 * s + half] : 0.f;
    gr[s] = live ? go[(long long)row * dstride + 2 * s + half] : 0.f;
  }
  const float ls = live ? lse[(long long)bh * N + row] : 0.f, dl = live ? delta[(long long)bh * N + row] : 0.f;
  ghr_acc dq[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) dq[t] = gx_splat(0.f);

  GhrSlab<2 * ND, 8 * ND> ks, vs;                              // 64 keys x D columns each; rows past N arrive as zeros
  ghr_fetch_in(ks, k, stride, 0, 0, N, D, vec, tid);
  ghr_fetch_in(vs, v, stride, 0, 0, N, D, vec, tid);
  for (int kt = 0; kt < N; kt += GH_XF_ATTN_BWD_STAGE) {
    __syncthreads();                                           // the previous stage has been read by every wave
    ghr_put(ks, s_k, P, tid);
    ghr_put(vs, s_v, P, tid);
    __syncthreads();
    if (kt + GH_XF_ATTN_BWD_STAGE < N) {
      ghr_fetch_in(ks, k, stride, kt + GH_XF_ATTN_BWD_STAGE, 0, N, D, vec, tid);
      ghr_fetch_in(vs, v, stride, kt + GH_XF_ATTN_BWD_STAGE, 0, N, D, vec, tid);
    }
    if (!wave_live) continue;                                  // wave-uniform; the barriers above are met by every wave
#pragma unroll 1
    for (int sub = 0; sub < GH_XF_ATTN_BWD_STAGE; sub += 32) {
      if (kt + sub >= N) break;                                // wave-uniform: the tile holds no key
      ghr_acc st = gx_splat(0.f), dp = gx_splat(0.f);
      const float* ap = s_k + (sub + col) * P + half;
      const float* vp = s_v + (sub + col) * P + half;
#pragma unroll
      for (int s = 0; s < 16 * ND; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], qr[s], st, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 16 * ND; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[2 * s], gr[s], dp, 0, 0, 0);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = expf(st[r] * scale - ls);
        ds[r] = kt + sub + ghr_acc_row(r, half) < N ? (p * (dp[r] - dl)) * scale : 0.f;
      }
#pragma unroll
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          dq[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_k[(sub + ghr_acc_row(r, half)) * P + 32 * t + col], ds[r], dq[t], 0, 0, 0);
      }
    }
  }
  if (live) {
    float* dst = dqkv + ((long long)b * N + row) * gstride + h * D;
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[32 * t + ghr_acc_row(r, half)] = dq[t][r];
    }
  }
}

// ---- attention: the key-block kernel owns dk and dv ------------------------------------------------------------------------------------
// The key on the lane; q and dout rows cross LDS 64 queries a stage with their lse and delta (s_ld: lse, then delta, of the stage's
// queries). `block` is the workgroup's index among the key blocks.
template <int ND>
__device__ __forceinline__ void gx_attn_dkv(int block, float* s_stage, float* s_ld, const float* __restrict__ qkv, long long stride,
                                            const float* __restrict__ dout, long long dstride, const float* __restrict__ lse,
                                            const float* __restrict__ delta, float* __restrict__ dqkv, long long gstride, int N, int H, float scale,
                                            int vec, int vec_d, int ntiles) {
  constexpr int D = 32 * ND, P = D + 1;
  float* s_q = s_stage;
  float* s_g = s_stage + GH_XF_ATTN_BWD_STAGE * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int ktile = block % ntiles, bh = block / ntiles, b = bh / H, h = bh - b * H;
  const int M = H * D;
  const float* q = qkv + (long long)b * N * stride + h * D;
  const float* k = q + M;
  const float* v = q + 2 * M;
  const float* go = dout + (long long)b * N * dstride + h * D;
  const int row = ktile * GH_XF_ATTN_BWD_ROWS + 32 * wave + col;
  const bool live = row < N, wave_live = ktile * GH_XF_ATTN_BWD_ROWS + 32 * wave < N;

  float kr[16 * ND], vr[16 * ND];
#pragma unroll
  for (int s = 0; s < 16 * ND; ++s) {
    kr[s] = live ? k[(long long)row * stride + 2 * s + half] : 0.f;
    vr[s] = live ? v[(long long)row * stride + 2 * s + half] : 0.f;
  }
  ghr_acc dk[ND], dv[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    dk[t] = gx_splat(0.f);
    dv[t] = gx_splat(0.f);
  }

  // thread i < 64 carries lse of the stage's query i, thread 64 + i its delta
  const float* ldsrc = (tid < GH_XF_ATTN_BWD_STAGE ? lse : delta) + (long long)bh * N;
  const int ldi = tid & (GH_XF_ATTN_BWD_STAGE - 1);
  GhrSlab<2 * ND, 8 * ND> qs, gs;                              // 64 queries x D columns each; rows past N arrive as zeros
  ghr_fetch_in(qs, q, stride, 0, 0, N, D, vec, tid);
  ghr_fetch_in(gs, go, dstride, 0, 0, N, D, vec_d, tid);
  float ld = tid < 2 * GH_XF_ATTN_BWD_STAGE && ldi < N ? ldsrc[ldi] : 0.f;
  for (int qt = 0; qt < N; qt += GH_XF_ATTN_BWD_STAGE) {
    __syncthreads();                                           // the previous stage has been read by every wave
    ghr_put(qs, s_q, P, tid);
    ghr_put(gs, s_g, P, tid);
    if (tid < 2 * GH_XF_ATTN_BWD_STAGE) s_ld[tid] = ld;
    __syncthreads();
    if (qt + GH_XF_ATTN_BWD_STAGE < N) {
      ghr_fetch_in(qs, q, stride, qt + GH_XF_ATTN_BWD_STAGE, 0, N, D, vec, tid);
      ghr_fetch_in(gs, go, dstride, qt + GH_XF_ATTN_BWD_STAGE, 0, N, D, vec_d, tid);
      ld = tid < 2 * GH_XF_ATTN_BWD_STAGE && qt + GH_XF_ATTN_BWD_STAGE + ldi < N ? ldsrc[qt + GH_XF_ATTN_BWD_STAGE + ldi] : 0.f;
    }
    if (!wave_live) continue;                                  // wave-uniform; the barriers above are met by every wave
#pragma unroll 1
    for (int sub = 0; sub < GH_XF_ATTN_BWD_STAGE; sub += 32) {
      if (qt + sub >= N) break;                                // wave-uniform: the tile holds no query
      ghr_acc st = gx_splat(0.f), dp = gx_splat(0.f);
      const float* ap = s_q + (sub + col) * P + half;
      const float* gp = s_g + (sub + col) * P + half;
#pragma unroll
      for (int s = 0; s < 16 * ND; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], kr[s], st, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 16 * ND; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(gp[2 * s], vr[s], dp, 0, 0, 0);
      float p[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = sub + ghr_acc_row(r, half);
        const bool ok = qt + qrow < N;                         // a query past N contributes exactly 0, whatever lse holds there
        const float pv = expf(st[r] * scale - s_ld[qrow]);
        p[r] = ok ? pv : 0.f;
        ds[r] = ok ? (pv * (dp[r] - s_ld[GH_XF_ATTN_BWD_STAGE + qrow])) * scale : 0.f;
      }
#pragma unroll
      for (int t = 0; t < ND; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = (sub + ghr_acc_row(r, half)) * P + 32 * t + col;
          dv[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_g[o], p[r], dv[t], 0, 0, 0);
          dk[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_q[o], ds[r], dk[t], 0, 0, 0);
        }
      }
    }
  }
  if (live) {                                                  // a key past N: its rows are not written
    float* dst = dqkv + ((long long)b * N + row) * gstride + M + h * D;
#pragma unroll
    for (int t = 0; t < ND; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dst[32 * t + ghr_acc_row(r, half)] = dk[t][r];
        dst[M + 32 * t + ghr_acc_row(r, half)] = dv[t][r];
      }
    }
  }
}

// One launch holds both kinds of workgroup: the first nkv own a key block each (dk, dv), the rest a query block each (dq). Neither kind
// reads what the other writes, so no workgroup waits for another; at B = 1 either kind alone would fill half the chip.
template <int ND>
__global__ __launch_bounds__(GHR_BLOCK) void gx_attn_bwd_kernel(const float* __restrict__ qkv, long long stride, const float* __restrict__ dout,
                                                                 long long dstride, const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 float* __restrict__ dqkv, long long gstride, int N, int H, float scale, int vec,
                                                                 int vec_d, int ntiles, int nkv) {
  __shared__ float s_stage[2 * GH_XF_ATTN_BWD_STAGE * (32 * ND + 1)];
  __shared__ float s_ld[2 * GH_XF_ATTN_BWD_STAGE];
  if ((int)blockIdx.x < nkv) {                                 // workgroup-uniform
    gx_attn_dkv<ND>((int)blockIdx.x, s_stage, s_ld, qkv, stride, dout, dstride, lse, delta, dqkv, gstride, N, H, scale, vec, vec_d, ntiles);
  } else {
    gx_attn_dq<ND>((int)blockIdx.x - nkv, s_stage, qkv, stride, dout, dstride, lse, delta, dqkv, gstride, N, H, scale, vec, ntiles);
  }
}

// ---- the feed-forward: [da | dg] in one pass --------------------------------------------------------------------------------------------
// gx_linear_kernel with two X slabs (the cotangent g, and h through LN3) and three W slabs for the same 64 x 64 tile of the F = 4M inner
// columns: du = g . W2 over w2t's rows, a and g' as the forward's GEGLU epilogue forms them.
__global__ __launch_bounds__(GHR_BLOCK) void gx_geglu_bwd_kernel(const float* __restrict__ g, long long g_stride, const float* __restrict__ h,
                                                                  long long h_stride, const float* __restrict__ mom, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ w1,
                                                                  const float* __restrict__ b1, const float* __restrict__ w2t, float* __restrict__ y,
                                                                  long long y_stride, int T, int M, int vec_g, int vec_h, int vec_w1, int vec_w2,
                                                                  int ncol_tiles) {
  __shared__ float s_all[2 * GX_TR * GX_P + 3 * GX_TC * GX_P];
  float* s_g = s_all;
  float* s_h = s_all + GX_TR * GX_P;
  float* s_wu = s_all + 2 * GX_TR * GX_P;
  float* s_wa = s_wu + GX_TC * GX_P;
  float* s_wg = s_wa + GX_TC * GX_P;
  const int F = 4 * M;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int tc = blockIdx.x % ncol_tiles, tr = blockIdx.x / ncol_tiles;
  const int row0 = tr * GX_TR, c0 = tc * GX_TC;

  float ln[2][2] = {{0.f, 1.f}, {0.f, 1.f}};
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int r = row0 + (tid + it * GHR_BLOCK) / 8;
    if (r < T) {
      ln[it][0] = mom[2 * (long long)r];
      ln[it][1] = mom[2 * (long long)r + 1];
    }
  }
  const int j = c0 + 32 * wc + col;                            // the lane's inner column: F is a multiple of 128, so j < F
  ghr_acc du = gx_splat(0.f), aa = gx_splat(b1[j]), ag = gx_splat(b1[F + j]);

  GhrSlab<2, 8> xg, xh, wu, wa, wg;
  auto fetch = [&](int k0) {
    ghr_fetch_in(xg, g, g_stride, row0, k0, T, M, vec_g, tid);
    ghr_fetch_in(xh, h, h_stride, row0, k0, T, M, vec_h, tid);
    ghr_fetch_in(wu, w2t, M, c0, k0, F, M, vec_w2, tid);
    ghr_fetch_in(wa, w1, M, c0, k0, F, M, vec_w1, tid);
    ghr_fetch_in(wg, w1 + (long long)F * M, M, c0, k0, F, M, vec_w1, tid);
  };
  fetch(0);
  for (int k0 = 0; k0 < M; k0 += GX_KS) {
    __syncthreads();                                           // the previous slab has been read by every wave
    ghr_put(xg, s_g, GX_P, tid);
#pragma unroll
    for (int it = 0; it < 2; ++it) {                           // the LayerNorm on the way in, as gx_put_x<PRO_LN>
      const int i = tid + it * GHR_BLOCK, r = i / 8, c = 4 * (i % 8);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) s_h[r * GX_P + c + jj] = ((xh.v[it][jj] - ln[it][0]) * ln[it][1]) * gamma[k0 + c + jj] + beta[k0 + c + jj];
    }
    ghr_put(wu, s_wu, GX_P, tid);
    ghr_put(wa, s_wa, GX_P, tid);
    ghr_put(wg, s_wg, GX_P, tid);
    __syncthreads();
    if (k0 + GX_KS < M) fetch(k0 + GX_KS);
    const int ao = (32 * wr + col) * GX_P + half, bo = (32 * wc + col) * GX_P + half;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float hv = s_h[ao + 2 * s];
      du = __builtin_amdgcn_mfma_f32_32x32x2f32(s_g[ao + 2 * s], s_wu[bo + 2 * s], du, 0, 0, 0);
      aa = __builtin_amdgcn_mfma_f32_32x32x2f32(hv, s_wa[bo + 2 * s], aa, 0, 0, 0);
      ag = __builtin_amdgcn_mfma_f32_32x32x2f32(hv, s_wg[bo + 2 * s], ag, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long t = row0 + 32 * wr + ghr_acc_row(r, half);
    if (t < T) {
      const float gv = ag[r], e = 1.0f + erff(gv * 0.70710678118654752440f);
      const float gelu = (0.5f * gv) * e;
      const float dgelu = 0.5f * e + (gv * 0.39894228f) * expf((-0.5f * gv) * gv);
      y[t * y_stride + j] = du[r] * gelu;
      y[t * y_stride + F + j] = (du[r] * aa[r]) * dgelu;
    }
  }
}

// ---- LayerNorm: one wave per row, g += the norm's backward of dn ---------------------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_ln_bwd_kernel(const float* __restrict__ dn, long long dn_stride, const float* __restrict__ x,
                                                               long long x_stride, const float* __restrict__ mom, const float* __restrict__ gamma,
                                                               int T, int K, float* __restrict__ g, long long g_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * GX_LN_ROWS + wave;
  if (row >= T) return;                                        // wave-uniform; the kernel has no barrier
  const float* dr = dn + row * dn_stride;
  const float* xr = x + row * x_stride;
  float* gr = g + row * g_stride;
  const float mean = mom[2 * row], rstd = mom[2 * row + 1];
  float s1 = 0.f, s2 = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = dr[k] * gamma[k], xh = (xr[k] - mean) * rstd;
    s1 += w;
    s2 = fmaf(w, xh, s2);
  }
  s1 = gx_wave_sum(s1) / (float)K;
  s2 = gx_wave_sum(s2) / (float)K;
  for (int k = lane; k < K; k += 64) {
    const float w = dr[k] * gamma[k], xh = (xr[k] - mean) * rstd;
    gr[k] = gr[k] + rstd * ((w - s1) - xh * s2);
  }
}

// ---- GroupNorm: the two sums per (batch, group), then the element-wise pass ---------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_gn_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                    const float* __restrict__ mom, const float* __restrict__ gamma, int C, int N,
                                                                    int G, int cpg, int nchunks, float eps, float* __restrict__ part) {
  __shared__ float s_red[4];
  const int chunk = blockIdx.x % nchunks, bg = blockIdx.x / nchunks, b = bg / G, gi = bg - b * G;
  const int n = chunk * GH_XF_GN_CHUNK + threadIdx.x;
  const long long base = ((long long)b * C + (long long)gi * cpg) * N + n;
  const float mean = mom[2 * (long long)bg], rstd = 1.0f / sqrtf(mom[2 * (long long)bg + 1] / ((float)cpg * (float)N) + eps);
  float s1 = 0.f, s2 = 0.f;
  if (n < N) {
    for (int c = 0; c < cpg; ++c) {
      const float w = dy[base + (long long)c * N] * gamma[gi * cpg + c], xh = (x[base + (long long)c * N] - mean) * rstd;
      s1 += w;
      s2 = fmaf(w, xh, s2);
    }
  }
  const float t1 = gx_block_sum(s1, s_red), t2 = gx_block_sum(s2, s_red);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = t1;
    part[2 * (long long)blockIdx.x + 1] = t2;
  }
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_gn_bwd_join_kernel(const float* __restrict__ part, int BG, int nchunks, float* __restrict__ sums) {
  const int bg = blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (bg >= BG) return;
  const float* p = part + 2 * (long long)bg * nchunks;
  float s1 = p[0], s2 = p[1];
  for (int c = 1; c < nchunks; ++c) {
    s1 += p[2 * c];
    s2 += p[2 * c + 1];
  }
  sums[2 * bg] = s1;
  sums[2 * bg + 1] = s2;
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_gn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                     const float* __restrict__ mom, const float* __restrict__ gamma,
                                                                     const float* __restrict__ sums, const float* __restrict__ dout,
                                                                     float* __restrict__ dx, int C, int N, int G, int cpg, int nchunks, float eps) {
  const int chunk = blockIdx.x % nchunks, bc = blockIdx.x / nchunks, b = bc / C, c = bc - b * C;
  const int n = chunk * GH_XF_GN_CHUNK + threadIdx.x;
  if (n >= N) return;
  const long long bg = (long long)b * G + c / cpg, i = (long long)bc * N + n;
  const float cnt = (float)cpg * (float)N;
  const float mean = mom[2 * bg], rstd = 1.0f / sqrtf(mom[2 * bg + 1] / cnt + eps);
  const float s1 = sums[2 * bg] / cnt, s2 = sums[2 * bg + 1] / cnt;
  const float w = dy[i] * gamma[c], xh = (x[i] - mean) * rstd;
  dx[i] = dout[i] + rstd * ((w - s1) - xh * s2);
}

// ---- host: the single launches of the backward -----------------------------------------------------------------------------------------
extern "C" size_t gh_xf_attention_backward_workspace_bytes(int B, int N, int heads) {
  if (B <= 0 || N <= 0 || heads <= 0 || (long long)B * N > GH_XF_MAX_T || heads > GH_XF_MAX_M / 32) return 0;
  return ghr_align((size_t)B * N * heads * sizeof(float));
}

extern "C" int gh_xf_attention_backward(const float* qkv, int64_t qkv_stride, const float* out, int64_t out_stride, const float* lse,
                                        const float* dout, int64_t dout_stride, int B, int N, int heads, int D, float* dqkv,
                                        int64_t dqkv_stride, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  int grid = 0;
  int rc = gx_check_attn(B, N, heads, D, &grid, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  const int M = heads * D, nt = (N + GH_XF_ATTN_BWD_ROWS - 1) / GH_XF_ATTN_BWD_ROWS;
  if (gx_tiles(2LL * B * heads, nt, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;   // key blocks, then query blocks
  const int nkv = grid / 2;
  const float* in[] = {qkv, out, lse, dout};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!dqkv || !ghr_al4(dqkv) || qkv_stride < 3 * M || out_stride < M || dout_stride < M || dqkv_stride < 3 * M) return GH_ERR_INVALID_ARG;
  if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_xf_attention_backward_workspace_bytes(B, N, heads)) return GH_ERR_WORKSPACE_SMALL;
  float* delta = (float*)workspace;
  const int vec = ghr_al16(qkv) && qkv_stride % 4 == 0, vec_d = ghr_al16(dout) && dout_stride % 4 == 0;
  const float scale = (float)(1.0 / sqrt((double)D));
  const long long T = (long long)B * N;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_attn_delta_kernel, dim3((unsigned)((T * heads + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, dout,
                     (long long)dout_stride, out, (long long)out_stride, T, N, heads, D, delta);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  if (D == 32) {
    hipLaunchKernelGGL(gx_attn_bwd_kernel<1>, dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, qkv, (long long)qkv_stride, dout, (long long)dout_stride,
                       lse, (const float*)delta, dqkv, (long long)dqkv_stride, N, heads, scale, vec, vec_d, nt, nkv);
  } else {
    hipLaunchKernelGGL(gx_attn_bwd_kernel<2>, dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, qkv, (long long)qkv_stride, dout, (long long)dout_stride,
                       lse, (const float*)delta, dqkv, (long long)dqkv_stride, N, heads, scale, vec, vec_d, nt, nkv);
  }
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_xf_geglu_backward(const float* g, int64_t g_stride, const float* h, int64_t h_stride, const float* moments, const float* gamma,
                                    const float* beta, const float* w1, const float* b1, const float* w2t, int T, int M, float* y,
                                    int64_t y_stride, void* hip_stream) {
  if (T < 0 || M < 1) return GH_ERR_INVALID_ARG;
  if (M % 32 != 0 || M > GH_XF_MAX_M || T > GH_XF_MAX_T) return GH_ERR_UNSUPPORTED;
  if (T == 0) return GH_OK;
  int grid;
  const int ncol = 4 * M / GX_TC;
  if (gx_tiles(ncol, (T + GX_TR - 1) / GX_TR, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;
  const float* in[] = {g, h, moments, gamma, beta, w1, b1, w2t};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!y || !ghr_al4(y) || g_stride < M || h_stride < M || y_stride < 8 * (int64_t)M) return GH_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_geglu_bwd_kernel, dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, g, (long long)g_stride, h, (long long)h_stride, moments, gamma,
                     beta, w1, b1, w2t, y, (long long)y_stride, T, M, (int)(ghr_al16(g) && g_stride % 4 == 0), (int)(ghr_al16(h) && h_stride % 4 == 0),
                     (int)ghr_al16(w1), (int)ghr_al16(w2t), ncol);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_xf_layernorm_backward(const float* dn, int64_t dn_stride, const float* x, int64_t x_stride, const float* moments,
                                        const float* gamma, int T, int K, float* g, int64_t g_stride, void* hip_stream) {
  if (T < 0 || K < 1) return GH_ERR_INVALID_ARG;
  if (T > GH_XF_MAX_T || K > GH_XF_MAX_K) return GH_ERR_UNSUPPORTED;
  if (T == 0) return GH_OK;
  const float* in[] = {dn, x, moments, gamma};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!g || !ghr_al4(g) || dn_stride < K || x_stride < K || g_stride < K) return GH_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_ln_bwd_kernel, dim3((unsigned)((T + GX_LN_ROWS - 1) / GX_LN_ROWS)), dim3(GHR_BLOCK), 0, s, dn, (long long)dn_stride, x,
                     (long long)x_stride, moments, gamma, T, K, g, (long long)g_stride);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

static int gx_check_gn_bwd(int B, int C, int N, int G, bool* empty) {
  const int rc = gx_check_groups(B, C, N, G, empty);
  if (rc != GH_OK || *empty) return rc;
  int grid;
  if (gx_tiles((long long)B * C, (N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, &grid) != GH_OK) { *empty = true; return GH_ERR_UNSUPPORTED; }
  return GH_OK;
}

// the chunks' partial sums (B G nchunks, 2), then the joined sums (B G, 2)
extern "C" size_t gh_xf_group_norm_backward_workspace_bytes(int B, int C, int N, int G) {
  bool empty;
  if (gx_check_gn_bwd(B, C, N, G, &empty) != GH_OK || empty) return 0;
  return ghr_align((size_t)B * G * ((N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK) * 2 * sizeof(float)) + ghr_align((size_t)B * G * 2 * sizeof(float));
}

extern "C" int gh_xf_group_norm_backward(const float* dy, const float* x, const float* moments, const float* gamma, const float* dout, float* dx,
                                         int B, int C, int N, int G, float eps, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_gn_bwd(B, C, N, G, &empty);
  if (rc != GH_OK) return rc;
  if (!(eps >= 0.f && isfinite(eps))) return GH_ERR_INVALID_ARG;
  if (empty) return GH_OK;
  const float* in[] = {dy, x, moments, gamma, dout};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!dx || !ghr_al4(dx) || dx == dy || dx == x || dx == dout || !workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_xf_group_norm_backward_workspace_bytes(B, C, N, G)) return GH_ERR_WORKSPACE_SMALL;
  const int nchunks = (N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK, BG = B * G, cpg = C / G;
  float* part = (float*)workspace;
  float* sums = (float*)((char*)workspace + ghr_align((size_t)BG * nchunks * 2 * sizeof(float)));
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_gn_bwd_part_kernel, dim3((unsigned)(BG * nchunks)), dim3(GHR_BLOCK), 0, s, dy, x, moments, gamma, C, N, G, cpg, nchunks, eps,
                     part);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(gx_gn_bwd_join_kernel, dim3((unsigned)((BG + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, (const float*)part, BG, nchunks,
                     sums);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(gx_gn_bwd_apply_kernel, dim3((unsigned)(B * C * nchunks)), dim3(GHR_BLOCK), 0, s, dy, x, moments, gamma, (const float*)sums, dout,
                     dx, C, N, G, cpg, nchunks, eps);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

// ==== the parameters' gradients (include/gh_xf.h) ========================================================================================
#define GW_TS GH_XF_WGRAD_ROWS     // rows of dY and of X per slab
#define GW_P 65                    // LDS pitch of a slab's 64 columns: odd, so that lane = row writes without a bank conflict

static_assert(GW_TS == 32 && GH_XF_WGRAD_CHUNK % GW_TS == 0, "GhrSlab<2, 16> is 32 rows x 64 columns; a chunk is whole slabs");

// One operand slab (32 rows x 64 columns) on its way into LDS. Rows: gh_rows.h's window, thread i moves rows i / 16 and (i + 256) / 16.
// Channel first: thread i owns slab row i & 31 and the columns (i >> 5) + 8 it.
struct GxWSlab {
  GhrSlab<2, 16> w;
  float g[8];
};

template <bool CF>
__device__ __forceinline__ void gx_wfetch(GxWSlab& t, const float* __restrict__ p, long long stride, long long stride_b, int N, int t0, int t_hi,
                                          int c0, int ncols, int vec, int tid) {
  if constexpr (CF) {
    const int tt = t0 + (tid & 31);
    const bool live = tt < t_hi;
    const int b = live ? tt / N : 0, n = live ? tt - b * N : 0;
    const long long base = (long long)b * stride_b + n;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int c = c0 + (tid >> 5) + 8 * it;
      t.g[it] = live && c < ncols ? p[base + (long long)c * stride] : 0.f;
    }
  } else {
    ghr_fetch_in(t.w, p, stride, t0, c0, t_hi, ncols, vec, tid);
  }
}

template <bool CF>
__device__ __forceinline__ void gx_wput(const GxWSlab& t, float* s, int tid) {
  if constexpr (CF) {
#pragma unroll
    for (int it = 0; it < 8; ++it) s[(tid & 31) * GW_P + (tid >> 5) + 8 * it] = t.g[it];
  } else {
    ghr_put(t.w, s, GW_P, tid);
  }
}

// X's slab through the prologue into LDS, each element formed as gx_put_x forms it; a row past t_hi or a column past K is zero
template <int PRO>
__device__ __forceinline__ void gx_wput_x(const GxWSlab& t, float* s, const GhXfWgrad& a, int t0, int t_hi, int k0, const float (&ln)[2][2], int tid) {
  if constexpr (PRO == GH_XF_PRO_GN) {
    const int tt = t0 + (tid & 31), N = a.rows_per_batch, cpg = a.K / a.groups;
    const bool live = tt < t_hi;
    const float* mom = a.moments + 2 * (long long)(live ? tt / N : 0) * a.groups;
    const float cnt = (float)cpg * (float)N;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int kk = (tid >> 5) + 8 * it, c = k0 + kk;
      float v = 0.f;
      if (live && c < a.K) {
        const int g = c / cpg;
        const float rstd = 1.0f / sqrtf(mom[2 * g + 1] / cnt + a.eps);
        v = ((t.g[it] - mom[2 * g]) * rstd) * a.gamma[c] + a.beta[c];
      }
      s[(tid & 31) * GW_P + kk] = v;
    }
  } else if constexpr (PRO == GH_XF_PRO_LN) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + it * GHR_BLOCK, r = i / 16, c = 4 * (i % 16);
      const bool live = t0 + r < t_hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + c + j;
        s[r * GW_P + c + j] = live && k < a.K ? ((t.w.v[it][j] - ln[it][0]) * ln[it][1]) * a.gamma[k] + a.beta[k] : 0.f;
      }
    }
  } else {
    gx_wput<PRO == GH_XF_PRO_CF>(t, s, tid);
  }
}

template <int PRO, bool DYCF>
__global__ __launch_bounds__(GHR_BLOCK) void gx_wgrad_kernel(GhXfWgrad a, int chunk, int nchunks, int ntj, int ntk, float* __restrict__ part_w,
                                                              float* __restrict__ part_b, int vec_x, int vec_dy) {
  __shared__ float s_dy[GW_TS * GW_P];
  __shared__ float s_x[GW_TS * GW_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, half = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int tk = blockIdx.x % ntk, rest = blockIdx.x / ntk, tj = rest % ntj, ch = rest / ntj;
  const int j0 = tj * 64, k0 = tk * 64;
  const int t_lo = ch * chunk, t_hi = a.T - t_lo < chunk ? a.T : t_lo + chunk;
  const bool want_w = a.dw != nullptr, want_b = a.db != nullptr && tk == 0;   // workgroup-uniform
  constexpr bool XCF = gx_cf<PRO>;

  ghr_acc acc = gx_splat(0.f);
  float bsum = 0.f;
  float ln[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  GxWSlab xs, ds;
  auto fetch = [&](int t0) {
    gx_wfetch<DYCF>(ds, a.dy, a.dy_stride, a.dy_stride_b, a.rows_per_batch, t0, t_hi, j0, a.N_out, vec_dy, tid);
    if (want_w) {
      gx_wfetch<XCF>(xs, a.x, a.x_stride, a.x_stride_b, a.rows_per_batch, t0, t_hi, k0, a.K, vec_x, tid);
      if constexpr (PRO == GH_XF_PRO_LN) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int r = t0 + (tid + it * GHR_BLOCK) / 16;
          if (r < t_hi) {
            ln[it][0] = a.moments[2 * (long long)r];
            ln[it][1] = a.moments[2 * (long long)r + 1];
          }
        }
      }
    }
  };
  fetch(t_lo);
  for (int t0 = t_lo; t0 < t_hi; t0 += GW_TS) {
    __syncthreads();                                           // the previous slab has been read by every wave
    gx_wput<DYCF>(ds, s_dy, tid);
    if (want_w) gx_wput_x<PRO>(xs, s_x, a, t0, t_hi, k0, ln, tid);
    __syncthreads();
    if (t0 + GW_TS < t_hi) fetch(t0 + GW_TS);                  // the next slab's loads fly under this slab's products
    if (want_w) {
      const float* ap = s_dy + half * GW_P + 32 * wr + col;
      const float* bp = s_x + half * GW_P + 32 * wc + col;
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * GW_P], bp[2 * s * GW_P], acc, 0, 0, 0);
    }
    if (want_b && wave == 0) {                                 // lane = column of the tile: one ascending chain over the rows
      const int rl = t_hi - t0 < GW_TS ? t_hi - t0 : GW_TS;
      for (int r = 0; r < rl; ++r) bsum += s_dy[r * GW_P + lane];
    }
  }

  if (want_w) {
    float* dst = nchunks > 1 ? part_w + (long long)ch * a.N_out * a.K : a.dw;
    const int k = k0 + 32 * wc + col;
    if (k < a.K) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + 32 * wr + ghr_acc_row(r, half);
        if (j < a.N_out) dst[(long long)j * a.K + k] = acc[r];
      }
    }
  }
  if (want_b && wave == 0 && j0 + lane < a.N_out) (nchunks > 1 ? part_b + (long long)ch * a.N_out : a.db)[j0 + lane] = bsum;
}

// element e of dw (nw of them), then of db (nb): the chunks' partials in ascending order
__global__ __launch_bounds__(GHR_BLOCK) void gx_wgrad_join_kernel(const float* __restrict__ part_w, long long nw, float* __restrict__ dw,
                                                                   const float* __restrict__ part_b, int nb, float* __restrict__ db, int nchunks) {
  const long long e = (long long)blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (e < nw) {
    float s = part_w[e];
    for (int c = 1; c < nchunks; ++c) s += part_w[c * nw + e];
    dw[e] = s;
  } else if (e - nw < nb) {
    const long long j = e - nw;
    float s = part_b[j];
    for (int c = 1; c < nchunks; ++c) s += part_b[(long long)c * nb + j];
    db[j] = s;
  }
}

// ---- LayerNorm: dgamma and dbeta, two stages ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_ln_pgrad_part_kernel(const float* __restrict__ dn, long long dn_stride, const float* __restrict__ x,
                                                                      long long x_stride, const float* __restrict__ mom, int T, int K, int nct,
                                                                      float* __restrict__ part) {
  __shared__ float s_red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ct = blockIdx.x % nct, rc = blockIdx.x / nct, k = ct * 64 + lane;
  const long long r0 = (long long)rc * GH_XF_LNP_ROWS, r1 = r0 + GH_XF_LNP_ROWS < T ? r0 + GH_XF_LNP_ROWS : T;
  float sg = 0.f, sb = 0.f;
  if (k < K) {
    for (long long r = r0 + wave; r < r1; r += 4) {
      const float d = dn[r * dn_stride + k], xh = (x[r * x_stride + k] - mom[2 * r]) * mom[2 * r + 1];
      sg = fmaf(d, xh, sg);
      sb += d;
    }
  }
  s_red[0][wave][lane] = sg;
  s_red[1][wave][lane] = sb;
  __syncthreads();
  if (wave == 0 && k < K) {
    part[(2 * (long long)rc) * K + k] = (s_red[0][0][lane] + s_red[0][1][lane]) + (s_red[0][2][lane] + s_red[0][3][lane]);
    part[(2 * (long long)rc + 1) * K + k] = (s_red[1][0][lane] + s_red[1][1][lane]) + (s_red[1][2][lane] + s_red[1][3][lane]);
  }
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_ln_pgrad_join_kernel(const float* __restrict__ part, int nrc, int K, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta) {
  const int k = blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (k >= K) return;
  float sg = part[k], sb = part[K + k];
  for (int c = 1; c < nrc; ++c) {
    sg += part[(2 * (long long)c) * K + k];
    sb += part[(2 * (long long)c + 1) * K + k];
  }
  if (dgamma) dgamma[k] = sg;
  if (dbeta) dbeta[k] = sb;
}

// ---- GroupNorm: dgamma and dbeta per channel, two stages ---------------------------------------------------------------------------------
__global__ __launch_bounds__(GHR_BLOCK) void gx_gn_pgrad_part_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ mom, int B, int C, int N, int G, int cpg, int nchunks,
                                                                      float eps, float* __restrict__ part) {
  __shared__ float s_red[4];
  const int chunk = blockIdx.x % nchunks, bc = blockIdx.x / nchunks, b = bc / C, c = bc - b * C;
  const int n = chunk * GH_XF_GN_CHUNK + threadIdx.x;
  const long long bg = (long long)b * G + c / cpg, i = (long long)bc * N + n;
  const float mean = mom[2 * bg], rstd = 1.0f / sqrtf(mom[2 * bg + 1] / ((float)cpg * (float)N) + eps);
  float sg = 0.f, sb = 0.f;
  if (n < N) {
    sb = dy[i];
    sg = sb * ((x[i] - mean) * rstd);
  }
  const float t1 = gx_block_sum(sg, s_red), t2 = gx_block_sum(sb, s_red);
  if (threadIdx.x == 0) {
    const long long o = 2 * (((long long)c * B + b) * nchunks + chunk);
    part[o] = t1;
    part[o + 1] = t2;
  }
}

__global__ __launch_bounds__(GHR_BLOCK) void gx_gn_pgrad_join_kernel(const float* __restrict__ part, int C, int per, float* __restrict__ dgamma,
                                                                      float* __restrict__ dbeta) {
  const int c = blockIdx.x * GHR_BLOCK + threadIdx.x;
  if (c >= C) return;
  const float* p = part + 2 * (long long)c * per;
  float sg = p[0], sb = p[1];
  for (int i = 1; i < per; ++i) {
    sg += p[2 * i];
    sb += p[2 * i + 1];
  }
  if (dgamma) dgamma[c] = sg;
  if (dbeta) dbeta[c] = sb;
}

// ---- host: the single launches of the parameters' gradients -------------------------------------------------------------------------------
static int gx_wgrad_sizes_ok(long long T, int K, int N_out) {
  return T >= 1 && T <= GH_XF_MAX_T && K >= 32 && K % 32 == 0 && K <= GH_XF_MAX_K && N_out >= 1 && N_out <= GH_XF_MAX_N_OUT;
}

extern "C" int gh_xf_linear_wgrad_chunk(int T, int K, int N_out) {
  if (!gx_wgrad_sizes_ok(T, K, N_out)) return 0;
  const long long tiles = (long long)((N_out + 63) / 64) * ((K + 63) / 64);
  long long c = GH_XF_WGRAD_CHUNK;
  while (c < T && tiles * ((T + c - 1) / c) > GH_XF_WGRAD_MAX_BLOCKS) c *= 2;
  return (int)c;
}

extern "C" size_t gh_xf_linear_wgrad_workspace_bytes(int T, int K, int N_out) {
  const int chunk = gh_xf_linear_wgrad_chunk(T, K, N_out);
  if (chunk == 0) return 0;
  const size_t nchunks = ((size_t)T + chunk - 1) / chunk;
  if (nchunks <= 1) return 0;
  return ghr_align(nchunks * N_out * K * sizeof(float)) + ghr_align(nchunks * N_out * sizeof(float));
}

template <int PRO>
static void gx_launch_wgrad(const GhXfWgrad& a, int chunk, int nchunks, int ntj, int ntk, float* pw, float* pb, int vec_x, int vec_dy, int grid,
                            hipStream_t s) {
  const dim3 g((unsigned)grid), blk(GHR_BLOCK);
  if (a.dy_cf) hipLaunchKernelGGL((gx_wgrad_kernel<PRO, true>), g, blk, 0, s, a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy);
  else hipLaunchKernelGGL((gx_wgrad_kernel<PRO, false>), g, blk, 0, s, a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy);
}

extern "C" int gh_xf_linear_wgrad(const GhXfWgrad* a, void* workspace, size_t ws_bytes, void* hip_stream) {
  if (!a || a->T < 0 || a->K < 1 || a->N_out < 1 || a->prologue < GH_XF_PRO_NONE || a->prologue > GH_XF_PRO_CF || (a->dy_cf != 0 && a->dy_cf != 1))
    return GH_ERR_INVALID_ARG;
  if (a->K % 32 != 0 || a->K > GH_XF_MAX_K || a->T > GH_XF_MAX_T || a->N_out > GH_XF_MAX_N_OUT) return GH_ERR_UNSUPPORTED;
  const bool xcf = a->prologue == GH_XF_PRO_GN || a->prologue == GH_XF_PRO_CF;
  const bool normed = a->prologue == GH_XF_PRO_LN || a->prologue == GH_XF_PRO_GN;
  if ((xcf || a->dy_cf) && a->T > 0 && (a->rows_per_batch < 1 || a->T % a->rows_per_batch != 0)) return GH_ERR_INVALID_ARG;
  if (a->prologue == GH_XF_PRO_GN && (a->groups < 1 || a->K % a->groups != 0 || !(a->eps >= 0.f && isfinite(a->eps)))) return GH_ERR_INVALID_ARG;
  if (a->T == 0 || (!a->dw && !a->db)) return GH_OK;
  if (!a->dy || !ghr_al4(a->dy) || !ghr_al4(a->dw) || !ghr_al4(a->db)) return GH_ERR_INVALID_ARG;
  if (!a->dy_cf && a->dy_stride < a->N_out) return GH_ERR_INVALID_ARG;
  if (a->dw) {
    if (!a->x || !ghr_al4(a->x) || (!xcf && a->x_stride < a->K)) return GH_ERR_INVALID_ARG;
    if (normed && (!a->gamma || !a->beta || !a->moments || !ghr_al4(a->gamma) || !ghr_al4(a->beta) || !ghr_al4(a->moments))) return GH_ERR_INVALID_ARG;
  }
  const int chunk = gh_xf_linear_wgrad_chunk(a->T, a->K, a->N_out), nchunks = (a->T + chunk - 1) / chunk;
  const int ntj = (a->N_out + 63) / 64, ntk = a->dw ? (a->K + 63) / 64 : 1;
  int grid;
  if (gx_tiles((long long)nchunks * ntj, ntk, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;
  float *pw = nullptr, *pb = nullptr;
  const long long nw = (long long)a->N_out * a->K;
  if (nchunks > 1) {
    if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
    if (ws_bytes < gh_xf_linear_wgrad_workspace_bytes(a->T, a->K, a->N_out)) return GH_ERR_WORKSPACE_SMALL;
    pw = (float*)workspace;
    pb = (float*)((char*)workspace + ghr_align((size_t)nchunks * nw * sizeof(float)));
  }
  const int vec_x = !xcf && a->x && ghr_al16(a->x) && a->x_stride % 4 == 0, vec_dy = !a->dy_cf && ghr_al16(a->dy) && a->dy_stride % 4 == 0;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  switch (a->prologue) {
    case GH_XF_PRO_NONE: gx_launch_wgrad<GH_XF_PRO_NONE>(*a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy, grid, s); break;
    case GH_XF_PRO_LN: gx_launch_wgrad<GH_XF_PRO_LN>(*a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy, grid, s); break;
    case GH_XF_PRO_CF: gx_launch_wgrad<GH_XF_PRO_CF>(*a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy, grid, s); break;
    default: gx_launch_wgrad<GH_XF_PRO_GN>(*a, chunk, nchunks, ntj, ntk, pw, pb, vec_x, vec_dy, grid, s); break;
  }
  if (!gx_launched()) return GH_ERR_LAUNCH;
  if (nchunks > 1) {
    const long long n_w = a->dw ? nw : 0;
    const int n_b = a->db ? a->N_out : 0;
    hipLaunchKernelGGL(gx_wgrad_join_kernel, dim3((unsigned)((n_w + n_b + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, (const float*)pw, n_w,
                       a->dw, (const float*)pb, n_b, a->db, nchunks);
    if (!gx_launched()) return GH_ERR_LAUNCH;
  }
  return GH_OK;
}

extern "C" size_t gh_xf_layernorm_param_grads_workspace_bytes(int T, int K) {
  if (T <= 0 || T > GH_XF_MAX_T || K < 1 || K > GH_XF_MAX_K) return 0;
  return ghr_align((size_t)((T + GH_XF_LNP_ROWS - 1) / GH_XF_LNP_ROWS) * 2 * K * sizeof(float));
}

extern "C" int gh_xf_layernorm_param_grads(const float* dn, int64_t dn_stride, const float* x, int64_t x_stride, const float* moments, int T, int K,
                                           float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* hip_stream) {
  if (T < 0 || K < 1) return GH_ERR_INVALID_ARG;
  if (T > GH_XF_MAX_T || K > GH_XF_MAX_K) return GH_ERR_UNSUPPORTED;
  if (T == 0 || (!dgamma && !dbeta)) return GH_OK;
  const int nrc = (T + GH_XF_LNP_ROWS - 1) / GH_XF_LNP_ROWS, nct = (K + 63) / 64;
  int grid;
  if (gx_tiles(nrc, nct, &grid) != GH_OK) return GH_ERR_UNSUPPORTED;
  const float* in[] = {dn, x, moments};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!ghr_al4(dgamma) || !ghr_al4(dbeta) || dn_stride < K || x_stride < K || !workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_xf_layernorm_param_grads_workspace_bytes(T, K)) return GH_ERR_WORKSPACE_SMALL;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_ln_pgrad_part_kernel, dim3((unsigned)grid), dim3(GHR_BLOCK), 0, s, dn, (long long)dn_stride, x, (long long)x_stride, moments, T,
                     K, nct, (float*)workspace);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(gx_ln_pgrad_join_kernel, dim3((unsigned)((K + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, (const float*)workspace, nrc, K,
                     dgamma, dbeta);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" size_t gh_xf_group_norm_param_grads_workspace_bytes(int B, int C, int N, int G) {
  bool empty;
  if (gx_check_gn_bwd(B, C, N, G, &empty) != GH_OK || empty) return 0;
  return ghr_align((size_t)B * C * ((N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK) * 2 * sizeof(float));
}

extern "C" int gh_xf_group_norm_param_grads(const float* dy, const float* x, const float* moments, int B, int C, int N, int G, float eps,
                                            float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_gn_bwd(B, C, N, G, &empty);
  if (rc != GH_OK) return rc;
  if (!(eps >= 0.f && isfinite(eps))) return GH_ERR_INVALID_ARG;
  if (empty || (!dgamma && !dbeta)) return GH_OK;
  const float* in[] = {dy, x, moments};
  for (const float* p : in) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  if (!ghr_al4(dgamma) || !ghr_al4(dbeta) || !workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_xf_group_norm_param_grads_workspace_bytes(B, C, N, G)) return GH_ERR_WORKSPACE_SMALL;
  const int nchunks = (N + GH_XF_GN_CHUNK - 1) / GH_XF_GN_CHUNK;
  if ((long long)B * nchunks > INT_MAX) return GH_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gx_gn_pgrad_part_kernel, dim3((unsigned)(B * C * nchunks)), dim3(GHR_BLOCK), 0, s, dy, x, moments, B, C, N, G, C / G, nchunks, eps,
                     (float*)workspace);
  if (!gx_launched()) return GH_ERR_LAUNCH;
  hipLaunchKernelGGL(gx_gn_pgrad_join_kernel, dim3((unsigned)((C + GHR_BLOCK - 1) / GHR_BLOCK)), dim3(GHR_BLOCK), 0, s, (const float*)workspace, C,
                     B * nchunks, dgamma, dbeta);
  return gx_launched() ? GH_OK : GH_ERR_LAUNCH;
}

// ---- host: the whole backward ------------------------------------------------------------------------------------------------------------
// the workspace: the stream's cotangent g (T, M), dn (T, M), wide (T, 8M) — [da | dg], or datt (T, M) followed by dqkv (T, 3M) —, the
// attention's delta, dy (B, C, N) of the GroupNorm, and the GroupNorm's partial sums
struct GxBackPlan {
  size_t g, dn, wide, delta, dy, gnw, total;
};

static GxBackPlan gx_back_plan(const GhXfDims* d) {
  const size_t T = (size_t)d->B * d->N, M = (size_t)d->heads * d->D, f = sizeof(float);
  GxBackPlan p;
  size_t at = 0;
  p.g = at; at += ghr_align(T * M * f);
  p.dn = at; at += ghr_align(T * M * f);
  p.wide = at; at += ghr_align(T * 8 * M * f);
  p.delta = at; at += gh_xf_attention_backward_workspace_bytes(d->B, d->N, d->heads);
  p.dy = at; at += ghr_align(T * d->C * f);
  p.gnw = at; at += gh_xf_group_norm_backward_workspace_bytes(d->B, d->C, d->N, d->G);
  p.total = at;
  return p;
}

extern "C" size_t gh_xf_backward_workspace_bytes(const GhXfDims* dims) {
  bool empty;
  if (gx_check_grad_dims(dims, &empty) != GH_OK || empty) return 0;
  return gx_back_plan(dims).total;
}

// what gh_xf_backward_params adds to the chain: the forward's weights (the norms' shifts, and what forms a * gelu(g) and the final stream
// again), where the gradients go, and its own parts of the workspace
struct GxParamJob {
  const GhXfStem* fs;
  const GhXfLayer* fl;
  const GhXfStemG* gs;
  const GhXfLayerG* gl;
  size_t ln, wg, np, total;                                    // the recomputed GEGLU's row moments; the product's partials; the norms' partials
};

static size_t gx_max(size_t a, size_t b) { return a > b ? a : b; }

static void gx_param_plan(const GhXfDims* d, GxParamJob* j) {
  const int T = d->B * d->N, M = d->heads * d->D, C = d->C;
  size_t at = gx_back_plan(d).total;
  j->ln = at; at += gh_xf_linear_workspace_bytes(T, GH_XF_PRO_LN);
  size_t wg = gh_xf_linear_wgrad_workspace_bytes(T, M, C);
  wg = gx_max(wg, gh_xf_linear_wgrad_workspace_bytes(T, C, M));
  wg = gx_max(wg, gh_xf_linear_wgrad_workspace_bytes(T, 4 * M, M));
  wg = gx_max(wg, gh_xf_linear_wgrad_workspace_bytes(T, M, 8 * M));
  wg = gx_max(wg, gh_xf_linear_wgrad_workspace_bytes(T, M, M));
  wg = gx_max(wg, gh_xf_linear_wgrad_workspace_bytes(T, M, 3 * M));
  j->wg = at; at += wg;
  j->np = at; at += gx_max(gh_xf_layernorm_param_grads_workspace_bytes(T, M), gh_xf_group_norm_param_grads_workspace_bytes(d->B, C, d->N, d->G));
  j->total = at;
}

// pj == nullptr: the backward to x alone. Otherwise the same launches in the same order with the parameters' beside them.
static int gx_backward(const GhXfDims* d, const GhXfStemT* stem, const GhXfLayerT* layers, const float* x, const void* tape_, const float* dout,
                       float* dx, void* workspace, size_t ws_bytes, void* hip_stream, const GxParamJob* pj) {
  int rc;
  if (!stem || (d->layers > 0 && !layers) || !x || !dout || (!dx && !pj) || dx == x || dx == dout || !ghr_al4(x) || !ghr_al4(dout) || !ghr_al4(dx))
    return GH_ERR_INVALID_ARG;
  const float* sp[] = {stem->gn_w, stem->in_t, stem->out_t};
  for (const float* p : sp) {
    if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
  }
  for (int i = 0; i < d->layers; ++i) {
    const GhXfLayerT& L = layers[i];
    const float* need[] = {L.ln1_w, L.qkv1_t, L.o1_t, L.ln3_w, L.ln3_b, L.ff1_w, L.ff1_b, L.ff1_t, L.ff2_t};
    for (const float* p : need) {
      if (!p || !ghr_al4(p)) return GH_ERR_INVALID_ARG;
    }
    if (L.qkv2_t && (!ghr_al4(L.qkv2_t) || !L.ln2_w || !ghr_al4(L.ln2_w) || !L.o2_t || !ghr_al4(L.o2_t))) return GH_ERR_INVALID_ARG;
  }
  if (!tape_ || !ghr_al16(tape_) || !workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  const GxBackPlan p = gx_back_plan(d);
  if (ws_bytes < (pj ? pj->total : p.total)) return GH_ERR_WORKSPACE_SMALL;
  const GxTape tp = gx_tape(d);
  char* tape = (char*)tape_;                                   // read only
  char* ws = (char*)workspace;
  float* g = (float*)(ws + p.g);
  float* dn = (float*)(ws + p.dn);
  float* wide = (float*)(ws + p.wide);
  float* dy = (float*)(ws + p.dy);
  const int T = d->B * d->N, M = d->heads * d->D, C = d->C, N = d->N;

  // the lowest layer the chain has to reach, and whether it goes on through proj_in
  bool below = true;
  int lowest = 0;
  if (pj) {
    if (!pj->fs || !pj->gs || (d->layers > 0 && (!pj->fl || !pj->gl))) return GH_ERR_INVALID_ARG;
    const float* fsp[] = {pj->fs->gn_w, pj->fs->gn_b, pj->fs->in_w, pj->fs->in_b, pj->fs->out_w, pj->fs->out_b};
    for (const float* q : fsp) {
      if (!q || !ghr_al4(q)) return GH_ERR_INVALID_ARG;
    }
    const float* gsp[] = {pj->gs->gn_w, pj->gs->gn_b, pj->gs->in_w, pj->gs->in_b, pj->gs->out_w, pj->gs->out_b};
    for (const float* q : gsp) {
      if (!ghr_al4(q)) return GH_ERR_INVALID_ARG;
    }
    for (int i = 0; i < d->layers; ++i) {
      const GhXfLayer& F = pj->fl[i];
      const float* need[] = {F.ln1_w, F.ln1_b, F.ln3_w, F.ln3_b, F.ff1_w, F.ff1_b, F.ff2_w, F.ff2_b};
      for (const float* q : need) {
        if (!q || !ghr_al4(q)) return GH_ERR_INVALID_ARG;
      }
      if (layers[i].qkv2_t && (!F.ln2_w || !F.ln2_b || !ghr_al4(F.ln2_w) || !ghr_al4(F.ln2_b))) return GH_ERR_INVALID_ARG;
      const GhXfLayerG& Q = pj->gl[i];
      const float* gq[] = {Q.ln1_w, Q.ln1_b, Q.qkv1, Q.o1_w, Q.o1_b, Q.ln2_w, Q.ln2_b, Q.qkv2, Q.o2_w, Q.o2_b, Q.ln3_w, Q.ln3_b, Q.ff1_w, Q.ff1_b, Q.ff2_w, Q.ff2_b};
      for (const float* q : gq) {
        if (!ghr_al4(q)) return GH_ERR_INVALID_ARG;
      }
    }
    below = dx || pj->gs->gn_w || pj->gs->gn_b || pj->gs->in_w || pj->gs->in_b;
    if (!below) {
      lowest = d->layers;
      for (int i = d->layers - 1; i >= 0; --i) {
        const GhXfLayerG& Q = pj->gl[i];
        const bool has2 = layers[i].qkv2_t != nullptr;
        if (Q.ln1_w || Q.ln1_b || Q.qkv1 || Q.o1_w || Q.o1_b || Q.ln3_w || Q.ln3_b || Q.ff1_w || Q.ff1_b || Q.ff2_w || Q.ff2_b ||
            (has2 && (Q.ln2_w || Q.ln2_b || Q.qkv2 || Q.o2_w || Q.o2_b)))
          lowest = i;
      }
    }
  }

  // y (T, n_out) = src (T, K) . wt^T, each element one ascending chain from zero
  auto data = [&](const float* src, int K, const float* wt, int n_out, float* y) {
    GhXfLinear l = {};
    l.T = T; l.K = K; l.N_out = n_out; l.prologue = GH_XF_PRO_NONE; l.epilogue = GH_XF_EPI_PLAIN; l.x = src; l.x_stride = K; l.w = wt; l.y = y;
    l.y_stride = n_out;
    return gh_xf_linear(&l, nullptr, 0, hip_stream);
  };
  // dw (n_out, K) = dysrc^T . P(xsrc) and db = the column sums of dysrc, both over rows (T, .)
  auto wgrad = [&](int pro, const float* xsrc, int K, const float* mom, const float* gamma, const float* beta, const float* dysrc, int n_out,
                   float* dw, float* db) {
    if (!dw && !db) return (int)GH_OK;
    GhXfWgrad w = {};
    w.T = T; w.K = K; w.N_out = n_out; w.prologue = pro; w.x = xsrc; w.x_stride = K; w.dy = dysrc; w.dy_stride = n_out; w.gamma = gamma;
    w.beta = beta; w.moments = mom; w.dw = dw; w.db = db;
    return gh_xf_linear_wgrad(&w, ws + pj->wg, pj->np - pj->wg, hip_stream);
  };
  auto norm_grads = [&](const float* dnp, const float* xp, const float* mom, float* dgamma, float* dbeta) {
    return gh_xf_layernorm_param_grads(dnp, M, xp, M, mom, T, M, dgamma, dbeta, ws + pj->np, pj->total - pj->np, hip_stream);
  };
  // ff (T, 4M) = a * gelu(g) of layer i, by the forward's own launches, into `wide`
  auto reform_ff = [&](int i) {
    const char* fs = gx_slot(tp, tape, i, 2);
    const GhXfLayer& F = pj->fl[i];
    GhXfLinear l = {};
    l.T = T; l.K = M; l.N_out = 4 * M; l.prologue = GH_XF_PRO_LN; l.epilogue = GH_XF_EPI_GEGLU; l.eps = d->ln_eps; l.x = (const float*)fs; l.x_stride = M;
    l.w = F.ff1_w; l.bias = F.ff1_b; l.gamma = F.ln3_w; l.beta = F.ln3_b; l.y = wide; l.y_stride = 4 * M;
    return gh_xf_linear(&l, ws + pj->ln, pj->wg - pj->ln, hip_stream);
  };

  bool ff_formed = false;                                      // `wide` holds the last layer's a * gelu(g)
  if (pj && (pj->gs->out_w || pj->gs->out_b)) {
    float* fin = dn;                                           // the final stream, in the buffer dn takes later
    if (pj->gs->out_w) {
      if (d->layers > 0) {
        const int i = d->layers - 1;
        rc = reform_ff(i);
        if (rc != GH_OK) return rc;
        ff_formed = true;
        GhXfLinear l = {};
        l.T = T; l.K = 4 * M; l.N_out = M; l.prologue = GH_XF_PRO_NONE; l.epilogue = GH_XF_EPI_BIAS_RES; l.x = wide; l.x_stride = 4 * M;
        l.w = pj->fl[i].ff2_w; l.bias = pj->fl[i].ff2_b; l.res = (const float*)gx_slot(tp, tape, i, 2); l.res_stride = M; l.y = fin; l.y_stride = M;
        rc = gh_xf_linear(&l, nullptr, 0, hip_stream);
      } else {
        GhXfLinear l = {};
        l.T = T; l.K = C; l.N_out = M; l.prologue = GH_XF_PRO_GN; l.epilogue = GH_XF_EPI_BIAS_RES; l.rows_per_batch = N; l.groups = d->G;
        l.eps = d->gn_eps; l.x = x; l.x_stride = N; l.x_stride_b = (int64_t)C * N; l.w = pj->fs->in_w; l.bias = pj->fs->in_b; l.gamma = pj->fs->gn_w;
        l.beta = pj->fs->gn_b; l.moments = (const float*)(tape + tp.gn); l.y = fin; l.y_stride = M;
        rc = gh_xf_linear(&l, nullptr, 0, hip_stream);
      }
      if (rc != GH_OK) return rc;
    }
    GhXfWgrad w = {};                                          // dW_out = dout_rows^T . fin, dout read channel first in place
    w.T = T; w.K = M; w.N_out = C; w.prologue = GH_XF_PRO_NONE; w.dy_cf = 1; w.rows_per_batch = N; w.x = fin; w.x_stride = M; w.dy = dout;
    w.dy_stride = N; w.dy_stride_b = (int64_t)C * N; w.dw = pj->gs->out_w; w.db = pj->gs->out_b;
    rc = gh_xf_linear_wgrad(&w, ws + pj->wg, pj->np - pj->wg, hip_stream);
    if (rc != GH_OK) return rc;
  }
  if (pj && !below && lowest >= d->layers) return GH_OK;       // nothing below proj_out is wanted

  GhXfLinear a = {};                                           // g = dout_rows . W_out, dout read channel first in place
  a.T = T; a.K = C; a.N_out = M; a.prologue = GH_XF_PRO_CF; a.epilogue = GH_XF_EPI_PLAIN; a.rows_per_batch = N; a.x = dout; a.x_stride = N;
  a.x_stride_b = (int64_t)C * N; a.w = stem->out_t; a.y = g; a.y_stride = M;
  rc = gh_xf_linear(&a, nullptr, 0, hip_stream);
  if (rc != GH_OK) return rc;

  for (int i = d->layers - 1; i >= lowest; --i) {
    const GhXfLayerT& L = layers[i];
    const char* fs = gx_slot(tp, tape, i, 2);
    const float* fmom = (const float*)(fs + tp.f_ln);
    if (pj && (pj->gl[i].ff2_w || pj->gl[i].ff2_b)) {          // before [da | dg] takes `wide`
      if (pj->gl[i].ff2_w && !ff_formed) {
        rc = reform_ff(i);
        if (rc != GH_OK) return rc;
      }
      rc = wgrad(GH_XF_PRO_NONE, wide, 4 * M, nullptr, nullptr, nullptr, g, M, pj->gl[i].ff2_w, pj->gl[i].ff2_b);
      if (rc != GH_OK) return rc;
    }
    ff_formed = false;
    rc = gh_xf_geglu_backward(g, M, (const float*)fs, M, fmom, L.ln3_w, L.ln3_b, L.ff1_w, L.ff1_b, L.ff2_t, T, M, wide, 8 * (int64_t)M, hip_stream);
    if (rc != GH_OK) return rc;
    if (pj) {
      rc = wgrad(GH_XF_PRO_LN, (const float*)fs, M, fmom, pj->fl[i].ln3_w, pj->fl[i].ln3_b, wide, 8 * M, pj->gl[i].ff1_w, pj->gl[i].ff1_b);
      if (rc != GH_OK) return rc;
    }
    rc = data(wide, 8 * M, L.ff1_t, M, dn);
    if (rc != GH_OK) return rc;
    if (pj) {
      rc = norm_grads(dn, (const float*)fs, fmom, pj->gl[i].ln3_w, pj->gl[i].ln3_b);
      if (rc != GH_OK) return rc;
    }
    rc = gh_xf_layernorm_backward(dn, M, (const float*)fs, M, fmom, L.ln3_w, T, M, g, M, hip_stream);
    if (rc != GH_OK) return rc;
    for (int which = 1; which >= 0; --which) {
      const float* wqkv_t = which ? L.qkv2_t : L.qkv1_t;
      if (!wqkv_t) continue;
      const char* as = gx_slot(tp, tape, i, which);
      const float* amom = (const float*)(as + tp.a_ln);
      float* datt = wide;
      float* dqkv = wide + (size_t)T * M;
      if (pj) {
        const GhXfLayerG& Q = pj->gl[i];
        rc = wgrad(GH_XF_PRO_NONE, (const float*)(as + tp.a_att), M, nullptr, nullptr, nullptr, g, M, which ? Q.o2_w : Q.o1_w, which ? Q.o2_b : Q.o1_b);
        if (rc != GH_OK) return rc;
      }
      rc = data(g, M, which ? L.o2_t : L.o1_t, M, datt);
      if (rc != GH_OK) return rc;
      rc = gh_xf_attention_backward((const float*)(as + tp.a_qkv), 3 * M, (const float*)(as + tp.a_att), M, (const float*)(as + tp.a_lse), datt, M,
                                    d->B, N, d->heads, d->D, dqkv, 3 * M, ws + p.delta, p.dy - p.delta, hip_stream);
      if (rc != GH_OK) return rc;
      if (pj) {
        const GhXfLayer& F = pj->fl[i];
        rc = wgrad(GH_XF_PRO_LN, (const float*)as, M, amom, which ? F.ln2_w : F.ln1_w, which ? F.ln2_b : F.ln1_b, dqkv, 3 * M,
                   which ? pj->gl[i].qkv2 : pj->gl[i].qkv1, nullptr);
        if (rc != GH_OK) return rc;
      }
      rc = data(dqkv, 3 * M, wqkv_t, M, dn);
      if (rc != GH_OK) return rc;
      if (pj) {
        rc = norm_grads(dn, (const float*)as, amom, which ? pj->gl[i].ln2_w : pj->gl[i].ln1_w, which ? pj->gl[i].ln2_b : pj->gl[i].ln1_b);
        if (rc != GH_OK) return rc;
      }
      rc = gh_xf_layernorm_backward(dn, M, (const float*)as, M, amom, which ? L.ln2_w : L.ln1_w, T, M, g, M, hip_stream);
      if (rc != GH_OK) return rc;
    }
  }
  if (!below) return GH_OK;

  if (pj && (pj->gs->in_w || pj->gs->in_b)) {                  // dW_in = g^T . GN(x), x read channel first through the norm
    GhXfWgrad w = {};
    w.T = T; w.K = C; w.N_out = M; w.prologue = GH_XF_PRO_GN; w.rows_per_batch = N; w.groups = d->G; w.eps = d->gn_eps; w.x = x; w.x_stride = N;
    w.x_stride_b = (int64_t)C * N; w.dy = g; w.dy_stride = M; w.gamma = pj->fs->gn_w; w.beta = pj->fs->gn_b; w.moments = (const float*)(tape + tp.gn);
    w.dw = pj->gs->in_w; w.db = pj->gs->in_b;
    rc = gh_xf_linear_wgrad(&w, ws + pj->wg, pj->np - pj->wg, hip_stream);
    if (rc != GH_OK) return rc;
  }
  if (!dx && !pj->gs->gn_w && !pj->gs->gn_b) return GH_OK;

  GhXfLinear z = {};                                           // dy = g . W_in, written channel first; neither bias nor residual
  z.T = T; z.K = M; z.N_out = C; z.prologue = GH_XF_PRO_NONE; z.epilogue = GH_XF_EPI_BIAS_RES_CF; z.rows_per_batch = N; z.x = g; z.x_stride = M;
  z.w = stem->in_t; z.y = dy; z.y_stride = N; z.y_stride_b = (int64_t)C * N;
  rc = gx_linear(&z, nullptr, 0, hip_stream, false);
  if (rc != GH_OK) return rc;
  if (pj) {
    rc = gh_xf_group_norm_param_grads(dy, x, (const float*)(tape + tp.gn), d->B, C, N, d->G, d->gn_eps, pj->gs->gn_w, pj->gs->gn_b, ws + pj->np,
                                      pj->total - pj->np, hip_stream);
    if (rc != GH_OK) return rc;
  }
  if (!dx) return GH_OK;
  return gh_xf_group_norm_backward(dy, x, (const float*)(tape + tp.gn), stem->gn_w, dout, dx, d->B, C, N, d->G, d->gn_eps, ws + p.gnw,
                                   p.total - p.gnw, hip_stream);
}

extern "C" int gh_xf_backward(const GhXfDims* d, const GhXfStemT* stem, const GhXfLayerT* layers, const float* x, const void* tape,
                              const float* dout, float* dx, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_grad_dims(d, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  return gx_backward(d, stem, layers, x, tape, dout, dx, workspace, ws_bytes, hip_stream, nullptr);
}

extern "C" size_t gh_xf_backward_params_workspace_bytes(const GhXfDims* dims) {
  bool empty;
  if (gx_check_grad_dims(dims, &empty) != GH_OK || empty) return 0;
  GxParamJob j = {};
  gx_param_plan(dims, &j);
  return j.total;
}

extern "C" int gh_xf_backward_params(const GhXfDims* d, const GhXfStemT* stem, const GhXfLayerT* layers, const GhXfStem* fstem,
                                     const GhXfLayer* flayers, const GhXfStemG* gstem, const GhXfLayerG* glayers, const float* x, const void* tape,
                                     const float* dout, float* dx, void* workspace, size_t ws_bytes, void* hip_stream) {
  bool empty;
  const int rc = gx_check_grad_dims(d, &empty);
  if (rc != GH_OK) return rc;
  if (empty) return GH_OK;
  GxParamJob j = {};
  j.fs = fstem; j.fl = flayers; j.gs = gstem; j.gl = glayers;
  gx_param_plan(d, &j);
  return gx_backward(d, stem, layers, x, tape, dout, dx, workspace, ws_bytes, hip_stream, &j);
}
