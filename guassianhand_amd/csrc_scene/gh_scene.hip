// gh_scene.hip — the texture scene code: token sum, 2 x 2 stride-2 transposed convolution per plane, planes joined, plane bias
// (include/gh_scene.h).
//
// One product shape, v_mfma_f32_32x32x2_f32: D[i][n] = fma chain over k of A[i][k] * B[k][n], exact float32.
//   operands   lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31]: one float each.
//   result     lane l holds column n = l & 31; its register r holds row ghr_acc_row(r, l >> 5) (gh_rows.h's "columns").
// The token is the column everywhere: a wave owns 32 consecutive tokens of one batch element, lane l the token l & 31.
//
// Forward, D[j][t] = sum_c W[c][j] x[c][t]. The weight is (Ci, 4 Co) and the tokens are (Ci, T) per batch element: lane l reads
// W[c0 + (l >> 5)][j0 + (l & 31)] and x[c0 + (l >> 5)][t0 + (l & 31)], two runs of 128 bytes per load, no LDS. The registers
// r .. r + 3 of a lane (r a multiple of 4) are rows j = j0 + 8 (r >> 2) + 4 (l >> 5) + {0, 1, 2, 3}: the (dy, dx) quad of one output
// channel, which leaves as two 8-byte stores; at S = 32 a half-wave writes one whole 256-byte row of a plane per store.
//
// Backward, D[c][t] = sum_j W[c][j] g[j][t]. k = l >> 5 is dx: the two lane halves read the two texels of one row that a token owns.
// The weight is now read along its row by the lane that owns row c: the strided operand. A slab of 32 rows x 32 columns is loaded
// coalesced and turned in LDS (pitch 33: a lane reads along its own row without a bank conflict).
//
// A workgroup is one wave and one 32 x 32 tile: at B = 1 and the config's shape the forward has 640 and the backward 1024 of them for
// 1024 SIMDs, and no sum is split. Each wave keeps the operands of the next 16 steps of the chain (32 channels forward, one slab
// backward) in flight while the matrix unit works on the current 16: two register sets that swap roles, loaded by plain loads that
// nothing selects from or adds to until the set is used — a select or a test behind a load makes the compiler wait for the load
// where it was issued, which cost the forward three quarters of its time. Addresses of tail lanes are clamped into the tensor and
// their operands replaced by 0 where they are used, so that every load is unconditional; whole sets take one address per operand
// and constant steps from it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gh_scene.h"
#include "../csrc_rows/gh_rows.h"

#define GS_WAVE 64
#define GS_TILE 32
#define GS_PITCH 33
#define GS_FWD_STEPS 16  // chain steps (of two channels) whose operands are fetched at once
#define GS_PB_BLOCK 256

struct GsFwd {
  const float *a, *b, *W, *cb, *pb;
  float* out;
  long long a_sb, a_sc, b_sb, b_sc, pb_sc, pb_sr, T;
  int Ci, Co, Np, S;
  unsigned tok_tiles, j_tiles;
  int per_plane, vec_out;
};

// token t of a batch element -> plane p, row y, column x_
__device__ __forceinline__ void gs_token(long long t, int S, int* p, int* y, int* x_) {
  const long long s2 = (long long)S * S;
  const long long rem = t % s2;
  *p = (int)(t / s2);
  *y = (int)(rem / S);
  *x_ = (int)(rem % S);
}

template <int HAS_B>
__global__ __launch_bounds__(GS_WAVE) void gs_forward_kernel(GsFwd a) {
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int J = 4 * a.Co;
  const unsigned jt = blockIdx.x % a.j_tiles;
  const unsigned rest = blockIdx.x / a.j_tiles;
  const unsigned tt = rest % a.tok_tiles;
  const long long b = rest / a.tok_tiles;
  const long long t = (long long)tt * GS_TILE + col;
  const bool live_t = t < a.T;
  const int j = (int)jt * GS_TILE + col;
  const bool live_j = j < J;
  const float* wp = a.W + (live_j ? j : J - 1);
  const float* xa = a.a + b * a.a_sb + (live_t ? t : a.T - 1);
  const float* xb = HAS_B ? a.b + b * a.b_sb + (live_t ? t : a.T - 1) : xa;

  ghr_acc acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // fetch only loads (nothing waits for a value), mac selects and multiplies: the loads of one set are in flight while the matrix
  // unit works through the other. HAS_B == 0: the third array is never touched.
  struct Ops { float w[GS_FWD_STEPS], x[GS_FWD_STEPS], y[GS_FWD_STEPS]; };
  auto fetch = [&](int c0, Ops& o) {
    if (c0 + 2 * GS_FWD_STEPS <= a.Ci) {                    // a whole set: one address per operand, constant steps from it
      const float* w = wp + (long long)(c0 + half) * J;
      const float* x = xa + (c0 + half) * a.a_sc;
      const float* y = xb + (c0 + half) * a.b_sc;
#pragma unroll
      for (int s = 0; s < GS_FWD_STEPS; ++s) {
        o.w[s] = w[(long long)(2 * s) * J];
        o.x[s] = x[2 * s * a.a_sc];
        if (HAS_B) o.y[s] = y[2 * s * a.b_sc];
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < GS_FWD_STEPS; ++s) {
      const int c = c0 + 2 * s + half;
      const long long cc = c < a.Ci ? c : a.Ci - 1;
      o.w[s] = wp[cc * J];
      o.x[s] = xa[cc * a.a_sc];
      if (HAS_B) o.y[s] = xb[cc * a.b_sc];
    }
  };
  auto mac = [&](int c0, const Ops& o) {
#pragma unroll
    for (int s = 0; s < GS_FWD_STEPS; ++s) {
      const bool ok = c0 + 2 * s + half < a.Ci;
      const float xv = HAS_B ? o.x[s] + o.y[s] : o.x[s];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32((ok && live_j) ? o.w[s] : 0.f, (ok && live_t) ? xv : 0.f, acc, 0, 0, 0);
    }
  };
  Ops p0, p1;
  fetch(0, p0);
  for (int c0 = 0; c0 < a.Ci; c0 += 4 * GS_FWD_STEPS) {
    fetch(c0 + 2 * GS_FWD_STEPS, p1);                       // past the end: clamped loads that nothing uses
    __builtin_amdgcn_sched_barrier(0);                      // every load of the next set is issued before the first product
    mac(c0, p0);
    if (c0 + 2 * GS_FWD_STEPS >= a.Ci) break;
    fetch(c0 + 4 * GS_FWD_STEPS, p0);
    __builtin_amdgcn_sched_barrier(0);
    mac(c0 + 2 * GS_FWD_STEPS, p1);
  }

  if (!live_t) return;
  int p, y, x_;
  gs_token(t, a.S, &p, &y, &x_);
  const long long S2 = 2LL * a.S;
  const long long row_len = a.per_plane ? S2 : S2 * a.Np;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int jq = (int)jt * GS_TILE + 8 * q + 4 * half;
    if (jq >= J) continue;
    const int o = jq >> 2;
    float v[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    if (a.cb) {
      const float cb = a.cb[o];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] + cb;
    }
    if (a.pb) {
      const float* pb = a.pb + o * a.pb_sc + (2LL * y) * a.pb_sr + 2 * x_;
      v[0] = v[0] + pb[0];
      v[1] = v[1] + pb[1];
      v[2] = v[2] + pb[a.pb_sr];
      v[3] = v[3] + pb[a.pb_sr + 1];
    }
    const long long plane_row = a.per_plane ? ((b * a.Np + p) * a.Co + o) * S2 : (b * a.Co + o) * S2;
    float* d = a.out + (plane_row + 2 * y) * row_len + (a.per_plane ? 0 : p * S2) + 2 * x_;
    if (a.vec_out) {
      *(float2*)d = make_float2(v[0], v[1]);
      *(float2*)(d + row_len) = make_float2(v[2], v[3]);
    } else {
      d[0] = v[0]; d[1] = v[1]; d[row_len] = v[2]; d[row_len + 1] = v[3];
    }
  }
}

struct GsBwd {
  const float *W, *g;
  float* d_tok;
  long long T;
  int Ci, Co, Np, S;
  unsigned tok_tiles, c_tiles;
  int per_plane;
};

__global__ __launch_bounds__(GS_WAVE) void gs_backward_kernel(GsBwd a) {
  __shared__ float s_w[GS_TILE * GS_PITCH];
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int J = 4 * a.Co;
  const unsigned ct = blockIdx.x % a.c_tiles;
  const unsigned rest = blockIdx.x / a.c_tiles;
  const unsigned tt = rest % a.tok_tiles;
  const long long b = rest / a.tok_tiles;
  const long long t = (long long)tt * GS_TILE + col;
  const bool live_t = t < a.T;
  const int c0 = (int)ct * GS_TILE;
  int p, y, x_;
  gs_token(live_t ? t : a.T - 1, a.S, &p, &y, &x_);
  const long long S2 = 2LL * a.S;
  const long long row_len = a.per_plane ? S2 : S2 * a.Np;
  const long long o_stride = S2 * row_len;
  // the lane's texel (dy = 0, dx = half) of output channel 0
  const float* gp = a.g + ((a.per_plane ? (b * a.Np + p) * a.Co : b * a.Co) * S2 + 2 * y) * row_len + (a.per_plane ? 0 : p * S2) + 2 * x_ + half;

  ghr_acc acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // fetch only loads; the zeros of the tails are put in where a value is used, so that nothing waits for a load it does not need yet
  struct Ops { float w[16], g[16]; };
  const bool rows_full = c0 + GS_TILE <= a.Ci;
  auto fetch = [&](int j0, Ops& o) {
    const int jc = j0 + col;                                 // the slab's column this lane loads
    const float* wcol = a.W + (jc < J ? jc : J - 1);
    const int o0 = j0 >> 2;                                  // j = j0 + 2 s + half = 4 o + 2 dy + dx: o = o0 + (s >> 1), dy = s & 1, dx = half
    if (rows_full && o0 + 8 <= a.Co) {                       // a whole slab: one address per operand, constant steps from it
      const float* w = wcol + (long long)(c0 + half) * J;
      const float* g = gp + o0 * o_stride;
#pragma unroll
      for (int i = 0; i < 16; ++i) o.w[i] = w[(long long)(2 * i) * J];
#pragma unroll
      for (int s = 0; s < 16; ++s) o.g[s] = g[(s >> 1) * o_stride + (s & 1) * row_len];
      return;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + 2 * i + half;
      o.w[i] = wcol[(long long)(c < a.Ci ? c : a.Ci - 1) * J];
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int oc = o0 + (s >> 1);
      o.g[s] = gp[(oc < a.Co ? oc : a.Co - 1) * o_stride + (s & 1) * row_len];
    }
  };
  auto slab = [&](int j0, const Ops& o, Ops& next) {
    const bool col_ok = j0 + col < J;
    __syncthreads();                                         // the previous slab has been read
#pragma unroll
    for (int i = 0; i < 16; ++i) s_w[(2 * i + half) * GS_PITCH + col] = (col_ok && c0 + 2 * i + half < a.Ci) ? o.w[i] : 0.f;
    __syncthreads();
    fetch(j0 + GS_TILE, next);                               // past the end: clamped loads that nothing uses
    __builtin_amdgcn_sched_barrier(0);                       // every load of the next slab is issued before the first product
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const bool ok = live_t && (j0 >> 2) + (s >> 1) < a.Co;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[col * GS_PITCH + 2 * s + half], ok ? o.g[s] : 0.f, acc, 0, 0, 0);
    }
  };
  Ops p0, p1;
  fetch(0, p0);
  for (int j0 = 0; j0 < J; j0 += 2 * GS_TILE) {
    slab(j0, p0, p1);
    if (j0 + GS_TILE >= J) break;
    slab(j0 + GS_TILE, p1, p0);
  }

  if (!live_t) return;
  float* d = a.d_tok + b * a.Ci * a.T + t;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = c0 + ghr_acc_row(r, half);
    if (c < a.Ci) d[c * a.T] = acc[r];
  }
}

// d_plane_bias[o, Y, X] for X < 2 S: one thread per element, b ascending and p ascending inside it. dout is the joined layout.
__global__ __launch_bounds__(GS_PB_BLOCK) void gs_plane_bias_kernel(const float* __restrict__ g, float* __restrict__ dpb, long long sc, long long sr,
                                                                    int B, int Co, int Np, int S, long long total) {
  const long long i = (long long)blockIdx.x * GS_PB_BLOCK + threadIdx.x;
  if (i >= total) return;
  const long long S2 = 2LL * S, row_len = S2 * Np;
  const long long X = i % S2, Y = (i / S2) % S2, o = i / (S2 * S2);
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* row = g + (((long long)b * Co + o) * S2 + Y) * row_len + X;
    for (int p = 0; p < Np; ++p) acc = acc + row[p * S2];
  }
  dpb[o * sc + Y * sr + X] = acc;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 gs_u128;

// GH_OK with T and the tile counts of both products filled in, or the status the header names
static int gs_dims(const GhSceneDims* d, long long* T, unsigned* tok_tiles, unsigned* j_tiles, unsigned* c_tiles) {
  if (!d) return GH_ERR_INVALID_ARG;
  if (d->B < 0 || d->Ci < 1 || d->Co < 1 || d->Np < 1 || d->S < 1 || (d->flags & ~(uint32_t)GH_SCENE_PER_PLANE)) return GH_ERR_INVALID_ARG;
  if (d->Ci > GH_SCENE_MAX_CI || d->Co > GH_SCENE_MAX_CO) return GH_ERR_UNSUPPORTED;
  const gs_u128 t = (gs_u128)d->Np * (gs_u128)d->S * (gs_u128)d->S;
  const gs_u128 tt = (t + GS_TILE - 1) / GS_TILE;
  const unsigned jt = (4u * (unsigned)d->Co + GS_TILE - 1) / GS_TILE, ct = ((unsigned)d->Ci + GS_TILE - 1) / GS_TILE;
  const gs_u128 nb = d->B > 0 ? (gs_u128)d->B : 1;
  const gs_u128 pb_blocks = ((gs_u128)d->Co * 4 * (gs_u128)d->S * (gs_u128)d->S + GS_PB_BLOCK - 1) / GS_PB_BLOCK;
  if (nb * tt * jt > (gs_u128)GH_SCENE_MAX_TILES || nb * tt * ct > (gs_u128)GH_SCENE_MAX_TILES || pb_blocks > (gs_u128)GH_SCENE_MAX_TILES)
    return GH_ERR_UNSUPPORTED;
  *T = (long long)t;
  *tok_tiles = (unsigned)tt;
  *j_tiles = jt;
  *c_tiles = ct;
  return GH_OK;
}

extern "C" int gh_scene_code_forward(const GhSceneDims* dims, const float* tok_a, int64_t a_stride_b, int64_t a_stride_c, const float* tok_b,
                                     int64_t b_stride_b, int64_t b_stride_c, const float* weight, const float* conv_bias,
                                     const float* plane_bias, int64_t pb_stride_c, int64_t pb_stride_r, float* out, void* hip_stream) {
  long long T;
  unsigned tok_tiles, j_tiles, c_tiles;
  const int rc = gs_dims(dims, &T, &tok_tiles, &j_tiles, &c_tiles);
  if (rc != GH_OK) return rc;
  if (!tok_a || !weight || !out) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(tok_a) || !ghr_al4(tok_b) || !ghr_al4(weight) || !ghr_al4(conv_bias) || !ghr_al4(plane_bias) || !ghr_al4(out)) return GH_ERR_INVALID_ARG;
  if (a_stride_b < 0 || a_stride_c < 0 || (tok_b && (b_stride_b < 0 || b_stride_c < 0))) return GH_ERR_INVALID_ARG;
  const int per_plane = (dims->flags & GH_SCENE_PER_PLANE) ? 1 : 0;
  if (plane_bias && (per_plane || pb_stride_c < 0 || pb_stride_r < 0)) return GH_ERR_INVALID_ARG;
  if (dims->B == 0) return GH_OK;
  GsFwd a;
  a.a = tok_a; a.b = tok_b; a.W = weight; a.cb = conv_bias; a.pb = plane_bias; a.out = out;
  a.a_sb = a_stride_b; a.a_sc = a_stride_c; a.b_sb = tok_b ? b_stride_b : 0; a.b_sc = tok_b ? b_stride_c : 0;
  a.pb_sc = pb_stride_c; a.pb_sr = pb_stride_r; a.T = T;
  a.Ci = dims->Ci; a.Co = dims->Co; a.Np = dims->Np; a.S = dims->S;
  a.tok_tiles = tok_tiles; a.j_tiles = j_tiles; a.per_plane = per_plane;
  a.vec_out = ((uintptr_t)out & 7u) == 0;                  // every quad starts at an even element of a row of even length
  const dim3 grid((unsigned)((unsigned long long)dims->B * tok_tiles * j_tiles));
  (void)hipGetLastError();
  if (tok_b) hipLaunchKernelGGL(gs_forward_kernel<1>, grid, dim3(GS_WAVE), 0, (hipStream_t)hip_stream, a);
  else hipLaunchKernelGGL(gs_forward_kernel<0>, grid, dim3(GS_WAVE), 0, (hipStream_t)hip_stream, a);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_scene_code_backward(const GhSceneDims* dims, const float* weight, const float* dout, float* d_tok, float* d_plane_bias,
                                      int64_t dpb_stride_c, int64_t dpb_stride_r, void* hip_stream) {
  long long T;
  unsigned tok_tiles, j_tiles, c_tiles;
  const int rc = gs_dims(dims, &T, &tok_tiles, &j_tiles, &c_tiles);
  if (rc != GH_OK) return rc;
  if (!weight || !dout) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(weight) || !ghr_al4(dout) || !ghr_al4(d_tok) || !ghr_al4(d_plane_bias)) return GH_ERR_INVALID_ARG;
  const int per_plane = (dims->flags & GH_SCENE_PER_PLANE) ? 1 : 0;
  if (d_plane_bias && (per_plane || dpb_stride_c < 0 || dpb_stride_r < 0)) return GH_ERR_INVALID_ARG;
  if (dims->B == 0 || (!d_tok && !d_plane_bias)) return GH_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  if (d_tok) {
    GsBwd a;
    a.W = weight; a.g = dout; a.d_tok = d_tok; a.T = T;
    a.Ci = dims->Ci; a.Co = dims->Co; a.Np = dims->Np; a.S = dims->S;
    a.tok_tiles = tok_tiles; a.c_tiles = c_tiles; a.per_plane = per_plane;
    const dim3 grid((unsigned)((unsigned long long)dims->B * tok_tiles * c_tiles));
    hipLaunchKernelGGL(gs_backward_kernel, grid, dim3(GS_WAVE), 0, st, a);
  }
  if (d_plane_bias) {
    const long long total = 4LL * dims->Co * dims->S * dims->S;
    const dim3 grid((unsigned)((total + GS_PB_BLOCK - 1) / GS_PB_BLOCK));
    hipLaunchKernelGGL(gs_plane_bias_kernel, grid, dim3(GS_PB_BLOCK), 0, st, dout, d_plane_bias, (long long)dpb_stride_c,
                       (long long)dpb_stride_r, dims->B, dims->Co, dims->Np, dims->S, total);
  }
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
