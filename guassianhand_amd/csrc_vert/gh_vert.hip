// gh_vert.hip — the fused vertex MLP block (include/gh_vert.h): vert_valid / vert_pos_refinement as one pass over the feature rows,
// and the backward that recomputes it.
//   tile      one 4-wave workgroup per GH_VERT_ROWS = 64 rows, lane = row, wave-uniform weights through the scalar cache. The rows'
//             features and positions are loaded coalesced (16-byte loads where x allows) into LDS at an odd pitch (D | 1), so that a
//             lane reads its own row without a bank conflict; the concatenation exists there only.
//   forward   LayerNorm in place (wave w sums the columns k = w mod 4), then fc1 / fc2 / fc through ghr_linear: wave w owns the
//             outputs w, w + 4, ..., three at a time, one LDS read of the input against three fmaf with an SGPR operand.
//   backward  the same forward with the normalised row kept un-scaled (the affine is applied on the fly), then the three layers
//             backwards through ghr_linear_t: wave w owns the inputs 16t + 4w .. + 3, one LDS read of a gradient against four fmaf;
//             the LayerNorm's backward in place; rows leave as coalesced runs. With parameter gradients: the tile's 64 rows are
//             summed in ascending row order into one partial per workgroup; a second launch adds the partials in a fixed order.
// No atomics; every float sum has a fixed order that depends on (Cf, K) — and, for parameter gradients, on P — alone.
#include "../../include/gh_vert.h"
#include "../csrc_rows/gh_rows.h"

#define GHV_BLOCK GHR_BLOCK
#define GHV_ROWS GH_VERT_ROWS
#define GHV_OP 3        // pitch of the output tile (K <= 3)
#define GHV_LDS_MAX (128 * 1024)  // the most LDS a workgroup of the backward takes (a CU has 160 KiB)

static_assert(GHV_ROWS == GHR_ROWS, "the shared row routines' tile: lane = row, four waves share a row's columns");
static_assert(GH_VERT_SEGMENTS == GHR_SEGMENTS, "the header documents the shared reduction's run count");

// the tile's R rows of (x, pts) -> s_z[row * ZP + col]; rows past the end are zeros
__device__ __forceinline__ void ghv_stage(float* s_z, int ZP, const float* __restrict__ x, long long x_stride,
                                          const float* __restrict__ pts, long long row0, int R, int nrows, int Cf, int vec_x, int tid) {
  ghr_stage(s_z, ZP, x, x_stride, row0, R, nrows, 0, Cf, vec_x, tid);
  for (int i = tid; i < R * 3; i += GHV_BLOCK) {
    const int r = i / 3, c = i - 3 * r;
    s_z[r * ZP + Cf + c] = r < nrows ? pts[row0 * 3 + i] : 0.f;
  }
}

// the epilogue of a layer for ghr_linear: out_row[j] = act(sum + b[j])
template <bool RELU>
__device__ __forceinline__ auto ghv_store(float* out_row, const float* __restrict__ b) {
  return [=](int j, float t) {
    float v = t + b[j];
    if (RELU) v = v > 0.f ? v : (v == v ? 0.f : v);  // (a NaN stays a NaN, as torch's relu keeps it)
    out_row[j] = v;
  };
}

// stage, LayerNorm in place, fc1, fc2, fc. s_z is left holding gamma * xhat + beta (AFFINE_LATER false) or xhat (true), and fc1 then
// applies the affine on the fly; returns rstd. s_h2 may alias s_z when AFFINE_LATER is false (the normalised row is dead once fc1 is
// through).
template <bool AFFINE_LATER>
__device__ __forceinline__ float ghv_forward_tile(float* s_red, float* s_z, float* s_h1, float* s_h2, float* s_o, int ZP, int HP,
                                                  const float* __restrict__ x, long long x_stride, const float* __restrict__ pts,
                                                  const GhrTile& t, int R, int Cf, int Hd, int K, float eps, GhVertParams p, int vec_x) {
  const int D = Cf + 3, lane = t.lane, wave = t.wave;
  ghv_stage(s_z, ZP, x, x_stride, pts, t.row0, R, t.nrows, Cf, vec_x, t.tid);
  __syncthreads();
  float* zr = s_z + lane * ZP;
  const GhrMoments mo = ghr_moments(zr, D, s_red, lane, wave);
  const float rstd = 1.0f / sqrtf(mo.m2 / (float)D + eps);
  for (int k = wave; k < D; k += 4) {
    const float xh = (zr[k] - mo.mean) * rstd;
    zr[k] = AFFINE_LATER ? xh : fmaf(xh, p.ln_weight[k], p.ln_bias[k]);
  }
  __syncthreads();
  ghr_linear(D, p.fc1_weight, Hd, wave, [&](int k) { return AFFINE_LATER ? fmaf(zr[k], p.ln_weight[k], p.ln_bias[k]) : zr[k]; },
             ghv_store<true>(s_h1 + lane * HP, p.fc1_bias));
  __syncthreads();
  const float* h1 = s_h1 + lane * HP;
  ghr_linear(Hd, p.fc2_weight, Hd, wave, [&](int k) { return h1[k]; }, ghv_store<false>(s_h2 + lane * HP, p.fc2_bias));
  __syncthreads();
  const float* h2 = s_h2 + lane * HP;
  ghr_linear(Hd, p.fc_weight, K, wave, [&](int k) { return h2[k]; }, ghv_store<false>(s_o + lane * GHV_OP, p.fc_bias));
  __syncthreads();
  return rstd;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHV_BLOCK) void ghv_fwd_kernel(const float* __restrict__ x, long long x_stride, const float* __restrict__ pts,
                                                            int P, int Cf, GhVertParams p, int K, unsigned act, float radius, float eps,
                                                            float* __restrict__ out, int vec_x) {
  extern __shared__ __attribute__((aligned(16))) float ghv_smem[];
  const int D = Cf + 3, Hd = D >> 2, ZP = D | 1, HP = Hd | 1;
  float* s_red = ghv_smem;                    // 2 x GHV_BLOCK
  float* s_z = s_red + 2 * GHV_BLOCK;         // GHV_ROWS x ZP; later the second hidden layer (HP < ZP)
  float* s_h1 = s_z + GHV_ROWS * ZP;          // GHV_ROWS x HP
  float* s_o = s_h1 + GHV_ROWS * HP;          // GHV_ROWS x GHV_OP
  const GhrTile t = ghr_tile<GHV_ROWS>(P);
  ghv_forward_tile<false>(s_red, s_z, s_h1, s_z, s_o, ZP, HP, x, x_stride, pts, t, GHV_ROWS, Cf, Hd, K, eps, p, vec_x);
  for (int e = t.tid; e < t.nrows * K; e += GHV_BLOCK) {  // the tile's contiguous run of the output
    const int r = e / K, c = e - r * K;
    const float v = s_o[r * GHV_OP + c];
    out[t.row0 * K + e] = act == GH_VERT_ACT_SIGMOID ? ghr_sigmoid(v) : pts[t.row0 * 3 + e] + tanhf(v) * radius;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// offsets of the eight parameters in a workgroup's partial, in GhVertParams order; [8] is the total
struct GhvOffsets { int o[9]; };
static inline GhvOffsets ghv_offsets(int D, int Hd, int K) {
  GhvOffsets f;
  const int n[8] = {D, D, Hd * D, Hd, Hd * Hd, Hd, K * Hd, K};
  f.o[0] = 0;
  for (int i = 0; i < 8; ++i) f.o[i + 1] = f.o[i] + n[i];
  return f;
}

// out[a * nb + b] = sum over the tile's rows, ascending, of A[row, a] * B[row, b] (AFFINE: of gamma[b] * B[row, b] + beta[b])
template <bool AFFINE>
__device__ __forceinline__ void ghv_outer(const float* A, int pa, int na, const float* B, int pb, int nb, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float* __restrict__ out, int R, int tid) {
  for (int e = tid; e < na * nb; e += GHV_BLOCK) {
    const int a = e / nb, b = e - a * nb;
    float ga = 1.f, be = 0.f;
    if (AFFINE) { ga = gamma[b]; be = beta[b]; }
    float s = 0.f;
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
      float bv = B[r * pb + b];
      if (AFFINE) bv = fmaf(bv, ga, be);
      s = fmaf(A[r * pa + a], bv, s);
    }
    out[e] = s;
  }
}

__device__ __forceinline__ void ghv_colsum(const float* A, int pa, int na, float* __restrict__ out, int R, int tid) {
  for (int e = tid; e < na; e += GHV_BLOCK) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += A[r * pa + e];
    out[e] = s;
  }
}

// R rows per workgroup: GHV_ROWS, or half of it where two R x D tiles of that many rows do not fit the LDS — lanes l and l + 32 then
// work on the same row and store the same values
template <bool WGRAD, int R>
__global__ __launch_bounds__(GHV_BLOCK) void ghv_bwd_kernel(const float* __restrict__ x, long long x_stride, const float* __restrict__ pts,
                                                            int P, int Cf, GhVertParams p, int K, unsigned act, float radius, float eps,
                                                            const float* __restrict__ g_out, float* __restrict__ grad_x,
                                                            long long gx_stride, float* __restrict__ grad_pts, float* __restrict__ part,
                                                            GhvOffsets off, int vec_x) {
  extern __shared__ __attribute__((aligned(16))) float ghv_smem[];
  const int D = Cf + 3, Hd = D >> 2, ZP = D | 1, HP = Hd | 1;
  float* s_red = ghv_smem;                     // 2 x GHV_BLOCK
  float* s_z = s_red + 2 * GHV_BLOCK;          // R x ZP: xhat
  float* s_gz = s_z + R * ZP;                  // R x ZP: the gradient of gamma * xhat + beta, later of z
  float* s_h1 = s_gz + R * ZP;                 // R x HP each
  float* s_h2 = s_h1 + R * HP;
  float* s_gh2 = s_h2 + R * HP;
  float* s_gp1 = s_gh2 + R * HP;
  float* s_o = s_gp1 + R * HP;                 // R x GHV_OP: o, then its gradient
  const GhrTile t = ghr_tile<R>(P);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const float rstd = ghv_forward_tile<true>(s_red, s_z, s_h1, s_h2, s_o, ZP, HP, x, x_stride, pts, t, R, Cf, Hd, K, eps, p, vec_x);

  // ---- the gradient of o; rows past the end are zeros (they enter the tile's sums of the parameter gradients) ----
  for (int e = tid; e < R * K; e += GHV_BLOCK) {
    const int r = e / K, c = e - r * K;
    float go = 0.f;
    if (r < t.nrows && g_out) {
      const float g = g_out[t.row0 * K + e], v = s_o[r * GHV_OP + c];
      if (act == GH_VERT_ACT_SIGMOID) {
        const float s = ghr_sigmoid(v);
        go = (g * (1.0f - s)) * s;
      } else {
        const float t = tanhf(v);
        go = (g * radius) * (1.0f - t * t);
      }
    }
    s_o[r * GHV_OP + c] = go;
  }
  __syncthreads();
  ghr_linear_t(s_o + lane * GHV_OP, K, p.fc_weight, Hd, wave, [&](int j, float a) { s_gh2[lane * HP + j] = a; });
  __syncthreads();
  ghr_linear_t(s_gh2 + lane * HP, Hd, p.fc2_weight, Hd, wave,
               [&](int i, float a) { s_gp1[lane * HP + i] = s_h1[lane * HP + i] > 0.f ? a : 0.f; });  // h1 > 0 exactly where pre1 > 0
  __syncthreads();
  const float* zr = s_z + lane * ZP;
  float* gr = s_gz + lane * ZP;
  float p1 = 0.f, p2 = 0.f;  // this wave's share of sum_k gxhat[k] and of sum_k gxhat[k] * xhat[k], gxhat = gamma * gzn
  ghr_linear_t(s_gp1 + lane * HP, Hd, p.fc1_weight, D, wave, [&](int k, float a) {
    gr[k] = a;
    const float gxh = a * p.ln_weight[k];
    p1 += gxh;
    p2 = fmaf(gxh, zr[k], p2);
  });
  s_red[wave * GHV_ROWS + lane] = p1;
  s_red[GHV_BLOCK + wave * GHV_ROWS + lane] = p2;
  __syncthreads();

  // ---- this tile's share of the parameter gradients, rows ascending ----
  if (WGRAD) {
    float* pw = part + (size_t)blockIdx.x * off.o[8];
    for (int k = tid; k < D; k += GHV_BLOCK) {
      float sg = 0.f, sb = 0.f;
      for (int r = 0; r < R; ++r) {
        const float g = s_gz[r * ZP + k];
        sg = fmaf(g, s_z[r * ZP + k], sg);
        sb += g;
      }
      pw[off.o[0] + k] = sg;
      pw[off.o[1] + k] = sb;
    }
    ghv_outer<true>(s_gp1, HP, Hd, s_z, ZP, D, p.ln_weight, p.ln_bias, pw + off.o[2], R, tid);
    ghv_colsum(s_gp1, HP, Hd, pw + off.o[3], R, tid);
    ghv_outer<false>(s_gh2, HP, Hd, s_h1, HP, Hd, nullptr, nullptr, pw + off.o[4], R, tid);
    ghv_colsum(s_gh2, HP, Hd, pw + off.o[5], R, tid);
    ghv_outer<false>(s_o, GHV_OP, K, s_h2, HP, Hd, nullptr, nullptr, pw + off.o[6], R, tid);
    ghv_colsum(s_o, GHV_OP, K, pw + off.o[7], R, tid);
    __syncthreads();
  }

  // ---- the LayerNorm's backward in place: gz = rstd * ((gxhat - mean(gxhat)) - xhat * mean(gxhat * xhat)) ----
  const float m1 = ghr_sum4(s_red, lane) / (float)D, m2 = ghr_sum4(s_red + GHV_BLOCK, lane) / (float)D;
  for (int k0 = 4 * wave; k0 < D; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + s;
      if (k < D) gr[k] = fmaf(-zr[k], m2, gr[k] * p.ln_weight[k] - m1) * rstd;
    }
  }
  __syncthreads();
  for (int i = tid; i < t.nrows * Cf; i += GHV_BLOCK) {
    const int r = i / Cf, c = i - r * Cf;
    grad_x[(t.row0 + r) * gx_stride + c] = s_gz[r * ZP + c];
  }
  if (grad_pts) {
    for (int i = tid; i < t.nrows * 3; i += GHV_BLOCK) {
      const int r = i / 3, c = i - 3 * r;
      grad_pts[t.row0 * 3 + i] = s_gz[r * ZP + Cf + c];
    }
  }
}

// the partials of the nblk workgroups, in workgroup order: GH_VERT_SEGMENTS contiguous runs, each summed in order, then the runs in order
__global__ __launch_bounds__(GHV_BLOCK) void ghv_reduce_kernel(const float* __restrict__ part, int nblk, GhvOffsets off, GhVertGrads g) {
  ghr_reduce(
      nblk, off.o[8], [&](int i, int el) { return part[(size_t)i * off.o[8] + el]; },
      [&](int el, float t) {
        float* dst = el < off.o[1] ? g.ln_weight + el
                   : el < off.o[2] ? g.ln_bias + (el - off.o[1])
                   : el < off.o[3] ? g.fc1_weight + (el - off.o[2])
                   : el < off.o[4] ? g.fc1_bias + (el - off.o[3])
                   : el < off.o[5] ? g.fc2_weight + (el - off.o[4])
                   : el < off.o[6] ? g.fc2_bias + (el - off.o[5])
                   : el < off.o[7] ? g.fc_weight + (el - off.o[6])
                                   : g.fc_bias + (el - off.o[7]);
        *dst = t;
      });
}

// ---- host --------------------------------------------------------------------------------------------------------------
static inline int ghv_blocks(int P) { return (P + GHV_ROWS - 1) / GHV_ROWS; }
static inline size_t ghv_bwd_lds(int D, int rows) {
  return (size_t)(2 * GHV_BLOCK + rows * (2 * (D | 1) + 4 * ((D / 4) | 1) + GHV_OP)) * sizeof(float);
}
// rows per workgroup of the backward: a function of D alone
static inline int ghv_bwd_rows(int D) { return ghv_bwd_lds(D, GHV_ROWS) <= GHV_LDS_MAX ? GHV_ROWS : GHV_ROWS / 2; }

static int ghv_check(int P, int Cf, const GhVertParams* p, const GhVertDesc* d) {
  if (!d || !p) return GH_ERR_INVALID_ARG;
  if (Cf < 1 || Cf > GH_VERT_MAX_CF || P < 0) return GH_ERR_INVALID_ARG;
  if (d->K != 1 && d->K != 3) return GH_ERR_INVALID_ARG;
  if (d->act != GH_VERT_ACT_SIGMOID && d->act != GH_VERT_ACT_TANH_OFFSET) return GH_ERR_INVALID_ARG;
  if (d->act == GH_VERT_ACT_TANH_OFFSET && d->K != 3) return GH_ERR_INVALID_ARG;
  if (!(d->eps >= 0.f)) return GH_ERR_INVALID_ARG;
  if (!p->ln_weight || !p->ln_bias || !p->fc1_weight || !p->fc1_bias || !p->fc2_weight || !p->fc2_bias || !p->fc_weight || !p->fc_bias)
    return GH_ERR_INVALID_ARG;
  return GH_OK;
}

extern "C" size_t gh_vert_workspace_bytes(int P, int D, int Hd, int K) {
  if (P < 1 || D < 4 || D > GH_VERT_MAX_CF + 3 || Hd != D / 4 || (K != 1 && K != 3)) return 0;
  const int rows = ghv_bwd_rows(D);
  return ghr_align((size_t)((P + rows - 1) / rows) * (size_t)ghv_offsets(D, Hd, K).o[8] * sizeof(float));
}

extern "C" int gh_vert_forward(const float* x, int64_t x_stride, const float* pts, int P, int Cf, const GhVertParams* params,
                               const GhVertDesc* desc, float* out, void* hip_stream) {
  const int rc = ghv_check(P, Cf, params, desc);
  if (rc != GH_OK) return rc;
  if (x_stride < Cf || !x || !pts || !out) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  const int D = Cf + 3, Hd = D / 4, ZP = D | 1, HP = Hd | 1;
  const int vec_x = ghr_al16(x) && Cf % 4 == 0 && x_stride % 4 == 0;
  const size_t lds = (size_t)(2 * GHV_BLOCK + GHV_ROWS * (ZP + HP + GHV_OP)) * sizeof(float);
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  ghr_allow_lds<ghv_fwd_kernel>(lds);
  hipLaunchKernelGGL(ghv_fwd_kernel, dim3((unsigned)ghv_blocks(P)), dim3(GHV_BLOCK), lds, s, x, (long long)x_stride, pts, P, Cf, *params,
                     (int)desc->K, desc->act, desc->radius, desc->eps, out, vec_x);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_vert_backward(const float* x, int64_t x_stride, const float* pts, int P, int Cf, const GhVertParams* params,
                                const GhVertDesc* desc, const float* g_out, float* grad_x, int64_t gx_stride, float* grad_pts,
                                const GhVertGrads* grads, void* workspace, size_t ws_bytes, void* hip_stream) {
  const int rc = ghv_check(P, Cf, params, desc);
  if (rc != GH_OK) return rc;
  if (x_stride < Cf || gx_stride < Cf || !x || !pts || !grad_x) return GH_ERR_INVALID_ARG;
  const bool wgrad = grads != nullptr;
  if (wgrad && (!grads->ln_weight || !grads->ln_bias || !grads->fc1_weight || !grads->fc1_bias || !grads->fc2_weight ||
                !grads->fc2_bias || !grads->fc_weight || !grads->fc_bias))
    return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  const int K = desc->K, D = Cf + 3, Hd = D / 4, rows = ghv_bwd_rows(D), nb = (P + rows - 1) / rows;
  if (wgrad) {
    if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
    if (ws_bytes < gh_vert_workspace_bytes(P, D, Hd, K)) return GH_ERR_WORKSPACE_SMALL;
  }
  const GhvOffsets off = ghv_offsets(D, Hd, K);
  const int vec_x = ghr_al16(x) && Cf % 4 == 0 && x_stride % 4 == 0;
  const size_t lds = ghv_bwd_lds(D, rows);
  const dim3 grid((unsigned)nb), block(GHV_BLOCK);
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
#define GHV_BWD(WG, RB)                                                                                                              \
  do {                                                                                                                              \
    ghr_allow_lds<ghv_bwd_kernel<WG, RB>>(lds);                                                                                     \
    hipLaunchKernelGGL((ghv_bwd_kernel<WG, RB>), grid, block, lds, s, x, (long long)x_stride, pts, P, Cf, *params, K, desc->act,   \
                       desc->radius, desc->eps, g_out, grad_x, (long long)gx_stride, grad_pts, (float*)workspace, off, vec_x);     \
  } while (0)
  if (wgrad) {
    if (rows == GHV_ROWS) GHV_BWD(true, GHV_ROWS); else GHV_BWD(true, GHV_ROWS / 2);
    hipLaunchKernelGGL(ghv_reduce_kernel, dim3(ghr_reduce_blocks(off.o[8])), block, 0, s,
                       (const float*)workspace, nb, off, *grads);
  } else {
    if (rows == GHV_ROWS) GHV_BWD(false, GHV_ROWS); else GHV_BWD(false, GHV_ROWS / 2);
  }
#undef GHV_BWD
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
