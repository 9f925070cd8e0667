// gh_mano.hip — the hand points: linear blend skinning of H hand models for B parameter sets and the folded midpoint subdivision,
// forward and backward (include/gh_mano.h).
//
// Forward, three launches:
//   gm_chain_fwd    one wave per (b, h), lane j = joint j: pose, Rodrigues, shaped joint, then the kinematic chain one tree depth per
//                   step through LDS; writes joints and the state (pose, R, G, A, Jt) the other kernels and the backward read.
//   gm_verts_fwd    one thread per vertex: 3 (NB + 9 (J - 1)) fmaf of blend shapes read along v (coalesced planes), the skinning
//                   transform as J fmaf per entry, the vertex into points[:, :V] in place; keeps v_posed for the backward.
//   gm_points_fwd   one thread per point p >= V: three vertices of the same call's points block, three weights.
// Backward, up to five launches:
//   gm_chain_f64    one wave per (b, h): R, G and Jt again, in float64, for everything below.
//   gm_colsum       partial column sums of d_points per GH_MANO_CHUNK points (transl's gradient).
//   gm_verts_bwd    one thread per vertex: the transposed stencil as a CSR row, then dv_posed = T^R^T g; float64 from the float32
//                   cotangents on, as is everything behind it.
//   gm_reduce       one workgroup per sum group of a (b, h): joint j's dA (12 sums over v), joint j's nine pose blend-shape sums, one
//                   shape sum. A sum is 256 strided serial sums joined by gm_block_sum, in float64.
//   gm_chain_bwd    one wave per (b, h): dA -> dG, the chain in reverse (a parent gathers its children in ascending order), the
//                   Rodrigues derivative in closed form, the joint terms of d_betas, the final transl sums; float64 throughout,
//                   rounded once where an output is written. The rotation gradient is the antisymmetric part of a matrix summed
//                   over every vertex and every descendant joint: in float32 it lost an order of magnitude to cancellation.
// A launch boundary stands wherever a kernel reads what every workgroup of the previous one wrote; nothing is handed over inside a
// launch, and there is no atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gh_mano.h"
#include "../csrc_rows/gh_rows.h"

#define GM_WAVE 64
#define GM_BLOCK 256
#define GM_MJ GH_MANO_MAX_J
// state of a (b, h), in floats
#define GM_S_POSE 0
#define GM_S_R (3 * GM_MJ)
#define GM_S_G (GM_S_R + 9 * GM_MJ)
#define GM_S_A (GM_S_G + 12 * GM_MJ)
#define GM_S_JT (GM_S_A + 12 * GM_MJ)
#define GM_S_BETA (GM_S_JT + 3 * GM_MJ)
#define GM_STATE (GM_S_BETA + GH_MANO_MAX_NB)
// the backward's own float64 chain of a (b, h), in doubles
#define GM_D_R 0
#define GM_D_G (9 * GM_MJ)
#define GM_D_JT (GM_D_G + 12 * GM_MJ)
#define GM_DSTATE (GM_D_JT + 3 * GM_MJ)
// reduced sums of a (b, h), in doubles
#define GM_R_A 0
#define GM_R_PF (12 * GM_MJ)
#define GM_R_SD (GM_R_PF + 9 * GM_MJ)
#define GM_RED (GM_R_SD + GH_MANO_MAX_NB + 16)

struct GmModels {
  GhManoModel m[GH_MANO_MAX_H];
  long long off[GH_MANO_MAX_H];  // first point of hand h in a row of `points`
};

struct GmCall {
  int B, H, J, NB, Vmax, nch;
  long long Ptot;
  float *state, *vp;
  double *g, *dvp, *red, *tp, *dst, *vpd;  // everything the backward sums stays in float64 until an output is written
};

__device__ __forceinline__ int gm_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// R = I + sin(a) K + (1 - cos(a)) K K with a = |r + 1e-8|, K = skew(r / a); K and K K are handed back for the derivative
__device__ __forceinline__ float gm_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double gm_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float gm_sin(float v) { return sinf(v); }
__device__ __forceinline__ double gm_sin(double v) { return sin(v); }
__device__ __forceinline__ float gm_cos(float v) { return cosf(v); }
__device__ __forceinline__ double gm_cos(double v) { return cos(v); }

template <typename T>
__device__ __forceinline__ void gm_rodrigues(const T* r, T* R, T* K, T* KK, T* ang, T* sn, T* cs) {
  const T eps = (T)1e-8f;  // the float32 constant in both precisions: the backward differentiates the forward's function
  const T x = r[0] + eps, y = r[1] + eps, z = r[2] + eps;
  const T a = gm_sqrt((x * x + y * y) + z * z);
  const T dx = r[0] / a, dy = r[1] / a, dz = r[2] / a;
  const T s = gm_sin(a), c = gm_cos(a), oc = (T)1 - c;
  K[0] = 0; K[1] = -dz; K[2] = dy;
  K[3] = dz; K[4] = 0; K[5] = -dx;
  K[6] = -dy; K[7] = dx; K[8] = 0;
  KK[0] = -(dz * dz) - dy * dy; KK[1] = dy * dx; KK[2] = dz * dx;
  KK[3] = dx * dy; KK[4] = -(dz * dz) - dx * dx; KK[5] = dz * dy;
  KK[6] = dx * dz; KK[7] = dy * dz; KK[8] = -(dy * dy) - dx * dx;
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? (T)1 : (T)0) + (s * K[i] + oc * KK[i]);
  *ang = a; *sn = s; *cs = c;
}

// the wave's butterfly (every lane ends with the same bits: a + b == b + a), then the four waves in order
__device__ __forceinline__ double gm_block_sum(double v, double* s4) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, GM_WAVE);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

__device__ __forceinline__ int gm_depth(const GhManoModel& m, int j) {
  int d = 0;
  for (int q = m.parents[j], n = 0; q >= 0 && n < GM_MJ; q = m.parents[q], ++n) ++d;
  return d;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GM_WAVE) void gm_chain_fwd(GmModels ms, GmCall a, GhManoParams p, float* __restrict__ joints) {
  __shared__ float s_G[12 * GM_MJ], s_Jt[3 * GM_MJ];
  const int h = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const long long bh = (long long)b * a.H + h;
  float* st = a.state + bh * GM_STATE;
  const bool live = j < a.J;
  int par = -1, depth = -1;
  float R[9], jt[3] = {0.f, 0.f, 0.f}, G[12];
  if (live) {
    par = m.parents[j];
    depth = gm_depth(m, j);
    float r[3], K[9], KK[9], ang, sn, cs;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float raw = j == 0 ? p.global_orient[bh * 3 + c] : p.hand_pose[bh * 3 * (a.J - 1) + 3 * (j - 1) + c];
      r[c] = raw + m.pose_mean[3 * j + c];
      st[GM_S_POSE + 3 * j + c] = r[c];
    }
    gm_rodrigues(r, R, K, KK, &ang, &sn, &cs);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double acc = m.j_template[3 * j + c];
      for (int n = 0; n < a.NB; ++n) acc = fma(m.j_shapedirs[(3 * j + c) * a.NB + n], (double)p.betas[bh * a.NB + n], acc);
      jt[c] = (float)acc;
      s_Jt[3 * j + c] = jt[c];
      st[GM_S_JT + 3 * j + c] = jt[c];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) st[GM_S_R + 9 * j + i] = R[i];
  }
  if (j < a.NB) st[GM_S_BETA + j] = p.betas[bh * a.NB + j];
  __syncthreads();
  for (int d = 0; d < a.J; ++d) {
    if (live && depth == d) {
      if (par < 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) G[4 * r + c] = R[3 * r + c];
          G[4 * r + 3] = jt[r];
        }
      } else {
        const float* Gp = s_G + 12 * par;
        const float rel[3] = {jt[0] - s_Jt[3 * par], jt[1] - s_Jt[3 * par + 1], jt[2] - s_Jt[3 * par + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) G[4 * r + c] = (Gp[4 * r] * R[c] + Gp[4 * r + 1] * R[3 + c]) + Gp[4 * r + 2] * R[6 + c];
          G[4 * r + 3] = ((Gp[4 * r] * rel[0] + Gp[4 * r + 1] * rel[1]) + Gp[4 * r + 2] * rel[2]) + Gp[4 * r + 3];
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) s_G[12 * j + i] = G[i];
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float t = G[4 * r + 3] - ((G[4 * r] * jt[0] + G[4 * r + 1] * jt[1]) + G[4 * r + 2] * jt[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) st[GM_S_A + 12 * j + 4 * r + c] = G[4 * r + c];
    st[GM_S_A + 12 * j + 4 * r + 3] = t;
    joints[(bh * a.J + j) * 3 + r] = G[4 * r + 3] + p.transl[bh * 3 + r];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) st[GM_S_G + 12 * j + i] = G[i];
}

__global__ __launch_bounds__(GM_BLOCK) void gm_verts_fwd(GmModels ms, GmCall a, GhManoParams p, float* __restrict__ points) {
  __shared__ float s_pf[9 * GM_MJ], s_A[12 * GM_MJ], s_beta[GH_MANO_MAX_NB];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const int V = m.V;
  if ((long long)blockIdx.x * GM_BLOCK >= V) return;
  const long long bh = (long long)b * a.H + h;
  const float* st = a.state + bh * GM_STATE;
  const int npf = 9 * (a.J - 1);
  if (tid < npf) s_pf[tid] = st[GM_S_R + 9 + tid] - ((tid % 9) % 4 == 0 ? 1.0f : 0.0f);
  if (tid < 12 * a.J) s_A[tid] = st[GM_S_A + tid];
  if (tid < a.NB) s_beta[tid] = p.betas[bh * a.NB + tid];
  __syncthreads();
  const int v = blockIdx.x * GM_BLOCK + tid;
  if (v >= V) return;
  float x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = m.v_template[(long long)c * V + v];
  for (int n = 0; n < a.NB; ++n) {
    const float* sd = m.shapedirs + (long long)n * 3 * V + v;
    const float bn = s_beta[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = fmaf(sd[(long long)c * V], bn, x[c]);
  }
  for (int k = 0; k < npf; ++k) {
    const float* pd = m.posedirs + (long long)k * 3 * V + v;
    const float f = s_pf[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = fmaf(pd[(long long)c * V], f, x[c]);
  }
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.f;
  for (int j = 0; j < a.J; ++j) {
    const float w = m.lbs_weights[(long long)j * V + v];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = fmaf(w, s_A[12 * j + e], T[e]);
  }
  float* out = points + ((long long)b * a.Ptot + ms.off[h] + v) * 3;
  float* vp = a.vp + bh * 3 * a.Vmax + v;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    out[r] = fmaf(T[4 * r + 2], x[2], fmaf(T[4 * r + 1], x[1], fmaf(T[4 * r], x[0], T[4 * r + 3]))) + p.transl[bh * 3 + r];
    vp[(long long)r * V] = x[r];
  }
}

__global__ __launch_bounds__(GM_BLOCK) void gm_points_fwd(GmModels ms, GmCall a, float* __restrict__ points) {
  const int h = blockIdx.y, b = blockIdx.z;
  const GhManoModel& m = ms.m[h];
  const long long pl = (long long)m.V + (long long)blockIdx.x * GM_BLOCK + threadIdx.x;
  if (pl >= m.P) return;
  const int pt = (int)pl;
  float* base = points + ((long long)b * a.Ptot + ms.off[h]) * 3;
  float acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* src = base + (long long)gm_clamp(m.st_idx[3LL * pt + k], m.V) * 3;
    const float w = m.st_w[3LL * pt + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = k == 0 ? w * src[c] : fmaf(w, src[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) base[3LL * pt + c] = acc[c];
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
// The chain once more in float64, from the float32 pose and betas the forward kept: R, G and Jt as the backward differentiates them.
// With the forward's float32 R, G and Jt the root's rotation gradient carried their rounding through the cancellation of
// dA^R - dA^t Jt^T: as far from float64 autograd as a float32 autograd is, which is not what the float64 sums behind it are for.
__global__ __launch_bounds__(GM_WAVE) void gm_chain_f64(GmModels ms, GmCall a) {
  __shared__ double s_G[12 * GM_MJ], s_Jt[3 * GM_MJ];
  const int h = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const long long bh = (long long)b * a.H + h;
  const float* st = a.state + bh * GM_STATE;
  double* ds = a.dst + bh * GM_DSTATE;
  const bool live = j < a.J;
  int par = -1, depth = -1;
  double R[9], jt[3] = {0., 0., 0.}, G[12];
  if (live) {
    par = m.parents[j];
    depth = gm_depth(m, j);
    double r[3], K[9], KK[9], ang, sn, cs;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = st[GM_S_POSE + 3 * j + c];
    gm_rodrigues(r, R, K, KK, &ang, &sn, &cs);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double acc = m.j_template[3 * j + c];
      for (int n = 0; n < a.NB; ++n) acc = fma(m.j_shapedirs[(3 * j + c) * a.NB + n], (double)st[GM_S_BETA + n], acc);
      jt[c] = acc;
      s_Jt[3 * j + c] = acc;
      ds[GM_D_JT + 3 * j + c] = acc;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ds[GM_D_R + 9 * j + i] = R[i];
  }
  __syncthreads();
  for (int d = 0; d < a.J; ++d) {
    if (live && depth == d) {
      if (par < 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) G[4 * r + c] = R[3 * r + c];
          G[4 * r + 3] = jt[r];
        }
      } else {
        const double* Gp = s_G + 12 * par;
        const double rel[3] = {jt[0] - s_Jt[3 * par], jt[1] - s_Jt[3 * par + 1], jt[2] - s_Jt[3 * par + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) G[4 * r + c] = (Gp[4 * r] * R[c] + Gp[4 * r + 1] * R[3 + c]) + Gp[4 * r + 2] * R[6 + c];
          G[4 * r + 3] = ((Gp[4 * r] * rel[0] + Gp[4 * r + 1] * rel[1]) + Gp[4 * r + 2] * rel[2]) + Gp[4 * r + 3];
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) { s_G[12 * j + i] = G[i]; ds[GM_D_G + 12 * j + i] = G[i]; }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(GM_BLOCK) void gm_colsum(GmModels ms, GmCall a, const float* __restrict__ d_points) {
  __shared__ double s4[4];
  const int h = blockIdx.y, b = blockIdx.z, ch = blockIdx.x, tid = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const long long p0 = (long long)ch * GH_MANO_CHUNK;
  if (p0 >= m.P) return;
  const float* g = d_points + ((long long)b * a.Ptot + ms.off[h] + p0) * 3;
  double acc[3] = {0., 0., 0.};
  for (int i = tid; i < GH_MANO_CHUNK && p0 + i < m.P; i += GM_BLOCK) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (double)g[3LL * i + c];
  }
  const long long bh = (long long)b * a.H + h;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = gm_block_sum(acc[c], s4);
    if (tid == 0) a.tp[(bh * a.nch + ch) * 3 + c] = s;
  }
}

__global__ __launch_bounds__(GM_BLOCK) void gm_verts_bwd(GmModels ms, GmCall a, const float* __restrict__ d_points) {
  __shared__ float s_A[12 * GM_MJ];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const int V = m.V;
  if ((long long)blockIdx.x * GM_BLOCK >= V) return;
  const long long bh = (long long)b * a.H + h;
  __shared__ double s_pf[9 * GM_MJ];
  const int npf = 9 * (a.J - 1);
  if (tid < 12 * a.J) s_A[tid] = a.state[bh * GM_STATE + GM_S_A + tid];
  if (tid < npf) s_pf[tid] = a.dst[bh * GM_DSTATE + GM_D_R + 9 + tid] - ((tid % 9) % 4 == 0 ? 1.0 : 0.0);
  __syncthreads();
  const int v = blockIdx.x * GM_BLOCK + tid;
  if (v >= V) return;
  {  // v_posed once more, in float64 (the forward's float32 copy stays with the forward)
    double x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = m.v_template[(long long)c * V + v];
    for (int n = 0; n < a.NB; ++n) {
      const float* sd = m.shapedirs + (long long)n * 3 * V + v;
      const double bn = a.state[bh * GM_STATE + GM_S_BETA + n];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = fma((double)sd[(long long)c * V], bn, x[c]);
    }
    for (int k = 0; k < npf; ++k) {
      const float* pd = m.posedirs + (long long)k * 3 * V + v;
      const double f = s_pf[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = fma((double)pd[(long long)c * V], f, x[c]);
    }
    double* vd = a.vpd + bh * 3 * a.Vmax + v;
#pragma unroll
    for (int c = 0; c < 3; ++c) vd[(long long)c * V] = x[c];
  }
  const float* gp = d_points + ((long long)b * a.Ptot + ms.off[h]) * 3;
  // a row of the transpose holds some sixty points at three levels: summed in float32, a vertex's cotangent is several ulp off, and
  // the rotation gradients, differences of sums over all vertices, showed it (d_global_orient 9 x the float32 reference's error)
  double g[3] = {0., 0., 0.};
  const int k0 = gm_clamp(m.tr_ptr[v], m.nnz + 1), k1 = gm_clamp(m.tr_ptr[v + 1], m.nnz + 1);
  for (int k = k0; k < k1; ++k) {
    const float* src = gp + (long long)gm_clamp(m.tr_point[k], m.P) * 3;
    const double w = m.tr_w[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = fma(w, (double)src[c], g[c]);
  }
  double T[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) T[e] = 0.;
  for (int j = 0; j < a.J; ++j) {
    const double w = m.lbs_weights[(long long)j * V + v];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) T[3 * r + c] = fma(w, (double)s_A[12 * j + 4 * r + c], T[3 * r + c]);
  }
  double* go = a.g + bh * 3 * a.Vmax + v;
  double* dv = a.dvp + bh * 3 * a.Vmax + v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    go[(long long)c * V] = g[c];
    dv[(long long)c * V] = (T[c] * g[0] + T[3 + c] * g[1]) + T[6 + c] * g[2];
  }
}

// groups of a (b, h): [0, J) joint j's dA; [J, 2 J - 1) joint j >= 1's nine pose blend-shape sums; [2 J - 1, 2 J - 1 + NB) a shape sum
__global__ __launch_bounds__(GM_BLOCK) void gm_reduce(GmModels ms, GmCall a, int want_pf, int want_sd) {
  __shared__ double s4[4];
  const int h = blockIdx.y, b = blockIdx.z, grp = blockIdx.x, tid = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const int V = m.V, J = a.J;
  const long long bh = (long long)b * a.H + h;
  const double* g = a.g + bh * 3 * a.Vmax;
  const double* dvp = a.dvp + bh * 3 * a.Vmax;
  double* red = a.red + bh * GM_RED;
  if (grp < J) {
    const double* vp = a.vpd + bh * 3 * a.Vmax;
    const float* w = m.lbs_weights + (long long)grp * V;
    double acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.;
    for (int v = tid; v < V; v += GM_BLOCK) {
      const double wv = w[v];
      const double x[3] = {vp[v], vp[(long long)V + v], vp[2LL * V + v]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double t = wv * g[(long long)r * V + v];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[4 * r + c] = fma(t, x[c], acc[4 * r + c]);
        acc[4 * r + 3] = acc[4 * r + 3] + t;
      }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const double s = gm_block_sum(acc[e], s4);
      if (tid == 0) red[GM_R_A + 12 * grp + e] = s;
    }
  } else if (grp < 2 * J - 1) {
    if (!want_pf) return;
    const int k0 = 9 * (grp - J);
    const float* pd = m.posedirs + (long long)k0 * 3 * V;
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.;
    for (int i = tid; i < 3 * V; i += GM_BLOCK) {
      const double d = dvp[i];
#pragma unroll
      for (int e = 0; e < 9; ++e) acc[e] = fma((double)pd[(long long)e * 3 * V + i], d, acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const double s = gm_block_sum(acc[e], s4);
      if (tid == 0) red[GM_R_PF + k0 + e] = s;
    }
  } else {
    if (!want_sd) return;
    const int n = grp - (2 * J - 1);
    const float* sd = m.shapedirs + (long long)n * 3 * V;
    double acc = 0.;
    for (int i = tid; i < 3 * V; i += GM_BLOCK) acc = fma((double)sd[i], dvp[i], acc);
    const double s = gm_block_sum(acc, s4);
    if (tid == 0) red[GM_R_SD + n] = s;
  }
}

__global__ __launch_bounds__(GM_WAVE) void gm_chain_bwd(GmModels ms, GmCall a, const float* __restrict__ d_joints, GhManoGrads out,
                                                         int has_red, int has_pf, int has_sd, int has_tp) {
  __shared__ double s_G[12 * GM_MJ], s_Jt[3 * GM_MJ], s_C[15 * GM_MJ], s_dJt[3 * GM_MJ];
  const int h = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
  const GhManoModel& m = ms.m[h];
  const int J = a.J;
  const long long bh = (long long)b * a.H + h;
  const float* st = a.state + bh * GM_STATE;
  const double* red = a.red + bh * GM_RED;
  const double* ds = a.dst + bh * GM_DSTATE;
  const bool live = j < J;
  int par = -1, depth = -1;
  double R[9], G[12], jt[3], dGR[9], dGt[3], dJt[3], dR[9];
  if (live) {
    par = m.parents[j];
    depth = gm_depth(m, j);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ds[GM_D_R + 9 * j + i];
#pragma unroll
    for (int i = 0; i < 12; ++i) { G[i] = ds[GM_D_G + 12 * j + i]; s_G[12 * j + i] = G[i]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { jt[c] = ds[GM_D_JT + 3 * j + c]; s_Jt[3 * j + c] = jt[c]; }
    double dA[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) dA[e] = has_red ? red[GM_R_A + 12 * j + e] : 0.;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dGR[3 * r + c] = dA[4 * r + c] - dA[4 * r + 3] * jt[c];
      dGt[r] = dA[4 * r + 3] + (d_joints ? (double)d_joints[(bh * J + j) * 3 + r] : 0.);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dJt[c] = -((G[c] * dA[3] + G[4 + c] * dA[7]) + G[8 + c] * dA[11]);
  }
  __syncthreads();
  for (int d = J - 1; d >= 1; --d) {
    if (live && depth == d) {
      const double* Gp = s_G + 12 * par;
      const double rel[3] = {jt[0] - s_Jt[3 * par], jt[1] - s_Jt[3 * par + 1], jt[2] - s_Jt[3 * par + 2]};
      double* C = s_C + 15 * j;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dR[3 * r + c] = (Gp[r] * dGR[c] + Gp[4 + r] * dGR[3 + c]) + Gp[8 + r] * dGR[6 + c];
          C[3 * r + c] = ((dGR[3 * r] * R[3 * c] + dGR[3 * r + 1] * R[3 * c + 1]) + dGR[3 * r + 2] * R[3 * c + 2]) + dGt[r] * rel[c];
        }
        const double drel = (Gp[r] * dGt[0] + Gp[4 + r] * dGt[1]) + Gp[8 + r] * dGt[2];
        C[9 + r] = dGt[r];
        C[12 + r] = drel;
        dJt[r] = dJt[r] + drel;
      }
    }
    __syncthreads();
    if (live && depth == d - 1) {
      for (int q = j + 1; q < J; ++q) {
        if (m.parents[q] != j) continue;
        const double* C = s_C + 15 * q;
#pragma unroll
        for (int i = 0; i < 9; ++i) dGR[i] = dGR[i] + C[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) { dGt[c] = dGt[c] + C[9 + c]; dJt[c] = dJt[c] - C[12 + c]; }
      }
    }
    __syncthreads();
  }
  if (live) {
    if (depth == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) dR[i] = dGR[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) dJt[c] = dJt[c] + dGt[c];
    } else if (has_red && has_pf) {
#pragma unroll
      for (int i = 0; i < 9; ++i) dR[i] = dR[i] + red[GM_R_PF + 9 * (j - 1) + i];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s_dJt[3 * j + c] = dJt[c];
    float* dst = j == 0 ? out.global_orient : out.hand_pose;
    if (dst) {
      double r[3], Rr[9], K[9], KK[9], ang, sn, cs;
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = st[GM_S_POSE + 3 * j + c];
      gm_rodrigues(r, Rr, K, KK, &ang, &sn, &cs);
      const double oc = 1.0 - cs;
      double ds = 0., doc = 0., dK[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) { ds = fma(dR[i], K[i], ds); doc = fma(dR[i], KK[i], doc); }
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          // (dR K^T + K^T dR)[r][c] = sum_k dR[r][k] K[c][k] + K[k][r] dR[k][c]
          double t = 0.;
#pragma unroll
          for (int k = 0; k < 3; ++k) t = t + (dR[3 * r_ + k] * K[3 * c + k] + K[3 * k + r_] * dR[3 * k + c]);
          dK[3 * r_ + c] = sn * dR[3 * r_ + c] + oc * t;
        }
      const double dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
      const double dir[3] = {r[0] / ang, r[1] / ang, r[2] / ang};
      const double da = (ds * cs + doc * sn) - ((dd[0] * dir[0] + dd[1] * dir[1]) + dd[2] * dir[2]) / ang;
      float* o = dst + (j == 0 ? bh * 3 : bh * 3 * (J - 1) + 3 * (j - 1));
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (float)(dd[c] / ang + da * ((r[c] + (double)1e-8f) / ang));
    }
  }
  __syncthreads();
  if (out.betas && j < a.NB) {
    double acc = (has_red && has_sd) ? red[GM_R_SD + j] : 0.;
    for (int i = 0; i < 3 * J; ++i) acc = fma(m.j_shapedirs[i * a.NB + j], s_dJt[i], acc);
    out.betas[bh * a.NB + j] = (float)acc;
  }
  if (out.transl && j < 3) {
    double acc = 0.;
    if (has_tp) {
      const int nch = (int)(((long long)m.P + GH_MANO_CHUNK - 1) / GH_MANO_CHUNK);
      for (int ch = 0; ch < nch; ++ch) acc = acc + a.tp[(bh * a.nch + ch) * 3 + j];
    }
    if (d_joints)
      for (int q = 0; q < J; ++q) acc = acc + (double)d_joints[(bh * J + q) * 3 + j];
    out.transl[bh * 3 + j] = (float)acc;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct GmPlan {
  GmModels ms;
  int Vmax, nch;
  long long Ptot, Pmax, extra;  // extra: the most points behind the vertices that any hand has
  size_t o_state, o_vp, o_g, o_dvp, o_red, o_tp, o_dst, o_vpd, total;  // bytes
};

// GH_OK with the plan filled in, or the status the header names (everything that can be judged without the tensors)
static int gm_plan(const GhManoDims* d, const GhManoModel* models, GmPlan* pl) {
  if (!d || !models) return GH_ERR_INVALID_ARG;
  if (d->B < 0 || d->H < 1 || d->J < 1 || d->NB < 1) return GH_ERR_INVALID_ARG;
  if (d->H > GH_MANO_MAX_H || d->J > GH_MANO_MAX_J || d->NB > GH_MANO_MAX_NB || d->B > GH_MANO_MAX_B) return GH_ERR_UNSUPPORTED;
  for (int h = 0; h < d->H; ++h) {
    const GhManoModel& m = models[h];
    if (m.V < 1 || m.P < m.V || m.levels < 0 || m.nnz < m.P || (m.levels == 0 && m.P != m.V)) return GH_ERR_INVALID_ARG;
    if (m.parents[0] != -1) return GH_ERR_INVALID_ARG;
    for (int i = 1; i < d->J; ++i)
      if (m.parents[i] < 0 || m.parents[i] >= i) return GH_ERR_INVALID_ARG;
  }
  for (int h = 0; h < d->H; ++h) {
    const GhManoModel& m = models[h];
    if (m.levels > GH_MANO_MAX_LEVELS || m.V > GH_MANO_MAX_V || m.P > GH_MANO_MAX_P) return GH_ERR_UNSUPPORTED;
  }
  pl->Vmax = 0; pl->Ptot = 0; pl->Pmax = 0; pl->extra = 0;
  for (int h = 0; h < GH_MANO_MAX_H; ++h) {
    pl->ms.m[h] = models[h < d->H ? h : 0];
    pl->ms.off[h] = 0;
    if (h >= d->H) continue;
    const GhManoModel& m = models[h];
    pl->ms.off[h] = pl->Ptot;
    pl->Ptot += m.P;
    if (m.V > pl->Vmax) pl->Vmax = m.V;
    if (m.P > pl->Pmax) pl->Pmax = m.P;
    if (m.P - m.V > pl->extra) pl->extra = m.P - m.V;
  }
  pl->nch = (int)((pl->Pmax + GH_MANO_CHUNK - 1) / GH_MANO_CHUNK);
  const size_t bh = (size_t)(d->B > 0 ? d->B : 1) * (size_t)d->H, f = sizeof(float);
  size_t o = 0;
  pl->o_state = o; o += ghr_align(bh * GM_STATE * f);
  pl->o_vp = o;    o += ghr_align(bh * 3 * (size_t)pl->Vmax * f);
  pl->o_g = o;     o += ghr_align(bh * 3 * (size_t)pl->Vmax * sizeof(double));
  pl->o_dvp = o;   o += ghr_align(bh * 3 * (size_t)pl->Vmax * sizeof(double));
  pl->o_red = o;   o += ghr_align(bh * GM_RED * sizeof(double));
  pl->o_tp = o;    o += ghr_align(bh * (size_t)pl->nch * 3 * sizeof(double));
  pl->o_dst = o;   o += ghr_align(bh * GM_DSTATE * sizeof(double));
  pl->o_vpd = o;   o += ghr_align(bh * 3 * (size_t)pl->Vmax * sizeof(double));
  pl->total = o;
  return GH_OK;
}

static void gm_call(const GhManoDims* d, const GmPlan& pl, void* ws, GmCall* a) {
  char* w = (char*)ws;
  a->B = d->B; a->H = d->H; a->J = d->J; a->NB = d->NB; a->Vmax = pl.Vmax; a->nch = pl.nch; a->Ptot = pl.Ptot;
  a->state = (float*)(w + pl.o_state); a->vp = (float*)(w + pl.o_vp); a->g = (double*)(w + pl.o_g);
  a->dvp = (double*)(w + pl.o_dvp); a->red = (double*)(w + pl.o_red); a->tp = (double*)(w + pl.o_tp);
  a->dst = (double*)(w + pl.o_dst); a->vpd = (double*)(w + pl.o_vpd);
}

// the model arrays every launch may touch: present and 4-byte aligned
static bool gm_models_ok(const GhManoDims* d, const GhManoModel* models, bool stencil, bool transpose) {
  for (int h = 0; h < d->H; ++h) {
    const GhManoModel& m = models[h];
    if (!m.v_template || !m.shapedirs || !m.lbs_weights || !m.j_template || !m.j_shapedirs || !m.pose_mean) return false;
    if (d->J > 1 && !m.posedirs) return false;
    if (stencil && m.P > m.V && (!m.st_idx || !m.st_w)) return false;
    if (transpose && (!m.tr_ptr || !m.tr_point || !m.tr_w)) return false;
    if (!ghr_al4(m.v_template) || !ghr_al4(m.shapedirs) || !ghr_al4(m.posedirs) || !ghr_al4(m.lbs_weights) || !ghr_al4(m.j_template) ||
        !ghr_al4(m.j_shapedirs) || !ghr_al4(m.pose_mean) || !ghr_al4(m.st_idx) || !ghr_al4(m.st_w) || !ghr_al4(m.tr_ptr) ||
        !ghr_al4(m.tr_point) || !ghr_al4(m.tr_w))
      return false;
  }
  return true;
}

extern "C" size_t gh_mano_workspace_bytes(const GhManoDims* dims, const GhManoModel* models) {
  GmPlan pl;
  return gm_plan(dims, models, &pl) == GH_OK ? pl.total : 0;
}

extern "C" int gh_mano_forward(const GhManoDims* dims, const GhManoModel* models, const GhManoParams* params, float* points, float* joints,
                               void* ws, size_t ws_bytes, void* hip_stream) {
  GmPlan pl;
  if (!params) return GH_ERR_INVALID_ARG;
  const int rc = gm_plan(dims, models, &pl);
  if (rc != GH_OK) return rc;
  if (!params->global_orient || !params->betas || !params->transl || (dims->J > 1 && !params->hand_pose) || !points || !joints || !ws)
    return GH_ERR_INVALID_ARG;
  if (!ghr_al4(params->global_orient) || !ghr_al4(params->hand_pose) || !ghr_al4(params->betas) || !ghr_al4(params->transl) ||
      !ghr_al4(points) || !ghr_al4(joints) || ((uintptr_t)ws & 7u) || !gm_models_ok(dims, models, true, false))
    return GH_ERR_INVALID_ARG;
  if (dims->B == 0) return GH_OK;
  if (ws_bytes < pl.total) return GH_ERR_WORKSPACE_SMALL;
  GmCall a;
  gm_call(dims, pl, ws, &a);
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gm_chain_fwd, dim3(dims->H, dims->B), dim3(GM_WAVE), 0, st, pl.ms, a, *params, joints);
  hipLaunchKernelGGL(gm_verts_fwd, dim3((pl.Vmax + GM_BLOCK - 1) / GM_BLOCK, dims->H, dims->B), dim3(GM_BLOCK), 0, st, pl.ms, a, *params,
                     points);
  if (pl.extra > 0)
    hipLaunchKernelGGL(gm_points_fwd, dim3((unsigned)((pl.extra + GM_BLOCK - 1) / GM_BLOCK), dims->H, dims->B), dim3(GM_BLOCK), 0, st, pl.ms, a,
                       points);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_mano_backward(const GhManoDims* dims, const GhManoModel* models, const float* d_points, const float* d_joints,
                                const GhManoGrads* grads, void* ws, size_t ws_bytes, void* hip_stream) {
  GmPlan pl;
  if (!grads) return GH_ERR_INVALID_ARG;
  const int rc = gm_plan(dims, models, &pl);
  if (rc != GH_OK) return rc;
  GhManoGrads out = *grads;
  if (dims->J == 1) out.hand_pose = nullptr;
  const bool deep = out.global_orient || out.hand_pose || out.betas;  // anything behind the skinning
  if (!ws || ((uintptr_t)ws & 7u) || !ghr_al4(d_points) || !ghr_al4(d_joints) || !ghr_al4(out.global_orient) || !ghr_al4(out.hand_pose) ||
      !ghr_al4(out.betas) || !ghr_al4(out.transl) || !gm_models_ok(dims, models, false, deep && d_points))
    return GH_ERR_INVALID_ARG;
  if (dims->B == 0 || (!deep && !out.transl)) return GH_OK;
  if (ws_bytes < pl.total) return GH_ERR_WORKSPACE_SMALL;
  GmCall a;
  gm_call(dims, pl, ws, &a);
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  const int has_tp = (out.transl && d_points) ? 1 : 0, has_red = (deep && d_points) ? 1 : 0;
  const int want_pf = out.hand_pose ? 1 : 0, want_sd = out.betas ? 1 : 0;
  if (has_tp) hipLaunchKernelGGL(gm_colsum, dim3(pl.nch, dims->H, dims->B), dim3(GM_BLOCK), 0, st, pl.ms, a, d_points);
  if (deep) hipLaunchKernelGGL(gm_chain_f64, dim3(dims->H, dims->B), dim3(GM_WAVE), 0, st, pl.ms, a);
  if (has_red) {
    hipLaunchKernelGGL(gm_verts_bwd, dim3((pl.Vmax + GM_BLOCK - 1) / GM_BLOCK, dims->H, dims->B), dim3(GM_BLOCK), 0, st, pl.ms, a, d_points);
    hipLaunchKernelGGL(gm_reduce, dim3(2 * dims->J - 1 + dims->NB, dims->H, dims->B), dim3(GM_BLOCK), 0, st, pl.ms, a, want_pf, want_sd);
  }
  hipLaunchKernelGGL(gm_chain_bwd, dim3(dims->H, dims->B), dim3(GM_WAVE), 0, st, pl.ms, a, d_joints, out, has_red, want_pf, want_sd, has_tp);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
