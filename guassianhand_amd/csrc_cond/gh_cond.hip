// gh_cond.hip — the point conditioning (include/gh_cond.h): the per-point rows of TGS._forward, and additional_features_fc over them
// with the batch-wide columns folded into per-batch constants.
//   tile      one 4-wave workgroup per GH_COND_ROWS = 64 rows, lane = row. The rows are BUILT in LDS (ghc_build: copies, sinf / cosf of
//             the rounded products, the code read through its stride) at an odd pitch, so that a lane reads its own row without a
//             bank conflict. gh_cond_rows copies the tile out; the MLP kernels never write it.
//   fold      one workgroup per batch element, float64: m_e, M_e, c1, c2; workgroup 0 also c0 and W1g.
//   forward   m_v, M_v (wave w sums the columns k = w mod 4), the pairwise combination with (m_e, M_e), the row centred in place, fc1
//             over W1g with the per-batch terms in the epilogue, fc2. Wave w owns the outputs w, w + 4, ..., three at a time.
//   backward  the same forward up to h1, W2^T . g gated in place, W1g^T . d1 with the two sums of the LayerNorm's backward gathered
//             on the way, dcode for the code columns. One launch.
// The moments and the two layer routines (ghr_moments, ghr_linear, ghr_linear_t) are csrc_rows/gh_rows.h's, shared with gh_vert.hip.
// Weights are wave-uniform (scalar cache); the per-batch constants are per-lane loads: a tile may hold rows of several batch
// elements. No atomics; every float sum has a fixed order that depends on the layout alone.
#include "../../include/gh_cond.h"
#include "../csrc_rows/gh_rows.h"

#define GHC_BLOCK GHR_BLOCK
#define GHC_ROWS GH_COND_ROWS
#define GHC_PI_F 3.14159274101257324219f  // float32(pi): f_l = float32(pi * 2^l) = float32(pi) * 2^l, the scaling being exact

static_assert(GHC_ROWS == GHR_ROWS, "the shared row routines' tile: lane = row, four waves share a row's columns");

struct GhcIn {
  const float *uv, *xyz, *flag, *code;
  long long code_stride;
  int Cc, L, Dv;
};

// one positional-encoding segment: x (P,C) -> columns [col0, col0 + 2C + 2CL) of the tile's rows
__device__ __forceinline__ void ghc_pe(float* s, int pitch, int col0, const float* __restrict__ x, int C, long long row0, int nrows, int L,
                                       int tid) {
  for (int i = tid; i < GHC_ROWS * C; i += GHC_BLOCK) {
    const int r = i / C, c = i - r * C;
    const float v = r < nrows ? x[row0 * C + i] : 0.f;
    float* d = s + r * pitch + col0 + c;
    d[0] = v;
    d[C] = v;
  }
  const int per = C * L;
  for (int i = tid; i < GHC_ROWS * per; i += GHC_BLOCK) {
    const int r = i / per, q = i - r * per, l = q / C, c = q - l * C;
    const float v = r < nrows ? x[(row0 + r) * C + c] : 0.f;
    const float y = (GHC_PI_F * (float)(1 << l)) * v;  // one rounding: the scale by 2^l is exact
    float* d = s + r * pitch + col0 + 2 * C + 2 * C * l + c;
    d[0] = sinf(y);
    d[C] = cosf(y);
  }
}

// the tile's rows -> s[row * pitch + col], col < Dv; rows past the end are built from zeros
__device__ __forceinline__ void ghc_build(float* s, int pitch, const GhcIn& in, long long row0, int nrows, int tid) {
  int col = 0;
  if (in.uv) {
    ghc_pe(s, pitch, col, in.uv, 2, row0, nrows, in.L, tid);
    col += 4 + 4 * in.L;
  }
  if (in.xyz) {
    ghc_pe(s, pitch, col, in.xyz, 3, row0, nrows, in.L, tid);
    col += 6 + 6 * in.L;
  }
  if (in.flag) {
    if (tid < GHC_ROWS) s[tid * pitch + col] = tid < nrows ? in.flag[row0 + tid] : 0.f;
    col += 1;
  }
  const int Cc = in.Cc;
  for (int i = tid; i < GHC_ROWS * Cc; i += GHC_BLOCK) {
    const int r = i / Cc, c = i - r * Cc;
    s[r * pitch + col + c] = r < nrows ? in.code[(row0 + r) * in.code_stride + c] : 0.f;
  }
}

// ---- the rows alone --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHC_BLOCK) void ghc_rows_kernel(GhcIn in, int P, float* __restrict__ out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float ghc_smem[];
  const GhrTile t = ghr_tile<GHC_ROWS>(P);
  const int Dv = in.Dv, VP = Dv | 1;
  ghc_build(ghc_smem, VP, in, t.row0, t.nrows, t.tid);
  __syncthreads();
  for (int i = t.tid; i < t.nrows * Dv; i += GHC_BLOCK) {
    const int r = i / Dv, c = i - r * Dv;
    out[(t.row0 + r) * out_stride + c] = ghc_smem[r * VP + c];
  }
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ghc_wave_sum(double v) {  // a fixed butterfly: every lane ends with the same sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum of every thread's v, in a fixed order (thread-strided partials, a butterfly per wave, then the waves in order)
__device__ __forceinline__ double ghc_block_sum(double v, double* s_w, int tid) {
  v = ghc_wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(GHC_BLOCK) void ghc_fold_kernel(const float* __restrict__ e, int De, int Dv, int Hd, GhCondParams p,
                                                             float* __restrict__ fold) {
  __shared__ double s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, D = Dv + De;
  const float* eb = e + (size_t)b * De;
  float* fb = fold + Hd + (size_t)Hd * Dv + (size_t)b * (2 + 2 * Hd);
  double s = 0.0;
  for (int k = tid; k < De; k += GHC_BLOCK) s += (double)eb[k];
  s = ghc_block_sum(s, s_w, tid);
  const float m32 = De > 0 ? (float)(s / (double)De) : 0.f;
  const double m = (double)m32;  // what the row kernels read: M_e and c2 are centred on the rounded value
  double q = 0.0;
  for (int k = tid; k < De; k += GHC_BLOCK) {
    const double d = (double)eb[k] - m;
    q += d * d;
  }
  q = ghc_block_sum(q, s_w, tid);
  if (tid == 0) {
    fb[0] = m32;
    fb[1] = (float)q;
  }
  for (int j = wave; j < Hd; j += 4) {
    const float* w = p.fc1_weight + (size_t)j * D + Dv;
    double a1 = 0.0, a2 = 0.0;
    for (int k = lane; k < De; k += 64) {
      const double wg = (double)w[k] * (double)p.ln_weight[Dv + k];
      a1 += wg;
      a2 += wg * ((double)eb[k] - m);
    }
    a1 = ghc_wave_sum(a1);
    a2 = ghc_wave_sum(a2);
    if (lane == 0) {
      fb[2 + j] = (float)a1;
      fb[2 + Hd + j] = (float)a2;
    }
  }
  if (b != 0) return;
  for (int j = wave; j < Hd; j += 4) {  // c0 = W1 . beta + b1
    const float* w = p.fc1_weight + (size_t)j * D;
    double a = 0.0;
    for (int k = lane; k < D; k += 64) a += (double)w[k] * (double)p.ln_bias[k];
    a = ghc_wave_sum(a);
    if (lane == 0) fold[j] = (float)(a + (double)p.fc1_bias[j]);
  }
  for (int i = tid; i < Hd * Dv; i += GHC_BLOCK) {  // W1g = W1_v * gamma_v
    const int j = i / Dv, k = i - j * Dv;
    fold[Hd + i] = p.fc1_weight[(size_t)j * D + k] * p.ln_weight[k];
  }
}

// ---- the LayerNorm + MLP over the rows ------------------------------------------------------------------------------------------
struct GhcRow {
  float rstd, dm;   // dm = m_e - mu
  const float* fb;  // the lane's batch element: m_e, M_e, c1[Hd], c2[Hd]
};

// build the rows, the LayerNorm's statistics, the rows centred in place (s_v holds v - mu), h1 = relu(pre1) in s_h
__device__ __forceinline__ GhcRow ghc_forward_tile(float* s_red, float* s_v, float* s_h, int VP, int HP, const GhcIn& in, int P, int N,
                                                   int De, int Hd, const float* __restrict__ fold, float eps, const GhrTile& t) {
  const int Dv = in.Dv, D = Dv + De, lane = t.lane, wave = t.wave;
  ghc_build(s_v, VP, in, t.row0, t.nrows, t.tid);
  __syncthreads();
  float* vr = s_v + lane * VP;
  const GhrMoments mo = ghr_moments(vr, Dv, s_red, lane, wave);
  const float m_v = mo.mean, M_v = mo.m2;
  const long long row = t.row0 + lane < (long long)P ? t.row0 + lane : (long long)P - 1;  // (lanes past the end read the last row's constants)
  GhcRow r;
  r.fb = fold + Hd + (size_t)Hd * Dv + (size_t)(row / N) * (2 + 2 * Hd);
  const float m_e = r.fb[0], M_e = r.fb[1];
  const float delta = m_e - m_v;
  const float mu = fmaf(delta, (float)De / (float)D, m_v);
  const float M = (M_v + M_e) + (delta * delta) * (float)((double)Dv * (double)De / (double)D);
  r.rstd = 1.0f / sqrtf(M / (float)D + eps);
  r.dm = m_e - mu;
  for (int k = wave; k < Dv; k += 4) vr[k] -= mu;
  __syncthreads();
  const float* c0 = fold;
  ghr_linear(Dv, fold + Hd, Hd, wave, [&](int k) { return vr[k]; }, [&](int j, float a) {
    float v = fmaf(r.rstd, (a + r.fb[2 + Hd + j]) + r.dm * r.fb[2 + j], c0[j]);
    v = v > 0.f ? v : (v == v ? 0.f : v);  // (a NaN stays a NaN, as torch's relu keeps it)
    s_h[lane * HP + j] = v;
  });
  __syncthreads();
  return r;
}

static inline int ghc_vp(int Dv, int Hd) { return (Dv > Hd ? Dv : Hd) | 1; }

__global__ __launch_bounds__(GHC_BLOCK) void ghc_fwd_kernel(GhcIn in, int P, int N, int De, int Hd, const float* __restrict__ fold,
                                                            const float* __restrict__ W2, const float* __restrict__ b2, float eps,
                                                            float* __restrict__ out, int VP) {
  extern __shared__ __attribute__((aligned(16))) float ghc_smem[];
  const int HP = Hd | 1;
  float* s_red = ghc_smem;              // 2 x GHC_BLOCK
  float* s_v = s_red + 2 * GHC_BLOCK;   // GHC_ROWS x VP: the row, later the output (VP >= Hd)
  float* s_h = s_v + GHC_ROWS * VP;     // GHC_ROWS x HP
  const GhrTile t = ghr_tile<GHC_ROWS>(P);
  ghc_forward_tile(s_red, s_v, s_h, VP, HP, in, P, N, De, Hd, fold, eps, t);
  const float* hr = s_h + t.lane * HP;
  float* outr = s_v + t.lane * VP;
  ghr_linear(Hd, W2, Hd, t.wave, [&](int k) { return hr[k]; }, [&](int j, float a) { outr[j] = a + b2[j]; });
  __syncthreads();
  for (int e = t.tid; e < t.nrows * Hd; e += GHC_BLOCK) {  // the tile's contiguous run of the output
    const int r = e / Hd, c = e - r * Hd;
    out[t.row0 * Hd + e] = s_v[r * VP + c];
  }
}

__global__ __launch_bounds__(GHC_BLOCK) void ghc_bwd_kernel(GhcIn in, int P, int N, int De, int Hd, const float* __restrict__ fold,
                                                            const float* __restrict__ W2, float eps, const float* __restrict__ g_out,
                                                            float* __restrict__ dcode, long long dcode_stride, int VP) {
  extern __shared__ __attribute__((aligned(16))) float ghc_smem[];
  const int HP = Hd | 1, Cc = in.Cc, CP = Cc | 1, Dv = in.Dv, D = Dv + De, code0 = Dv - Cc;
  float* s_red = ghc_smem;              // 2 x GHC_BLOCK
  float* s_v = s_red + 2 * GHC_BLOCK;   // GHC_ROWS x VP: v - mu
  float* s_h = s_v + GHC_ROWS * VP;     // GHC_ROWS x HP: h1, then d1 in place
  float* s_g = s_h + GHC_ROWS * HP;     // GHC_ROWS x HP: the cotangent
  float* s_a = s_g + GHC_ROWS * HP;     // GHC_ROWS x CP: a over the code columns, then dcode in place
  const GhrTile t = ghr_tile<GHC_ROWS>(P);
  const int lane = t.lane, wave = t.wave;
  const GhcRow r = ghc_forward_tile(s_red, s_v, s_h, VP, HP, in, P, N, De, Hd, fold, eps, t);
  for (int e = t.tid; e < GHC_ROWS * Hd; e += GHC_BLOCK) {  // rows past the end, and a null cotangent, are zeros
    const int rr = e / Hd, c = e - rr * Hd;
    s_g[rr * HP + c] = (rr < t.nrows && g_out) ? g_out[t.row0 * Hd + e] : 0.f;
  }
  __syncthreads();
  float* hr = s_h + lane * HP;
  ghr_linear_t(s_g + lane * HP, Hd, W2, Hd, wave, [&](int i, float a) { hr[i] = hr[i] > 0.f ? a : 0.f; });  // h1 > 0 exactly where pre1 > 0
  __syncthreads();
  const float* vr = s_v + lane * VP;
  float* ar = s_a + lane * CP;
  float p1 = 0.f, p2 = 0.f;  // this wave's share of s1 and s2
  ghr_linear_t(hr, Hd, fold + Hd, Dv, wave, [&](int k, float a) {
    p1 += a;
    p2 = fmaf(a, r.rstd * vr[k], p2);
    if (k >= code0) ar[k - code0] = a;
  });
  float q1 = 0.f, q2 = 0.f;
  for (int j = wave; j < Hd; j += 4) {
    const float d1 = hr[j], c1 = r.fb[2 + j];
    q1 = fmaf(d1, c1, q1);
    q2 = fmaf(d1, r.fb[2 + Hd + j] + r.dm * c1, q2);
  }
  s_red[wave * GHC_ROWS + lane] = p1 + q1;
  s_red[GHC_BLOCK + wave * GHC_ROWS + lane] = fmaf(r.rstd, q2, p2);
  __syncthreads();
  const float m1 = ghr_sum4(s_red, lane) / (float)D, m2 = ghr_sum4(s_red + GHC_BLOCK, lane) / (float)D;
  for (int k = wave; k < Cc; k += 4) ar[k] = fmaf(-(r.rstd * vr[code0 + k]), m2, ar[k] - m1) * r.rstd;
  __syncthreads();
  for (int i = t.tid; i < t.nrows * Cc; i += GHC_BLOCK) {
    const int rr = i / Cc, c = i - rr * Cc;
    dcode[(t.row0 + rr) * dcode_stride + c] = s_a[rr * CP + c];
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int ghc_layout(const GhCondRows* in, GhcIn* o) {
  if (!in) return GH_ERR_INVALID_ARG;
  if (in->levels < 1 || in->levels > GH_COND_MAX_LEVELS || in->Cc < 0 || in->Cc > GH_COND_MAX_CODE) return GH_ERR_INVALID_ARG;
  if ((in->Cc > 0) != (in->code != nullptr) || in->code_stride < in->Cc) return GH_ERR_INVALID_ARG;
  const int L = in->levels;
  const int Dv = (in->uv ? 4 + 4 * L : 0) + (in->xyz ? 6 + 6 * L : 0) + (in->flag ? 1 : 0) + in->Cc;
  if (Dv < 1) return GH_ERR_INVALID_ARG;
  if (o) {
    o->uv = in->uv; o->xyz = in->xyz; o->flag = in->flag; o->code = in->code;
    o->code_stride = (long long)in->code_stride; o->Cc = in->Cc; o->L = L; o->Dv = Dv;
  }
  return Dv;
}

static inline unsigned ghc_blocks(int P) { return (unsigned)((P + GHC_ROWS - 1) / GHC_ROWS); }

extern "C" int gh_cond_width(const GhCondRows* in) { return ghc_layout(in, nullptr); }

extern "C" size_t gh_cond_fold_bytes(int B, int Dv, int Hd) {
  if (B < 1 || Dv < 1 || Hd < 1 || Hd > GH_COND_MAX_HD) return 0;
  return ((size_t)Hd + (size_t)Hd * Dv + (size_t)B * (2 + 2 * Hd)) * sizeof(float);
}

extern "C" int gh_cond_rows(const GhCondRows* in, int P, float* out, int64_t out_stride, void* hip_stream) {
  GhcIn g;
  const int Dv = ghc_layout(in, &g);
  if (Dv < 0) return Dv;
  if (P < 0 || !out || out_stride < Dv) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(ghc_rows_kernel, dim3(ghc_blocks(P)), dim3(GHC_BLOCK), (size_t)GHC_ROWS * (Dv | 1) * sizeof(float),
                     (hipStream_t)hip_stream, g, P, out, (long long)out_stride);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

static bool ghc_params_ok(const GhCondParams* p) {
  return p && p->ln_weight && p->ln_bias && p->fc1_weight && p->fc1_bias && p->fc2_weight && p->fc2_bias;
}

extern "C" int gh_cond_fold(const float* e, int B, int De, int Dv, int Hd, const GhCondParams* params, float* fold, size_t fold_bytes,
                            void* hip_stream) {
  if (B < 0 || De < 0 || Dv < 1 || Hd < 1 || Hd > GH_COND_MAX_HD || !ghc_params_ok(params) || !fold) return GH_ERR_INVALID_ARG;
  if (De > 0 && !e) return GH_ERR_INVALID_ARG;
  if (B == 0) return GH_OK;
  if (fold_bytes < gh_cond_fold_bytes(B, Dv, Hd)) return GH_ERR_WORKSPACE_SMALL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(ghc_fold_kernel, dim3((unsigned)B), dim3(GHC_BLOCK), 0, (hipStream_t)hip_stream, e, De, Dv, Hd, *params, fold);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

static int ghc_mlp_check(int Dv, int P, int N, int De, int Hd, const GhCondParams* params, const float* fold, float eps) {
  if (Dv < 0) return Dv;
  if (P < 0 || N < 1 || P % N != 0 || De < 0 || Hd < 1 || Hd > GH_COND_MAX_HD || !ghc_params_ok(params) || !fold) return GH_ERR_INVALID_ARG;
  if (!(eps >= 0.f)) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

extern "C" int gh_cond_mlp_forward(const GhCondRows* in, int P, int N, int De, int Hd, const GhCondParams* params, const float* fold,
                                   float eps, float* out, void* hip_stream) {
  GhcIn g;
  const int Dv = ghc_layout(in, &g);
  const int rc = ghc_mlp_check(Dv, P, N, De, Hd, params, fold, eps);
  if (rc != GH_OK) return rc;
  if (!out) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  const int VP = ghc_vp(Dv, Hd), HP = Hd | 1;
  const size_t lds = (size_t)(2 * GHC_BLOCK + GHC_ROWS * (VP + HP)) * sizeof(float);
  (void)hipGetLastError();
  ghr_allow_lds<ghc_fwd_kernel>(lds);
  hipLaunchKernelGGL(ghc_fwd_kernel, dim3(ghc_blocks(P)), dim3(GHC_BLOCK), lds, (hipStream_t)hip_stream, g, P, N, De, Hd, fold,
                     params->fc2_weight, params->fc2_bias, eps, out, VP);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_cond_mlp_backward(const GhCondRows* in, int P, int N, int De, int Hd, const GhCondParams* params, const float* fold,
                                    float eps, const float* g_out, float* dcode, int64_t dcode_stride, void* hip_stream) {
  GhcIn g;
  const int Dv = ghc_layout(in, &g);
  const int rc = ghc_mlp_check(Dv, P, N, De, Hd, params, fold, eps);
  if (rc != GH_OK) return rc;
  if (g.Cc < 1 || !dcode || dcode_stride < g.Cc) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  const int VP = ghc_vp(Dv, Hd), HP = Hd | 1, CP = g.Cc | 1;
  const size_t lds = (size_t)(2 * GHC_BLOCK + GHC_ROWS * (VP + 2 * HP + CP)) * sizeof(float);
  (void)hipGetLastError();
  ghr_allow_lds<ghc_bwd_kernel>(lds);
  hipLaunchKernelGGL(ghc_bwd_kernel, dim3(ghc_blocks(P)), dim3(GHC_BLOCK), lds, (hipStream_t)hip_stream, g, P, N, De, Hd, fold,
                     params->fc2_weight, eps, g_out, dcode, (long long)dcode_stride, VP);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
