// gh_attn_rows.hip — the row work around the interaction attention's core (include/gh_attn_rows.h): the gather, the two LayerNorms,
// the six linear layers, the residuals and the scatter of SelfAttn.forward as one launch ahead of gh_attn_forward / behind
// gh_attn_backward and one on the other side, over all listed rows at once. Frozen weights: no parameter gradients.
//   tile      one 4-wave workgroup per 64 listed rows, lane = row, wave-uniform weights through the scalar cache (gh_rows.h:
//             ghr_tile, ghr_moments, ghr_linear, ghr_linear_t, ghr_sum4). A listed row is gathered into LDS at an odd pitch
//             (ghr_stage_rows) and leaves as a coalesced run of its own row of Out / dX; the contiguous operands (the core's
//             buffers, y, dy) cross with ghr_stage.
//   LDS       computed from the actual widths; a kernel whose tile of 64 rows would take more than GAR_LDS_MAX runs 32 rows per
//             workgroup, every row on two lanes (as gh_vert.hip's backward does).
//   forward   a layer's input is dead once the barrier behind the layer is passed, so the tile holds two row buffers: the F-wide
//             row (x, then y, then LayerNorm2(y), then the feed-forward's output) and one of max(HD, hid) (q / k / v in turn;
//             the core's output, then relu(fc1)). y goes to memory before it is normalised in place and is read back, by the thread
//             that wrote it, for the last residual.
//   backward  post: dz, xhat2 and one max(HD, hid) buffer (dh, then da); LayerNorm2's backward is folded into dz in place.
//             pre: xhat1, the sum of the three projections' gradients, and dq / dk / dv in turn.
#include "../../include/gh_attn_rows.h"
#include "../csrc_rows/gh_rows.h"

#define GAR_BLOCK GHR_BLOCK
#define GAR_ROWS GHR_ROWS
#define GAR_LDS_MAX (128 * 1024)  // the most LDS a workgroup takes (a CU has 160 KiB)

static_assert(GH_ATTN_D == 32, "HD = 32 H: the mask words and the 16-byte staging of the core's buffers count on it");

// f(r, c) for the columns c < n of the tile's nrows rows, consecutive threads on consecutive columns
template <class Fn>
__device__ __forceinline__ void gar_each(int nrows, int n, int tid, Fn f) {
  for (int i = tid; i < nrows * n; i += GAR_BLOCK) {
    const int r = i / n;
    f(r, i - r * n);
  }
}

__device__ __forceinline__ long long gar_row(const int* __restrict__ idx, long long i) { return idx ? (long long)idx[i] : i; }

// the saved (mean, rstd) of the lane's row; zeros for a row past the end
__device__ __forceinline__ float2 gar_stats(const float* __restrict__ stats, const GhrTile& t) {
  float2 s = make_float2(0.f, 0.f);
  if (t.lane < t.nrows) s = make_float2(stats[2 * (t.row0 + t.lane)], stats[2 * (t.row0 + t.lane) + 1]);
  return s;
}

// ---- ahead of the core, forward: LayerNorm1 and the three projections --------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(GAR_BLOCK) void gar_pre_fwd_kernel(const float* __restrict__ X, long long x_stride, const int* __restrict__ idx,
                                                                int V, int F, int HD, float eps, GhAttnRowsParams p,
                                                                float* __restrict__ qkv, float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float gar_smem[];
  const int FP = F | 1, OP = HD | 1;
  float* s_red = gar_smem;               // 2 x GAR_BLOCK
  float* s_x = s_red + 2 * GAR_BLOCK;    // R x FP: x, then LayerNorm1(x)
  float* s_o = s_x + R * FP;             // R x OP: q, k, v in turn
  const GhrTile t = ghr_tile<R>(V);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  ghr_stage_rows(s_x, FP, X, x_stride, idx, t.row0, R, t.nrows, F, tid);
  __syncthreads();
  float* xr = s_x + lane * FP;
  const GhrMoments mo = ghr_moments(xr, F, s_red, lane, wave);
  const float rstd = 1.0f / sqrtf(mo.m2 / (float)F + eps);
  for (int k = wave; k < F; k += 4) xr[k] = fmaf((xr[k] - mo.mean) * rstd, p.ln1_weight[k], p.ln1_bias[k]);
  if (tid < R && tid < t.nrows) {
    stats[2 * (t.row0 + tid)] = mo.mean;
    stats[2 * (t.row0 + tid) + 1] = rstd;
  }
  __syncthreads();
  for (int part = 0; part < 3; ++part) {
    const float* __restrict__ W = part == 0 ? p.wq_weight : part == 1 ? p.wk_weight : p.wv_weight;
    const float* __restrict__ b = part == 0 ? p.wq_bias : part == 1 ? p.wk_bias : p.wv_bias;
    ghr_linear(F, W, HD, wave, [&](int k) { return xr[k]; }, [&](int j, float s) { s_o[lane * OP + j] = s + b[j]; });
    __syncthreads();
    gar_each(t.nrows, HD, tid, [&](int r, int c) { qkv[(t.row0 + r) * (3LL * HD) + part * HD + c] = s_o[r * OP + c]; });
    __syncthreads();
  }
}

// ---- behind the core, forward: fc, the residual, LayerNorm2, fc1, ReLU, fc2, the residual, the scatter ------------------------------
template <int R>
__global__ __launch_bounds__(GAR_BLOCK) void gar_post_fwd_kernel(const float* __restrict__ X, long long x_stride, const int* __restrict__ idx,
                                                                 const float* __restrict__ a, int V, int F, int HD, int hid, float eps,
                                                                 GhAttnRowsParams p, float* __restrict__ Out, long long out_stride, float* y,
                                                                 float* __restrict__ stats, unsigned* __restrict__ mask, int vec_a) {
  extern __shared__ __attribute__((aligned(16))) float gar_smem[];
  const int FP = F | 1, BP = (HD > hid ? HD : hid) | 1, MW = (hid + 31) >> 5;
  float* s_red = gar_smem;               // 2 x GAR_BLOCK
  float* s_y = s_red + 2 * GAR_BLOCK;    // R x FP: x, y, LayerNorm2(y), fc2's output
  float* s_b = s_y + R * FP;             // R x BP: the core's output, then relu(fc1)
  const GhrTile t = ghr_tile<R>(V);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  ghr_stage_rows(s_y, FP, X, x_stride, idx, t.row0, R, t.nrows, F, tid);
  ghr_stage(s_b, BP, a, HD, t.row0, R, t.nrows, 0, HD, vec_a, tid);
  __syncthreads();
  float* yr = s_y + lane * FP;
  float* br = s_b + lane * BP;
  ghr_linear(HD, p.fc_weight, F, wave, [&](int k) { return br[k]; }, [&](int j, float s) { yr[j] = yr[j] + (s + p.fc_bias[j]); });
  __syncthreads();
  gar_each(t.nrows, F, tid, [&](int r, int c) { y[(t.row0 + r) * F + c] = s_y[r * FP + c]; });
  const GhrMoments mo = ghr_moments(yr, F, s_red, lane, wave);
  const float rstd = 1.0f / sqrtf(mo.m2 / (float)F + eps);
  for (int k = wave; k < F; k += 4) yr[k] = fmaf((yr[k] - mo.mean) * rstd, p.ln2_weight[k], p.ln2_bias[k]);
  if (tid < R && tid < t.nrows) {
    stats[2 * (t.row0 + tid)] = mo.mean;
    stats[2 * (t.row0 + tid) + 1] = rstd;
  }
  __syncthreads();
  ghr_linear(F, p.fc1_weight, hid, wave, [&](int k) { return yr[k]; }, [&](int j, float s) {
    const float v = s + p.fc1_bias[j];
    br[j] = v > 0.f ? v : (v == v ? 0.f : v);  // (a NaN stays a NaN, as torch's relu keeps it)
  });
  __syncthreads();
  for (int w = wave; w < MW; w += 4) {  // the ReLU's mask, bit j of word j / 32: h[j] > 0
    unsigned bits = 0u;
    const int n = hid - 32 * w < 32 ? hid - 32 * w : 32;
    for (int j = 0; j < n; ++j) bits |= (br[32 * w + j] > 0.f ? 1u : 0u) << j;
    if ((tid & 63) < R && lane < t.nrows) mask[(t.row0 + lane) * MW + w] = bits;
  }
  ghr_linear(hid, p.fc2_weight, F, wave, [&](int k) { return br[k]; }, [&](int j, float s) { yr[j] = s + p.fc2_bias[j]; });
  __syncthreads();
  // every thread reads back the elements of y that it stored itself above
  gar_each(t.nrows, F, tid, [&](int r, int c) { Out[gar_row(idx, t.row0 + r) * out_stride + c] = y[(t.row0 + r) * F + c] + s_y[r * FP + c]; });
}

// ---- ahead of the core, backward: the feed-forward block, LayerNorm2 and the residual backwards; da = Wfc^T dy --------------------------
template <int R>
__global__ __launch_bounds__(GAR_BLOCK) void gar_post_bwd_kernel(const float* __restrict__ dOut, long long dout_stride,
                                                                 const int* __restrict__ idx, const float* __restrict__ y,
                                                                 const float* __restrict__ stats, const unsigned* __restrict__ mask, int V,
                                                                 int F, int HD, int hid, GhAttnRowsParams p, float* __restrict__ da,
                                                                 float* __restrict__ dy, int vec_y) {
  extern __shared__ __attribute__((aligned(16))) float gar_smem[];
  const int FP = F | 1, BP = (HD > hid ? HD : hid) | 1, MW = (hid + 31) >> 5, MP = MW | 1;
  float* s_red = gar_smem;               // 2 x GAR_BLOCK
  float* s_g = s_red + 2 * GAR_BLOCK;    // R x FP: dz, then dy
  float* s_y = s_g + R * FP;             // R x FP: y, then xhat
  float* s_b = s_y + R * FP;             // R x BP: dh, then da
  unsigned* s_m = (unsigned*)(s_b + R * BP);  // R x MP
  const GhrTile t = ghr_tile<R>(V);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  ghr_stage_rows(s_g, FP, dOut, dout_stride, idx, t.row0, R, t.nrows, F, tid);
  ghr_stage(s_y, FP, y, F, t.row0, R, t.nrows, 0, F, vec_y, tid);
  for (int i = tid; i < R * MW; i += GAR_BLOCK) {
    const int r = i / MW, c = i - r * MW;
    s_m[r * MP + c] = r < t.nrows ? mask[(t.row0 + r) * MW + c] : 0u;
  }
  const float2 st = gar_stats(stats, t);
  const float mean = st.x, rstd = st.y;
  __syncthreads();
  float* gr = s_g + lane * FP;
  float* yr = s_y + lane * FP;
  float* br = s_b + lane * BP;
  const unsigned* mr = s_m + lane * MP;
  for (int k = wave; k < F; k += 4) yr[k] = (yr[k] - mean) * rstd;
  ghr_linear_t(gr, F, p.fc2_weight, hid, wave, [&](int i, float v) { br[i] = (mr[i >> 5] >> (i & 31)) & 1u ? v : 0.f; });
  __syncthreads();
  float p1 = 0.f, p2 = 0.f;  // this wave's share of sum_k g[k] and of sum_k g[k] * xhat[k], g = weight * dyn
  ghr_linear_t(br, hid, p.fc1_weight, F, wave, [&](int k, float v) {
    const float g = v * p.ln2_weight[k];
    p1 += g;
    p2 = fmaf(g, yr[k], p2);
    gr[k] = fmaf(g, rstd, gr[k]);
  });
  s_red[wave * GAR_ROWS + lane] = p1;
  s_red[GAR_BLOCK + wave * GAR_ROWS + lane] = p2;
  __syncthreads();
  const float m1 = ghr_sum4(s_red, lane) / (float)F, m2 = ghr_sum4(s_red + GAR_BLOCK, lane) / (float)F;
  for (int k0 = 4 * wave; k0 < F; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + s;
      if (k < F) gr[k] = fmaf(-rstd, fmaf(yr[k], m2, m1), gr[k]);
    }
  }
  __syncthreads();
  gar_each(t.nrows, F, tid, [&](int r, int c) { dy[(t.row0 + r) * F + c] = s_g[r * FP + c]; });
  ghr_linear_t(gr, F, p.fc_weight, HD, wave, [&](int c, float v) { br[c] = v; });
  __syncthreads();
  gar_each(t.nrows, HD, tid, [&](int r, int c) { da[(t.row0 + r) * HD + c] = s_b[r * BP + c]; });
}

// ---- behind the core, backward: the three projections and LayerNorm1 backwards, the residual, the scatter --------------------------------
template <int R>
__global__ __launch_bounds__(GAR_BLOCK) void gar_pre_bwd_kernel(const float* __restrict__ X, long long x_stride, const int* __restrict__ idx,
                                                                const float* __restrict__ stats, const float* __restrict__ dq,
                                                                const float* __restrict__ dk, const float* __restrict__ dv,
                                                                const float* __restrict__ dy, int V, int F, int HD, GhAttnRowsParams p,
                                                                float* __restrict__ dX, long long dx_stride, int vec_d) {
  extern __shared__ __attribute__((aligned(16))) float gar_smem[];
  const int FP = F | 1, OP = HD | 1;
  float* s_red = gar_smem;               // 2 x GAR_BLOCK
  float* s_x = s_red + 2 * GAR_BLOCK;    // R x FP: x, then xhat
  float* s_n = s_x + R * FP;             // R x FP: dxn, g, then LayerNorm1's backward
  float* s_d = s_n + R * FP;             // R x OP: dq, dk, dv in turn
  const GhrTile t = ghr_tile<R>(V);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  ghr_stage_rows(s_x, FP, X, x_stride, idx, t.row0, R, t.nrows, F, tid);
  ghr_stage(s_d, OP, dq, HD, t.row0, R, t.nrows, 0, HD, vec_d & 1, tid);
  const float2 st = gar_stats(stats, t);
  const float mean = st.x, rstd = st.y;
  __syncthreads();
  float* xr = s_x + lane * FP;
  float* nr = s_n + lane * FP;
  const float* dr = s_d + lane * OP;
  for (int k = wave; k < F; k += 4) xr[k] = (xr[k] - mean) * rstd;
  ghr_linear_t(dr, HD, p.wq_weight, F, wave, [&](int k, float v) { nr[k] = v; });
  __syncthreads();
  ghr_stage(s_d, OP, dk, HD, t.row0, R, t.nrows, 0, HD, vec_d & 2, tid);
  __syncthreads();
  ghr_linear_t(dr, HD, p.wk_weight, F, wave, [&](int k, float v) { nr[k] = nr[k] + v; });
  __syncthreads();
  ghr_stage(s_d, OP, dv, HD, t.row0, R, t.nrows, 0, HD, vec_d & 4, tid);
  __syncthreads();
  float p1 = 0.f, p2 = 0.f;  // this wave's share of sum_k g[k] and of sum_k g[k] * xhat[k], g = weight * dxn
  ghr_linear_t(dr, HD, p.wv_weight, F, wave, [&](int k, float v) {
    const float g = (nr[k] + v) * p.ln1_weight[k];
    p1 += g;
    p2 = fmaf(g, xr[k], p2);
    nr[k] = g;
  });
  s_red[wave * GAR_ROWS + lane] = p1;
  s_red[GAR_BLOCK + wave * GAR_ROWS + lane] = p2;
  __syncthreads();
  const float m1 = ghr_sum4(s_red, lane) / (float)F, m2 = ghr_sum4(s_red + GAR_BLOCK, lane) / (float)F;
  for (int k0 = 4 * wave; k0 < F; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + s;
      if (k < F) nr[k] = fmaf(-xr[k], m2, nr[k] - m1) * rstd;
    }
  }
  __syncthreads();
  gar_each(t.nrows, F, tid, [&](int r, int c) { dX[gar_row(idx, t.row0 + r) * dx_stride + c] = dy[(t.row0 + r) * F + c] + s_n[r * FP + c]; });
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
enum { GAR_PRE_FWD, GAR_POST_FWD, GAR_POST_BWD, GAR_PRE_BWD };

// bytes of LDS a tile of `rows` rows takes in kernel `which`, from the actual widths
static inline size_t gar_lds(int which, int rows, int F, int HD, int hid) {
  const int FP = F | 1, OP = HD | 1, BP = (HD > hid ? HD : hid) | 1, MP = ((hid + 31) >> 5) | 1;
  const int per_row = which == GAR_PRE_FWD ? FP + OP : which == GAR_POST_FWD ? FP + BP : which == GAR_POST_BWD ? 2 * FP + BP + MP : 2 * FP + OP;
  return (size_t)(2 * GAR_BLOCK + rows * per_row) * sizeof(float);
}
static inline int gar_rows(int which, int F, int HD, int hid) { return gar_lds(which, GAR_ROWS, F, HD, hid) <= GAR_LDS_MAX ? GAR_ROWS : GAR_ROWS / 2; }

static int gar_check(const GhAttnRowsDims* d, const GhAttnRowsParams* p) {
  if (!d || !p) return GH_ERR_INVALID_ARG;
  if (d->V < 0) return GH_ERR_INVALID_ARG;
  if (d->H < 1 || d->H > GH_ATTN_ROWS_MAX_H || d->F < 1 || d->F > GH_ATTN_ROWS_MAX_F || d->hid < 1 || d->hid > GH_ATTN_ROWS_MAX_F ||
      d->V > GH_ATTN_MAX_V)
    return GH_ERR_UNSUPPORTED;
  if (!(d->eps1 >= 0.f) || !(d->eps2 >= 0.f)) return GH_ERR_INVALID_ARG;
  const float* const* q = &p->wq_weight;
  for (int i = 0; i < 16; ++i)
    if (!q[i]) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

static inline bool gar_ws_ok(const GhAttnRowsDims* d, const void* ws, size_t ws_bytes, int* rc) {
  if (!ws || !ghr_al16(ws)) { *rc = GH_ERR_INVALID_ARG; return false; }
  if (ws_bytes < gh_attn_rows_workspace_bytes(d)) { *rc = GH_ERR_WORKSPACE_SMALL; return false; }
  return true;
}

extern "C" size_t gh_attn_rows_workspace_bytes(const GhAttnRowsDims* d) {
  if (!d || d->V < 1 || d->V > GH_ATTN_MAX_V || d->F < 1 || d->F > GH_ATTN_ROWS_MAX_F || d->H < 1 || d->H > GH_ATTN_ROWS_MAX_H ||
      d->hid < 1 || d->hid > GH_ATTN_ROWS_MAX_F)
    return 0;
  return ghr_align((size_t)d->V * (size_t)d->F * sizeof(float));
}

// launch kernel K<64> or K<32>, whichever `rows` names, with its LDS
#define GAR_LAUNCH(K, which, ...)                                                                                                   \
  do {                                                                                                                              \
    const int rows_ = gar_rows(which, F, HD, hid);                                                                                  \
    const size_t lds_ = gar_lds(which, rows_, F, HD, hid);                                                                          \
    const dim3 grid_((unsigned)((d->V + rows_ - 1) / rows_)), block_(GAR_BLOCK);                                                    \
    (void)hipGetLastError();                                                                                                        \
    if (rows_ == GAR_ROWS) {                                                                                                        \
      ghr_allow_lds<K<GAR_ROWS>>(lds_);                                                                                             \
      hipLaunchKernelGGL((K<GAR_ROWS>), grid_, block_, lds_, (hipStream_t)hip_stream, __VA_ARGS__);                                 \
    } else {                                                                                                                        \
      ghr_allow_lds<K<GAR_ROWS / 2>>(lds_);                                                                                         \
      hipLaunchKernelGGL((K<GAR_ROWS / 2>), grid_, block_, lds_, (hipStream_t)hip_stream, __VA_ARGS__);                             \
    }                                                                                                                               \
    return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;                                                                 \
  } while (0)

extern "C" int gh_attn_rows_pre_forward(const GhAttnRowsDims* d, const GhAttnRowsParams* p, const float* X, const int32_t* idx, float* qkv,
                                        float* stats1, void* hip_stream) {
  const int rc = gar_check(d, p);
  if (rc != GH_OK) return rc;
  if (!X || !qkv || !stats1 || d->x_stride < d->F) return GH_ERR_INVALID_ARG;
  if (d->V == 0) return GH_OK;
  const int F = d->F, HD = d->H * GH_ATTN_D, hid = d->hid;
  GAR_LAUNCH(gar_pre_fwd_kernel, GAR_PRE_FWD, X, (long long)d->x_stride, (const int*)idx, (int)d->V, F, HD, d->eps1, *p, qkv, stats1);
}

extern "C" int gh_attn_rows_post_forward(const GhAttnRowsDims* d, const GhAttnRowsParams* p, const float* X, const int32_t* idx,
                                         const float* a, float* Out, float* y, float* stats2, uint32_t* relu_mask, void* hip_stream) {
  const int rc = gar_check(d, p);
  if (rc != GH_OK) return rc;
  if (!X || !a || !Out || !y || !stats2 || !relu_mask || d->x_stride < d->F || d->out_stride < d->F) return GH_ERR_INVALID_ARG;
  if (d->V == 0) return GH_OK;
  const int F = d->F, HD = d->H * GH_ATTN_D, hid = d->hid;
  const int vec_a = ghr_al16(a);
  GAR_LAUNCH(gar_post_fwd_kernel, GAR_POST_FWD, X, (long long)d->x_stride, (const int*)idx, a, (int)d->V, F, HD, hid, d->eps2, *p, Out,
             (long long)d->out_stride, y, stats2, (unsigned*)relu_mask, vec_a);
}

extern "C" int gh_attn_rows_post_backward(const GhAttnRowsDims* d, const GhAttnRowsParams* p, const float* dOut, const int32_t* idx,
                                          const float* y, const float* stats2, const uint32_t* relu_mask, float* da, void* workspace,
                                          size_t ws_bytes, void* hip_stream) {
  int rc = gar_check(d, p);
  if (rc != GH_OK) return rc;
  if (!dOut || !y || !stats2 || !relu_mask || !da || d->dout_stride < d->F) return GH_ERR_INVALID_ARG;
  if (d->V == 0) return GH_OK;
  if (!gar_ws_ok(d, workspace, ws_bytes, &rc)) return rc;
  const int F = d->F, HD = d->H * GH_ATTN_D, hid = d->hid;
  const int vec_y = ghr_al16(y) && F % 4 == 0;
  GAR_LAUNCH(gar_post_bwd_kernel, GAR_POST_BWD, dOut, (long long)d->dout_stride, (const int*)idx, y, stats2, (const unsigned*)relu_mask,
             (int)d->V, F, HD, hid, *p, da, (float*)workspace, vec_y);
}

extern "C" int gh_attn_rows_pre_backward(const GhAttnRowsDims* d, const GhAttnRowsParams* p, const float* X, const int32_t* idx,
                                         const float* stats1, const float* dq, const float* dk, const float* dv, const void* workspace,
                                         size_t ws_bytes, float* dX, void* hip_stream) {
  int rc = gar_check(d, p);
  if (rc != GH_OK) return rc;
  if (!X || !stats1 || !dq || !dk || !dv || !dX || d->x_stride < d->F || d->dx_stride < d->F) return GH_ERR_INVALID_ARG;
  if (d->V == 0) return GH_OK;
  if (!gar_ws_ok(d, workspace, ws_bytes, &rc)) return rc;
  const int F = d->F, HD = d->H * GH_ATTN_D, hid = d->hid;
  const int vec_d = (ghr_al16(dq) ? 1 : 0) | (ghr_al16(dk) ? 2 : 0) | (ghr_al16(dv) ? 4 : 0);
  GAR_LAUNCH(gar_pre_bwd_kernel, GAR_PRE_BWD, X, (long long)d->x_stride, (const int*)idx, stats1, dq, dk, dv, (const float*)workspace,
             (int)d->V, F, HD, p[0], dX, (long long)d->dx_stride, vec_d);
}
