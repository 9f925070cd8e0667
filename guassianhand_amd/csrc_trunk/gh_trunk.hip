// gh_trunk.hip — the fused Gaussian trunk (include/gh_trunk.h): forward_gs's trunk MLP and Gaussian head in one pass each way.
//
// gh_res.hip's product shape, v_mfma_f32_32x32x2_f32 with the point as the column: a wave owns 32 rows of x, lane l the point l & 31;
// lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], and its result register r holds row
// gt_row(r, l >> 5) = (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31. The weights are the A operand and cross LDS in slabs the four
// waves share (ghr_fetch_in / ghr_put, two barriers a slab): 32 columns of all rows of W in the forward products (read along the row,
// pitch 33), 32 rows of up to 128 columns in the backward's products with W^T (read along the column). A layer's result stays in the
// accumulators and is the B operand of the next product register by register; the activation is applied to it on the way.
//   forward   v1 (x from global memory, Cin padded with zero columns to the k step), v2, y, then the head's O rows as one more product
//             over y; its pre-activations cross LDS ([row][o], pitch 59) to the per-row activations, which are gh_head.hip's and leave
//             as each output's contiguous run of the tile.
//   backward  graw from `raw` and the cotangents into LDS ([row][o]); dy = Wh^T graw and W3^T dy first, then v1 and v2 are recomputed
//             (so that at most three sets of four accumulators are alive, and of those the half of one that only waits is parked
//             in graw's tile, which is free by then), dv2, dv1, and grad_x in chunks of 128 columns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_trunk.h"
#include "../csrc_rows/gh_rows.h"

#define GT_BLOCK GHR_BLOCK
#define GT_ROWS GH_TRUNK_ROWS
#define GT_PITCH 33        // the forward products' slab: a lane reads along its own row
#define GT_RP 59           // pitch of the [row][o] tile of raw / graw: odd, lane = row is conflict-free
#define GT_SLAB (128 * GT_PITCH)  // floats of the weight slab: 128 rows x 32 columns at pitch 33, or 32 rows x 128 columns
#define GT_GP 65           // the backward's pitch of that tile: its 128 x 65 floats also park two accumulator tiles per thread
#define GT_EPS 1e-12f      // F.normalize's floor

static_assert(GT_ROWS == (GT_BLOCK / 64) * 32, "four waves of 32 rows");
static_assert(GT_RP >= GH_HEAD_MAX_O && (GT_RP & 1), "a row of raw fits the pitch");
static_assert(GH_TRUNK_MAX_CIN % 32 == 0, "whole slabs");
static_assert(GT_GP >= GH_HEAD_MAX_O && (GT_GP & 1) && GT_ROWS * GT_GP >= 2 * 16 * GT_BLOCK, "graw's tile holds the parked accumulators");

typedef float gt_acc __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int gt_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
__device__ __forceinline__ float gt_act(float v, bool relu) { return relu ? (v < 0.f ? 0.f : v) : v / (1.0f + expf(-v)); }
// d * act'(v)
__device__ __forceinline__ float gt_dact(float v, float d, bool relu) {
  if (relu) return v > 0.f ? d : 0.f;
  const float s = ghr_sigmoid(v);
  return d * (s * (1.0f + v * (1.0f - s)));
}

template <int NT>
__device__ __forceinline__ void gt_fill(gt_acc (&h)[NT], const float* __restrict__ b, int half) {  // b: the bias, or null for zeros
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) h[t][k] = b ? b[32 * t + gt_row(k, half)] : 0.f;
  }
}

// h[t] += W[32 t .., 0 .. Cin) . x[p]: W (32 NH, Cin) contiguous, k ascending; the last slab's missing columns are zeros on both sides
template <int NH>
__device__ __forceinline__ void gt_layer_x(gt_acc (&h)[NH], float* s_w, const float* __restrict__ W, int Cin, int vec, const float* __restrict__ xp,
                                           bool live, int tid, int col, int half) {
  for (int k0 = 0; k0 < Cin; k0 += 32) {
    const int kc = Cin - k0 < 32 ? Cin - k0 : 32;
    GhrSlab<NH, 8> w;                                          // 32 NH rows x 32 columns
    ghr_fetch_in(w, W, Cin, 0, k0, 32 * NH, Cin, vec, tid);
    float xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) xv[s] = (live && 2 * s + half < kc) ? xp[k0 + 2 * s + half] : 0.f;
    __syncthreads();                                           // the previous slab has been read by every wave
    ghr_put(w, s_w, GT_PITCH, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (2 * s < kc) {
#pragma unroll
        for (int t = 0; t < NH; ++t)
          h[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(32 * t + col) * GT_PITCH + 2 * s + half], xv[s], h[t], 0, 0, 0);
      }
    }
  }
}

// d[t] += W[32 t .., :] . f(src) for t < nt: W (nrows, 32 NS) contiguous, src's channels in register order; f is the activation, or the
// identity where `plain`. Rows of W past nrows are zeros.
template <int NS, int ND>
__device__ __forceinline__ void gt_layer(gt_acc (&d)[ND], int nt, const gt_acc (&src)[NS], bool plain, bool relu, float* s_w,
                                         const float* __restrict__ W, int nrows, int vec, int tid, int col, int half) {
#pragma unroll
  for (int jt = 0; jt < NS; ++jt) {
    GhrSlab<ND, 8> w;                                          // 32 ND rows x 32 columns
    ghr_fetch_in(w, W, 32 * NS, 0, 32 * jt, nrows, 32 * NS, vec, tid);
    __syncthreads();
    ghr_put(w, s_w, GT_PITCH, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float hv = plain ? src[jt][k] : gt_act(src[jt][k], relu);
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(32 * t + col) * GT_PITCH + gt_row(k, half)], hv, d[t], 0, 0, 0);
      }
    }
  }
}

// d[t] += (W[:, c0 + 32 t ..])^T . src for t < nt: W (32 NS, ncols) with row stride `stride`, its rows in register order; the window is
// 32 ND columns from c0, columns past ncols are zeros
template <int NS, int ND>
__device__ __forceinline__ void gt_layer_t(gt_acc (&d)[ND], int nt, const gt_acc (&src)[NS], float* s_w, const float* __restrict__ W,
                                           int stride, int c0, int ncols, int vec, int tid, int col, int half) {
  constexpr int CW = 32 * ND;
#pragma unroll
  for (int jt = 0; jt < NS; ++jt) {
    GhrSlab<ND, CW / 4> w;                                     // 32 rows x 32 ND columns
    ghr_fetch_in(w, W, stride, 32 * jt, c0, 32 * NS, ncols, vec, tid);
    __syncthreads();
    ghr_put(w, s_w, CW, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[gt_row(k, half) * CW + 32 * t + col], src[jt][k], d[t], 0, 0, 0);
      }
    }
  }
}

struct GtOut {  // the contiguous arrays of one direction, and which of them may be accessed 16 bytes at a time
  float *xyz, *scaling, *rotation, *opacity, *shs, *raw;
  unsigned vec;
};
enum { GT_V_XYZ = 1, GT_V_SCALING = 2, GT_V_ROTATION = 4, GT_V_OPACITY = 8, GT_V_SHS = 16, GT_V_RAW = 32 };

struct GtArgs {
  const float *x, *pts, *raw, *W1, *b1, *W2, *b2, *W3, *b3, *Wh, *bh;
  float *grad_x, *grad_pts;
  GtOut o;  // forward: the outputs; backward: the cotangents
  long long x_stride, gx_stride;
  int P, Cin, O, width, relu, vec_w1, vec_w, vec_gx;
  unsigned flags;
  float clip;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int NH, int NC>
__global__ __launch_bounds__(GT_BLOCK, 2) void gt_forward_kernel(GtArgs a) {
  __shared__ float s_w[GT_SLAB];
  __shared__ float s_raw[GT_ROWS * GT_RP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const long long row0 = (long long)blockIdx.x * GT_ROWS;
  const int nrows = (int)((long long)a.P - row0 < GT_ROWS ? (long long)a.P - row0 : GT_ROWS);
  const int trow = wave * 32 + col;
  const bool live = trow < nrows, relu = a.relu;
  const int O = a.O, no = (O + 31) >> 5;

  gt_acc r[2];
  {
    gt_acc y[NC];
    {
      gt_acc v2[NH];
      {
        gt_acc v1[NH];
        gt_fill<NH>(v1, a.b1, half);
        gt_layer_x<NH>(v1, s_w, a.W1, a.Cin, a.vec_w1, a.x + (live ? row0 + trow : 0) * a.x_stride, live, tid, col, half);
        gt_fill<NH>(v2, a.b2, half);
        gt_layer<NH, NH>(v2, NH, v1, false, relu, s_w, a.W2, 32 * NH, a.vec_w, tid, col, half);
      }
      gt_fill<NC>(y, a.b3, half);
      gt_layer<NH, NC>(y, NC, v2, false, relu, s_w, a.W3, 32 * NC, a.vec_w, tid, col, half);
    }
    gt_fill<2>(r, nullptr, half);                              // the head's bias is added last, as gh_head.hip adds it
    gt_layer<NC, 2>(r, no, y, true, relu, s_w, a.Wh, O, a.vec_w, tid, col, half);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int o = 32 * t + gt_row(k, half);
      if (o < O) s_raw[trow * GT_RP + o] = r[t][k] + a.bh[o];
    }
  }
  __syncthreads();

  // ---- activations (gh_head.hip's): every output's tile is one contiguous run ----
  const GtOut& out = a.o;
  const int width = a.width;
  const unsigned flags = a.flags;
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32), clip = a.clip;
  const float* pt = a.pts + row0 * 3;
  ghr_store_run(out.xyz + row0 * 3, nrows * 3, out.vec & GT_V_XYZ, tid, [&](int e) {
    const float p = pt[e];
    if (!xyz_off) return p;
    const int rr = e / 3;
    float v = s_raw[rr * GT_RP + (e - 3 * rr)];
    if (restrict_off) v = (ghr_sigmoid(v) - 0.5f) * max_step;
    return v + p;
  });
  ghr_store_run(out.scaling + row0 * 3, nrows * 3, out.vec & GT_V_SCALING, tid, [&](int e) {
    const int rr = e / 3;
    float s = expf(s_raw[rr * GT_RP + 3 + (e - 3 * rr)]);
    if (clipped) s = fminf(fmaxf(s, 0.f), clip);
    return s;
  });
  if (tid < nrows) {
    const float* v = s_raw + tid * GT_RP + 6;
    const float qa = v[0], qb = v[1], qc = v[2], qd = v[3];
    const float den = fmaxf(sqrtf(((qa * qa + qb * qb) + qc * qc) + qd * qd), GT_EPS);
    float* dst = out.rotation + (row0 + tid) * 4;
    if (out.vec & GT_V_ROTATION) {
      *(float4*)dst = make_float4(qa / den, qb / den, qc / den, qd / den);
    } else {
      dst[0] = qa / den; dst[1] = qb / den; dst[2] = qc / den; dst[3] = qd / den;
    }
  }
  ghr_store_run(out.opacity + row0, nrows, out.vec & GT_V_OPACITY, tid, [&](int e) { return ghr_sigmoid(s_raw[e * GT_RP + 10]); });
  ghr_store_run(out.shs + row0 * width, nrows * width, out.vec & GT_V_SHS, tid, [&](int e) {
    const int rr = e / width;
    const float v = s_raw[rr * GT_RP + 11 + (e - rr * width)];
    return use_rgb ? ghr_sigmoid(v) : v;
  });
  if (out.raw) {
    ghr_store_run(out.raw + row0 * O, nrows * O, out.vec & GT_V_RAW, tid, [&](int e) {
      const int rr = e / O;
      return s_raw[rr * GT_RP + (e - rr * O)];
    });
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <int NH, int NC>
__global__ __launch_bounds__(GT_BLOCK, 2) void gt_backward_kernel(GtArgs a) {
  __shared__ float s_w[GT_SLAB];
  __shared__ float s_g[GT_ROWS * GT_GP];  // the gradient of raw[row, o] at s_g[row * GT_GP + o]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const long long row0 = (long long)blockIdx.x * GT_ROWS;
  const int nrows = (int)((long long)a.P - row0 < GT_ROWS ? (long long)a.P - row0 : GT_ROWS);
  const int trow = wave * 32 + col;
  const bool live = trow < nrows, relu = a.relu;
  const int O = a.O, width = a.width;
  const unsigned flags = a.flags;
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32), clip = a.clip;
  const GtOut& g = a.o;
  const float* rt = a.raw + row0 * O;

  // ---- the gradient of the pre-activations (gh_head.hip's formulas); rows past the end are zeros ----
  for (int e = tid; e < GT_ROWS * 3; e += GT_BLOCK) {
    const int r = e / 3, c = e - 3 * r;
    float gx = 0.f, gs = 0.f;
    if (r < nrows) {
      const float go = g.xyz ? g.xyz[row0 * 3 + e] : 0.f;
      if (a.grad_pts) a.grad_pts[row0 * 3 + e] = go;
      if (xyz_off) {
        gx = go;
        if (restrict_off) {
          const float s = ghr_sigmoid(rt[r * O + c]);
          gx = ((go * max_step) * (1.0f - s)) * s;
        }
      }
      if (g.scaling) {
        const float v = rt[r * O + 3 + c], s = expf(v);
        const bool pass = !clipped || (s >= 0.f && s <= clip);
        gs = pass ? g.scaling[row0 * 3 + e] * expf(fminf(v, 15.0f)) : 0.f;
      }
    }
    s_g[r * GT_GP + c] = gx;
    s_g[r * GT_GP + 3 + c] = gs;
  }
  if (tid < GT_ROWS) {
    const int r = tid;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, gop = 0.f;
    if (r < nrows) {
      if (g.rotation) {
        const float* v = rt + r * O + 6;
        const float* gr = g.rotation + (row0 + r) * 4;
        const float qa = v[0], qb = v[1], qc = v[2], qd = v[3];
        const float g0 = gr[0], g1 = gr[1], g2 = gr[2], g3 = gr[3];
        const float n = sqrtf(((qa * qa + qb * qb) + qc * qc) + qd * qd);
        if (n >= GT_EPS) {
          const float n0 = qa / n, n1 = qb / n, n2 = qc / n, n3 = qd / n;
          const float dot = ((n0 * g0 + n1 * g1) + n2 * g2) + n3 * g3;
          o0 = (g0 - n0 * dot) / n; o1 = (g1 - n1 * dot) / n; o2 = (g2 - n2 * dot) / n; o3 = (g3 - n3 * dot) / n;
        } else {  // below the floor the denominator is the constant
          o0 = g0 / GT_EPS; o1 = g1 / GT_EPS; o2 = g2 / GT_EPS; o3 = g3 / GT_EPS;
        }
      }
      if (g.opacity) {
        const float s = ghr_sigmoid(rt[r * O + 10]);
        gop = (g.opacity[row0 + r] * (1.0f - s)) * s;
      }
    }
    float* d = s_g + r * GT_GP;
    d[6] = o0; d[7] = o1; d[8] = o2; d[9] = o3; d[10] = gop;
  }
  for (int e = tid; e < GT_ROWS * width; e += GT_BLOCK) {
    const int r = e / width, c = e - r * width;
    float gv = 0.f;
    if (r < nrows && g.shs) {
      gv = g.shs[row0 * width + e];
      if (use_rgb) {
        const float s = ghr_sigmoid(rt[r * O + 11 + c]);
        gv = (gv * (1.0f - s)) * s;
      }
    }
    s_g[r * GT_GP + 11 + c] = gv;
  }
  __syncthreads();

  gt_acc d2[NH];
  gt_fill<NH>(d2, nullptr, half);
  {
    // ---- dy = Wh^T . graw, o ascending; then W3^T . dy ----
    gt_acc dy[NC];
    gt_fill<NC>(dy, nullptr, half);
    for (int c0 = 0; c0 < O; c0 += 32) {
      GhrSlab<NC, 8 * NC> w;                                   // 32 rows x Cout columns
      ghr_fetch_in(w, a.Wh, 32 * NC, c0, 0, O, 32 * NC, a.vec_w, tid);
      float gv[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) gv[s] = c0 + 2 * s + half < O ? s_g[trow * GT_GP + c0 + 2 * s + half] : 0.f;
      __syncthreads();
      ghr_put(w, s_w, 32 * NC, tid);
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        if (c0 + 2 * s < O) {
#pragma unroll
          for (int t = 0; t < NC; ++t)
            dy[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(2 * s + half) * (32 * NC) + 32 * t + col], gv[s], dy[t], 0, 0, 0);
        }
      }
    }
    gt_layer_t<NC, NH>(d2, NH, dy, s_w, a.W3, 32 * NH, 0, 32 * NH, a.vec_w, tid, col, half);
  }
  // Three sets of accumulators would be alive from here on (this one, v1 and v2; later dv2, v1 and W2^T . dv2): the upper NPARK tiles
  // of the set that only waits are parked in graw's tile, which every wave has finished reading (the barriers of the product above).
  constexpr int NPARK = NH / 2, NKEEP = NH - NPARK;
  float* s_park = s_g + tid;
#pragma unroll
  for (int t = NKEEP; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) s_park[((t - NKEEP) * 16 + k) * GT_BLOCK] = d2[t][k];
  }

  // ---- v1, v2 again, as the forward computed them ----
  gt_acc v1[NH];
  gt_fill<NH>(v1, a.b1, half);
  gt_layer_x<NH>(v1, s_w, a.W1, a.Cin, a.vec_w1, a.x + (live ? row0 + trow : 0) * a.x_stride, live, tid, col, half);
  {
    gt_acc v2[NH];
    gt_fill<NH>(v2, a.b2, half);
    gt_layer<NH, NH>(v2, NH, v1, false, relu, s_w, a.W2, 32 * NH, a.vec_w, tid, col, half);
#pragma unroll
    for (int t = 0; t < NH; ++t) {
#pragma unroll
      for (int k = 0; k < 16; ++k) d2[t][k] = gt_dact(v2[t][k], t < NKEEP ? d2[t][k] : s_park[((t - NKEEP) * 16 + k) * GT_BLOCK], relu);
    }
  }
#pragma unroll
  for (int t = NKEEP; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) s_park[((t - NKEEP) * 16 + k) * GT_BLOCK] = v1[t][k];
  }
  gt_acc d1[NH];
  gt_fill<NH>(d1, nullptr, half);
  gt_layer_t<NH, NH>(d1, NH, d2, s_w, a.W2, 32 * NH, 0, 32 * NH, a.vec_w, tid, col, half);
#pragma unroll
  for (int t = 0; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) d1[t][k] = gt_dact(t < NKEEP ? v1[t][k] : s_park[((t - NKEEP) * 16 + k) * GT_BLOCK], d1[t][k], relu);
  }

  // ---- grad_x = W1^T . dv1, 128 columns a time ----
  float* gxr = a.grad_x + (live ? row0 + trow : 0) * a.gx_stride;
  for (int k0 = 0; k0 < a.Cin; k0 += 128) {
    const int cw = a.Cin - k0 < 128 ? a.Cin - k0 : 128, nt = (cw + 31) >> 5;
    gt_acc d[4];
    gt_fill<4>(d, nullptr, half);
    gt_layer_t<NH, 4>(d, nt, d1, s_w, a.W1, a.Cin, k0, a.Cin, a.vec_w1, tid, col, half);
    if (live) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 32 * t + 8 * q + 4 * half;
          float* dst = gxr + k0 + c;
          if (a.vec_gx && c + 4 <= cw) {
            *(float4*)dst = make_float4(d[t][4 * q], d[t][4 * q + 1], d[t][4 * q + 2], d[t][4 * q + 3]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (c + j < cw) dst[j] = d[t][4 * q + j];
            }
          }
        }
      }
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
static inline bool gt_al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
static bool gt_tiles_ok(int n) { return n == 32 || n == 64 || n == 96 || n == 128; }
static bool gt_width_ok(int w) { return w == 3 || w == 12 || w == 27 || w == 48; }

static int gt_check(const GhHeadDesc* d, int P, int Cin, int H, int Cout, int activation) {
  if (!d) return GH_ERR_INVALID_ARG;
  if (!gt_width_ok(d->shs_width)) return GH_ERR_UNSUPPORTED;
  if (d->flags & ~(GH_HEAD_USE_RGB | GH_HEAD_XYZ_OFFSET | GH_HEAD_RESTRICT_OFFSET | GH_HEAD_CLIP_SCALING)) return GH_ERR_INVALID_ARG;
  if ((d->flags & GH_HEAD_USE_RGB) && d->shs_width != 3) return GH_ERR_UNSUPPORTED;
  if ((d->flags & GH_HEAD_CLIP_SCALING) && !(d->clip_scaling >= 0.f)) return GH_ERR_INVALID_ARG;
  if (P < 0 || Cin < 1 || H < 1 || Cout < 1) return GH_ERR_INVALID_ARG;
  if (activation != GH_TRUNK_SILU && activation != GH_TRUNK_RELU) return GH_ERR_INVALID_ARG;
  if (Cin > GH_TRUNK_MAX_CIN || !gt_tiles_ok(H) || !gt_tiles_ok(Cout)) return GH_ERR_UNSUPPORTED;
  return GH_OK;
}

// one instantiation per (H / 32, Cout / 32)
#define GT_DISPATCH(KERNEL)                                                                                   \
  switch (4 * (H / 32 - 1) + (Cout / 32 - 1)) {                                                               \
    case 0: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 1: hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 2: hipLaunchKernelGGL((KERNEL<1, 3>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 3: hipLaunchKernelGGL((KERNEL<1, 4>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 4: hipLaunchKernelGGL((KERNEL<2, 1>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 5: hipLaunchKernelGGL((KERNEL<2, 2>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 6: hipLaunchKernelGGL((KERNEL<2, 3>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 7: hipLaunchKernelGGL((KERNEL<2, 4>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 8: hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 9: hipLaunchKernelGGL((KERNEL<3, 2>), grid, dim3(GT_BLOCK), 0, st, a); break;                        \
    case 10: hipLaunchKernelGGL((KERNEL<3, 3>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
    case 11: hipLaunchKernelGGL((KERNEL<3, 4>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
    case 12: hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
    case 13: hipLaunchKernelGGL((KERNEL<4, 2>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
    case 14: hipLaunchKernelGGL((KERNEL<4, 3>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
    default: hipLaunchKernelGGL((KERNEL<4, 4>), grid, dim3(GT_BLOCK), 0, st, a); break;                       \
  }

extern "C" int gh_trunk_forward(const float* x, int64_t x_stride, int P, int Cin, int H, int Cout, const float* pts, const float* W1,
                                const float* b1, const float* W2, const float* b2, const float* W3, const float* b3, const float* Wh,
                                const float* bh, const GhHeadDesc* desc, int activation, float* xyz, float* scaling, float* rotation,
                                float* opacity, float* shs, float* raw, void* hip_stream) {
  const int rc = gt_check(desc, P, Cin, H, Cout, activation);
  if (rc != GH_OK) return rc;
  if (!x || !pts || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !Wh || !bh || !xyz || !scaling || !rotation || !opacity || !shs)
    return GH_ERR_INVALID_ARG;
  if (!gt_al4(x) || !gt_al4(pts) || !gt_al4(W1) || !gt_al4(b1) || !gt_al4(W2) || !gt_al4(b2) || !gt_al4(W3) || !gt_al4(b3) || !gt_al4(Wh) ||
      !gt_al4(bh) || !gt_al4(xyz) || !gt_al4(scaling) || !gt_al4(rotation) || !gt_al4(opacity) || !gt_al4(shs) || !gt_al4(raw))
    return GH_ERR_INVALID_ARG;
  if (x_stride < Cin) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  GtArgs a = {};
  a.x = x; a.pts = pts; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3; a.Wh = Wh; a.bh = bh;
  a.o = {xyz, scaling, rotation, opacity, shs, raw, 0u};
  a.o.vec = (ghr_al16(xyz) ? GT_V_XYZ : 0u) | (ghr_al16(scaling) ? GT_V_SCALING : 0u) | (ghr_al16(rotation) ? GT_V_ROTATION : 0u) |
            (ghr_al16(opacity) ? GT_V_OPACITY : 0u) | (ghr_al16(shs) ? GT_V_SHS : 0u) | (raw && ghr_al16(raw) ? GT_V_RAW : 0u);
  a.x_stride = x_stride;
  a.P = P; a.Cin = Cin; a.width = desc->shs_width; a.O = 11 + desc->shs_width; a.relu = activation == GH_TRUNK_RELU;
  a.vec_w1 = ghr_al16(W1) && Cin % 4 == 0;
  a.vec_w = ghr_al16(W2) && ghr_al16(W3) && ghr_al16(Wh);
  a.flags = desc->flags; a.clip = desc->clip_scaling;
  const dim3 grid((unsigned)(((long long)P + GT_ROWS - 1) / GT_ROWS));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  GT_DISPATCH(gt_forward_kernel)
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_trunk_backward(const float* raw, const float* x, int64_t x_stride, int P, int Cin, int H, int Cout, const float* W1,
                                 const float* b1, const float* W2, const float* b2, const float* W3, const float* Wh,
                                 const GhHeadDesc* desc, int activation, const float* g_xyz, const float* g_scaling,
                                 const float* g_rotation, const float* g_opacity, const float* g_shs, float* grad_x, int64_t gx_stride,
                                 float* grad_pts, void* hip_stream) {
  const int rc = gt_check(desc, P, Cin, H, Cout, activation);
  if (rc != GH_OK) return rc;
  if (!raw || !x || !W1 || !b1 || !W2 || !b2 || !W3 || !Wh || !grad_x) return GH_ERR_INVALID_ARG;
  if (!gt_al4(raw) || !gt_al4(x) || !gt_al4(W1) || !gt_al4(b1) || !gt_al4(W2) || !gt_al4(b2) || !gt_al4(W3) || !gt_al4(Wh) || !gt_al4(g_xyz) ||
      !gt_al4(g_scaling) || !gt_al4(g_rotation) || !gt_al4(g_opacity) || !gt_al4(g_shs) || !gt_al4(grad_x) || !gt_al4(grad_pts))
    return GH_ERR_INVALID_ARG;
  if (x_stride < Cin || gx_stride < Cin) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  GtArgs a = {};
  a.raw = raw; a.x = x; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.Wh = Wh;
  a.o = {(float*)g_xyz, (float*)g_scaling, (float*)g_rotation, (float*)g_opacity, (float*)g_shs, nullptr, 0u};
  a.grad_x = grad_x; a.grad_pts = grad_pts;
  a.x_stride = x_stride; a.gx_stride = gx_stride;
  a.P = P; a.Cin = Cin; a.width = desc->shs_width; a.O = 11 + desc->shs_width; a.relu = activation == GH_TRUNK_RELU;
  a.vec_w1 = ghr_al16(W1) && Cin % 4 == 0;
  a.vec_w = ghr_al16(W2) && ghr_al16(W3) && ghr_al16(Wh);
  a.vec_gx = ghr_al16(grad_x) && gx_stride % 4 == 0;
  a.flags = desc->flags; a.clip = desc->clip_scaling;
  const dim3 grid((unsigned)(((long long)P + GT_ROWS - 1) / GT_ROWS));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  GT_DISPATCH(gt_backward_kernel)
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
