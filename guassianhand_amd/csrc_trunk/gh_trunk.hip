// gh_trunk.hip — the fused Gaussian trunk (include/gh_trunk.h): forward_gs's trunk MLP and Gaussian head in one pass each way.
//
// gh_res.hip's product shape, gh_rows.h's "columns": v_mfma_f32_32x32x2_f32 with the point as the column, a wave owns 32 rows of x, lane l
// the point l & 31. The weights are the A operand and cross LDS in slabs the four waves share (two barriers a slab): 32 columns of all
// rows of W in the forward products (ghr_mm_x, ghr_mm), 32 rows of up to 128 columns in the backward's products with W^T (ghr_mm_tg,
// ghr_mm_t), every window bounded. A layer's result stays in the accumulators and is the B operand of the next product register by
// register; the activation is applied to it on the way.
//   forward   v1 (x from global memory, Cin padded with zero columns to the k step), v2, y, then the head's O rows as one more product
//             over y; its pre-activations cross LDS ([row][o], pitch 59) to the per-row activations (gh_head_act.h), which leave as
//             each output's contiguous run of the tile.
//   backward  graw from `raw` and the cotangents into LDS ([row][o]); dy = Wh^T graw and W3^T dy first, then v1 and v2 are recomputed
//             (so that at most three sets of four accumulators are alive, and of those the half of one that only waits is parked
//             in graw's tile, which is free by then), dv2, dv1, and grad_x in chunks of 128 columns.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_trunk.h"
#include "../csrc_head/gh_head_act.h"

#define GT_BLOCK GHR_BLOCK
#define GT_ROWS GH_TRUNK_ROWS
#define GT_RP 59           // pitch of the [row][o] tile of raw / graw: odd, lane = row is conflict-free
#define GT_SLAB (128 * GHR_WP)  // floats of the weight slab: 128 rows x 32 columns at pitch 33, or 32 rows x 128 columns
#define GT_GP 65           // the backward's pitch of that tile: its 128 x 65 floats also park two accumulator tiles per thread

static_assert(GT_ROWS == (GT_BLOCK / 64) * 32, "four waves of 32 rows");
static_assert(GT_RP >= GH_HEAD_MAX_O && (GT_RP & 1), "a row of raw fits the pitch");
static_assert(GH_TRUNK_MAX_CIN % 32 == 0, "whole slabs");
static_assert(GT_GP >= GH_HEAD_MAX_O && (GT_GP & 1) && GT_ROWS * GT_GP >= 2 * 16 * GT_BLOCK, "graw's tile holds the parked accumulators");

__device__ __forceinline__ float gt_act(float v, bool relu) { return relu ? (v < 0.f ? 0.f : v) : v / (1.0f + expf(-v)); }
struct GtAct {  // what a product applies to its source on the way: the activation, or nothing where `plain`
  bool plain, relu;
  __device__ __forceinline__ float operator()(float v) const { return plain ? v : gt_act(v, relu); }
};
// d * act'(v)
__device__ __forceinline__ float gt_dact(float v, float d, bool relu) {
  if (relu) return v > 0.f ? d : (v == v ? 0.f : v);  // (a NaN pre-activation reaches the gradient, as it reaches the output)
  const float s = ghr_sigmoid(v);
  return d * (s * (1.0f + v * (1.0f - s)));
}

struct GtArgs {
  const float *x, *pts, *raw, *W1, *b1, *W2, *b2, *W3, *b3, *Wh, *bh;
  float *grad_x, *grad_pts;
  GhaOut o;  // forward: the outputs; backward: the cotangents
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

  const GtAct act = {false, relu};

  ghr_acc r[2];
  {
    ghr_acc y[NC];
    {
      ghr_acc v2[NH];
      {
        ghr_acc v1[NH];
        ghr_fill<NH>(v1, a.b1, half);
        ghr_mm_x<NH>(v1, s_w, a.W1, a.Cin, a.vec_w1, a.x + (live ? row0 + trow : 0) * a.x_stride, live, tid, col, half);
        ghr_fill<NH>(v2, a.b2, half);
        ghr_mm<false, NH, NH>(v2, NH, v1, act, s_w, a.W2, 32 * NH, a.vec_w, tid, col, half);
      }
      ghr_fill<NC>(y, a.b3, half);
      ghr_mm<false, NH, NC>(y, NC, v2, act, s_w, a.W3, 32 * NC, a.vec_w, tid, col, half);
    }
    ghr_fill<2>(r, nullptr, half);                             // the head's bias is added last, as gh_head.hip adds it
    ghr_mm<false, NC, 2>(r, no, y, GtAct{true, relu}, s_w, a.Wh, O, a.vec_w, tid, col, half);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int o = 32 * t + ghr_acc_row(k, half);
      if (o < O) s_raw[trow * GT_RP + o] = r[t][k] + a.bh[o];
    }
  }
  __syncthreads();
  gha_forward<GT_ROWS>(s_raw, [](int rr, int o) { return rr * GT_RP + o; }, a.o, a.pts, row0, nrows, O, a.width, a.flags, a.clip, tid);
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
  const int O = a.O;
  gha_backward<GT_ROWS>(s_g, [](int r, int o) { return r * GT_GP + o; }, a.o, a.raw, a.grad_pts, row0, nrows, O, a.width, a.flags, a.clip, tid);
  __syncthreads();

  ghr_acc d2[NH];
  ghr_fill<NH>(d2, nullptr, half);
  {
    // ---- dy = Wh^T . graw, o ascending; then W3^T . dy ----
    ghr_acc dy[NC];
    ghr_fill<NC>(dy, nullptr, half);
    ghr_mm_tg<false, NC>(dy, s_w, a.Wh, 32 * NC, 0, O, 32 * NC, a.vec_w, s_g + trow * GT_GP, true, tid, col, half);
    ghr_mm_t<false, NC, NH>(d2, NH, dy, s_w, a.W3, 32 * NH, 0, 32 * NH, a.vec_w, tid, col, half);
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
  ghr_acc v1[NH];
  ghr_fill<NH>(v1, a.b1, half);
  ghr_mm_x<NH>(v1, s_w, a.W1, a.Cin, a.vec_w1, a.x + (live ? row0 + trow : 0) * a.x_stride, live, tid, col, half);
  {
    ghr_acc v2[NH];
    ghr_fill<NH>(v2, a.b2, half);
    ghr_mm<false, NH, NH>(v2, NH, v1, GtAct{false, relu}, s_w, a.W2, 32 * NH, a.vec_w, tid, col, half);
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
  ghr_acc d1[NH];
  ghr_fill<NH>(d1, nullptr, half);
  ghr_mm_t<false, NH, NH>(d1, NH, d2, s_w, a.W2, 32 * NH, 0, 32 * NH, a.vec_w, tid, col, half);
#pragma unroll
  for (int t = 0; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) d1[t][k] = gt_dact(t < NKEEP ? v1[t][k] : s_park[((t - NKEEP) * 16 + k) * GT_BLOCK], d1[t][k], relu);
  }

  // ---- grad_x = W1^T . dv1, 128 columns a time ----
  float* gxr = a.grad_x + (live ? row0 + trow : 0) * a.gx_stride;
  for (int k0 = 0; k0 < a.Cin; k0 += 128) {
    const int cw = a.Cin - k0 < 128 ? a.Cin - k0 : 128, nt = (cw + 31) >> 5;
    ghr_acc d[4];
    ghr_fill<4>(d, nullptr, half);
    ghr_mm_t<false, NH, 4>(d, nt, d1, s_w, a.W1, a.Cin, k0, a.Cin, a.vec_w1, tid, col, half);
    if (live) {  // (written out: ghr_store_tiles has no column bound)
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
static bool gt_tiles_ok(int n) { return n == 32 || n == 64 || n == 96 || n == 128; }

static int gt_check(const GhHeadDesc* d, int P, int Cin, int H, int Cout, int activation) {
  const int rc = gha_check_desc(d);
  if (rc != GH_OK) return rc;
  if (P < 0 || Cin < 1 || H < 1 || Cout < 1) return GH_ERR_INVALID_ARG;
  if (activation != GH_TRUNK_SILU && activation != GH_TRUNK_RELU) return GH_ERR_INVALID_ARG;
  if (Cin > GH_TRUNK_MAX_CIN || !gt_tiles_ok(H) || !gt_tiles_ok(Cout)) return GH_ERR_UNSUPPORTED;
  return GH_OK;
}

// one instantiation per (H / 32, Cout / 32)
#define GT_DISPATCH(KERNEL) \
  ghr_tiles(H / 32, [&](auto nh) { ghr_tiles(Cout / 32, [&](auto nc) { hipLaunchKernelGGL((KERNEL<nh(), nc()>), grid, dim3(GT_BLOCK), 0, st, a); }); });

extern "C" int gh_trunk_forward(const float* x, int64_t x_stride, int P, int Cin, int H, int Cout, const float* pts, const float* W1,
                                const float* b1, const float* W2, const float* b2, const float* W3, const float* b3, const float* Wh,
                                const float* bh, const GhHeadDesc* desc, int activation, float* xyz, float* scaling, float* rotation,
                                float* opacity, float* shs, float* raw, void* hip_stream) {
  const int rc = gt_check(desc, P, Cin, H, Cout, activation);
  if (rc != GH_OK) return rc;
  if (!x || !pts || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !Wh || !bh || !xyz || !scaling || !rotation || !opacity || !shs)
    return GH_ERR_INVALID_ARG;
  if (!ghr_al4(x) || !ghr_al4(pts) || !ghr_al4(W1) || !ghr_al4(b1) || !ghr_al4(W2) || !ghr_al4(b2) || !ghr_al4(W3) || !ghr_al4(b3) || !ghr_al4(Wh) ||
      !ghr_al4(bh) || !ghr_al4(xyz) || !ghr_al4(scaling) || !ghr_al4(rotation) || !ghr_al4(opacity) || !ghr_al4(shs) || !ghr_al4(raw))
    return GH_ERR_INVALID_ARG;
  if (x_stride < Cin) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  GtArgs a = {};
  a.x = x; a.pts = pts; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3; a.Wh = Wh; a.bh = bh;
  a.o = gha_out(xyz, scaling, rotation, opacity, shs, raw);
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
  if (!ghr_al4(raw) || !ghr_al4(x) || !ghr_al4(W1) || !ghr_al4(b1) || !ghr_al4(W2) || !ghr_al4(b2) || !ghr_al4(W3) || !ghr_al4(Wh) || !ghr_al4(g_xyz) ||
      !ghr_al4(g_scaling) || !ghr_al4(g_rotation) || !ghr_al4(g_opacity) || !ghr_al4(g_shs) || !ghr_al4(grad_x) || !ghr_al4(grad_pts))
    return GH_ERR_INVALID_ARG;
  if (x_stride < Cin || gx_stride < Cin) return GH_ERR_INVALID_ARG;
  if (P == 0) return GH_OK;
  GtArgs a = {};
  a.raw = raw; a.x = x; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.Wh = Wh;
  a.o = gha_out(g_xyz, g_scaling, g_rotation, g_opacity, g_shs, nullptr);
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
