// gh_metrics.hip — MSE / PSNR / SSIM of rendered views against their targets (include/gh_metrics.h), three launches:
//   1. rows:     per (view, band of rows) workgroup: the bounding box of mask_at_box and the sum of squared differences
//                (bbox_mask applied to pred on the fly) -> one fixed slot each.
//   2. ssim:     per (view, 32x16 tile) workgroup: reads its view's box from the row slots, returns at once outside the crop's
//                interior; else stages the tile + 3-pixel halo of both images (3 channels) in LDS, forms the 7x7 box sums as a
//                horizontal then a vertical pass in double and writes the sum of S over its pixels -> one fixed slot.
//   3. finalize: per view: the slots summed in a fixed order -> mse, psnr, ssim, bbox.
// Double precision for the moments: E[x^2] - E[x]^2 of 49 samples in [0,1] loses about 6 of fp32's 7 digits where the
// window is flat, while x*y of two floats is exact in double and the 49-term sums stay within a few ulp, so the result
// tracks a float64 restatement to ~1e-12 with no centring pass. The SSIM kernel is the longest of the three (56 of ~95 us at
// 8 views of 512x334 under a kernel trace).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_metrics.h"
#include "../csrc_rows/gh_rows.h"

#define GHM_BLOCK 256
#define GHM_WAVES (GHM_BLOCK / 64)
#define GHM_ROW_SLOTS 128            // row bands per view (fewer when H is smaller)
#define GHM_TX 32                    // SSIM output tile: 32 x 16 pixels, 2 per thread
#define GHM_TY 16
#define GHM_HALO 3                   // (7 - 1) / 2
#define GHM_LX (GHM_TX + 2 * GHM_HALO)
#define GHM_LY (GHM_TY + 2 * GHM_HALO)

struct GhmImage {
  const float* p;
  size_t chan, pix;                  // element strides of a channel and of a pixel inside one view
  __device__ float at(size_t view3, size_t pixel, int c) const { return p[view3 + c * chan + pixel * pix]; }
};

static inline GhmImage ghm_image(const float* p, bool hwc, size_t HW) { return GhmImage{p, hwc ? 1 : HW, hwc ? 3u : 1u}; }

static inline int ghm_row_slots(int H) { return H < GHM_ROW_SLOTS ? H : GHM_ROW_SLOTS; }

struct GhmLayout {
  size_t sse, box, ssim, total;      // byte offsets: double[Nv * slots], int4[Nv * slots], double[Nv * tiles]
  int slots, gx, gy;
};

static bool ghm_layout(int NV, int H, int W, GhmLayout* L) {
  if (NV < 1 || H < 1 || W < 1) return false;
  L->slots = ghm_row_slots(H);
  L->gx = (W + GHM_TX - 1) / GHM_TX;
  L->gy = (H + GHM_TY - 1) / GHM_TY;
  const size_t rows = (size_t)NV * L->slots, tiles = (size_t)NV * L->gx * L->gy;
  L->sse = 0;
  L->box = ghr_align(L->sse + rows * sizeof(double));
  L->ssim = ghr_align(L->box + rows * sizeof(int4));
  L->total = ghr_align(L->ssim + tiles * sizeof(double));
  return true;
}

// ---- fixed-order block reductions (256 threads: a 64-lane butterfly, then the 4 wave results in wave order) ----------
__device__ __forceinline__ double ghm_block_sum(double v) {
  __shared__ double s_w[GHM_WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                   // s_w may still be read by a previous call
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// (xmin, xmax, ymin, ymax) over the block; integer min / max, so the order does not matter
__device__ __forceinline__ int4 ghm_block_box(int4 b) {
  __shared__ int4 s_b[GHM_WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    b.x = min(b.x, __shfl_xor(b.x, o, 64));
    b.y = max(b.y, __shfl_xor(b.y, o, 64));
    b.z = min(b.z, __shfl_xor(b.z, o, 64));
    b.w = max(b.w, __shfl_xor(b.w, o, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6] = b;
  __syncthreads();
  int4 r = s_b[0];
#pragma unroll
  for (int k = 1; k < GHM_WAVES; ++k) {
    r.x = min(r.x, s_b[k].x); r.y = max(r.y, s_b[k].y); r.z = min(r.z, s_b[k].z); r.w = max(r.w, s_b[k].w);
  }
  return r;
}

// the view's box as (x, y, w, h) from its row slots; (0, 0, 0, 0) when the mask is empty
__device__ __forceinline__ int4 ghm_view_box(const int4* __restrict__ part, int slots) {
  int4 b = make_int4(INT_MAX, -1, INT_MAX, -1);
  for (int i = threadIdx.x; i < slots; i += GHM_BLOCK) {
    const int4 q = part[i];
    b.x = min(b.x, q.x); b.y = max(b.y, q.y); b.z = min(b.z, q.z); b.w = max(b.w, q.w);
  }
  b = ghm_block_box(b);
  if (b.y < 0) return make_int4(0, 0, 0, 0);
  return make_int4(b.x, b.z, b.y - b.x + 1, b.w - b.z + 1);
}

// ---- 1. rows: box of mask_at_box + sum of squared differences ------------------------------------------------------
__global__ __launch_bounds__(GHM_BLOCK) void gh_metrics_rows_kernel(GhmImage pred, GhmImage gt, const uint8_t* __restrict__ mbox,
                                                                    const uint8_t* __restrict__ bbm, int H, int W, int slots,
                                                                    double* __restrict__ sse_part, int4* __restrict__ box_part) {
  const int s = blockIdx.x, v = blockIdx.y;
  const int y0 = (int)((long long)s * H / slots), y1 = (int)((long long)(s + 1) * H / slots);
  const size_t HW = (size_t)H * W, v3 = (size_t)v * 3 * HW, vm = (size_t)v * HW;
  const int n = (y1 - y0) * W;
  double acc = 0.0;
  int4 b = make_int4(INT_MAX, -1, INT_MAX, -1);
  for (int i = threadIdx.x; i < n; i += GHM_BLOCK) {
    const size_t p = (size_t)y0 * W + i;
    const bool keep = bbm == nullptr || bbm[vm + p] != 0;      // test_step: pred[bbox_mask == 0] = 0 (pred not read there)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = (double)(keep ? pred.at(v3, p, c) : 0.0f) - (double)gt.at(v3, p, c);
      acc += d * d;
    }
    if (mbox[vm + p] != 0) {
      const int yy = y0 + i / W, xx = i - (i / W) * W;
      b.x = min(b.x, xx); b.y = max(b.y, xx); b.z = min(b.z, yy); b.w = max(b.w, yy);
    }
  }
  acc = ghm_block_sum(acc);
  b = ghm_block_box(b);
  if (threadIdx.x == 0) {
    sse_part[(size_t)v * slots + s] = acc;
    box_part[(size_t)v * slots + s] = b;
  }
}

// ---- 2. SSIM over the crop's interior ------------------------------------------------------------------------------
__global__ __launch_bounds__(GHM_BLOCK) void gh_metrics_ssim_kernel(GhmImage pred, GhmImage gt, const uint8_t* __restrict__ bbm,
                                                                    int H, int W, int slots, const int4* __restrict__ box_part,
                                                                    double C1, double C2, double* __restrict__ ssim_part) {
  __shared__ float s_x[3][GHM_LY][GHM_LX];
  __shared__ float s_y[3][GHM_LY][GHM_LX];
  __shared__ double s_h[5][GHM_LY][GHM_TX];          // horizontal 7-sums of x, y, x^2, y^2, xy
  const int v = blockIdx.z;
  const size_t slot = ((size_t)v * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int4 box = ghm_view_box(box_part + (size_t)v * slots, slots);
  const int tx0 = blockIdx.x * GHM_TX, ty0 = blockIdx.y * GHM_TY;
  // pixels whose 7x7 window lies inside the crop: [x + 3, x + w - 3) x [y + 3, y + h - 3)
  const int ox0 = max(tx0, box.x + GHM_HALO), ox1 = min(tx0 + GHM_TX, box.x + box.z - GHM_HALO);
  const int oy0 = max(ty0, box.y + GHM_HALO), oy1 = min(ty0 + GHM_TY, box.y + box.w - GHM_HALO);
  if (box.z < 7 || box.w < 7 || ox0 >= ox1 || oy0 >= oy1) {       // uniform over the block (box is the block's reduction)
    if (threadIdx.x == 0) ssim_part[slot] = 0.0;
    return;
  }
  const size_t HW = (size_t)H * W, v3 = (size_t)v * 3 * HW, vm = (size_t)v * HW;
  // stage tile + halo; only pixels inside the crop are read (the rest is never part of a counted window)
  for (int i = threadIdx.x; i < GHM_LY * GHM_LX; i += GHM_BLOCK) {
    const int ly = i / GHM_LX, lx = i - ly * GHM_LX;
    const int gy = ty0 - GHM_HALO + ly, gx = tx0 - GHM_HALO + lx;
    const bool in = gx >= box.x && gx < box.x + box.z && gy >= box.y && gy < box.y + box.w;
    const size_t p = in ? (size_t)gy * W + gx : 0;
    const bool keep = in && (bbm == nullptr || bbm[vm + p] != 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_x[c][ly][lx] = keep ? pred.at(v3, p, c) : 0.0f;
      s_y[c][ly][lx] = in ? gt.at(v3, p, c) : 0.0f;
    }
  }
  const double inv = 1.0 / 49.0, cov_norm = 49.0 / 48.0;
  const int j = threadIdx.x & (GHM_TX - 1), r0 = threadIdx.x / GHM_TX;      // column, first of the thread's two rows
  double acc = 0.0;
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                 // staging done / previous channel's vertical pass done with s_h
    for (int i = threadIdx.x; i < GHM_LY * GHM_TX; i += GHM_BLOCK) {
      const int ly = i / GHM_TX, lx = i - ly * GHM_TX;
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const double x = s_x[c][ly][lx + k], y = s_y[c][ly][lx + k];
        sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
      }
      s_h[0][ly][lx] = sx; s_h[1][ly][lx] = sy; s_h[2][ly][lx] = sxx; s_h[3][ly][lx] = syy; s_h[4][ly][lx] = sxy;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < GHM_TY / (GHM_BLOCK / GHM_TX); ++t) {
      const int r = r0 + t * (GHM_BLOCK / GHM_TX), ox = tx0 + j, oy = ty0 + r;
      if (ox < ox0 || ox >= ox1 || oy < oy0 || oy >= oy1) continue;
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += s_h[q][r + k][j];
      }
      const double ux = m[0] * inv, uy = m[1] * inv, uxx = m[2] * inv, uyy = m[3] * inv, uxy = m[4] * inv;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      acc += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
  }
  acc = ghm_block_sum(acc);
  if (threadIdx.x == 0) ssim_part[slot] = acc;
}

// ---- 3. finalize: one workgroup per view ---------------------------------------------------------------------------
__global__ __launch_bounds__(GHM_BLOCK) void gh_metrics_finalize_kernel(int NV, int H, int W, int slots, int tiles,
                                                                        const double* __restrict__ sse_part,
                                                                        const int4* __restrict__ box_part,
                                                                        const double* __restrict__ ssim_part,
                                                                        double* __restrict__ scores, int32_t* __restrict__ bbox) {
  const int v = blockIdx.x;
  const int4 box = ghm_view_box(box_part + (size_t)v * slots, slots);
  double a = 0.0;
  for (int i = threadIdx.x; i < slots; i += GHM_BLOCK) a += sse_part[(size_t)v * slots + i];
  const double sse = ghm_block_sum(a);
  double b = 0.0;
  for (int i = threadIdx.x; i < tiles; i += GHM_BLOCK) b += ssim_part[(size_t)v * tiles + i];
  const double ssum = ghm_block_sum(b);
  if (threadIdx.x == 0) {
    const double mse = sse / (3.0 * (double)H * (double)W);
    scores[v] = mse;
    scores[NV + v] = -10.0 * log10(mse);                                     // mse == 0 -> +inf, as numpy gives
    scores[2 * NV + v] = (box.z < 7 || box.w < 7) ? (double)NAN : ssum / (3.0 * (double)(box.z - 6) * (double)(box.w - 6));
    bbox[4 * v + 0] = box.x; bbox[4 * v + 1] = box.y; bbox[4 * v + 2] = box.z; bbox[4 * v + 3] = box.w;
  }
}

extern "C" size_t gh_image_scores_workspace(int n_views, int H, int W) {
  GhmLayout L;
  return ghm_layout(n_views, H, W, &L) ? L.total : 0;
}

extern "C" int gh_image_scores(const float* pred, const float* gt, const uint8_t* mask_at_box, const uint8_t* bbox_mask, int n_views,
                               int H, int W, unsigned layout, double data_range, double* scores, int32_t* bbox, void* workspace,
                               size_t ws_bytes, void* hip_stream) {
  GhmLayout L;
  if (!ghm_layout(n_views, H, W, &L)) return GH_ERR_INVALID_ARG;
  if (!pred || !gt || !mask_at_box || !scores || !bbox || !workspace) return GH_ERR_INVALID_ARG;
  if ((layout & ~GH_METRICS_HWC) != 0 || !(data_range > 0.0) || !isfinite(data_range)) return GH_ERR_INVALID_ARG;
  if ((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)bbox) & 3) != 0 || ((uintptr_t)scores & 7) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return GH_ERR_INVALID_ARG;
  if ((long long)H * W > INT_MAX || n_views > 65535 || L.gy > 65535) return GH_ERR_UNSUPPORTED;   // int pixel indices; grid limits
  if (ws_bytes < L.total) return GH_ERR_WORKSPACE_SMALL;
  (void)hipGetLastError();
  const size_t HW = (size_t)H * W;
  const GhmImage P = ghm_image(pred, layout & GH_METRICS_PRED_HWC, HW), G = ghm_image(gt, layout & GH_METRICS_GT_HWC, HW);
  char* ws = (char*)workspace;
  double* sse_part = (double*)(ws + L.sse);
  int4* box_part = (int4*)(ws + L.box);
  double* ssim_part = (double*)(ws + L.ssim);
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  hipStream_t s = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(gh_metrics_rows_kernel, dim3((unsigned)L.slots, (unsigned)n_views), dim3(GHM_BLOCK), 0, s, P, G, mask_at_box,
                     bbox_mask, H, W, L.slots, sse_part, box_part);
  hipLaunchKernelGGL(gh_metrics_ssim_kernel, dim3((unsigned)L.gx, (unsigned)L.gy, (unsigned)n_views), dim3(GHM_BLOCK), 0, s, P, G,
                     bbox_mask, H, W, L.slots, (const int4*)box_part, C1, C2, ssim_part);
  hipLaunchKernelGGL(gh_metrics_finalize_kernel, dim3((unsigned)n_views), dim3(GHM_BLOCK), 0, s, n_views, H, W, L.slots, L.gx * L.gy,
                     (const double*)sse_part, (const int4*)box_part, (const double*)ssim_part, scores, bbox);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
