// gh_lpips.hip — the evaluator's perceptual score, LPIPS over AlexNet, forward only (include/gh_lpips.h): the dense convolution of
// kernel 3, 5 or 11 and stride 1 or 4, the 3x3 stride-2 max pooling, LPIPS' head per tap, the crop-quantise-scale prologue and the
// host call that chains them.
//
// The convolution is gh_conv.hip's product with another gather: the output pixel is the column of v_mfma_f32_32x32x2_f32, a wave owns
// 32 output pixels, an accumulator 32 output channels, and the weights (the A operand) cross LDS in slabs of (32 NH) x 32 out of ONE
// layout wp[co][(K ky + kx) Cin + ci]. A lane takes the 16 consecutive reduction indices 16 half .. 16 half + 15 of a slab as its B
// operands, so step s multiplies the indices s and 16 + s: the order the header states. Where Cin is small (FLAT) a slab runs through
// the flattened index and a lane walks (ky, kx, ci) with three counters; else a slab is 32 channels of one tap, as in gh_conv.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_lpips.h"
#include "../csrc_conv/gh_conv_tile.h"

static inline int gl_pad(int c) { return (c + GH_LPIPS_CHUNK - 1) / GH_LPIPS_CHUNK * GH_LPIPS_CHUNK; }
static inline int gl_out(int H, int K, int s, int p) { return H + 2 * p < K ? 0 : (H + 2 * p - K) / s + 1; }
static inline int gl_pool_out(int H) { return H < 3 ? 0 : (H - 3) / 2 + 1; }
static inline bool gl_al8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// ---- the convolution -------------------------------------------------------------------------------------------------------------------
struct GlConvArgs {
  const float* in;    // (N, H, W, Ci)
  const float* w;     // (CoP, Rp)
  const float* bias;  // (Co,) or null
  float* out;         // (N, Ho, Wo, Co)
  long long NP;       // N Ho Wo
  int H, W, Ho, Wo, Ci, Co, CoP, K, stride, pad, R, Rp, relu, vec_w, vec_in, vec_out;
};

// One slab of the product, the single statement of it in this file: the fetched weights go to LDS behind the previous slab's readers,
// then step s = 0 .. kc - 1 (16 at most) multiplies the slab's columns c0 + s — s and 16 + s over the two lane halves — into every
// accumulator. Every thread of the workgroup calls it (two barriers).
template <int NH>
__device__ __forceinline__ void gl_slab_product(ghr_acc (&h)[NH], float* s_w, const GhrSlab<NH, 8>& w, const float (&xv)[16], int kc, int tid,
                                                int col, int c0) {
  __syncthreads();                                                   // the previous slab has been read by every wave
  ghr_put(w, s_w, GHR_WP, tid);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    if (s < kc) {
#pragma unroll
      for (int t = 0; t < NH; ++t)
        h[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(32 * t + col) * GHR_WP + c0 + s], xv[s], h[t], 0, 0, 0);
    }
  }
}

template <int NH, bool FLAT>
__global__ __launch_bounds__(GHR_BLOCK) void gl_conv_kernel(GlConvArgs a) {
  __shared__ float s_w[32 * NH * GHR_WP];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long p = (long long)blockIdx.x * GH_LPIPS_PIXELS + 32 * wave + col;
  const bool live_p = p < a.NP;
  const int co0 = blockIdx.y * 32 * NH;
  const long long hwo = (long long)a.Ho * a.Wo;
  const long long n = live_p ? p / hwo : 0;
  const long long rem = live_p ? p - n * hwo : 0;
  const int iy0 = (int)(rem / a.Wo) * a.stride - a.pad, ix0 = (int)(rem % a.Wo) * a.stride - a.pad;  // the window's first row and column
  const float* __restrict__ img = a.in + n * a.H * a.W * a.Ci;
  const int Ci = a.Ci, K = a.K;
  const int c0 = 16 * half;                                          // the lane's indices of a slab: c0 .. c0 + 15

  ghr_acc h[NH];
#pragma unroll
  for (int t = 0; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = co0 + 32 * t + ghr_acc_row(k, half);
      h[t][k] = (a.bias && c < a.Co) ? a.bias[c] : 0.f;
    }
  }

  if constexpr (FLAT) {
    for (int k0 = 0; k0 < a.R; k0 += 32) {
      const int kc = a.R - k0 < 32 ? a.R - k0 : 32;
      GhrSlab<NH, 8> w;                                              // 32 NH rows x 32 columns
      ghr_fetch_in(w, a.w, a.Rp, co0, k0, a.CoP, a.Rp, a.vec_w, tid);
      float xv[16];
      const int r = k0 + c0;                                         // (ky, kx, ci) of the lane's first index, then counted on
      int t = r / Ci, ci = r - t * Ci, ky = t / K, kx = t - ky * K;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = live_p && ky < K && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;   // ky >= K: past R
        xv[s] = ok ? img[((long long)iy * a.W + ix) * Ci + ci] : 0.f;
        if (++ci == Ci) {
          ci = 0;
          if (++kx == K) { kx = 0; ++ky; }
        }
      }
      gl_slab_product(h, s_w, w, xv, kc, tid, col, c0);
    }
  } else {
    for (int tap = 0; tap < K * K; ++tap) {
      const int iy = iy0 + tap / K, ix = ix0 + tap % K;
      const bool live = live_p && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const float* __restrict__ xp = img + (live ? ((long long)iy * a.W + ix) * Ci : 0);
      for (int k0 = 0; k0 < Ci; k0 += 32) {
        const int kc = Ci - k0 < 32 ? Ci - k0 : 32;
        GhrSlab<NH, 8> w;
        ghr_fetch_in(w, a.w, a.Rp, co0, tap * Ci + k0, a.CoP, tap * Ci + Ci, a.vec_w, tid);   // bounded at the tap's last channel
        float xv[16];
        if (a.vec_in && kc == 32) {
#pragma unroll
          for (int v4 = 0; v4 < 4; ++v4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = *(const float4*)(xp + k0 + c0 + 4 * v4);
            xv[4 * v4] = v.x; xv[4 * v4 + 1] = v.y; xv[4 * v4 + 2] = v.z; xv[4 * v4 + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int s = 0; s < 16; ++s) xv[s] = (live && c0 + s < kc) ? xp[k0 + c0 + s] : 0.f;
        }
        gl_slab_product(h, s_w, w, xv, kc, tid, col, c0);
      }
    }
  }

  if (!live_p) return;
  float* __restrict__ orow = a.out + p * a.Co;
#pragma unroll
  for (int t = 0; t < NH; ++t) {
    const int cb = co0 + 32 * t;
    if (cb >= a.Co) break;
    if (a.relu) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float v = h[t][k];
        h[t][k] = v < 0.f ? 0.f : v;
      }
    }
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int c = cb + 8 * q4 + 4 * half;
      if (a.vec_out) {
        if (c < a.Co) *(float4*)(orow + c) = make_float4(h[t][4 * q4], h[t][4 * q4 + 1], h[t][4 * q4 + 2], h[t][4 * q4 + 3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (c + e < a.Co) orow[c + e] = h[t][4 * q4 + e];
        }
      }
    }
  }
}

// the header's first two groups of checks; *NP receives the number of output pixels
static int gl_conv_sizes(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, uint32_t flags, int chunk, long long* NP) {
  if (N < 0 || H < 0 || W < 0 || Cin < 1 || Cout < 1) return GH_ERR_INVALID_ARG;
  if ((K != 3 && K != 5 && K != 11) || (stride != 1 && stride != 4) || pad < 0 || pad >= K) return GH_ERR_INVALID_ARG;
  if ((flags & ~(uint32_t)GH_LPIPS_RELU) || !gct_chunk_ok(chunk)) return GH_ERR_INVALID_ARG;
  if (Cin > GH_LPIPS_MAX_C || Cout > GH_LPIPS_MAX_C) return GH_ERR_UNSUPPORTED;
  *NP = (long long)N * gl_out(H, K, stride, pad) * gl_out(W, K, stride, pad);
  if ((*NP + GH_LPIPS_PIXELS - 1) / GH_LPIPS_PIXELS > 2147483647LL) return GH_ERR_UNSUPPORTED;
  return GH_OK;
}

extern "C" size_t gh_conv2d_weight_floats(int Cin, int Cout, int K) {
  if (Cin < 1 || Cout < 1 || Cin > GH_LPIPS_MAX_C || Cout > GH_LPIPS_MAX_C || (K != 3 && K != 5 && K != 11)) return 0;
  return (size_t)gl_pad(Cout) * (size_t)((K * K * Cin + 3) / 4 * 4);
}

extern "C" int gh_conv2d_forward(const float* x, int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, const float* wp,
                                 const float* bias, uint32_t flags, int chunk, float* y, void* hip_stream) {
  long long NP;
  const int rc = gl_conv_sizes(N, H, W, Cin, Cout, K, stride, pad, flags, chunk, &NP);
  if (rc != GH_OK) return rc;
  if (NP == 0) return GH_OK;
  if (!x || !wp || !y || !ghr_al4(x) || !ghr_al4(wp) || !ghr_al4(bias) || !ghr_al4(y)) return GH_ERR_INVALID_ARG;
  const bool flat = Cin <= GH_LPIPS_FLAT_CIN;
  GlConvArgs a;
  a.in = x; a.w = wp; a.bias = bias; a.out = y; a.NP = NP;
  a.H = H; a.W = W; a.Ho = gl_out(H, K, stride, pad); a.Wo = gl_out(W, K, stride, pad);
  a.Ci = Cin; a.Co = Cout; a.CoP = gl_pad(Cout); a.K = K; a.stride = stride; a.pad = pad;
  a.R = K * K * Cin; a.Rp = (a.R + 3) / 4 * 4; a.relu = (flags & GH_LPIPS_RELU) ? 1 : 0;
  gct_vec(a, flat || Cin % 4 == 0);                                 // a slab starts at a multiple of 4 floats of a row of Rp
  const long long tiles = (NP + GH_LPIPS_PIXELS - 1) / GH_LPIPS_PIXELS;
  if (chunk == 0) chunk = gct_auto_chunk(tiles, a.CoP, GH_LPIPS_CHUNK, GH_LPIPS_FILL);
  const dim3 grid((unsigned)tiles, (unsigned)((Cout + chunk - 1) / chunk));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  gct_nh(chunk, [&](auto nh) {
    if (flat) hipLaunchKernelGGL((gl_conv_kernel<nh(), true>), grid, dim3(GHR_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((gl_conv_kernel<nh(), false>), grid, dim3(GHR_BLOCK), 0, st, a);
  });
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

// ---- 3x3 stride-2 max pooling -----------------------------------------------------------------------------------------------------------
#define GL_BLOCK 256

__global__ __launch_bounds__(GL_BLOCK) void gl_pool_kernel(const float* __restrict__ x, float* __restrict__ y, long long n_out, int H, int W,
                                                           int Ho, int Wo, int C) {
  const long long e = (long long)blockIdx.x * GL_BLOCK + threadIdx.x;
  if (e >= n_out) return;
  const int c = (int)(e % C);
  long long r = e / C;
  const int jo = (int)(r % Wo);
  r /= Wo;
  const int io = (int)(r % Ho);
  const long long n = r / Ho;
  const float* src = x + (((n * H + 2 * io) * W) + 2 * jo) * C + c;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float v = src[((long long)(k / 3) * W + (k % 3)) * C];
    if (v > m || v != v) m = v;
  }
  y[e] = m;
}

extern "C" int gh_maxpool3x3s2_forward(const float* x, int N, int H, int W, int C, float* y, void* hip_stream) {
  if (N < 0 || H < 0 || W < 0 || C < 1) return GH_ERR_INVALID_ARG;
  if (C > GH_LPIPS_MAX_C) return GH_ERR_UNSUPPORTED;
  const int Ho = gl_pool_out(H), Wo = gl_pool_out(W);
  const long long n = (long long)N * Ho * Wo * C, blocks = (n + GL_BLOCK - 1) / GL_BLOCK;
  if (blocks > 2147483647LL) return GH_ERR_UNSUPPORTED;
  if (n == 0) return GH_OK;
  if (!x || !y || !ghr_al4(x) || !ghr_al4(y)) return GH_ERR_INVALID_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gl_pool_kernel, dim3((unsigned)blocks), dim3(GL_BLOCK), 0, (hipStream_t)hip_stream, x, y, n, H, W, Ho, Wo, C);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

// ---- LPIPS' head for one tap -----------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T gl_butterfly(T v) {                    // every lane receives the same bits: a + b is commutative
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// A wave per pixel, lane l the channels l, l + 64, ...: NV = ceil(C / 64) values of each image in registers.
template <int NV>
__global__ __launch_bounds__(GL_BLOCK) void gl_head_kernel(const float* __restrict__ f, const float* __restrict__ lin, double* __restrict__ part,
                                                           long long P, int C, int N, long long nb) {
  __shared__ double s_acc[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long n = blockIdx.x / nb, tile = blockIdx.x - n * nb;
  float wl[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) wl[k] = lane + 64 * k < C ? lin[lane + 64 * k] : 0.f;
  const long long p0 = tile * GH_LPIPS_HEAD_PIXELS + (GH_LPIPS_HEAD_PIXELS / 4) * wave;
  double acc = 0.0;
  for (int q = 0; q < GH_LPIPS_HEAD_PIXELS / 4; ++q) {
    const long long p = p0 + q;
    if (p >= P) break;                                               // wave-uniform
    const float* __restrict__ r0 = f + (n * P + p) * C;
    const float* __restrict__ r1 = f + ((n + N) * P + p) * C;
    float a[NV], b[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const bool in = lane + 64 * k < C;
      a[k] = in ? r0[lane + 64 * k] : 0.f;
      b[k] = in ? r1[lane + 64 * k] : 0.f;
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      s0 = fmaf(a[k], a[k], s0);
      s1 = fmaf(b[k], b[k], s1);
    }
    const float n0 = sqrtf(gl_butterfly(s0)) + 1e-10f, n1 = sqrtf(gl_butterfly(s1)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const float e = a[k] / n0 - b[k] / n1;
      d = fmaf(wl[k], e * e, d);
    }
    acc += (double)gl_butterfly(d);
  }
  if (lane == 0) s_acc[wave] = acc;
  __syncthreads();
  if (tid == 0) part[n * nb + tile] = ((s_acc[0] + s_acc[1]) + s_acc[2]) + s_acc[3];
}

__global__ __launch_bounds__(64) void gl_head_finish_kernel(const double* __restrict__ part, long long nb, long long P, int accumulate,
                                                            double* __restrict__ score, double* __restrict__ term) {
  const long long n = blockIdx.x;
  const int lane = threadIdx.x;
  double s = 0.0;
  for (long long i = lane; i < nb; i += 64) s += part[n * nb + i];
  s = gl_butterfly(s);
  if (lane == 0) {
    const double d = s / (double)P;
    if (term) term[n] = d;
    score[n] = accumulate ? score[n] + d : d;
  }
}

static long long gl_head_blocks(long long P) { return (P + GH_LPIPS_HEAD_PIXELS - 1) / GH_LPIPS_HEAD_PIXELS; }

extern "C" size_t gh_lpips_layer_workspace(int N, long long P) {
  if (N < 0 || P < 0 || (double)N * (double)gl_head_blocks(P) > 2147483647.0) return 0;
  return ghr_align((size_t)N * (size_t)gl_head_blocks(P) * sizeof(double));
}

extern "C" int gh_lpips_layer(const float* f, int N, long long P, int C, const float* lin, int accumulate, double* score, double* term,
                              void* workspace, size_t ws_bytes, void* hip_stream) {
  if (N < 0 || P < 0 || C < 1) return GH_ERR_INVALID_ARG;
  if (C > GH_LPIPS_MAX_C) return GH_ERR_UNSUPPORTED;
  const long long nb = gl_head_blocks(P);
  if ((double)N * (double)nb > 2147483647.0) return GH_ERR_UNSUPPORTED;
  if (N == 0 || P == 0) return GH_OK;
  if (!f || !lin || !score || !workspace || !ghr_al4(f) || !ghr_al4(lin) || !gl_al8(score) || !gl_al8(term) || !gl_al8(workspace))
    return GH_ERR_INVALID_ARG;
  if (ws_bytes < gh_lpips_layer_workspace(N, P)) return GH_ERR_INVALID_ARG;
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)(N * nb));
  (void)hipGetLastError();
  switch ((C + 63) / 64) {
    case 1: hipLaunchKernelGGL(gl_head_kernel<1>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
    case 2: hipLaunchKernelGGL(gl_head_kernel<2>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
    case 3: hipLaunchKernelGGL(gl_head_kernel<3>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
    case 4: hipLaunchKernelGGL(gl_head_kernel<4>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
    case 5: case 6: hipLaunchKernelGGL(gl_head_kernel<6>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
    default: hipLaunchKernelGGL(gl_head_kernel<8>, grid, dim3(GL_BLOCK), 0, st, f, lin, part, P, C, N, nb); break;
  }
  hipLaunchKernelGGL(gl_head_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, (const double*)part, nb, P, accumulate, score, term);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

// ---- crop, mask, quantise, scale: the network's input -----------------------------------------------------------------------------------
struct GlPrepArgs {
  const float* img[2];  // pred, gt
  const uint8_t* bbox_mask;
  const int32_t* bbox;
  const float* shift;
  const float* scale;
  float* x;
  long long n_pix;      // 2 N h w
  int N, H, W, h, w, hwc[2], quantize, is_signed;
};

__global__ __launch_bounds__(GL_BLOCK) void gl_prepare_kernel(GlPrepArgs a) {
  const long long e = (long long)blockIdx.x * GL_BLOCK + threadIdx.x;
  if (e >= a.n_pix) return;
  const int j = (int)(e % a.w);
  long long r = e / a.w;
  const int i = (int)(r % a.h);
  const long long m = r / a.h;                                       // image of the output: member * N + view
  const int member = m >= a.N ? 1 : 0;
  const long long n = m - (long long)member * a.N;
  int bx = 0, by = 0, bw = a.w, bh = a.h;
  if (a.bbox) { bx = a.bbox[4 * n]; by = a.bbox[4 * n + 1]; bw = a.bbox[4 * n + 2]; bh = a.bbox[4 * n + 3]; }
  float* __restrict__ o = a.x + 3 * e;
  if (bw != a.w || bh != a.h || bx < 0 || by < 0 || bx > a.W - a.w || by > a.H - a.h) {
    o[0] = o[1] = o[2] = NAN;
    return;
  }
  const long long y = by + i, xx = bx + j, plane = (long long)a.H * a.W, pix = y * a.W + xx;
  const bool zero = member == 0 && a.bbox_mask && a.bbox_mask[n * plane + pix] == 0;
  const float* __restrict__ src = a.img[member];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = a.hwc[member] ? src[(n * plane + pix) * 3 + c] : src[(n * 3 + c) * plane + pix];
    if (zero) v = 0.f;
    if (!a.is_signed) {
      float t = v * 255.f;
      if (a.quantize) {
        t = rintf(t);
        t = t < 0.f ? 0.f : t;                                       // a NaN passes both
        t = t > 255.f ? 255.f : t;
      }
      v = (float)((double)t / 127.5 - 1.0);
    }
    o[c] = (v - a.shift[c]) / a.scale[c];
  }
}

extern "C" int gh_lpips_prepare(const float* pred, const float* gt, const uint8_t* bbox_mask, const int32_t* bbox, int N, int H, int W, int h,
                                int w, uint32_t flags, const float* shift, const float* scale, float* x, void* hip_stream) {
  if (N < 0 || H < 0 || W < 0 || h < 0 || w < 0) return GH_ERR_INVALID_ARG;
  if (flags & ~(GH_LPIPS_PRED_HWC | GH_LPIPS_GT_HWC | GH_LPIPS_QUANTIZE | GH_LPIPS_SIGNED)) return GH_ERR_INVALID_ARG;
  if ((flags & GH_LPIPS_QUANTIZE) && (flags & GH_LPIPS_SIGNED)) return GH_ERR_INVALID_ARG;
  if (h > H || w > W) return GH_ERR_INVALID_ARG;
  const long long n_pix = 2LL * N * h * w, blocks = (n_pix + GL_BLOCK - 1) / GL_BLOCK;
  if (blocks > 2147483647LL) return GH_ERR_UNSUPPORTED;
  if (n_pix == 0) return GH_OK;
  if (!pred || !gt || !shift || !scale || !x) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(pred) || !ghr_al4(gt) || !ghr_al4(bbox) || !ghr_al4(shift) || !ghr_al4(scale) || !ghr_al4(x)) return GH_ERR_INVALID_ARG;
  GlPrepArgs a;
  a.img[0] = pred; a.img[1] = gt; a.bbox_mask = bbox_mask; a.bbox = bbox; a.shift = shift; a.scale = scale; a.x = x; a.n_pix = n_pix;
  a.N = N; a.H = H; a.W = W; a.h = h; a.w = w;
  a.hwc[0] = (flags & GH_LPIPS_PRED_HWC) ? 1 : 0; a.hwc[1] = (flags & GH_LPIPS_GT_HWC) ? 1 : 0;
  a.quantize = (flags & GH_LPIPS_QUANTIZE) ? 1 : 0; a.is_signed = (flags & GH_LPIPS_SIGNED) ? 1 : 0;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gl_prepare_kernel, dim3((unsigned)blocks), dim3(GL_BLOCK), 0, (hipStream_t)hip_stream, a);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

// ---- the chain -------------------------------------------------------------------------------------------------------------------------
// AlexNet's five convolutions, and which of them a pooling precedes
static const int GL_K[GH_LPIPS_TAPS] = {11, 5, 3, 3, 3}, GL_S[GH_LPIPS_TAPS] = {4, 1, 1, 1, 1}, GL_P[GH_LPIPS_TAPS] = {2, 2, 1, 1, 1};
static const bool GL_POOL[GH_LPIPS_TAPS] = {false, true, true, false, false};

// The maps go back and forth between two buffers: a convolution writes the one its input is not in, a pooling likewise. *fa, *fb
// receive the floats of the two, *part the bytes of the largest head workspace. False where a size is out of range.
struct GlPlan {
  int h[GH_LPIPS_TAPS], w[GH_LPIPS_TAPS];       // the taps' sizes
  int ph[GH_LPIPS_TAPS], pw[GH_LPIPS_TAPS];     // the pooled inputs' sizes (where GL_POOL)
  size_t fa, fb, part;
};

static bool gl_plan(int N, int h, int w, const int* widths, GlPlan* pl) {
  size_t need[2] = {0, 0};
  pl->part = 0;
  int cur = -1, ch = h, cw = w;                                      // the buffer the current map is in: -1 = the caller's x
  for (int l = 0; l < GH_LPIPS_TAPS; ++l) {
    if (GL_POOL[l]) {
      ch = gl_pool_out(ch); cw = gl_pool_out(cw);
      pl->ph[l] = ch; pl->pw[l] = cw;
      cur = cur == 0 ? 1 : 0;
      const size_t n = (size_t)2 * N * ch * cw * widths[l - 1];
      if (n > need[cur]) need[cur] = n;
    }
    ch = gl_out(ch, GL_K[l], GL_S[l], GL_P[l]); cw = gl_out(cw, GL_K[l], GL_S[l], GL_P[l]);
    if (ch < 1 || cw < 1) return false;
    pl->h[l] = ch; pl->w[l] = cw;
    cur = cur == 0 ? 1 : 0;
    const size_t n = (size_t)2 * N * ch * cw * widths[l];
    if (n > need[cur]) need[cur] = n;
    const size_t pb = gh_lpips_layer_workspace(N, (long long)ch * cw);
    if (pb > pl->part) pl->part = pb;
  }
  pl->fa = need[0]; pl->fb = need[1];
  return true;
}

static int gl_forward_sizes(int N, int h, int w, const int* widths) {
  if (N < 0 || h < 0 || w < 0 || !widths) return GH_ERR_INVALID_ARG;
  for (int l = 0; l < GH_LPIPS_TAPS; ++l) {
    if (widths[l] < 1) return GH_ERR_INVALID_ARG;
  }
  for (int l = 0; l < GH_LPIPS_TAPS; ++l) {
    if (widths[l] > GH_LPIPS_MAX_C) return GH_ERR_UNSUPPORTED;
  }
  if (h < GH_LPIPS_MIN_SIZE || w < GH_LPIPS_MIN_SIZE) return GH_ERR_UNSUPPORTED;
  const int h1 = gl_out(h, 11, 4, 2), w1 = gl_out(w, 11, 4, 2);      // the first tap is the largest launch of the chain
  if (2.0 * N * h1 * w1 * 512.0 / GL_BLOCK > 2147483647.0) return GH_ERR_UNSUPPORTED;
  return GH_OK;
}

extern "C" size_t gh_lpips_workspace(int N, int h, int w, const int* widths) {
  GlPlan pl;
  if (gl_forward_sizes(N, h, w, widths) != GH_OK || !gl_plan(N, h, w, widths, &pl)) return 0;
  return ghr_align(pl.fa * sizeof(float)) + ghr_align(pl.fb * sizeof(float)) + pl.part;
}

extern "C" int gh_lpips_forward(const float* x, int N, int h, int w, const int* widths, const GhLpipsWeights* weights, double* scores,
                                double* terms, void* workspace, size_t ws_bytes, void* hip_stream) {
  if (!weights) return GH_ERR_INVALID_ARG;
  int rc = gl_forward_sizes(N, h, w, widths);
  if (rc != GH_OK) return rc;
  if (N == 0) return GH_OK;
  GlPlan pl;
  if (!gl_plan(N, h, w, widths, &pl)) return GH_ERR_UNSUPPORTED;
  if (!x || !scores || !workspace || !ghr_al4(x) || !gl_al8(scores) || !gl_al8(terms) || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  for (int l = 0; l < GH_LPIPS_TAPS; ++l) {
    if (!weights->w[l] || !weights->lin[l] || !ghr_al4(weights->w[l]) || !ghr_al4(weights->b[l]) || !ghr_al4(weights->lin[l]))
      return GH_ERR_INVALID_ARG;
  }
  if (ws_bytes < gh_lpips_workspace(N, h, w, widths)) return GH_ERR_INVALID_ARG;
  float* buf[2] = {(float*)workspace, (float*)((char*)workspace + ghr_align(pl.fa * sizeof(float)))};
  void* part = (char*)buf[1] + ghr_align(pl.fb * sizeof(float));
  const float* cur = x;
  int at = -1, ch = h, cw = w, cc = 3;
  for (int l = 0; l < GH_LPIPS_TAPS; ++l) {
    if (GL_POOL[l]) {
      at = at == 0 ? 1 : 0;
      rc = gh_maxpool3x3s2_forward(cur, 2 * N, ch, cw, cc, buf[at], hip_stream);
      if (rc != GH_OK) return rc;
      cur = buf[at]; ch = pl.ph[l]; cw = pl.pw[l];
    }
    at = at == 0 ? 1 : 0;
    rc = gh_conv2d_forward(cur, 2 * N, ch, cw, cc, widths[l], GL_K[l], GL_S[l], GL_P[l], weights->w[l], weights->b[l], GH_LPIPS_RELU, 0,
                           buf[at], hip_stream);
    if (rc != GH_OK) return rc;
    cur = buf[at]; ch = pl.h[l]; cw = pl.w[l]; cc = widths[l];
    rc = gh_lpips_layer(cur, N, (long long)ch * cw, cc, weights->lin[l], l > 0, scores, terms ? terms + (size_t)l * N : nullptr, part, pl.part,
                        hip_stream);
    if (rc != GH_OK) return rc;
  }
  return GH_OK;
}
