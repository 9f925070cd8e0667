// gh_conv.hip — the perceptual loss's 3x3 convolution, forward and backward-data, and its 2x2 max pooling (include/gh_conv.h).
//
// One kernel serves both directions of the convolution: out[p, co] = b[co] + sum_t sum_ci w[t][co][ci] in[p + tap t, ci] over a
// tap-major weight layout whose rows are padded with zeros to whole chunks. The backward calls it with the flipped, transposed layout,
// the channel counts exchanged, no bias, and the forward's gate bits applied to its operand as it is read.
//
// The product is gh_rows.h's "columns" form: the pixel is the column of v_mfma_f32_32x32x2_f32, a wave owns 32 pixels, an accumulator
// 32 output channels, and the weights (the A operand) cross LDS in slabs of (32 NH) x 32 that the four waves share. Unlike ghr_mm_x a
// lane takes the 16 CONSECUTIVE channels 16 half .. 16 half + 15 of a slab as its B operands (four 16-byte loads), so step s of a
// slab multiplies the channels s and 16 + s: the order include/gh_conv.h states. csrc_conv/gh_conv_tile.h holds the host's launch
// rules, which gh_lpips.hip's convolution shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gh_conv.h"
#include "gh_conv_tile.h"

#define GC_T32(c) (((c) + 31) / 32)

static inline int gc_pad(int c) { return (c + GH_CONV_CHUNK - 1) / GH_CONV_CHUNK * GH_CONV_CHUNK; }

struct GcArgs {
  const float* in;       // (NP, Ci)
  const uint32_t* gate;  // GATE: (NP, T32(Ci)) bits of `in`'s channels
  const float* w;        // (9, CoP, Ci)
  const float* bias;     // (Co,) or null
  float* out;            // (NP, Co)
  uint16_t* gate_out;    // (NP, T32(Co), 2) or null: the bits of `out`'s pre-activations
  long long NP;          // N H W
  int H, W, Ci, Co, CoP, relu, vec_w, vec_in, vec_out;
};

// bit of channel c (0 .. 31) of a gate word: the register order of the result (include/gh_conv.h)
__device__ __forceinline__ int gc_bit(int c) { return 16 * ((c >> 2) & 1) + (c & 3) + 4 * (c >> 3); }

template <int NH, bool GATE>
__global__ __launch_bounds__(GHR_BLOCK) void gc_conv_kernel(GcArgs a) {
  __shared__ float s_w[32 * NH * GHR_WP];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long p = (long long)blockIdx.x * GH_CONV_PIXELS + 32 * wave + col;
  const bool live_p = p < a.NP;
  const int co0 = blockIdx.y * 32 * NH;
  const long long hw = (long long)a.H * a.W;
  const long long rem = live_p ? p % hw : 0;
  const int i = (int)(rem / a.W), j = (int)(rem % a.W);
  const int Ci = a.Ci, t32i = GC_T32(Ci);

  ghr_acc h[NH];
#pragma unroll
  for (int t = 0; t < NH; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = co0 + 32 * t + ghr_acc_row(k, half);
      h[t][k] = (a.bias && c < a.Co) ? a.bias[c] : 0.f;
    }
  }

  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const bool live = live_p && (unsigned)(i + dy) < (unsigned)a.H && (unsigned)(j + dx) < (unsigned)a.W;
    const long long q = live ? p + (long long)dy * a.W + dx : 0;     // the tap's pixel (of the same image: i + dy, j + dx are inside it)
    const float* __restrict__ xp = a.in + q * Ci;
    const float* __restrict__ wt = a.w + (long long)tap * a.CoP * Ci;
    for (int k0 = 0; k0 < Ci; k0 += 32) {
      const int kc = Ci - k0 < 32 ? Ci - k0 : 32;
      GhrSlab<NH, 8> w;                                              // 32 NH rows x 32 columns
      ghr_fetch_in(w, wt, Ci, co0, k0, a.CoP, Ci, a.vec_w, tid);
      float xv[16];
      const int c0 = 16 * half;                                      // the lane's channels of the slab: c0 .. c0 + 15
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
      if constexpr (GATE) {
        const uint32_t g = live ? a.gate[q * t32i + (k0 >> 5)] : 0u;
#pragma unroll
        for (int s = 0; s < 16; ++s) xv[s] = ((g >> gc_bit(c0 + s)) & 1u) ? xv[s] : 0.f;
      }
      __syncthreads();                                               // the previous slab has been read by every wave
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
  }

  if (!live_p) return;
  float* __restrict__ orow = a.out + p * a.Co;
  const int t32o = GC_T32(a.Co);
#pragma unroll
  for (int t = 0; t < NH; ++t) {
    const int cb = co0 + 32 * t;
    if (cb >= a.Co) break;
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float v = h[t][k];
      bits |= (v > 0.f ? 1u : 0u) << k;
      if (a.relu) h[t][k] = v < 0.f ? 0.f : v;
    }
    if (a.gate_out) a.gate_out[2 * (p * t32o + (cb >> 5)) + half] = (uint16_t)bits;
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

// The checks both directions share, and the launch. Ci / Co are the product's input and output channel counts.
static int gc_conv(const float* in, const uint32_t* gate, int N, int H, int W, int Ci, int Co, const float* w, const float* bias,
                   uint32_t flags, int chunk, float* out, uint32_t* gate_out, bool gated, void* hip_stream) {
  if (N < 0 || H < 0 || W < 0 || Ci < 1 || Co < 1 || (flags & ~(uint32_t)GH_CONV_RELU)) return GH_ERR_INVALID_ARG;
  if (!gct_chunk_ok(chunk)) return GH_ERR_INVALID_ARG;
  if (Ci > GH_CONV_MAX_C || Co > GH_CONV_MAX_C) return GH_ERR_UNSUPPORTED;
  const long long NP = (long long)N * H * W;
  const long long tiles = (NP + GH_CONV_PIXELS - 1) / GH_CONV_PIXELS;
  if (tiles > 2147483647LL) return GH_ERR_UNSUPPORTED;
  if (NP == 0) return GH_OK;
  const bool relu = (flags & GH_CONV_RELU) != 0;
  if (!in || !w || !out || (relu && !(gated ? (const void*)gate : (const void*)gate_out))) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(in) || !ghr_al4(gate) || !ghr_al4(w) || !ghr_al4(bias) || !ghr_al4(out) || !ghr_al4(gate_out)) return GH_ERR_INVALID_ARG;
  GcArgs a;
  a.in = in; a.gate = (gated && relu) ? gate : nullptr; a.w = w; a.bias = bias; a.out = out;
  a.gate_out = (!gated && relu) ? (uint16_t*)gate_out : nullptr;
  a.NP = NP; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.CoP = gc_pad(Co); a.relu = (!gated && relu) ? 1 : 0;
  gct_vec(a, Ci % 4 == 0);
  if (chunk == 0) chunk = gct_auto_chunk(tiles, a.CoP, GH_CONV_CHUNK, GH_CONV_FILL);
  const dim3 grid((unsigned)tiles, (unsigned)((Co + chunk - 1) / chunk));
  hipStream_t st = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  gct_nh(chunk, [&](auto nh) {
    if (a.gate) hipLaunchKernelGGL((gc_conv_kernel<nh(), true>), grid, dim3(GHR_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((gc_conv_kernel<nh(), false>), grid, dim3(GHR_BLOCK), 0, st, a);
  });
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" size_t gh_conv3x3_weight_floats(int Cin_, int Cout_) {
  if (Cin_ < 1 || Cout_ < 1 || Cin_ > GH_CONV_MAX_C || Cout_ > GH_CONV_MAX_C) return 0;
  return (size_t)9 * gc_pad(Cout_) * Cin_;
}

extern "C" int gh_conv3x3_forward(const float* x, int N, int H, int W, int Cin, int Cout, const float* wf, const float* bias, uint32_t flags,
                                  int chunk, float* y, uint32_t* gate, void* hip_stream) {
  return gc_conv(x, nullptr, N, H, W, Cin, Cout, wf, bias, flags, chunk, y, gate, false, hip_stream);
}

extern "C" int gh_conv3x3_backward_data(const float* dy, const uint32_t* gate, int N, int H, int W, int Cin, int Cout, const float* wb,
                                        uint32_t flags, int chunk, float* dx, void* hip_stream) {
  return gc_conv(dy, gate, N, H, W, Cout, Cin, wb, nullptr, flags, chunk, dx, nullptr, true, hip_stream);
}

// ---- 2x2 max pooling ---------------------------------------------------------------------------------------------------------------
#define GC_POOL_BLOCK 256

__global__ __launch_bounds__(GC_POOL_BLOCK) void gc_pool_forward_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                        uint8_t* __restrict__ choice, long long n_out, int H, int W, int C) {
  const long long e = (long long)blockIdx.x * GC_POOL_BLOCK + threadIdx.x;
  if (e >= n_out) return;
  const int Ho = H / 2, Wo = W / 2;
  const int c = (int)(e % C);
  long long r = e / C;
  const int jo = (int)(r % Wo);
  r /= Wo;
  const int io = (int)(r % Ho);
  const long long n = r / Ho;
  const float* src = x + (((n * H + 2 * io) * W) + 2 * jo) * C + c;
  float m = -INFINITY;
  int q = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float v = src[((long long)(k >> 1) * W + (k & 1)) * C];
    if (v > m || v != v) { m = v; q = k; }
  }
  if (y) y[e] = m;
  if (choice) choice[e] = (uint8_t)q;
}

__global__ __launch_bounds__(GC_POOL_BLOCK) void gc_pool_backward_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ choice,
                                                                         float* __restrict__ dx, long long n_in, int H, int W, int C) {
  const long long e = (long long)blockIdx.x * GC_POOL_BLOCK + threadIdx.x;
  if (e >= n_in) return;
  const int Ho = H / 2, Wo = W / 2;
  const int c = (int)(e % C);
  long long r = e / C;
  const int j = (int)(r % W);
  r /= W;
  const int i = (int)(r % H);
  const long long n = r / H;
  float g = 0.f;
  if ((i >> 1) < Ho && (j >> 1) < Wo) {
    const long long o = (((n * Ho + (i >> 1)) * Wo) + (j >> 1)) * C + c;
    if (choice[o] == (uint8_t)(2 * (i & 1) + (j & 1))) g = dy[o];
  }
  dx[e] = g;
}

static int gc_pool_sizes(int N, int H, int W, int C, bool backward, long long* n, long long* blocks) {
  if (N < 0 || H < 0 || W < 0 || C < 1) return GH_ERR_INVALID_ARG;
  *n = backward ? (long long)N * H * W * C : (long long)N * (H / 2) * (W / 2) * C;
  *blocks = (*n + GC_POOL_BLOCK - 1) / GC_POOL_BLOCK;
  return *blocks > 2147483647LL ? GH_ERR_UNSUPPORTED : GH_OK;
}

extern "C" int gh_maxpool2x2_forward(const float* x, int N, int H, int W, int C, float* y, uint8_t* choice, void* hip_stream) {
  long long n, blocks;
  const int rc = gc_pool_sizes(N, H, W, C, false, &n, &blocks);
  if (rc != GH_OK) return rc;
  if (n == 0) return GH_OK;
  if (!x || (!y && !choice) || !ghr_al4(x) || !ghr_al4(y)) return GH_ERR_INVALID_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gc_pool_forward_kernel, dim3((unsigned)blocks), dim3(GC_POOL_BLOCK), 0, (hipStream_t)hip_stream, x, y, choice, n, H, W, C);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_maxpool2x2_backward(const float* dy, const uint8_t* choice, int N, int H, int W, int C, float* dx, void* hip_stream) {
  long long n, blocks;
  const int rc = gc_pool_sizes(N, H, W, C, true, &n, &blocks);
  if (rc != GH_OK) return rc;
  if (n == 0) return GH_OK;
  const bool has_out = (long long)(H / 2) * (W / 2) > 0;
  if (!dx || !ghr_al4(dx) || !ghr_al4(dy) || (has_out && (!dy || !choice))) return GH_ERR_INVALID_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gc_pool_backward_kernel, dim3((unsigned)blocks), dim3(GC_POOL_BLOCK), 0, (hipStream_t)hip_stream, dy, choice, dx, n, H, W, C);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
