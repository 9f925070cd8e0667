// gh_plane.hip — the plane fetch (include/gh_plane.h): bilinear sampling of a channel-first (C, Hp, Wp) plane at per-point UVs and
// its ordered backward; F.grid_sample(bilinear, align_corners=True, zeros) as query_triplane_texture calls it.
//   forward (2 launches)  transpose: a 64-texel x 64-channel tile crosses LDS (pitch 65), read in 256-byte runs along the texels of a
//                                    channel and written in 256-byte runs along the channels of a texel -> the channel-last copy in
//                                    the workspace
//                         sample:    gh_uv_sample_forward (csrc/gh_uv.hip) on the copy: its values are the contract
//   index (1 + 3)         keys:      one thread per pair e = 4 * point + corner: the pair's linear texel (-1 outside the map) and its
//                                    bilinear weight, gh_bilinear's arithmetic statement for statement
//                         plan:      gh_pool_plan sorts the 4N pairs by texel (stable: ascending e inside a texel); -1 is its "no cell"
//   backward (1 launch)   one 4-wave workgroup per (16 consecutive texels of one map row, 64-channel slab), lanes are channels. A wave
//                         takes texels w, w + 4, w + 8, w + 12 of the run, one after the other, and walks each texel's list ONCE from
//                         its first pair to its last: 64 list entries and their weights are fetched by one coalesced load and one
//                         gather and handed out by v_readlane, four 256-byte gradient-row segments in flight, the products added in
//                         list order into one accumulator. The (16 x 64) tile crosses LDS so that the channel-first gradient is
//                         written in 64-byte runs along x. A list is never split: the chain of additions is gh_uv_scatter_sorted's.
// A workgroup lasts as long as its slowest wave: the sum of the lengths of the four lists that wave walks.
// No atomics here; the only ones of the whole path are the integer LDS atomics of the plan's histogram.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gh_plane.h"
#include "../csrc_rows/gh_rows.h"

#define GHL_BLOCK 256
#define GHL_WAVES (GHL_BLOCK / 64)
#define GHL_TILE 64   // texels and channels per transpose tile
#define GHL_TX 16     // texels of one map row per backward workgroup

static_assert(GHL_TX % GHL_WAVES == 0, "every wave takes the same number of texels");

// ---- forward: (C, HW) -> (HW, C) --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHL_BLOCK) void ghl_transpose_kernel(const float* __restrict__ plane, float* __restrict__ out, int C, int HW) {
  __shared__ float s[GHL_TILE][GHL_TILE + 1];
  const int t0 = blockIdx.x * GHL_TILE, ch0 = blockIdx.y * GHL_TILE;
  for (int i = threadIdx.x; i < GHL_TILE * GHL_TILE; i += GHL_BLOCK) {
    const int cl = i / GHL_TILE, tl = i % GHL_TILE;
    if (ch0 + cl < C && t0 + tl < HW) s[cl][tl] = plane[(size_t)(ch0 + cl) * HW + t0 + tl];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GHL_TILE * GHL_TILE; i += GHL_BLOCK) {
    const int tl = i / GHL_TILE, cl = i % GHL_TILE;
    if (ch0 + cl < C && t0 + tl < HW) out[(size_t)(t0 + tl) * C + ch0 + cl] = s[cl][tl];
  }
}

// ---- index: texel and weight of every (point, corner) pair --------------------------------------------------------------------------
// The arithmetic of gh_bilinear and of gh_uv_sample_fwd_kernel's weights (csrc/gh_uv.hip), which the forward above runs.
__global__ __launch_bounds__(GHL_BLOCK) void ghl_keys_kernel(const float* __restrict__ uv, int n_pairs, int Hp, int Wp,
                                                             int* __restrict__ keys, float* __restrict__ w) {
  const int e = blockIdx.x * GHL_BLOCK + threadIdx.x;
  if (e >= n_pairs) return;
  const int n = e >> 2, corner = e & 3;
  const float ix = ((uv[2 * n] + 1.0f) * 0.5f) * (float)(Wp - 1);
  const float iy = ((uv[2 * n + 1] + 1.0f) * 0.5f) * (float)(Hp - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  const float wx1 = ix - fx, wy1 = iy - fy;
  const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  const long long x = (long long)(int)fx + (corner & 1), y = (long long)(int)fy + (corner >> 1);
  const bool inside = x >= 0 && x < Wp && y >= 0 && y < Hp;         // integers, before anything is addressed by them
  keys[e] = inside ? (int)(y * Wp + x) : -1;
  w[e] = ((corner & 1) ? wx1 : wx0) * ((corner >> 1) ? wy1 : wy0);
}

__global__ __launch_bounds__(GHL_BLOCK) void ghl_zero_starts_kernel(int* __restrict__ texel_start, int n) {
  const int i = blockIdx.x * GHL_BLOCK + threadIdx.x;
  if (i < n) texel_start[i] = 0;
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GHL_BLOCK) void ghl_bwd_kernel(const float* __restrict__ g, const int* __restrict__ texel_start,
                                                            const int* __restrict__ pairs, const float* __restrict__ w,
                                                            float* __restrict__ gp, int n_pairs, int C, int Hp, int Wp, int chunks) {
  __shared__ float s_t[GHL_TX][65];
  __shared__ int s_cs[GHL_TX + 1];
  const int y = blockIdx.x / chunks, x0 = (blockIdx.x % chunks) * GHL_TX, nx = min(GHL_TX, Wp - x0);
  const int t0 = y * Wp + x0, HW = Hp * Wp;
  const int ch0 = blockIdx.y * 64, lane = threadIdx.x & 63, ch = ch0 + lane;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = ch < C;
  if (threadIdx.x <= GHL_TX) s_cs[threadIdx.x] = min(max(texel_start[t0 + min((int)threadIdx.x, nx)], 0), n_pairs);
  __syncthreads();
  for (int k = 0; k < GHL_TX / GHL_WAVES; ++k) {
    const int xl = k * GHL_WAVES + wv;                                // past the row's end: s_cs repeats, the list is empty
    const int lo = __builtin_amdgcn_readfirstlane(s_cs[xl]), hi = __builtin_amdgcn_readfirstlane(s_cs[xl + 1]);
    float acc = 0.0f;
    for (int j0 = lo; j0 < hi; j0 += 64) {
      const int m = min(64, hi - j0);
      int e_mine = -1;
      float w_mine = 0.0f;
      if (lane < m) {
        const int e = pairs[j0 + lane];
        if (e >= 0 && e < n_pairs) { e_mine = e; w_mine = w[e]; }
      }
      const int w_bits = __float_as_int(w_mine);
      auto row = [&](int e) { return (on && e >= 0) ? g[(size_t)(e >> 2) * C + ch] : 0.0f; };
      int j = 0;
      for (; j + 4 <= m; j += 4) {
        const int e0 = __builtin_amdgcn_readlane(e_mine, j), e1 = __builtin_amdgcn_readlane(e_mine, j + 1);
        const int e2 = __builtin_amdgcn_readlane(e_mine, j + 2), e3 = __builtin_amdgcn_readlane(e_mine, j + 3);
        const float v0 = row(e0), v1 = row(e1), v2 = row(e2), v3 = row(e3);
        acc += v0 * __int_as_float(__builtin_amdgcn_readlane(w_bits, j));
        acc += v1 * __int_as_float(__builtin_amdgcn_readlane(w_bits, j + 1));
        acc += v2 * __int_as_float(__builtin_amdgcn_readlane(w_bits, j + 2));
        acc += v3 * __int_as_float(__builtin_amdgcn_readlane(w_bits, j + 3));
      }
      for (; j < m; ++j) acc += row(__builtin_amdgcn_readlane(e_mine, j)) * __int_as_float(__builtin_amdgcn_readlane(w_bits, j));
    }
    s_t[xl][lane] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < GHL_TX * 64; i += GHL_BLOCK) {
    const int chl = i / GHL_TX, xl = i % GHL_TX;
    if (ch0 + chl < C && xl < nx) gp[(size_t)(ch0 + chl) * HW + t0 + xl] = s_t[xl][chl];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct GhlLayout {
  size_t copy;                // forward: the channel-last copy, from byte 0
  size_t flag, plan, plan_bytes, index;   // index: keys from byte 0, the plan's flag word, the plan's workspace; `index` bytes in all
  size_t total;
};

static bool ghl_layout(int N, int C, int Hp, int Wp, GhlLayout* L) {
  if (N < 0 || C < 1 || Hp < 1 || Wp < 1) return false;
  if ((long long)Hp * Wp > INT_MAX || N > INT_MAX / 4 || (C + 63) / 64 > 65535) return false;
  const size_t HW = (size_t)Hp * Wp;
  L->copy = ghr_align(HW * (size_t)C * sizeof(float));
  L->flag = L->plan = L->plan_bytes = L->index = 0;
  if (N >= 1 && HW <= GH_POOL_MAX_CELLS) {
    L->flag = ghr_align((size_t)4 * N * sizeof(int));
    L->plan = L->flag + ghr_align(sizeof(uint32_t));
    L->plan_bytes = gh_pool_plan_workspace(4 * N, (int)HW);
    L->index = L->plan + L->plan_bytes;
  }
  L->total = L->copy > L->index ? L->copy : L->index;
  return true;
}

static bool ghl_apart(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
}

extern "C" size_t gh_plane_workspace(int N, int C, int Hp, int Wp) {
  GhlLayout L;
  return ghl_layout(N, C, Hp, Wp, &L) ? L.total : 0;
}

extern "C" int gh_plane_sample_forward(const float* plane, const float* uv, float* out, int N, int C, int Hp, int Wp, void* workspace,
                                       size_t ws_bytes, void* hip_stream) {
  if (N < 0 || C < 1 || Hp < 1 || Wp < 1) return GH_ERR_INVALID_ARG;
  GhlLayout L;
  if (!ghl_layout(N, C, Hp, Wp, &L)) return GH_ERR_UNSUPPORTED;
  if (N == 0) return GH_OK;
  if (!plane || !uv || !out || !workspace) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(plane) || !ghr_al4(uv) || !ghr_al4(out) || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if (ws_bytes < L.copy) return GH_ERR_WORKSPACE_SMALL;
  const int HW = Hp * Wp;
  (void)hipGetLastError();
  float* copy = (float*)workspace;
  const dim3 grid((unsigned)((HW + GHL_TILE - 1) / GHL_TILE), (unsigned)((C + GHL_TILE - 1) / GHL_TILE));
  hipLaunchKernelGGL(ghl_transpose_kernel, grid, dim3(GHL_BLOCK), 0, (hipStream_t)hip_stream, plane, copy, C, HW);
  if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  return gh_uv_sample_forward(copy, uv, out, N, C, Hp, Wp, hip_stream);
}

extern "C" int gh_plane_index(const float* uv, int N, int Hp, int Wp, int32_t* texel_start, int32_t* pairs, float* w, void* workspace,
                              size_t ws_bytes, void* hip_stream) {
  if (N < 0 || Hp < 1 || Wp < 1 || !texel_start || !ghr_al4(texel_start)) return GH_ERR_INVALID_ARG;
  if (N > 0 && (!uv || !pairs || !w || !workspace)) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(uv) || !ghr_al4(pairs) || !ghr_al4(w) || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
  if ((long long)Hp * Wp > GH_POOL_MAX_CELLS) return GH_ERR_UNSUPPORTED;
  GhlLayout L;
  if (!ghl_layout(N, 1, Hp, Wp, &L)) return GH_ERR_UNSUPPORTED;
  if (ws_bytes < L.index) return GH_ERR_WORKSPACE_SMALL;
  const int HW = Hp * Wp;
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  if (N == 0) {
    hipLaunchKernelGGL(ghl_zero_starts_kernel, dim3((unsigned)((HW + 1 + GHL_BLOCK - 1) / GHL_BLOCK)), dim3(GHL_BLOCK), 0, s, texel_start,
                       HW + 1);
    return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
  }
  char* ws = (char*)workspace;
  int* keys = (int*)ws;
  const int n_pairs = 4 * N;
  hipLaunchKernelGGL(ghl_keys_kernel, dim3((unsigned)((n_pairs + GHL_BLOCK - 1) / GHL_BLOCK)), dim3(GHL_BLOCK), 0, s, uv, n_pairs, Hp, Wp,
                     keys, w);
  if (hipGetLastError() != hipSuccess) return GH_ERR_LAUNCH;
  return gh_pool_plan(keys, 0, n_pairs, HW, texel_start, pairs, (uint32_t*)(ws + L.flag), ws + L.plan, L.plan_bytes, hip_stream);
}

extern "C" int gh_plane_sample_backward(const float* grad_out, const int32_t* texel_start, const int32_t* pairs, const float* w,
                                        float* grad_plane, int N, int C, int Hp, int Wp, void* hip_stream) {
  if (N < 0 || C < 1 || Hp < 1 || Wp < 1 || !texel_start || !grad_plane) return GH_ERR_INVALID_ARG;
  if (N > 0 && (!grad_out || !pairs || !w)) return GH_ERR_INVALID_ARG;
  if (!ghr_al4(grad_out) || !ghr_al4(texel_start) || !ghr_al4(pairs) || !ghr_al4(w) || !ghr_al4(grad_plane))
    return GH_ERR_INVALID_ARG;
  GhlLayout L;
  if (!ghl_layout(N, C, Hp, Wp, &L)) return GH_ERR_UNSUPPORTED;
  const size_t HW = (size_t)Hp * Wp, gp_bytes = HW * C * sizeof(float), pair_bytes = (size_t)4 * N * sizeof(int);
  if (!ghl_apart(grad_plane, gp_bytes, texel_start, (HW + 1) * sizeof(int))) return GH_ERR_INVALID_ARG;
  if (N > 0 && (!ghl_apart(grad_plane, gp_bytes, grad_out, (size_t)N * C * sizeof(float)) || !ghl_apart(grad_plane, gp_bytes, pairs, pair_bytes) ||
                !ghl_apart(grad_plane, gp_bytes, w, pair_bytes)))
    return GH_ERR_INVALID_ARG;
  const int chunks = (Wp + GHL_TX - 1) / GHL_TX;
  if ((long long)Hp * chunks > INT_MAX) return GH_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  const dim3 grid((unsigned)(Hp * chunks), (unsigned)((C + 63) / 64));
  hipLaunchKernelGGL(ghl_bwd_kernel, grid, dim3(GHL_BLOCK), 0, (hipStream_t)hip_stream, grad_out, texel_start, pairs, w, grad_plane, 4 * N, C,
                     Hp, Wp, chunks);
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
