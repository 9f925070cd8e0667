// gh_head.hip — the fused Gaussian head (include/gh_head.h): GSLayer.forward's five linear heads and their activations in one pass
// over the feature rows, and the mirrored backward.
//   forward   one 4-wave workgroup per GH_HEAD_ROWS = 64 rows. The rows' features cross LDS in passes of 128 columns: loaded with
//             coalesced 16-byte (4-byte where x is not 16-byte aligned) loads, stored at a pitch of 129 floats, so that lane = row reads
//             its own row without a bank conflict. Wave w owns the outputs (4g + w) * 4 .. + 3 of every group g of 16; their weights are
//             wave-uniform, read through the scalar cache. The 64 x O pre-activations meet in LDS, and the five outputs (and raw) leave
//             as 16-byte stores over each tile's contiguous run of the output.
//   backward  the same tile. The gradients of the pre-activations are written TRANSPOSED into LDS (g[o][row], pitch 68), then
//             grad_x: lanes are columns, wave w holds rows 16w .. 16w + 15 x 2 columns in registers and walks o = 0 .. O-1 reading
//                     16 gradients as four broadcast 16-byte LDS reads and 2 weights (coalesced) per step; rows leave as 256-byte runs;
//             grad_W: (only when asked for) x crosses LDS as in the forward, wave w owns the outputs as in the forward, lanes are
//                     columns, and the tile's 64 rows are summed in ascending row order -> one partial per workgroup in the workspace.
//   reduce    16 elements x 16 runs of partials per workgroup: a run is summed in workgroup order, the 16 runs in run order.
// No atomics; every float sum has a fixed order that depends on (Cin, O) — and, for grad_W / grad_b, on P — alone.
#include "gh_head_act.h"

#define GHH_BLOCK GHR_BLOCK
#define GHH_ROWS GH_HEAD_ROWS
#define GHH_KC 128             // feature columns per pass through LDS
#define GHH_XP (GHH_KC + 1)    // pitch of the x tile: odd, so lane = row is conflict-free
#define GHH_GP (GHH_ROWS + 4)  // pitch of the transposed gradient tile: 16-byte aligned rows
#define GHH_MAX_CIN (1 << 20)  // O * Cin stays far inside an int

static_assert(GHH_ROWS == 64 && GHH_BLOCK == 4 * GHH_ROWS, "lane = row in the forward; 16 rows per wave in the backward");
static_assert(GH_HEAD_SEGMENTS == GHR_SEGMENTS, "the header documents the shared reduction's run count");

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int NG>  // groups of 16 outputs: ceil(O / 16)
__global__ __launch_bounds__(GHH_BLOCK) void ghh_fwd_kernel(const float* __restrict__ x, long long x_stride, int P, int Cin,
                                                            const float* __restrict__ pts, const float* __restrict__ W,
                                                            const float* __restrict__ b, int O, int width, unsigned flags, float clip,
                                                            GhaOut out, int vec_x) {
  extern __shared__ __attribute__((aligned(16))) float ghh_smem[];
  float* s_x = ghh_smem;                        // GHH_ROWS x GHH_XP
  float* s_raw = ghh_smem + GHH_ROWS * GHH_XP;  // GHH_ROWS x RP
  const int RP = O | 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long row0 = (long long)blockIdx.x * GHH_ROWS;
  const int nrows = (int)((long long)P - row0 < GHH_ROWS ? (long long)P - row0 : GHH_ROWS);

  float acc[NG][4][4];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[g][j][s] = 0.f;

  for (int k0 = 0; k0 < Cin; k0 += GHH_KC) {
    const int kc = Cin - k0 < GHH_KC ? Cin - k0 : GHH_KC;
    if (k0) __syncthreads();
    ghr_stage(s_x, GHH_XP, x, x_stride, row0, GHH_ROWS, nrows, k0, kc, vec_x, tid);
    __syncthreads();
    const float* xr = s_x + lane * GHH_XP;
    const int k4 = kc & ~3, tail = kc & 3;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int ob = (g * 4 + wave) * 4;
      const float* w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = W + (size_t)(ob + j < O ? ob + j : O - 1) * Cin + k0;  // (outputs past O are computed and dropped)
#pragma unroll 2
      for (int k = 0; k < k4; k += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float xv = xr[k + s];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][j][s] = fmaf(xv, w[j][k + s], acc[g][j][s]);
        }
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) {  // GHH_KC is a multiple of 4: column k0 + k4 + s belongs to partial sum s
        if (s < tail) {
          const float xv = xr[k4 + s];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][j][s] = fmaf(xv, w[j][k4 + s], acc[g][j][s]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int ob = (g * 4 + wave) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ob + j < O) s_raw[lane * RP + ob + j] = ((acc[g][j][0] + acc[g][j][1]) + (acc[g][j][2] + acc[g][j][3])) + b[ob + j];
    }
  }
  __syncthreads();
  gha_forward<GHH_ROWS>(s_raw, [&](int r, int o) { return r * RP + o; }, out, pts, row0, nrows, O, width, flags, clip, tid);
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <bool WGRAD>
__global__ __launch_bounds__(GHH_BLOCK) void ghh_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ x,
                                                            long long x_stride, int P, int Cin, const float* __restrict__ W, int O,
                                                            int width, unsigned flags, float clip, GhaOut g /* the output gradients */,
                                                            float* __restrict__ grad_x, long long gx_stride, float* __restrict__ grad_pts,
                                                            float* __restrict__ part_W, float* __restrict__ part_b, int vec_x) {
  extern __shared__ __attribute__((aligned(16))) float ghh_smem[];
  float* s_g = ghh_smem;                // O x GHH_GP: the gradient of raw[row, o] at s_g[o * GHH_GP + row]
  float* s_x = ghh_smem + O * GHH_GP;   // WGRAD: GHH_ROWS x GHH_XP
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long row0 = (long long)blockIdx.x * GHH_ROWS;
  const int nrows = (int)((long long)P - row0 < GHH_ROWS ? (long long)P - row0 : GHH_ROWS);
  // the gradient of the pre-activations, transposed; rows past the end are zeros (they enter the tile's sums of grad_W)
  gha_backward<GHH_ROWS>(s_g, [](int r, int o) { return o * GHH_GP + r; }, g, raw, grad_pts, row0, nrows, O, width, flags, clip, tid);
  __syncthreads();

  // ---- grad_x[row, c] = sum over o of g[row, o] * W[o, c]: one chain of fmaf in ascending o ----
  const int r0 = wave * 16;
  if (r0 < nrows) {
    for (int c0 = 0; c0 < Cin; c0 += 2 * 64) {
      const int ca = c0 + lane, cb = ca + 64;
      float acc[16][2];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r][0] = acc[r][1] = 0.f;
#pragma unroll 2
      for (int o = 0; o < O; ++o) {
        const float wa = ca < Cin ? W[(size_t)o * Cin + ca] : 0.f;
        const float wb = cb < Cin ? W[(size_t)o * Cin + cb] : 0.f;
        const float4* gq = (const float4*)(s_g + o * GHH_GP + r0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 gv = gq[q];
          acc[4 * q + 0][0] = fmaf(gv.x, wa, acc[4 * q + 0][0]); acc[4 * q + 0][1] = fmaf(gv.x, wb, acc[4 * q + 0][1]);
          acc[4 * q + 1][0] = fmaf(gv.y, wa, acc[4 * q + 1][0]); acc[4 * q + 1][1] = fmaf(gv.y, wb, acc[4 * q + 1][1]);
          acc[4 * q + 2][0] = fmaf(gv.z, wa, acc[4 * q + 2][0]); acc[4 * q + 2][1] = fmaf(gv.z, wb, acc[4 * q + 2][1]);
          acc[4 * q + 3][0] = fmaf(gv.w, wa, acc[4 * q + 3][0]); acc[4 * q + 3][1] = fmaf(gv.w, wb, acc[4 * q + 3][1]);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r0 + r < nrows) {
          float* dst = grad_x + (row0 + r0 + r) * gx_stride;
          if (ca < Cin) dst[ca] = acc[r][0];
          if (cb < Cin) dst[cb] = acc[r][1];
        }
      }
    }
  }

  // ---- this tile's share of grad_W[o, c] = sum over rows of g[row, o] * x[row, c], rows ascending; grad_b[o] likewise ----
  if (WGRAD) {
    if (tid < O) {
      float s = 0.f;
      for (int r = 0; r < GHH_ROWS; ++r) s += s_g[tid * GHH_GP + r];
      part_b[(size_t)blockIdx.x * O + tid] = s;
    }
    float* pw = part_W + (size_t)blockIdx.x * O * Cin;
    for (int k0 = 0; k0 < Cin; k0 += GHH_KC) {
      const int kc = Cin - k0 < GHH_KC ? Cin - k0 : GHH_KC;
      if (k0) __syncthreads();
      ghr_stage(s_x, GHH_XP, x, x_stride, row0, GHH_ROWS, nrows, k0, kc, vec_x, tid);
      __syncthreads();
#pragma unroll 1
      for (int ob = wave * 4; ob < O; ob += 16) {
        float acc[4][2];
        const float* gq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j][0] = acc[j][1] = 0.f;
          gq[j] = s_g + (ob + j < O ? ob + j : O - 1) * GHH_GP;
        }
#pragma unroll 2
        for (int r = 0; r < GHH_ROWS; r += 4) {
          float gv[4][4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 t = *(const float4*)(gq[j] + r);
            gv[j][0] = t.x; gv[j][1] = t.y; gv[j][2] = t.z; gv[j][3] = t.w;
          }
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float xa = s_x[(r + rr) * GHH_XP + lane], xb = s_x[(r + rr) * GHH_XP + 64 + lane];  // (columns past kc: never stored)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[j][0] = fmaf(gv[j][rr], xa, acc[j][0]);
              acc[j][1] = fmaf(gv[j][rr], xb, acc[j][1]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (ob + j < O) {
            if (lane < kc) pw[(size_t)(ob + j) * Cin + k0 + lane] = acc[j][0];
            if (lane + 64 < kc) pw[(size_t)(ob + j) * Cin + k0 + 64 + lane] = acc[j][1];
          }
        }
      }
    }
  }
}

// the partials of the nblk workgroups, in workgroup order: GH_HEAD_SEGMENTS contiguous runs, each summed in order, then the runs in order
__global__ __launch_bounds__(GHH_BLOCK) void ghh_reduce_kernel(const float* __restrict__ part_W, const float* __restrict__ part_b, int nblk,
                                                               int OC, int O, float* __restrict__ grad_W, float* __restrict__ grad_b) {
  ghr_reduce(
      nblk, OC + O, [&](int i, int el) { return el < OC ? part_W[(size_t)i * OC + el] : part_b[(size_t)i * O + (el - OC)]; },
      [&](int el, float t) { *(el < OC ? grad_W + el : grad_b + (el - OC)) = t; });
}

// ---- host --------------------------------------------------------------------------------------------------------------
static inline int ghh_blocks(int P) { return (P + GHH_ROWS - 1) / GHH_ROWS; }

extern "C" size_t gh_head_workspace_bytes(int P, int Cin, int O) {
  if (P < 1 || Cin < 1 || Cin > GHH_MAX_CIN || O < 11 || O > GH_HEAD_MAX_O || !gha_width_ok(O - 11)) return 0;
  const size_t nb = (size_t)ghh_blocks(P);
  return ghr_align(nb * (size_t)O * (size_t)Cin * sizeof(float)) + ghr_align(nb * (size_t)O * sizeof(float));
}

extern "C" int gh_head_forward(const float* x, int64_t x_stride, int P, int Cin, const float* pts, const float* W, const float* b,
                               const GhHeadDesc* desc, float* xyz, float* scaling, float* rotation, float* opacity, float* shs,
                               float* raw, void* hip_stream) {
  const int rc = gha_check_desc(desc);
  if (rc != GH_OK) return rc;
  if (P < 1 || Cin < 1 || x_stride < Cin) return GH_ERR_INVALID_ARG;
  if (Cin > GHH_MAX_CIN) return GH_ERR_UNSUPPORTED;
  if (!x || !pts || !W || !b || !xyz || !scaling || !rotation || !opacity || !shs) return GH_ERR_INVALID_ARG;
  const int width = desc->shs_width, O = 11 + width;
  const GhaOut out = gha_out(xyz, scaling, rotation, opacity, shs, raw);
  const int vec_x = ghr_al16(x) && Cin % 4 == 0 && x_stride % 4 == 0;
  const size_t lds = (size_t)(GHH_ROWS * GHH_XP + GHH_ROWS * (O | 1)) * sizeof(float);
  const dim3 grid((unsigned)ghh_blocks(P)), block(GHH_BLOCK);
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  ghr_tiles((O + 15) / 16, [&](auto ng) {
    hipLaunchKernelGGL(ghh_fwd_kernel<ng()>, grid, block, lds, s, x, (long long)x_stride, P, Cin, pts, W, b, O, width, desc->flags,
                       desc->clip_scaling, out, vec_x);
  });
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_head_backward(const float* raw, const float* x, int64_t x_stride, int P, int Cin, const float* W,
                                const GhHeadDesc* desc, const float* g_xyz, const float* g_scaling, const float* g_rotation,
                                const float* g_opacity, const float* g_shs, float* grad_x, int64_t gx_stride, float* grad_pts,
                                float* grad_W, float* grad_b, void* workspace, size_t ws_bytes, void* hip_stream) {
  const int rc = gha_check_desc(desc);
  if (rc != GH_OK) return rc;
  if (P < 1 || Cin < 1 || gx_stride < Cin) return GH_ERR_INVALID_ARG;
  if (Cin > GHH_MAX_CIN) return GH_ERR_UNSUPPORTED;
  if (!raw || !W || !grad_x) return GH_ERR_INVALID_ARG;
  if ((grad_W == nullptr) != (grad_b == nullptr)) return GH_ERR_INVALID_ARG;
  const bool wgrad = grad_W != nullptr;
  const int width = desc->shs_width, O = 11 + width, nb = ghh_blocks(P);
  float *part_W = nullptr, *part_b = nullptr;
  if (wgrad) {
    if (!x || x_stride < Cin) return GH_ERR_INVALID_ARG;
    const size_t need = gh_head_workspace_bytes(P, Cin, O);
    if (!workspace || !ghr_al16(workspace)) return GH_ERR_INVALID_ARG;
    if (ws_bytes < need) return GH_ERR_WORKSPACE_SMALL;
    part_W = (float*)workspace;
    part_b = (float*)((char*)workspace + ghr_align((size_t)nb * O * Cin * sizeof(float)));
  }
  const GhaOut g = gha_out(g_xyz, g_scaling, g_rotation, g_opacity, g_shs, nullptr);
  const int vec_x = wgrad && ghr_al16(x) && Cin % 4 == 0 && x_stride % 4 == 0;
  const size_t lds = (size_t)(O * GHH_GP + (wgrad ? GHH_ROWS * GHH_XP : 0)) * sizeof(float);
  const dim3 grid((unsigned)nb), block(GHH_BLOCK);
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
  if (wgrad) {
    hipLaunchKernelGGL(ghh_bwd_kernel<true>, grid, block, lds, s, raw, x, (long long)x_stride, P, Cin, W, O, width, desc->flags,
                       desc->clip_scaling, g, grad_x, (long long)gx_stride, grad_pts, part_W, part_b, vec_x);
    const int OC = O * Cin;
    hipLaunchKernelGGL(ghh_reduce_kernel, dim3(ghr_reduce_blocks(OC + O)), block, 0, s, (const float*)part_W,
                       (const float*)part_b, nb, OC, O, grad_W, grad_b);
  } else {
    hipLaunchKernelGGL(ghh_bwd_kernel<false>, grid, block, lds, s, raw, x, (long long)x_stride, P, Cin, W, O, width, desc->flags,
                       desc->clip_scaling, g, grad_x, (long long)gx_stride, grad_pts, part_W, part_b, vec_x);
  }
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}
