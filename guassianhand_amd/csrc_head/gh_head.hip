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
#include "../../include/gh_head.h"
#include "../csrc_rows/gh_rows.h"

#define GHH_BLOCK GHR_BLOCK
#define GHH_ROWS GH_HEAD_ROWS
#define GHH_KC 128             // feature columns per pass through LDS
#define GHH_XP (GHH_KC + 1)    // pitch of the x tile: odd, so lane = row is conflict-free
#define GHH_GP (GHH_ROWS + 4)  // pitch of the transposed gradient tile: 16-byte aligned rows
#define GHH_EPS 1e-12f         // F.normalize's floor
#define GHH_MAX_CIN (1 << 20)  // O * Cin stays far inside an int

static_assert(GHH_ROWS == 64 && GHH_BLOCK == 4 * GHH_ROWS, "lane = row in the forward; 16 rows per wave in the backward");
static_assert(GH_HEAD_SEGMENTS == GHR_SEGMENTS, "the header documents the shared reduction's run count");

struct GhhOut {  // the contiguous arrays of one direction, and which of them may be accessed 16 bytes at a time
  float *xyz, *scaling, *rotation, *opacity, *shs, *raw;
  unsigned vec;
};
enum { GHH_V_XYZ = 1, GHH_V_SCALING = 2, GHH_V_ROTATION = 4, GHH_V_OPACITY = 8, GHH_V_SHS = 16, GHH_V_RAW = 32 };

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int NG>  // groups of 16 outputs: ceil(O / 16)
__global__ __launch_bounds__(GHH_BLOCK) void ghh_fwd_kernel(const float* __restrict__ x, long long x_stride, int P, int Cin,
                                                            const float* __restrict__ pts, const float* __restrict__ W,
                                                            const float* __restrict__ b, int O, int width, unsigned flags, float clip,
                                                            GhhOut out, int vec_x) {
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

  // ---- activations: every output's tile is one contiguous run ----
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32);
  const float* pt = pts + row0 * 3;
  ghr_store_run(out.xyz + row0 * 3, nrows * 3, out.vec & GHH_V_XYZ, tid, [&](int e) {
    const float p = pt[e];
    if (!xyz_off) return p;
    const int r = e / 3;
    float v = s_raw[r * RP + (e - 3 * r)];
    if (restrict_off) v = (ghr_sigmoid(v) - 0.5f) * max_step;
    return v + p;
  });
  ghr_store_run(out.scaling + row0 * 3, nrows * 3, out.vec & GHH_V_SCALING, tid, [&](int e) {
    const int r = e / 3;
    float s = expf(s_raw[r * RP + 3 + (e - 3 * r)]);
    if (clipped) s = fminf(fmaxf(s, 0.f), clip);
    return s;
  });
  if (tid < nrows) {
    const float* v = s_raw + tid * RP + 6;
    const float a = v[0], bq = v[1], c = v[2], d = v[3];
    const float den = fmaxf(sqrtf(((a * a + bq * bq) + c * c) + d * d), GHH_EPS);
    float* dst = out.rotation + (row0 + tid) * 4;
    if (out.vec & GHH_V_ROTATION) {
      *(float4*)dst = make_float4(a / den, bq / den, c / den, d / den);
    } else {
      dst[0] = a / den; dst[1] = bq / den; dst[2] = c / den; dst[3] = d / den;
    }
  }
  ghr_store_run(out.opacity + row0, nrows, out.vec & GHH_V_OPACITY, tid, [&](int e) { return ghr_sigmoid(s_raw[e * RP + 10]); });
  ghr_store_run(out.shs + row0 * width, nrows * width, out.vec & GHH_V_SHS, tid, [&](int e) {
    const int r = e / width;
    const float v = s_raw[r * RP + 11 + (e - r * width)];
    return use_rgb ? ghr_sigmoid(v) : v;
  });
  if (out.raw) {
    ghr_store_run(out.raw + row0 * O, nrows * O, out.vec & GHH_V_RAW, tid, [&](int e) {
      const int r = e / O;
      return s_raw[r * RP + (e - r * O)];
    });
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
template <bool WGRAD>
__global__ __launch_bounds__(GHH_BLOCK) void ghh_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ x,
                                                            long long x_stride, int P, int Cin, const float* __restrict__ W, int O,
                                                            int width, unsigned flags, float clip, GhhOut g /* the output gradients */,
                                                            float* __restrict__ grad_x, long long gx_stride, float* __restrict__ grad_pts,
                                                            float* __restrict__ part_W, float* __restrict__ part_b, int vec_x) {
  extern __shared__ __attribute__((aligned(16))) float ghh_smem[];
  float* s_g = ghh_smem;                // O x GHH_GP: the gradient of raw[row, o] at s_g[o * GHH_GP + row]
  float* s_x = ghh_smem + O * GHH_GP;   // WGRAD: GHH_ROWS x GHH_XP
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long row0 = (long long)blockIdx.x * GHH_ROWS;
  const int nrows = (int)((long long)P - row0 < GHH_ROWS ? (long long)P - row0 : GHH_ROWS);
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32);
  const float* rt = raw + row0 * O;

  // ---- the gradient of the pre-activations; rows past the end are zeros (they enter the tile's sums of grad_W) ----
  for (int e = tid; e < GHH_ROWS * 3; e += GHH_BLOCK) {
    const int r = e / 3, c = e - 3 * r;
    float gx = 0.f, gs = 0.f;
    if (r < nrows) {
      const float go = g.xyz ? g.xyz[row0 * 3 + e] : 0.f;
      if (grad_pts) grad_pts[row0 * 3 + e] = go;
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
    s_g[c * GHH_GP + r] = gx;
    s_g[(3 + c) * GHH_GP + r] = gs;
  }
  if (tid < GHH_ROWS) {
    const int r = tid;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, gop = 0.f;
    if (r < nrows) {
      if (g.rotation) {
        const float* v = rt + r * O + 6;
        const float* gr = g.rotation + (row0 + r) * 4;
        const float a = v[0], bq = v[1], c = v[2], d = v[3];
        const float g0 = gr[0], g1 = gr[1], g2 = gr[2], g3 = gr[3];
        const float n = sqrtf(((a * a + bq * bq) + c * c) + d * d);
        if (n >= GHH_EPS) {
          const float n0 = a / n, n1 = bq / n, n2 = c / n, n3 = d / n;
          const float dot = ((n0 * g0 + n1 * g1) + n2 * g2) + n3 * g3;
          o0 = (g0 - n0 * dot) / n; o1 = (g1 - n1 * dot) / n; o2 = (g2 - n2 * dot) / n; o3 = (g3 - n3 * dot) / n;
        } else {  // below the floor the denominator is the constant
          o0 = g0 / GHH_EPS; o1 = g1 / GHH_EPS; o2 = g2 / GHH_EPS; o3 = g3 / GHH_EPS;
        }
      }
      if (g.opacity) {
        const float s = ghr_sigmoid(rt[r * O + 10]);
        gop = (g.opacity[row0 + r] * (1.0f - s)) * s;
      }
    }
    s_g[6 * GHH_GP + r] = o0; s_g[7 * GHH_GP + r] = o1; s_g[8 * GHH_GP + r] = o2; s_g[9 * GHH_GP + r] = o3;
    s_g[10 * GHH_GP + r] = gop;
  }
  for (int e = tid; e < GHH_ROWS * width; e += GHH_BLOCK) {
    const int r = e / width, c = e - r * width;
    float gv = 0.f;
    if (r < nrows && g.shs) {
      gv = g.shs[row0 * width + e];
      if (use_rgb) {
        const float s = ghr_sigmoid(rt[r * O + 11 + c]);
        gv = (gv * (1.0f - s)) * s;
      }
    }
    s_g[(11 + c) * GHH_GP + r] = gv;
  }
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
static bool ghh_width_ok(int w) { return w == 3 || w == 12 || w == 27 || w == 48; }
static inline int ghh_blocks(int P) { return (P + GHH_ROWS - 1) / GHH_ROWS; }

static int ghh_check_desc(const GhHeadDesc* d) {
  if (!d) return GH_ERR_INVALID_ARG;
  if (!ghh_width_ok(d->shs_width)) return GH_ERR_UNSUPPORTED;
  if (d->flags & ~(GH_HEAD_USE_RGB | GH_HEAD_XYZ_OFFSET | GH_HEAD_RESTRICT_OFFSET | GH_HEAD_CLIP_SCALING)) return GH_ERR_INVALID_ARG;
  if ((d->flags & GH_HEAD_USE_RGB) && d->shs_width != 3) return GH_ERR_UNSUPPORTED;
  if ((d->flags & GH_HEAD_CLIP_SCALING) && !(d->clip_scaling >= 0.f)) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

extern "C" size_t gh_head_workspace_bytes(int P, int Cin, int O) {
  if (P < 1 || Cin < 1 || Cin > GHH_MAX_CIN || O < 11 || O > GH_HEAD_MAX_O || !ghh_width_ok(O - 11)) return 0;
  const size_t nb = (size_t)ghh_blocks(P);
  return ghr_align(nb * (size_t)O * (size_t)Cin * sizeof(float)) + ghr_align(nb * (size_t)O * sizeof(float));
}

extern "C" int gh_head_forward(const float* x, int64_t x_stride, int P, int Cin, const float* pts, const float* W, const float* b,
                               const GhHeadDesc* desc, float* xyz, float* scaling, float* rotation, float* opacity, float* shs,
                               float* raw, void* hip_stream) {
  const int rc = ghh_check_desc(desc);
  if (rc != GH_OK) return rc;
  if (P < 1 || Cin < 1 || x_stride < Cin) return GH_ERR_INVALID_ARG;
  if (Cin > GHH_MAX_CIN) return GH_ERR_UNSUPPORTED;
  if (!x || !pts || !W || !b || !xyz || !scaling || !rotation || !opacity || !shs) return GH_ERR_INVALID_ARG;
  const int width = desc->shs_width, O = 11 + width;
  GhhOut out = {xyz, scaling, rotation, opacity, shs, raw, 0u};
  out.vec = (ghr_al16(xyz) ? GHH_V_XYZ : 0u) | (ghr_al16(scaling) ? GHH_V_SCALING : 0u) | (ghr_al16(rotation) ? GHH_V_ROTATION : 0u) |
            (ghr_al16(opacity) ? GHH_V_OPACITY : 0u) | (ghr_al16(shs) ? GHH_V_SHS : 0u) | (raw && ghr_al16(raw) ? GHH_V_RAW : 0u);
  const int vec_x = ghr_al16(x) && Cin % 4 == 0 && x_stride % 4 == 0;
  const size_t lds = (size_t)(GHH_ROWS * GHH_XP + GHH_ROWS * (O | 1)) * sizeof(float);
  const dim3 grid((unsigned)ghh_blocks(P)), block(GHH_BLOCK);
  hipStream_t s = (hipStream_t)hip_stream;
  (void)hipGetLastError();
#define GHH_FWD(NG)                                                                                                               \
  hipLaunchKernelGGL(ghh_fwd_kernel<NG>, grid, block, lds, s, x, (long long)x_stride, P, Cin, pts, W, b, O, width, desc->flags, \
                     desc->clip_scaling, out, vec_x)
  switch ((O + 15) / 16) {
    case 1: GHH_FWD(1); break;
    case 2: GHH_FWD(2); break;
    case 3: GHH_FWD(3); break;
    default: GHH_FWD(4); break;
  }
#undef GHH_FWD
  return hipGetLastError() == hipSuccess ? GH_OK : GH_ERR_LAUNCH;
}

extern "C" int gh_head_backward(const float* raw, const float* x, int64_t x_stride, int P, int Cin, const float* W,
                                const GhHeadDesc* desc, const float* g_xyz, const float* g_scaling, const float* g_rotation,
                                const float* g_opacity, const float* g_shs, float* grad_x, int64_t gx_stride, float* grad_pts,
                                float* grad_W, float* grad_b, void* workspace, size_t ws_bytes, void* hip_stream) {
  const int rc = ghh_check_desc(desc);
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
  GhhOut g = {(float*)g_xyz, (float*)g_scaling, (float*)g_rotation, (float*)g_opacity, (float*)g_shs, nullptr, 0u};
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
