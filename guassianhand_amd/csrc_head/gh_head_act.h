// gh_head_act.h — the Gaussian head's activations (include/gh_head.h), stated once for the kernels that end in them: gh_head.hip and
// csrc_trunk/gh_trunk.hip. Internal: not part of the C-ABI.
//   host      the five outputs' (or cotangents') arrays and which of them take 16-byte stores (GhaOut, gha_out); the descriptor's
//             checks (gha_width_ok, gha_check_desc).
//   device    gha_forward: a tile's pre-activations in LDS -> the five outputs and `raw`, each one contiguous run of the tile;
//             gha_backward: `raw` and the cotangents -> the gradient of the pre-activations in LDS, and grad_pts.
// A caller says where the pre-activation (row, o) of its tile lives in LDS through `at(row, o)`; the formulas know no pitch.
#ifndef GH_HEAD_ACT_H
#define GH_HEAD_ACT_H

#include "../../include/gh_head.h"
#include "../csrc_rows/gh_rows.h"

#define GHA_EPS 1e-12f  // F.normalize's floor

struct GhaOut {  // the contiguous arrays of one direction; vec: which of the forward's outputs take 16-byte stores (the backward reads none)
  float *xyz, *scaling, *rotation, *opacity, *shs, *raw;
  unsigned vec;
};
enum { GHA_V_XYZ = 1, GHA_V_SCALING = 2, GHA_V_ROTATION = 4, GHA_V_OPACITY = 8, GHA_V_SHS = 16, GHA_V_RAW = 32 };

static inline GhaOut gha_out(const float* xyz, const float* scaling, const float* rotation, const float* opacity, const float* shs,
                             const float* raw) {
  GhaOut o = {(float*)xyz, (float*)scaling, (float*)rotation, (float*)opacity, (float*)shs, (float*)raw, 0u};
  o.vec = (ghr_al16(xyz) ? GHA_V_XYZ : 0u) | (ghr_al16(scaling) ? GHA_V_SCALING : 0u) | (ghr_al16(rotation) ? GHA_V_ROTATION : 0u) |
          (ghr_al16(opacity) ? GHA_V_OPACITY : 0u) | (ghr_al16(shs) ? GHA_V_SHS : 0u) | (raw && ghr_al16(raw) ? GHA_V_RAW : 0u);
  return o;
}

static inline bool gha_width_ok(int w) { return w == 3 || w == 12 || w == 27 || w == 48; }

static inline int gha_check_desc(const GhHeadDesc* d) {
  if (!d) return GH_ERR_INVALID_ARG;
  if (!gha_width_ok(d->shs_width)) return GH_ERR_UNSUPPORTED;
  if (d->flags & ~(GH_HEAD_USE_RGB | GH_HEAD_XYZ_OFFSET | GH_HEAD_RESTRICT_OFFSET | GH_HEAD_CLIP_SCALING)) return GH_ERR_INVALID_ARG;
  if ((d->flags & GH_HEAD_USE_RGB) && d->shs_width != 3) return GH_ERR_UNSUPPORTED;
  if ((d->flags & GH_HEAD_CLIP_SCALING) && !(d->clip_scaling >= 0.f)) return GH_ERR_INVALID_ARG;
  return GH_OK;
}

// The forward's epilogue, after the barrier behind the last write of s: the tile's R rows from row0, nrows of them inside P, their O
// pre-activations at s[at(row, o)]. Every output's tile is one contiguous run.
template <int R, class At>
__device__ __forceinline__ void gha_forward(const float* s, At at, const GhaOut& out, const float* __restrict__ pts, long long row0, int nrows,
                                            int O, int width, unsigned flags, float clip, int tid) {
  static_assert(R <= GHR_BLOCK, "one thread per row normalises the rotation");
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32);
  const float* pt = pts + row0 * 3;
  ghr_store_run(out.xyz + row0 * 3, nrows * 3, out.vec & GHA_V_XYZ, tid, [&](int e) {
    const float p = pt[e];
    if (!xyz_off) return p;
    const int r = e / 3;
    float v = s[at(r, e - 3 * r)];
    if (restrict_off) v = (ghr_sigmoid(v) - 0.5f) * max_step;
    return v + p;
  });
  ghr_store_run(out.scaling + row0 * 3, nrows * 3, out.vec & GHA_V_SCALING, tid, [&](int e) {
    const int r = e / 3;
    float v = expf(s[at(r, 3 + (e - 3 * r))]);
    if (clipped) v = fminf(fmaxf(v, 0.f), clip);
    return v;
  });
  if (tid < nrows) {
    const float a = s[at(tid, 6)], bq = s[at(tid, 7)], c = s[at(tid, 8)], d = s[at(tid, 9)];
    const float den = fmaxf(sqrtf(((a * a + bq * bq) + c * c) + d * d), GHA_EPS);
    float* dst = out.rotation + (row0 + tid) * 4;
    if (out.vec & GHA_V_ROTATION) {
      *(float4*)dst = make_float4(a / den, bq / den, c / den, d / den);
    } else {
      dst[0] = a / den; dst[1] = bq / den; dst[2] = c / den; dst[3] = d / den;
    }
  }
  ghr_store_run(out.opacity + row0, nrows, out.vec & GHA_V_OPACITY, tid, [&](int e) { return ghr_sigmoid(s[at(e, 10)]); });
  ghr_store_run(out.shs + row0 * width, nrows * width, out.vec & GHA_V_SHS, tid, [&](int e) {
    const int r = e / width;
    const float v = s[at(r, 11 + (e - r * width))];
    return use_rgb ? ghr_sigmoid(v) : v;
  });
  if (out.raw) {
    ghr_store_run(out.raw + row0 * O, nrows * O, out.vec & GHA_V_RAW, tid, [&](int e) {
      const int r = e / O;
      return s[at(r, e - r * O)];
    });
  }
}

// The backward's prologue: the gradient of the pre-activation (row, o) goes to s[at(row, o)] for all R rows of the tile and every
// o < O; rows past the end are zeros (they enter a tile's sums). g holds the cotangents, null where an output was not used; grad_pts
// (or null) takes the cotangent of xyz. The caller's barrier follows.
template <int R, class At>
__device__ __forceinline__ void gha_backward(float* s, At at, const GhaOut& g, const float* __restrict__ raw, float* __restrict__ grad_pts,
                                             long long row0, int nrows, int O, int width, unsigned flags, float clip, int tid) {
  static_assert(R <= GHR_BLOCK, "one thread per row for the rotation and the opacity");
  const bool use_rgb = flags & GH_HEAD_USE_RGB, xyz_off = flags & GH_HEAD_XYZ_OFFSET, restrict_off = flags & GH_HEAD_RESTRICT_OFFSET,
             clipped = flags & GH_HEAD_CLIP_SCALING;
  const float max_step = (float)(1.2 / 32);
  const float* rt = raw + row0 * O;
  for (int e = tid; e < R * 3; e += GHR_BLOCK) {
    const int r = e / 3, c = e - 3 * r;
    float gx = 0.f, gs = 0.f;
    if (r < nrows) {
      const float go = g.xyz ? g.xyz[row0 * 3 + e] : 0.f;
      if (grad_pts) grad_pts[row0 * 3 + e] = go;
      if (xyz_off) {
        gx = go;
        if (restrict_off) {
          const float sg = ghr_sigmoid(rt[r * O + c]);
          gx = ((go * max_step) * (1.0f - sg)) * sg;
        }
      }
      if (g.scaling) {
        const float v = rt[r * O + 3 + c], ev = expf(v);
        const bool pass = !clipped || (ev >= 0.f && ev <= clip);
        gs = pass ? g.scaling[row0 * 3 + e] * expf(fminf(v, 15.0f)) : 0.f;
      }
    }
    s[at(r, c)] = gx;
    s[at(r, 3 + c)] = gs;
  }
  if (tid < R) {
    const int r = tid;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, gop = 0.f;
    if (r < nrows) {
      if (g.rotation) {
        const float* v = rt + r * O + 6;
        const float* gr = g.rotation + (row0 + r) * 4;
        const float a = v[0], bq = v[1], c = v[2], d = v[3];
        const float g0 = gr[0], g1 = gr[1], g2 = gr[2], g3 = gr[3];
        const float n = sqrtf(((a * a + bq * bq) + c * c) + d * d);
        if (n >= GHA_EPS) {
          const float n0 = a / n, n1 = bq / n, n2 = c / n, n3 = d / n;
          const float dot = ((n0 * g0 + n1 * g1) + n2 * g2) + n3 * g3;
          o0 = (g0 - n0 * dot) / n; o1 = (g1 - n1 * dot) / n; o2 = (g2 - n2 * dot) / n; o3 = (g3 - n3 * dot) / n;
        } else {  // below the floor the denominator is the constant
          o0 = g0 / GHA_EPS; o1 = g1 / GHA_EPS; o2 = g2 / GHA_EPS; o3 = g3 / GHA_EPS;
        }
      }
      if (g.opacity) {
        const float sg = ghr_sigmoid(rt[r * O + 10]);
        gop = (g.opacity[row0 + r] * (1.0f - sg)) * sg;
      }
    }
    s[at(r, 6)] = o0; s[at(r, 7)] = o1; s[at(r, 8)] = o2; s[at(r, 9)] = o3;
    s[at(r, 10)] = gop;
  }
  for (int e = tid; e < R * width; e += GHR_BLOCK) {
    const int r = e / width, c = e - r * width;
    float gv = 0.f;
    if (r < nrows && g.shs) {
      gv = g.shs[row0 * width + e];
      if (use_rgb) {
        const float sg = ghr_sigmoid(rt[r * O + 11 + c]);
        gv = (gv * (1.0f - sg)) * sg;
      }
    }
    s[at(r, 11 + c)] = gv;
  }
}

#endif
