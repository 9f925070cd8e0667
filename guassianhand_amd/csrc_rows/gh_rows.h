// gh_rows.h — what the row-tile blocks (csrc_head/gh_head.hip, csrc_vert/gh_vert.hip, csrc_cond/gh_cond.hip) share. Internal: not part
// of the C-ABI.
//   tile      one 4-wave workgroup per 64 rows; the rows' feature columns cross LDS at an odd pitch, so that lane = row reads its own
//             row without a bank conflict (ghr_stage, head and vert; cond builds its rows there). ghr_tile is the prologue of the vert
//             and cond kernels.
//   layers    vert and cond: the LayerNorm's moments (ghr_moments), row . W^T (ghr_linear) and g . W (ghr_linear_t) for the lane's row
//             with wave-uniform weights, the four waves' partial sums through ghr_sum4. The caller supplies how an input column is read
//             and where a sum goes; the routines know no block.
//   reduce    the per-workgroup partials of a backward are summed by a second launch, GHR_RED_EL elements x GHR_SEGMENTS runs per
//             workgroup: a run is summed in workgroup order, then the runs in run order (ghr_reduce; head and vert).
//   host      ghr_allow_lds (vert, cond): more than 64 KB of dynamic LDS, told to the runtime once per kernel.
//   walk      pool and res: a wave walks a run of a plan's `order`, four rows in flight (ghr_walk, ghr_walk_store); ghr_part cuts a
//             cell's list into the four waves' quarters.
//   slabs     res and trunk: a window of a weight matrix on its way into LDS, every load issued before the barrier (ghr_fetch,
//             ghr_fetch_in for a window that reaches past the matrix, ghr_put). head and trunk: a tile's contiguous run of an output
//             (ghr_store_run).
//   columns   res, trunk, scene and attn: the 32x32x2 float32 matrix-instruction product with the point as the column — the accumulator
//             and its register-to-row map (ghr_acc, ghr_acc_row). res and trunk: a set of accumulators filled with a bias or zeros
//             (ghr_fill), and the products of a weight matrix that crosses LDS in slabs with an operand from memory (ghr_mm_x,
//             ghr_mm_tg) or from the previous product's accumulators (ghr_mm, ghr_mm_t), the window whole or bounded at compile
//             time. res: whole tiles stored to the lane's row (ghr_store_tiles). ghr_tiles is the host's switch into a kernel
//             template's tile count.
// gh_pool.hip and gh_metrics.hip take ghr_align from here; gh_attn.hip takes ghr_stage. csrc_attn_rows/gh_attn_rows.hip takes the tile,
// the layers and ghr_allow_lds, and gathers its rows through a list (ghr_stage_rows). ghr_al4 is every block's test of a float pointer.
// csrc_conv/gh_conv.hip and csrc_lpips/gh_lpips.hip take the slabs (ghr_fetch_in, ghr_put, GHR_WP) and the accumulator map for their
// own convolution products, whose operand gather is theirs.
#ifndef GH_ROWS_H
#define GH_ROWS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#define GHR_BLOCK 256
#define GHR_ROWS 64      // rows per tile: lane = row
#define GHR_SEGMENTS 16  // runs of partials (GH_HEAD_SEGMENTS, GH_VERT_SEGMENTS)
#define GHR_RED_EL 16    // elements per workgroup of the reduction

static_assert(GHR_SEGMENTS * GHR_RED_EL == GHR_BLOCK, "one thread per (run, element) of the reduction");
static_assert(GHR_BLOCK == 4 * GHR_ROWS, "lane = row, four waves share a row's columns");

static inline size_t ghr_align(size_t x) { return (x + 255) & ~(size_t)255; }  // workspace parts start on 256 bytes
static inline bool ghr_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static inline bool ghr_al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }  // a float array (null passes)

__device__ __forceinline__ float ghr_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// columns [k0, k0 + kc) of the tile's R rows -> s[row * pitch + col]; rows past the end of x are zeros.
// vec: x is 16-byte aligned and its width and x_stride are multiples of 4 — so is every row, and so are k0 and kc.
__device__ __forceinline__ void ghr_stage(float* s, int pitch, const float* __restrict__ x, long long x_stride, long long row0, int R,
                                          int nrows, int k0, int kc, int vec, int tid) {
  if (vec) {
    const int q = kc >> 2;
    for (int i = tid; i < R * q; i += GHR_BLOCK) {
      const int r = i / q, c = 4 * (i - r * q);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nrows) v = *(const float4*)(x + (row0 + r) * x_stride + k0 + c);
      float* d = s + r * pitch + c;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    for (int i = tid; i < R * kc; i += GHR_BLOCK) {
      const int r = i / kc, c = i - r * kc;
      s[r * pitch + c] = r < nrows ? x[(row0 + r) * x_stride + k0 + c] : 0.f;
    }
  }
}

// ghr_stage through a row list (attn_rows): tile row r is row idx[row0 + r] of x, or row row0 + r where idx is null; all kc columns
// from column 0. Scalar loads: the start of a listed row has no alignment to count on.
__device__ __forceinline__ void ghr_stage_rows(float* s, int pitch, const float* __restrict__ x, long long x_stride,
                                               const int* __restrict__ idx, long long row0, int R, int nrows, int kc, int tid) {
  for (int i = tid; i < R * kc; i += GHR_BLOCK) {
    const int r = i / kc, c = i - r * kc;
    float v = 0.f;
    if (r < nrows) {
      const long long src = idx ? (long long)idx[row0 + r] : row0 + r;
      v = x[src * x_stride + c];
    }
    s[r * pitch + c] = v;
  }
}

// The body of a reduce kernel (GHR_BLOCK threads). Element el of n is store(el, t), t the sum of load(i, el) over the nblk
// workgroups' partials i: GHR_SEGMENTS contiguous runs of i, each summed in ascending i, then the runs in run order.
template <class Load, class Store>
__device__ __forceinline__ void ghr_reduce(int nblk, int n, Load load, Store store) {
  __shared__ float s_red[GHR_SEGMENTS][GHR_RED_EL];
  const int tid = threadIdx.x, el = blockIdx.x * GHR_RED_EL + (tid & (GHR_RED_EL - 1)), seg = tid / GHR_RED_EL;
  const int per = (nblk + GHR_SEGMENTS - 1) / GHR_SEGMENTS;
  const int lo = seg * per, hi = lo + per < nblk ? lo + per : nblk;
  float s = 0.f;
  if (el < n) {
    for (int i = lo; i < hi; ++i) s += load(i, el);
  }
  s_red[seg][tid & (GHR_RED_EL - 1)] = s;
  __syncthreads();
  if (tid < GHR_RED_EL && el < n) {
    float t = 0.f;
    for (int q = 0; q < GHR_SEGMENTS; ++q) t += s_red[q][tid];
    store(el, t);
  }
}

static inline unsigned ghr_reduce_blocks(int n) { return (unsigned)((n + GHR_RED_EL - 1) / GHR_RED_EL); }

// ---- the LayerNorm-MLP row kernels (vert, cond) -----------------------------------------------------------------------------------
// a row kernel's prologue: workgroup b works on the rows [row0, row0 + nrows) of P, R of them but for the last; `lane` is the
// thread's row in the tile (R = 32: lanes l and l + 32 share one), `wave` is wave-uniform
struct GhrTile {
  int tid, lane, wave, nrows;
  long long row0;
};

template <int R>
__device__ __forceinline__ GhrTile ghr_tile(int P) {
  GhrTile t;
  t.tid = threadIdx.x;
  t.lane = t.tid & (R - 1);
  t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
  t.row0 = (long long)blockIdx.x * R;
  t.nrows = (int)((long long)P - t.row0 < R ? (long long)P - t.row0 : R);
  return t;
}

// (s0 + s1) + (s2 + s3) of the four waves' partial sums of the lane's row
__device__ __forceinline__ float ghr_sum4(const float* s_red, int lane) {
  return (s_red[lane] + s_red[GHR_ROWS + lane]) + (s_red[2 * GHR_ROWS + lane] + s_red[3 * GHR_ROWS + lane]);
}

struct GhrMoments { float mean, m2; };  // m2: the sum of the squared deviations from the mean

// the moments of the n columns of the lane's row vr: wave w sums the columns k = w mod 4 in ascending order, the four shares are added
// by ghr_sum4. The first pass's mean carries the rounding of a sum of n values, a few ulp of the mean itself — all of the deviation of a
// row whose mean dwarfs it — so the second pass also sums the deviations from it: their mean corrects the first, and m2 is taken about
// the corrected mean (sum d^2 - (sum d)^2 / n). s_red is 2 x GHR_BLOCK floats; three barriers, so every thread of the workgroup calls it.
// Its last reads touch both halves of s_red: a caller puts a barrier before it writes either half again.
__device__ __forceinline__ GhrMoments ghr_moments(const float* vr, int n, float* s_red, int lane, int wave) {
  GhrMoments r;
  float s = 0.f;
  for (int k = wave; k < n; k += 4) s += vr[k];
  s_red[wave * GHR_ROWS + lane] = s;
  __syncthreads();
  const float mean = ghr_sum4(s_red, lane) / (float)n;
  float q = 0.f, e = 0.f;
  for (int k = wave; k < n; k += 4) {
    const float d = vr[k] - mean;
    e += d;
    q = fmaf(d, d, q);
  }
  s_red[GHR_BLOCK + wave * GHR_ROWS + lane] = q;
  __syncthreads();  // (every read of the first half lies before this barrier: it is free for the deviations' sums)
  s_red[wave * GHR_ROWS + lane] = e;
  __syncthreads();
  const float es = ghr_sum4(s_red, lane), c = es / (float)n;
  r.mean = mean + c;
  const float m2 = fmaf(-es, c, ghr_sum4(s_red + GHR_BLOCK, lane));
  r.m2 = m2 < 0.f ? 0.f : m2;  // (the difference can round below 0 where every deviation is the same; a NaN stays)
  return r;
}

// emit(j, sum_k in(k) * W[j, k]) for the lane's row, W (m, n): four partial sums (k mod 4), one fmaf per term, (s0 + s1) + (s2 + s3).
// Wave w owns j = w, w + 4, ..., three at a time: one read of the input against three fmaf with a wave-uniform weight.
template <class In, class Emit>
__device__ __forceinline__ void ghr_linear(int n, const float* __restrict__ W, int m, int wave, In in, Emit emit) {
  const int n4 = n & ~3, tail = n & 3;
  for (int j0 = wave; j0 < m; j0 += 12) {
    const float* w[3];
    float acc[3][4];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int j = j0 + 4 * u;
      w[u] = W + (size_t)(j < m ? j : m - 1) * n;  // (outputs past m are computed and dropped)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[u][s] = 0.f;
    }
#pragma unroll 2
    for (int k = 0; k < n4; k += 4) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float xv = in(k + s);
#pragma unroll
        for (int u = 0; u < 3; ++u) acc[u][s] = fmaf(xv, w[u][k + s], acc[u][s]);
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {  // column n4 + s belongs to partial sum s
      if (s < tail) {
        const float xv = in(n4 + s);
#pragma unroll
        for (int u = 0; u < 3; ++u) acc[u][s] = fmaf(xv, w[u][n4 + s], acc[u][s]);
      }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int j = j0 + 4 * u;
      if (j < m) emit(j, (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]));
    }
  }
}

// emit(k, sum_i gr[i] * W[i, k]) for the lane's row, W (m, ncols): one chain of fmaf in ascending i; wave w owns k = 16t + 4w .. 16t + 4w + 3
template <class Emit>
__device__ __forceinline__ void ghr_linear_t(const float* gr, int m, const float* __restrict__ W, int ncols, int wave, Emit emit) {
  for (int k0 = 4 * wave; k0 < ncols; k0 += 16) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (k0 + 4 <= ncols) {
#pragma unroll 2
      for (int i = 0; i < m; ++i) {
        const float g = gr[i];
        const float* wr = W + (size_t)i * ncols + k0;
        a0 = fmaf(g, wr[0], a0); a1 = fmaf(g, wr[1], a1); a2 = fmaf(g, wr[2], a2); a3 = fmaf(g, wr[3], a3);
      }
    } else {  // the last, partial block: columns past the end repeat the last one and are dropped
      const int c1 = k0 + 1 < ncols ? 1 : 0, c2 = k0 + 2 < ncols ? 2 : c1;
      for (int i = 0; i < m; ++i) {
        const float g = gr[i];
        const float* wr = W + (size_t)i * ncols + k0;
        a0 = fmaf(g, wr[0], a0); a1 = fmaf(g, wr[c1], a1); a2 = fmaf(g, wr[c2], a2);
      }
    }
    emit(k0, a0);
    if (k0 + 1 < ncols) emit(k0 + 1, a1);
    if (k0 + 2 < ncols) emit(k0 + 2, a2);
    if (k0 + 3 < ncols) emit(k0 + 3, a3);
  }
}

// ---- walking a run of a pooling plan's `order` (pool, res) ------------------------------------------------------------------------------
// Calls f(point) for order[lo .. hi) in ascending position, 64 list entries fetched by one coalesced load and handed out by
// v_readlane, four rows per step so that four loads are in flight. lo, hi are wave-uniform.
template <typename Load, typename Use>
__device__ __forceinline__ void ghr_walk(const int* __restrict__ order, int lo, int hi, Load load, Use use) {
  const int lane = threadIdx.x & 63;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int m = min(64, hi - j0);
    const int mine = lane < m ? order[j0 + lane] : 0;
    int k = 0;
    for (; k + 4 <= m; k += 4) {
      const int p0 = __builtin_amdgcn_readlane(mine, k), p1 = __builtin_amdgcn_readlane(mine, k + 1);
      const int p2 = __builtin_amdgcn_readlane(mine, k + 2), p3 = __builtin_amdgcn_readlane(mine, k + 3);
      const float v0 = load(p0), v1 = load(p1), v2 = load(p2), v3 = load(p3);
      use(p0, v0); use(p1, v1); use(p2, v2); use(p3, v3);
    }
    for (; k < m; ++k) {
      const int p = __builtin_amdgcn_readlane(mine, k);
      use(p, load(p));
    }
  }
}

// the same walk for a pass that only writes
template <typename Store>
__device__ __forceinline__ void ghr_walk_store(const int* __restrict__ order, int lo, int hi, Store store) {
  const int lane = threadIdx.x & 63;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int m = min(64, hi - j0);
    const int mine = lane < m ? order[j0 + lane] : 0;
    for (int k = 0; k < m; ++k) store(__builtin_amdgcn_readlane(mine, k));
  }
}

__device__ __forceinline__ int ghr_part(int a, int n, int w) { return a + (int)((long long)n * w / (GHR_BLOCK / 64)); }

// ---- weight slabs of the matrix-instruction row kernels (res, trunk) ------------------------------------------------------------------
// One matrix window on its way into LDS: element (r, c) of the window W[row0 + r][col0 + c] goes to s[r * pitch + c]. The window has
// 4 Q columns and IT * GHR_BLOCK / Q rows, a thread moves IT runs of four floats. vec: W is 16-byte aligned and stride and col0 are
// multiples of 4. ghr_fetch issues every load of the window before anything waits for one; ghr_put writes what it brought.
template <int IT, int Q>
struct GhrSlab {
  float v[IT][4];
};

template <int IT, int Q>
__device__ __forceinline__ void ghr_fetch(GhrSlab<IT, Q>& t, const float* __restrict__ W, long long stride, int row0, int col0, int vec, int tid) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int i = tid + it * GHR_BLOCK, r = i / Q, c = 4 * (i % Q);
    const float* src = W + (long long)(row0 + r) * stride + col0 + c;
    if (vec) {
      const float4 v = *(const float4*)src;
      t.v[it][0] = v.x; t.v[it][1] = v.y; t.v[it][2] = v.z; t.v[it][3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) t.v[it][j] = src[j];
    }
  }
}

// ghr_fetch of a window that may reach past the matrix: W has nrows rows of ncols columns, and what lies outside arrives as zeros
template <int IT, int Q>
__device__ __forceinline__ void ghr_fetch_in(GhrSlab<IT, Q>& t, const float* __restrict__ W, long long stride, int row0, int col0, int nrows,
                                             int ncols, int vec, int tid) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int i = tid + it * GHR_BLOCK, r = row0 + i / Q, c = col0 + 4 * (i % Q);
    const float* src = W + (long long)r * stride + c;
    if (vec && r < nrows && c + 4 <= ncols) {
      const float4 v = *(const float4*)src;
      t.v[it][0] = v.x; t.v[it][1] = v.y; t.v[it][2] = v.z; t.v[it][3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) t.v[it][j] = (r < nrows && c + j < ncols) ? src[j] : 0.f;
    }
  }
}

template <int IT, int Q>
__device__ __forceinline__ void ghr_put(const GhrSlab<IT, Q>& t, float* s, int pitch, int tid) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int i = tid + it * GHR_BLOCK, r = i / Q, c = 4 * (i % Q);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[r * pitch + c + j] = t.v[it][j];
  }
}

// n floats of a tile's contiguous run of an output (head, trunk): 16-byte stores where the run's base allows, the tail element by element
template <class F>
__device__ __forceinline__ void ghr_store_run(float* __restrict__ dst, int n, bool vec, int tid, F f) {
  if (vec) {
    for (int q = tid; 4 * q < n; q += GHR_BLOCK) {
      const int e = 4 * q;
      if (e + 4 <= n) {
        *(float4*)(dst + e) = make_float4(f(e), f(e + 1), f(e + 2), f(e + 3));
      } else {
        for (int j = e; j < n; ++j) dst[j] = f(j);
      }
    }
  } else {
    for (int e = tid; e < n; e += GHR_BLOCK) dst[e] = f(e);
  }
}

// ---- columns: the 32x32x2 float32 matrix-instruction product with the point as the column (res, trunk; scene and attn: the map) -------
// v_mfma_f32_32x32x2_f32, D[i][j] = fma chain over k of A[i][k] * B[k][j]: lane l gives A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31], one float each, and holds column col = l & 31 of D; with half = l >> 5 its register r is row
// ghr_acc_row(r, half). A wave owns 32 points, lane l the point col; tiles of 32 channels are accumulators.
typedef float ghr_acc __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int ghr_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <int NT>
__device__ __forceinline__ void ghr_fill(ghr_acc (&h)[NT], const float* __restrict__ b, int half) {  // b: the bias, or null for zeros
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int k = 0; k < 16; ++k) h[t][k] = b ? b[32 * t + ghr_acc_row(k, half)] : 0.f;
  }
}

// y holds [channel][point on the lane] of NT tiles of 32 channels: the lane writes them to its point's row, four floats a time (the
// registers r & 3 are four consecutive channels). For rows of whole tiles: a store with a column bound (the trunk's grad_x) stays with
// its kernel, because here the compiler folds the bounded tail's fourth store into the 16-byte one and splits that into 12 + 4 bytes.
template <int NT>
__device__ __forceinline__ void ghr_store_tiles(const ghr_acc (&y)[NT], float* __restrict__ row, int half, bool live, int vec) {
  if (!live) return;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* d = row + 32 * t + 8 * q + 4 * half;
      if (vec) {
        *(float4*)d = make_float4(y[t][4 * q], y[t][4 * q + 1], y[t][4 * q + 2], y[t][4 * q + 3]);
      } else {
        d[0] = y[t][4 * q]; d[1] = y[t][4 * q + 1]; d[2] = y[t][4 * q + 2]; d[3] = y[t][4 * q + 3];
      }
    }
  }
}

// The weights are the A operand and cross LDS in slabs the four waves share, two barriers a slab: every load of the slab and of the
// lane's operands is issued, then the barrier behind the previous slab's readers, ghr_put, the barrier. A slab is 32 columns of a
// matrix's rows, read along the row at pitch GHR_WP (W . src), or 32 rows of up to 128 columns, read along the column (W^T . src).
// WHOLE: the window lies inside the matrix (ghr_fetch); otherwise what lies outside is zeros (ghr_fetch_in).
#define GHR_WP 33

template <bool WHOLE, int IT, int Q>
__device__ __forceinline__ void ghr_window(GhrSlab<IT, Q>& t, const float* __restrict__ W, long long stride, int row0, int col0, int nrows,
                                           int ncols, int vec, int tid) {
  if constexpr (WHOLE) ghr_fetch(t, W, stride, row0, col0, vec, tid);
  else ghr_fetch_in(t, W, stride, row0, col0, nrows, ncols, vec, tid);
}

// h[t] += W[32 t .., 0 .. n) . x: W (32 NH, n) contiguous, x = xp[0 .. n) (zeros where not live), k ascending; the last slab's
// missing columns are zeros on both sides
template <int NH>
__device__ __forceinline__ void ghr_mm_x(ghr_acc (&h)[NH], float* s_w, const float* __restrict__ W, int n, int vec, const float* __restrict__ xp,
                                         bool live, int tid, int col, int half) {
  for (int k0 = 0; k0 < n; k0 += 32) {
    const int kc = n - k0 < 32 ? n - k0 : 32;
    GhrSlab<NH, 8> w;                                          // 32 NH rows x 32 columns
    ghr_fetch_in(w, W, n, 0, k0, 32 * NH, n, vec, tid);
    float xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) xv[s] = (live && 2 * s + half < kc) ? xp[k0 + 2 * s + half] : 0.f;
    __syncthreads();                                           // the previous slab has been read by every wave
    ghr_put(w, s_w, GHR_WP, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (2 * s < kc) {
#pragma unroll
        for (int t = 0; t < NH; ++t)
          h[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(32 * t + col) * GHR_WP + 2 * s + half], xv[s], h[t], 0, 0, 0);
      }
    }
  }
}

// d[t] += W[32 t .., :] . f(src) for t < nt: W (nrows, 32 NS) contiguous, src's channels in register order, f the activation on the way
template <bool WHOLE, int NS, int ND, class F>
__device__ __forceinline__ void ghr_mm(ghr_acc (&d)[ND], int nt, const ghr_acc (&src)[NS], F f, float* s_w, const float* __restrict__ W,
                                       int nrows, int vec, int tid, int col, int half) {
#pragma unroll
  for (int jt = 0; jt < NS; ++jt) {
    GhrSlab<ND, 8> w;                                          // 32 ND rows x 32 columns
    ghr_window<WHOLE>(w, W, 32 * NS, 0, 32 * jt, nrows, 32 * NS, vec, tid);
    __syncthreads();
    ghr_put(w, s_w, GHR_WP, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float hv = f(src[jt][k]);
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(32 * t + col) * GHR_WP + ghr_acc_row(k, half)], hv, d[t], 0, 0, 0);
      }
    }
  }
}

// d[t] += (W[:, c0 + 32 t ..])^T . src for t < nt: W (32 NS, ncols) with row stride `stride`, its rows in register order; the window is
// 32 ND columns from c0
template <bool WHOLE, int NS, int ND>
__device__ __forceinline__ void ghr_mm_t(ghr_acc (&d)[ND], int nt, const ghr_acc (&src)[NS], float* s_w, const float* __restrict__ W,
                                         long long stride, int c0, int ncols, int vec, int tid, int col, int half) {
  constexpr int CW = 32 * ND;
#pragma unroll
  for (int jt = 0; jt < NS; ++jt) {
    GhrSlab<ND, CW / 4> w;                                     // 32 rows x 32 ND columns
    ghr_window<WHOLE>(w, W, stride, 32 * jt, c0, 32 * NS, ncols, vec, tid);
    __syncthreads();
    ghr_put(w, s_w, CW, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[ghr_acc_row(k, half) * CW + 32 * t + col], src[jt][k], d[t], 0, 0, 0);
      }
    }
  }
}

// d[t] += (W[0 .. n, c0 + 32 t ..])^T . g: g = gp[0 .. n) from memory or LDS (zeros where not live), the rows of W ascending; the
// window is 32 ND columns from c0 of W's ncols. WHOLE: n is a multiple of 32 as well.
template <bool WHOLE, int ND>
__device__ __forceinline__ void ghr_mm_tg(ghr_acc (&d)[ND], float* s_w, const float* __restrict__ W, long long stride, int c0, int n, int ncols,
                                          int vec, const float* __restrict__ gp, bool live, int tid, int col, int half) {
  constexpr int CW = 32 * ND;
  for (int r0 = 0; r0 < n; r0 += 32) {
    GhrSlab<ND, CW / 4> w;                                     // 32 rows x 32 ND columns
    ghr_window<WHOLE>(w, W, stride, r0, c0, n, ncols, vec, tid);
    float gv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) gv[s] = (live && (WHOLE || r0 + 2 * s + half < n)) ? gp[r0 + 2 * s + half] : 0.f;
    __syncthreads();
    ghr_put(w, s_w, CW, tid);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (WHOLE || r0 + 2 * s < n) {
#pragma unroll
        for (int t = 0; t < ND; ++t) d[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[(2 * s + half) * CW + 32 * t + col], gv[s], d[t], 0, 0, 0);
      }
    }
  }
}

// f(std::integral_constant<int, n>) for a tile count n = 1 .. 4 (anything else is 4): a host switch into a kernel template
template <class F>
static inline void ghr_tiles(int n, F f) {
  switch (n) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// A kernel that may ask for more than 64 KB of dynamic LDS says so, once per process, where the runtime wants to be told (the call sets
// an upper limit, a CU's 160 KiB, and enqueues nothing). The flag belongs to the kernel, not to its function type: kernels of equal
// signature, such as the instantiations of one template, are told each on its own first launch.
template <auto Kern>
static void ghr_allow_lds(size_t lds) {
  static bool told = false;
  if (lds > 64 * 1024 && !told) {
    (void)hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    told = true;
  }
}

#endif
