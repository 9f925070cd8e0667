/*
 * gh_mano.h — C-ABI of the hand points: MANO-style linear blend skinning of H hand models for B parameter sets, and the fixed
 * edge-midpoint subdivision of the skinned meshes, forward and backward. What the reference's dataset does on the CPU per frame
 * (dataset_one_shot.py:299-325: an smplx MANO layer per hand, then mis_utils.edge_subdivide three times) as device launches, with a
 * gradient back to the four pose inputs. The models are frozen: no gradient of a model array exists here.
 *
 * One model (V vertices, J joints, NB shape coefficients), per parameter set (b, h):
 *     pose          = cat(global_orient, hand_pose) + pose_mean, read as (J, 3)
 *     R_j           = I + sin(a) K + (1 - cos(a)) K K,   a = |pose_j + 1e-8| (the constant on every component), K = skew(pose_j / a)
 *     v_shaped      = v_template + shapedirs . betas;    Jt = j_template + j_shapedirs . betas  (the joint regressor folded into both)
 *     v_posed       = v_shaped + posedirs^T . (R_1 - I, ..., R_{J-1} - I)   (joint-major, each 3 x 3 row-major)
 *     G_0           = [R_0 | Jt_0];   G_j = G_parent(j) [R_j | Jt_j - Jt_parent(j)];   A_j = [G_j^R | G_j^t - G_j^R Jt_j]
 *     vertex_v      = (sum_j lbs_weights[v, j] A_j) [v_posed_v; 1] + transl;          joint_j = G_j^t + transl
 *     point_p       = vertex_p for p < V;  sum_k st_w[p, k] vertex_{st_idx[p, k]} (k = 0, 1, 2) for V <= p < P
 * The stencil (st_idx, st_w) is the composition of `levels` <= 3 midpoint subdivisions, built by the host once per model (every point
 * is a combination of at most three vertices with weights in multiples of 1/8); (tr_ptr, tr_point, tr_w) is its transpose as a CSR over
 * vertices, rows sorted by point, holding every non-zero weight including the 1 of a vertex's own point.
 *
 * Model arrays, float32 unless noted, laid out so that consecutive vertices are consecutive addresses:
 *     v_template (3, V)   shapedirs (NB, 3, V)   posedirs (9 (J - 1), 3, V)   lbs_weights (J, V)
 *     j_template (J, 3) and j_shapedirs (J, 3, NB), both float64 (folded in float64 by the host);  pose_mean (3 J)
 *     st_idx int32 (P, 3), st_w (P, 3): rows p < V are not read; an unused slot has weight 0 and a valid index
 *     tr_ptr int32 (V + 1), tr_point int32 (nnz), tr_w (nnz)
 * `parents` lives in the struct itself (host memory): parents[0] = -1, 0 <= parents[i] < i.
 *
 * Tensors. global_orient (B, H, 3), hand_pose (B, H, 3 (J - 1)) (NULL allowed at J = 1), betas (B, H, NB), transl (B, H, 3);
 * points (B, sum_h P_h, 3) with hand h's block behind hand h - 1's, every element written in place; joints (B, H J, 3). All contiguous.
 *
 * Launches. The forward is three: the chain (one wave per (b, h): lane j owns joint j, the chain advances one tree depth per step),
 * the vertices (one thread per vertex) and the points p >= V (one thread per point; skipped when every P_h = V). They are separate
 * launches because each reads what every workgroup of the one before wrote. The backward is up to five: the chain once more in float64 (R, G, Jt from the kept pose and betas), the column sums of d_points
 * in chunks of GH_MANO_CHUNK points (only when transl's gradient is wanted), the transposed stencil with the skinning's transpose
 * (one thread per vertex), the reductions over vertices (one workgroup per sum group), and the chain in reverse with the closed-form
 * Rodrigues derivative, which also finishes every output. A gradient output that is NULL is not computed: with transl's alone only
 * the column sums and the last launch run; without hand_pose's the 9 (J - 1) pose blend-shape sums are skipped, without betas' the NB
 * shape sums. d_points == NULL or d_joints == NULL is a cotangent of zeros that is never read.
 *
 * Arithmetic contract (the library is built with -ffp-contract=off; fmaf / fma only where stated). No atomics. The forward is float32.
 * The backward reads the float32 cotangents, the float32 inputs and the model and works in float64 from there on — the chain and
 * v_posed over again, the transposed stencil, dv_posed (through the forward's float32 A), the sums over vertices and over points, the chain and the Rodrigues derivative — rounding once, where an output
 * is written: the rotation gradients are differences of sums over every vertex and every descendant joint, and a vertex's cotangent
 * is itself a sum over some sixty points; in float32 those cost the root's gradient an order of magnitude against a float32 autograd.
 * Every sum has one order that depends on the model alone: blend shapes and skinning are fmaf chains in ascending coefficient / joint
 * order; a sum over vertices is 256 strided serial sums (thread t takes elements t, t + 256, ...) joined by a fixed butterfly; the
 * chunked column sums are joined in chunk order; a parent joint adds its children in ascending order. So results are bitwise
 * reproducible and do not depend on B, on the batch or hand slot a parameter set is in, or on the launch size.
 *
 * Workspace. The forward writes its state (pose, R, G, A, Jt per (b, h) and v_posed) into `ws`; the backward of the same call reads it
 * and uses the rest as scratch: pass the same buffer, untouched in between. gh_mano_workspace_bytes covers both.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. Every address is formed in
 * 64 bits. 4-byte alignment suffices for every float32 tensor and model array, 8-byte for j_template and j_shapedirs; `ws` is 8-byte aligned (it holds the backward's float64 sums).
 *
 * Status, judged in this order, before any launch:
 *   GH_ERR_INVALID_ARG      dims, models or params NULL; B < 0; H, J or NB < 1
 *   GH_ERR_UNSUPPORTED      H > GH_MANO_MAX_H; J > GH_MANO_MAX_J; NB > GH_MANO_MAX_NB; B > GH_MANO_MAX_B
 *   GH_ERR_INVALID_ARG      a model with V < 1, P < V, levels < 0, nnz < P, levels = 0 with P != V, parents[0] != -1 or a parents[i]
 *                           outside [0, i)
 *   GH_ERR_UNSUPPORTED      a model with levels > GH_MANO_MAX_LEVELS, V > GH_MANO_MAX_V or P > GH_MANO_MAX_P
 *   GH_ERR_INVALID_ARG      a required pointer is NULL (an output among them), any pointer is not 4-byte aligned or `ws` not 8-byte
 *   GH_OK                   B = 0 (nothing is launched)
 *   GH_ERR_WORKSPACE_SMALL  ws_bytes < gh_mano_workspace_bytes
 *   GH_ERR_LAUNCH           the runtime refused a launch
 */
#ifndef GH_MANO_H
#define GH_MANO_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_MANO_MAX_H 4          /* hand models per call */
#define GH_MANO_MAX_J 16         /* joints */
#define GH_MANO_MAX_NB 16        /* shape coefficients */
#define GH_MANO_MAX_LEVELS 3     /* subdivisions folded into one three-entry stencil */
#define GH_MANO_MAX_V 65536      /* vertices of a model */
#define GH_MANO_MAX_P 4194304    /* points of a model (V = 65536 after three levels of a closed mesh stays below) */
#define GH_MANO_MAX_B 65535      /* parameter sets per call (a grid dimension) */
#define GH_MANO_CHUNK 4096       /* points per partial column sum of d_points */

typedef struct GhManoDims {
  int32_t B, H, J, NB;
} GhManoDims;

typedef struct GhManoModel {
  int32_t V, P, levels, nnz;
  int32_t parents[GH_MANO_MAX_J];
  const float* v_template;
  const float* shapedirs;
  const float* posedirs;
  const float* lbs_weights;
  const double* j_template;
  const double* j_shapedirs;
  const float* pose_mean;
  const int32_t* st_idx;
  const float* st_w;
  const int32_t* tr_ptr;
  const int32_t* tr_point;
  const float* tr_w;
} GhManoModel;

typedef struct GhManoParams {
  const float* global_orient;
  const float* hand_pose;
  const float* betas;
  const float* transl;
} GhManoParams;

typedef struct GhManoGrads {
  float* global_orient;
  float* hand_pose;
  float* betas;
  float* transl;
} GhManoGrads;

/* Bytes of the workspace for `dims` over models[0 .. H): state and scratch. 0 for arguments the entry points refuse. */
size_t gh_mano_workspace_bytes(const GhManoDims* dims, const GhManoModel* models);

/* points and joints are required; every element of both is written. st_idx / st_w may be NULL for a model with P = V. */
int gh_mano_forward(const GhManoDims* dims, const GhManoModel* models, const GhManoParams* params, float* points, float* joints,
                    void* ws, size_t ws_bytes, void* hip_stream);

/* d_points (B, sum_h P_h, 3) and d_joints (B, H J, 3), either NULL; every non-NULL member of `grads` is written whole (hand_pose's
 * is ignored at J = 1). `ws` is the forward's. tr_ptr / tr_point / tr_w are required when d_points is given and a gradient other
 * than transl's is wanted. */
int gh_mano_backward(const GhManoDims* dims, const GhManoModel* models, const float* d_points, const float* d_joints,
                     const GhManoGrads* grads, void* ws, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_MANO_H */
