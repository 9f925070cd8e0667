/*
 * gh_lpips.h — C-ABI of the perceptual score of the evaluator: LPIPS over AlexNet, `lpips.LPIPS(net='alex')` version 0.1 in eval mode
 * with spatial=False, as the reference's evaluator feeds it (evaluator.py:26-65). Forward only: the reference never differentiates it.
 * The result is specified by its mathematics, unpinned against the package.
 *
 *   1. x0, x1 (N, 3, h, w) in [-1, 1]; the scaling layer gives (x - shift[c]) / scale[c].
 *   2. torchvision AlexNet `features`, the five ReLU outputs being the taps: conv(3 -> C1, k 11, s 4, p 2), pool, conv(C1 -> C2, k 5, p 2),
 *      pool, conv(C2 -> C3, k 3, p 1), conv(C3 -> C4, k 3, p 1), conv(C4 -> C5, k 3, p 1); pool = max pooling, kernel 3, stride 2, floor.
 *   3. per tap l and pixel: n = sqrt(sum_c f_c^2), u = f / (n + 1e-10) for both images; d_l = mean_pixels sum_c lin_l[c] (u0_c - u1_c)^2.
 *   4. lpips = sum_l d_l, one value per pair. The smallest legal image is GH_LPIPS_MIN_SIZE = 31 in both directions.
 *
 * Tensors are float32, channels-last (N, H, W, C), contiguous; the two members of pair n are the images n and n + N of a (2N, ...) map.
 *
 * gh_conv2d_forward. y[n,i,j,co] = b[co] + sum_{ky,kx,ci} W[co,ci,ky,kx] x[n, s i + ky - p, s j + kx - p, ci], zero padding p, stride s,
 * output size floor((H + 2p - K) / s) + 1 (0 where H + 2p < K), a ReLU on request. K is 3, 5 or 11, s is 1 or 4, 0 <= p < K.
 * Weight layout, prepared by the host once per module from W (Cout, Cin, K, K): the reduction index r = (K ky + kx) Cin + ci, R = K K Cin,
 * Rp = R rounded up to a multiple of 4, pad(C) = C rounded up to a multiple of GH_LPIPS_CHUNK (128):
 *     wp[co][r] = W[co][ci][ky][kx]                   (pad(Cout), Rp), rows co >= Cout and columns r >= R are zeros
 *
 * Arithmetic contract (the library is built with -ffp-contract=off; float32 throughout). Every output element is ONE chain of fmaf,
 * acc = fmaf(w, v, acc), from acc = b[co] (0 without a bias). Its order depends on (Cin, K) alone: not on the pixel's position, not on
 * N, H, W, s or p, not on the tile or the chunk of output channels the element falls in.
 *   Cin <= GH_LPIPS_FLAT_CIN (16), the flattened order: r ascending in slabs of 32, r0 = 0, 32, ..., and inside a slab r0 + s, r0 + 16 + s
 *     for s = 0 .. 15 in that order (the two lane halves of one matrix-instruction step). A slab's steps s with r0 + s >= R are skipped; in
 *     a step that runs, an index r0 + 16 + s >= R contributes fmaf(0, 0, acc). (AlexNet's first layer: 363 indices in 12 slabs, where
 *     a slab per tap would run 121 with three live channels each.)
 *   Cin > GH_LPIPS_FLAT_CIN, gh_conv.h's order: the taps t = K ky + kx ascending, inside a tap the input channels in slabs of 32,
 *     k0 = 0, 32, ..., inside a slab the channels k0 + s, k0 + 16 + s for s = 0 .. 15; steps with k0 + s >= Cin are skipped, a channel
 *     k0 + 16 + s >= Cin of a step that runs contributes fmaf(0, 0, acc).
 * In both, a tap that falls into the padding contributes an exact fmaf(w, 0, acc) per channel — the same bits an explicit zero pixel
 * gives. Then the ReLU, v < 0 ? 0 : v (a NaN stays). The products run on v_mfma_f32_32x32x2_f32, which is such a chain bit for bit.
 * Kernel shape: one 256-thread workgroup per (GH_LPIPS_PIXELS = 128 consecutive output pixels, chunk of 32, 64 or 128 output channels);
 * a lane owns one output pixel (the column of the product), the weights cross LDS in slabs of chunk x 32. A tile may start mid-row and
 * straddle images. `chunk` = 0 lets the library choose (the largest of 128, 64, 32 that does not exceed the padded channel count and
 * still gives GH_LPIPS_FILL workgroups, else 32); no result depends on it.
 *
 * gh_maxpool3x3s2_forward. Kernel 3, stride 2, floor, no padding: out (N, Ho, Wo, C), Ho = (H - 3) / 2 + 1 (0 where H < 3). The
 * maximum is taken in window order (0,0), (0,1), ..., (2,2) by F.max_pool2d's rule, from m = -inf: a value replaces the maximum when
 * v > m or v is a NaN. So a NaN wins over numbers and a window of -inf gives -inf. Trailing rows and columns no window reaches are
 * dropped. Values are exact.
 *
 * gh_lpips_layer. f (2N, P, C), P pixels per image; lin (C,). Per pixel, in float32: s = the sum of f_c^2 as fmaf(f, f, s), lane l of a
 * wave summing the channels l, l + 64, ... in ascending order, the 64 shares added by the butterfly of distances 32, 16, 8, 4, 2, 1;
 * nrm = sqrtf(s) + 1e-10f; u = f / nrm; d = the sum of lin_c (u0_c - u1_c)^2 as e = u0 - u1, d = fmaf(lin_c, e * e, d), in the same
 * order. A pixel whose features are all zero in both images contributes exactly 0; identical rows contribute exactly 0; exchanging the
 * two images changes no bit. The pixels are summed in float64: a wave adds its GH_LPIPS_HEAD_PIXELS / 4 consecutive pixels in ascending
 * order, a workgroup its four waves as ((s0 + s1) + s2) + s3 into its slot of the workspace, and one wave per pair finishes: lane l
 * adds the slots l, l + 64, ... in ascending order, then the same butterfly. d_l = that sum / P. score[n] becomes d_l (accumulate = 0) or
 * score[n] + d_l; term[n], where given, receives d_l. No atomics: every result is bitwise reproducible and independent of N and of
 * the slot n.
 *
 * gh_lpips_prepare. Builds the network's input x (2N, h, w, 3), members n (the prediction) and n + N (the target), from the caller's
 * images (N, 3, H, W) — or (N, H, W, 3) where the layout bit is set — read in place and not written. Per view, (bx, by, bw, bh) =
 * bbox[n] (gh_image_scores' format; NULL: (0, 0, w, h)). Where (bw, bh) != (w, h), or the box does not lie inside the image, every
 * element of both members is NaN and nothing of the images is read. Else, per element v of pixel (by + i, bx + j):
 *     the prediction is taken as 0 where bbox_mask[n, by + i, bx + j] == 0 (bbox_mask may be NULL);
 *     GH_LPIPS_SIGNED: x = v (the images are in [-1, 1] already); else t = v * 255, with GH_LPIPS_QUANTIZE
 *     t = min(max(rint(t), 0), 255) (to nearest, ties to even; the 8-bit PNG the reference writes and reads back), everything up to
 *     here in float32, and x = float32(double(t) / 127.5 - 1) (im2tensor);
 *     out = (x - shift[c]) / scale[c].
 * A NaN stays a NaN and makes that view's score NaN (OpenCV's conversion of a NaN to 8 bits is not emulated).
 *
 * gh_lpips_forward runs the chain on a prepared x for N pairs of one crop size: 5 convolutions, 2 poolings and 5 x 2 head launches.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. Every address is formed in
 * 64 bits. Float arrays need 4-byte alignment, float64 arrays and workspaces 8.
 *
 * Status, judged in this order, before any launch:
 *   GH_ERR_INVALID_ARG   a size < 0 (N, H, W, P, h, w); a channel count < 1; K not 3, 5 or 11; stride not 1 or 4; padding < 0 or >= K;
 *                        an unknown flag, or GH_LPIPS_QUANTIZE with GH_LPIPS_SIGNED; chunk not 0, 32, 64 or 128; h > H or w > W
 *                        (prepare); a NULL widths or weights struct (forward and gh_lpips_workspace's 0)
 *   GH_ERR_UNSUPPORTED   a channel count > GH_LPIPS_MAX_C; more workgroups than a launch holds (2^31 - 1); h or w < GH_LPIPS_MIN_SIZE
 *                        (forward)
 *   GH_OK                an empty output: N = 0, or no output pixel (nothing is launched; gh_lpips_layer with P = 0 is empty too)
 *   GH_ERR_INVALID_ARG   a required pointer is NULL or any pointer is misaligned; a workspace smaller than its size function says
 *   GH_ERR_LAUNCH        the runtime refused a launch
 */
#ifndef GH_LPIPS_H
#define GH_LPIPS_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_LPIPS_RELU 1          /* gh_conv2d_forward flags: apply a ReLU */
#define GH_LPIPS_MAX_C 512       /* 1 <= Cin, Cout, C <= 512 */
#define GH_LPIPS_PIXELS 128      /* output pixels per workgroup of the convolution */
#define GH_LPIPS_CHUNK 128       /* the largest chunk of output channels per workgroup, and the row padding of the weight layout */
#define GH_LPIPS_FILL 512        /* chunk = 0: workgroups wanted before a larger chunk is chosen */
#define GH_LPIPS_FLAT_CIN 16     /* Cin up to here: the flattened reduction order */
#define GH_LPIPS_HEAD_PIXELS 256 /* pixels per workgroup of gh_lpips_layer */
#define GH_LPIPS_TAPS 5
#define GH_LPIPS_MIN_SIZE 31     /* the smallest image the network takes */

/* gh_lpips_prepare flags */
#define GH_LPIPS_PRED_HWC 1u /* the prediction's memory is (N, H, W, 3) */
#define GH_LPIPS_GT_HWC 2u   /* the target's memory is (N, H, W, 3) */
#define GH_LPIPS_QUANTIZE 4u /* round to 8 bits as the reference's PNG round trip does */
#define GH_LPIPS_SIGNED 8u   /* the images are in [-1, 1] already */

/* The frozen parameters: w[l] the packed layout of convolution l (above), b[l] (C_l,), lin[l] (C_l,). */
typedef struct GhLpipsWeights {
  const float* w[GH_LPIPS_TAPS];
  const float* b[GH_LPIPS_TAPS];
  const float* lin[GH_LPIPS_TAPS];
} GhLpipsWeights;

/* Floats of the packed layout: pad(Cout) Rp (0 for sizes out of range). */
size_t gh_conv2d_weight_floats(int Cin, int Cout, int K);

/* x (N, H, W, Cin), wp (required); bias (Cout,) or NULL; y (N, Ho, Wo, Cout), every element written (required). One launch. */
int gh_conv2d_forward(const float* x, int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, const float* wp,
                      const float* bias, uint32_t flags, int chunk, float* y, void* hip_stream);

/* x (N, H, W, C) -> y (N, Ho, Wo, C). One launch. */
int gh_maxpool3x3s2_forward(const float* x, int N, int H, int W, int C, float* y, void* hip_stream);

/* Bytes of gh_lpips_layer's workspace: N ceil(P / GH_LPIPS_HEAD_PIXELS) float64 (0 for sizes out of range). */
size_t gh_lpips_layer_workspace(int N, long long P);

/* f (2N, P, C), lin (C,), score (N,) float64 (required); term (N,) float64 or NULL. Two launches. */
int gh_lpips_layer(const float* f, int N, long long P, int C, const float* lin, int accumulate, double* score, double* term,
                   void* workspace, size_t ws_bytes, void* hip_stream);

/*
 * pred, gt: (N, 3, H, W) or (N, H, W, 3) by `flags`; bbox_mask (N, H, W) uint8 or NULL; bbox (N, 4) int32 on the device or NULL;
 * shift, scale (3,) on the device; x (2N, h, w, 3), every element written. One launch.
 */
int gh_lpips_prepare(const float* pred, const float* gt, const uint8_t* bbox_mask, const int32_t* bbox, int N, int H, int W, int h,
                     int w, uint32_t flags, const float* shift, const float* scale, float* x, void* hip_stream);

/* Bytes of gh_lpips_forward's workspace for N pairs of h x w and the five widths (0 for sizes out of range). */
size_t gh_lpips_workspace(int N, int h, int w, const int* widths);

/*
 * x (2N, h, w, 3) as gh_lpips_prepare writes it; widths: the five channel counts (host memory); scores (N,) float64, every element
 * written; terms (5, N) float64 or NULL: d_l of tap l at terms[l N + n]. scores = ((((d_1 + d_2) + d_3) + d_4) + d_5) in float64.
 */
int gh_lpips_forward(const float* x, int N, int h, int w, const int* widths, const GhLpipsWeights* weights, double* scores,
                     double* terms, void* workspace, size_t ws_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_LPIPS_H */
