/*
 * gh_conv.h — C-ABI of the perceptual loss's network pieces: the dense 3x3 convolution of VGG19's feature stack (torchvision
 * `features` up to relu4_1, the reference's Vgg19 slices, utils.py:875-908) forward and backward-data, and its 2x2 max pooling.
 * The weights are frozen (utils.py:897-899) and only the image gradient is wanted: no weight or bias gradient exists here.
 *
 * Tensors are float32, channels-last (N, H, W, C), contiguous. A "pixel" is p = (n H + i) W + j.
 *
 *     y[n,i,j,co]  = b[co] + sum_{ky,kx,ci} W[co,ci,ky,kx] x[n,i+ky-1,j+kx-1,ci]          zero padding 1, stride 1;  y = relu(y) on request
 *     dx[n,i,j,ci] = sum_{ky,kx,co} W[co,ci,ky,kx] g[n,i-ky+1,j-kx+1,co],   g = dy where the forward's pre-activation was > 0 (with a
 *                    ReLU; g = dy without one) and an exact 0 elsewhere
 *
 * Weight layouts, prepared by the host once per module. W is the (Cout, Cin, 3, 3) convolution weight, tap t = 3 ky + kx, and
 * pad(C) = C rounded up to a multiple of GH_CONV_CHUNK (128):
 *     forward        wf[t][co][ci] = W[co][ci][ky][kx]                  (9, pad(Cout), Cin), rows co >= Cout are zeros
 *     backward-data  wb[t][ci][co] = W[co][ci][2-ky][2-kx]              (9, pad(Cin), Cout), rows ci >= Cin are zeros
 * so that the backward is the forward's product with (Cin, Cout) exchanged: dx[p, ci] = sum_t sum_co wb[t][ci][co] g[p + tap t, co].
 * The zero rows let a workgroup fetch its whole chunk of output channels without a bound.
 *
 * Arithmetic contract (the library is built with -ffp-contract=off; float32 throughout). Every output element is ONE chain of fmaf,
 * acc = fmaf(w, v, acc), from acc = b[co] (forward; 0 without a bias and in the backward): the taps t = 0 .. 8 in ascending order,
 * inside a tap the input channels in slabs of 32, k0 = 0, 32, ..., and inside a slab the channels k0 + s, k0 + 16 + s for s = 0 .. 15
 * in that order (the two lane halves of one matrix-instruction step). A slab's steps s with k0 + s beyond the last input channel are
 * skipped; in a step that runs, a channel k0 + 16 + s beyond the last contributes fmaf(0, 0, acc). A tap that falls into the padding
 * contributes fmaf(w, 0, acc) per channel, an exact zero product — the same bits an explicit zero pixel gives. Then the ReLU,
 * v < 0 ? 0 : v (a NaN stays). The order depends on the number of input channels alone: not on the pixel's position, not on N, H, W,
 * not on the tile or the chunk of output channels the element falls in. The products run on v_mfma_f32_32x32x2_f32, which is such
 * a chain bit for bit. No atomics and no sum split across workgroups: every result is bitwise reproducible.
 *
 * The gate. With GH_CONV_RELU the forward writes one bit per activation, pre-activation > 0 (false for a NaN), and the backward
 * reads nothing else of the forward: gate is uint32[N H W][ceil(Cout / 32)], and channel c's bit is bit 16 ((c >> 2) & 1) +
 * (c & 3) + 4 ((c & 31) >> 3) of word gate[p ceil(Cout / 32) + (c >> 5)] (the register order of the matrix instruction's result, so
 * that a lane packs its own 16 bits). Bits of channels >= Cout in the last word are 0.
 *
 * Kernel shape. One 256-thread workgroup per (GH_CONV_PIXELS = 128 consecutive pixels, chunk of 32, 64 or 128 output channels): a
 * wave owns 32 pixels, a lane one pixel (the column of the product), the accumulators 32 output channels each. A tap's weights
 * cross LDS in slabs of chunk x 32; a lane reads its own pixel's 16 channels of the slab from memory (four 16-byte loads where
 * the channel count is a multiple of 4). A tile of pixels may start mid-row and straddle images: every lane derives its own
 * (n, i, j). `chunk` = 0 lets the library choose (the largest of 128, 64, 32 that does not exceed the padded channel count and still
 * gives GH_CONV_FILL workgroups, else 32); a result does not depend on it.
 *
 * Pooling. Kernel 2, stride 2, floor: out (N, H/2, W/2, C). The maximum is taken in window order (0,0),(0,1),(1,0),(1,1) by
 * F.max_pool2d's rule, from m = -inf at position 0: position q replaces the maximum when v > m or v is a NaN. So the first of equal
 * values wins, a NaN wins over numbers, the last NaN of a window is the one chosen, and a window of -inf keeps position 0.
 * choice is uint8 (N, H/2, W/2, C), q = 2 dy + dx. The backward writes every element of dx: dy at the chosen position, 0 at the
 * other three and in a trailing odd row or column.
 *
 * The feature distance of the loss, mean|f - t| and sign(f - t) / n, is gh_l1_loss of gh_raster.h.
 *
 * Conventions are those of gh_raster.h: caller-allocated buffers, all work enqueued on `hip_stream`, no host synchronisation, no
 * allocation, HIP-graph capturable; GhStatus return codes, returned before any launch for bad arguments. Every address is formed in
 * 64 bits. 4-byte alignment suffices everywhere.
 *
 * Status, judged in this order, before any launch:
 *   GH_ERR_INVALID_ARG   N, H or W < 0; a channel count < 1; a flag other than GH_CONV_RELU; chunk not 0, 32, 64 or 128
 *   GH_ERR_UNSUPPORTED   a channel count > GH_CONV_MAX_C (convolution); more workgroups than a launch holds (2^31 - 1)
 *   GH_OK                an empty tensor (nothing is launched)
 *   GH_ERR_INVALID_ARG   a required pointer is NULL or any pointer is not 4-byte aligned; GH_CONV_RELU without a gate
 *   GH_ERR_LAUNCH        the runtime refused a launch
 */
#ifndef GH_CONV_H
#define GH_CONV_H

#include "gh_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GH_CONV_RELU 1     /* flags: the forward applied (applies) a ReLU; the gate is written (read) */
#define GH_CONV_MAX_C 512  /* 1 <= Cin, Cout <= 512 */
#define GH_CONV_PIXELS 128 /* pixels per workgroup */
#define GH_CONV_CHUNK 128  /* the largest chunk of output channels per workgroup, and the padding of the weight layouts */
#define GH_CONV_FILL 512   /* chunk = 0: workgroups wanted before a larger chunk is chosen */

/* Floats of a prepared weight layout whose product has Cout_ output and Cin_ input channels: 9 pad(Cout_) Cin_ (0 for sizes out of range). */
size_t gh_conv3x3_weight_floats(int Cin_, int Cout_);

/*
 * x (N, H, W, Cin), wf (9, pad(Cout), Cin) (required); bias (Cout,) or NULL; y (N, H, W, Cout), every element written (required);
 * gate: uint32[N H W ceil(Cout / 32)], every word written, required with GH_CONV_RELU and ignored without. One launch.
 */
int gh_conv3x3_forward(const float* x, int N, int H, int W, int Cin, int Cout, const float* wf, const float* bias, uint32_t flags,
                       int chunk, float* y, uint32_t* gate, void* hip_stream);

/*
 * dy (N, H, W, Cout), wb (9, pad(Cin), Cout) (required); gate as the forward wrote it, required with GH_CONV_RELU; dx (N, H, W, Cin),
 * every element written (required). One launch.
 */
int gh_conv3x3_backward_data(const float* dy, const uint32_t* gate, int N, int H, int W, int Cin, int Cout, const float* wb,
                             uint32_t flags, int chunk, float* dx, void* hip_stream);

/* x (N, H, W, C) -> y, choice (N, H/2, W/2, C); either output may be NULL (not both). One launch. */
int gh_maxpool2x2_forward(const float* x, int N, int H, int W, int C, float* y, uint8_t* choice, void* hip_stream);

/* dy, choice (N, H/2, W/2, C) -> dx (N, H, W, C), every element written. One launch. */
int gh_maxpool2x2_backward(const float* dy, const uint8_t* choice, int N, int H, int W, int C, float* dx, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* GH_CONV_H */
