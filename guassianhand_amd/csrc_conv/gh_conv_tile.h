// gh_conv_tile.h — the host's launch rules of the pixel-column convolution tile that csrc_conv/gh_conv.hip (the perceptual loss's 3x3
// convolution, both directions) and csrc_lpips/gh_lpips.hip (LPIPS' dense convolution) are both built on: a 256-thread workgroup owns
// 128 pixels x a chunk of 32 NH output channels. Internal: not part of the C-ABI. The device side of the tile stays stated in each
// file: moved into functions here it computed the same bits (tests/test_gpu_conv_bits.py holds them) but the compiler allocated
// registers differently and launches moved by up to 3% either way (profiles/conv_tile_before_after.txt).
#ifndef GH_CONV_TILE_H
#define GH_CONV_TILE_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../csrc_rows/gh_rows.h"

static inline bool gct_chunk_ok(int chunk) { return chunk == 0 || chunk == 32 || chunk == 64 || chunk == 128; }

// The chunk of a launch that names none: the largest of max_chunk, max_chunk / 2, .. that still gives `fill` workgroups, else 32.
static inline int gct_auto_chunk(long long tiles, int CoP, int max_chunk, int fill) {
  for (int ch = max_chunk; ch > 32; ch /= 2) {
    if (tiles * (CoP / ch) >= fill) return ch;
  }
  return 32;
}

// Writes a.vec_w / vec_in / vec_out: 16-byte accesses where the base is 16-byte aligned and every row starts at a multiple of 4 floats.
// Reads a.w, a.in, a.out, a.Ci and a.Co: call it once those are filled in.
template <class A>
static inline void gct_vec(A& a, bool w_rows4) {
  a.vec_w = (ghr_al16(a.w) && w_rows4) ? 1 : 0;
  a.vec_in = (ghr_al16(a.in) && a.Ci % 4 == 0) ? 1 : 0;
  a.vec_out = (ghr_al16(a.out) && a.Co % 4 == 0) ? 1 : 0;
}

// f(std::integral_constant<int, NH>) for a chunk of 128, 64 or 32 output channels: the host's switch into a kernel template
template <class F>
static inline void gct_nh(int chunk, F f) {
  if (chunk == 128) f(std::integral_constant<int, 4>());
  else if (chunk == 64) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 1>());
}

#endif
