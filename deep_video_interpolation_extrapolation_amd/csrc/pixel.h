// The per-pixel primitives of the video kernels, each defined once: the uint8 <-> [-1, 1] maps
// (synth.hip, tile.hip), the argmax over logits and the quad's label store (synth.hip, tile.hip),
// the geometry of a canvas row (synth.hip, tile.hip) and the integer luma (scene.hip, motion.hip).
// The tests pin them bit for bit (array_equal against numpy, and the padded and tiled paths
// against the plain one), so a change here changes every path at once.
#pragma once
#include <math.h>

#include "common.h"

namespace dvie {

// uint8 -> [-1, 1].  clip.hip (the training path) has the one other copy of this expression; the
// two must agree bit for bit.
__device__ __forceinline__ float px_normalise(uint8_t s) { return ((float)s / 255.f - 0.5f) / 0.5f; }

// t * 127.5 + 127.5 with the multiply and the add rounded separately: an fma changes bits at the
// half-points (43.5 comes out just below and rounds to 43).  HIP's __fmul_rn / __fadd_rn are a
// plain * and +, which the default -ffp-contract=fast fuses, so contraction is switched off here.
__device__ __forceinline__ float px_scale_unfused(float t) {
#pragma clang fp contract(off)
  const float m = t * 127.5f;
  return m + 127.5f;
}

// [-1, 1] (clamped) -> 0 .. 255, half to even
__device__ __forceinline__ int px_quantise(float v) {
  const float t = fminf(fmaxf(v, -1.f), 1.f);
  return (int)rintf(px_scale_unfused(t));
}

// One group of four logits, channels c0 .. c0 + 3, against the running maximum: strict >, so the
// first maximum wins; padding channels (>= n_classes) are never compared.
__device__ __forceinline__ void argmax_step(f32x4 v, int c0, int n_classes, float& best, int& bi) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < n_classes && v[k] > best) {
      best = v[k];
      bi = c0 + k;
    }
}

// argmax over a pixel's logits (16-byte loads; s is 16-byte aligned)
__device__ __forceinline__ int argmax_logits(const float* s, int n_classes) {
  float best = -INFINITY;  // (an all -inf row keeps index 0, as argmax does)
  int bi = 0;
#pragma unroll 2
  for (int c0 = 0; c0 < n_classes; c0 += 4) argmax_step(*(const f32x4*)(s + c0), c0, n_classes, best, bi);
  return bi;
}

// The four lanes of a quad (threadIdx.x & ~3 .. + 3) exchange their labels in registers and lane 0
// stores them as one dword at dst, which is 4-byte aligned (only lane 0's dst is used).  All four
// lanes must call this; `store` false keeps the exchange and drops the store.
__device__ __forceinline__ void label_quad_store(uint8_t* dst_of_quad_lane0, uint32_t lab, bool store = true) {
  const int j = threadIdx.x & 3;
  uint32_t w = lab << (8 * j);
  w |= __shfl_xor(w, 1);
  w |= __shfl_xor(w, 2);
  if (store && j == 0) *(uint32_t*)dst_of_quad_lane0 = w;
}

// The padded-canvas kernels launch one block row per canvas row: blockIdx.x = image * hp + y.
struct canvas_pos {
  int row, img, y;
};
__device__ __forceinline__ canvas_pos canvas_row(int hp) {
  canvas_pos c;
  c.row = blockIdx.x;
  c.img = c.row / hp;
  c.y = c.row - c.img * hp;
  return c;
}

// the integer luma of an 8-bit pixel, 0 .. 255 (the weights sum to 256)
__device__ __forceinline__ uint32_t px_luma(uint32_t r, uint32_t g, uint32_t b) {
  return (77u * r + 150u * g + 29u * b + 128u) >> 8;
}
__device__ __forceinline__ uint32_t px_luma(uint32_t px) {  // px = R | G << 8 | B << 16
  return px_luma(px & 255u, (px >> 8) & 255u, (px >> 16) & 255u);
}
__device__ __forceinline__ uint32_t px_luma(const uint8_t* q) { return px_luma(q[0], q[1], q[2]); }

}  // namespace dvie
