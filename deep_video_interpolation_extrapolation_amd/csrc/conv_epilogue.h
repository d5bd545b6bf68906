// The epilogue every bf16 MFMA convolution kernel ends with, on the 8 consecutive channels a
// lane owns after the accumulator transposition: bias, residual, accumulate target (beta),
// activation, activation derivative taken from z, pack / store.  A kernel keeps what is its
// own -- where the operands come from, the bounds tests, the addresses, the store instruction
// -- and takes the arithmetic from here.
//
// Written so that a kernel built on these helpers compiles to the code of the hand-written
// sequence: operand flags known at compile time are template parameters (if constexpr), and
// operands already in registers are passed by pointer, never by value.
#pragma once
#include "common.h"

namespace dvie {

// F32OUT: the epilogue stores fp32 (e.g. the fp32 head outputs of a bf16 plan): ELU / tanh
// through expm1f / tanhf; the short v_exp_f32 forms (common.h) are for bf16 stores only
template <bool F32OUT = false>
__device__ __forceinline__ void act8(float* v, int act, float alpha) {
  if (act == DVIE_ACT_LRELU) {
    for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * alpha;
  } else if (act == DVIE_ACT_RELU) {
    for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
  } else if (act == DVIE_ACT_ELU) {
    for (int k = 0; k < 8; ++k) v[k] = F32OUT ? (v[k] > 0.f ? v[k] : expm1f(v[k])) : elu_bf(v[k]);
  } else if (act == DVIE_ACT_TANH) {
    for (int k = 0; k < 8; ++k) v[k] = F32OUT ? tanhf(v[k]) : tanh_bf(v[k]);
  }
}

// v *= act'(.) expressed through the activation OUTPUT z (ReLU as a select: a zero keeps v's
// sign out of the result and stops a non-finite v)
__device__ __forceinline__ void dact8(float* v, const float* z, int dact, float alpha) {
  if (dact == DVIE_ACT_LRELU) {
    for (int k = 0; k < 8; ++k) v[k] *= z[k] > 0.f ? 1.f : alpha;
  } else if (dact == DVIE_ACT_RELU) {
    for (int k = 0; k < 8; ++k) v[k] = z[k] > 0.f ? v[k] : 0.f;
  } else if (dact == DVIE_ACT_ELU) {
    for (int k = 0; k < 8; ++k) v[k] *= z[k] > 0.f ? 1.f : z[k] + 1.f;
  } else if (dact == DVIE_ACT_TANH) {
    for (int k = 0; k < 8; ++k) v[k] *= 1.f - z[k] * z[k];
  }
}

__device__ __forceinline__ void unpack_bf16x8(const i32x4 t, float* v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = __uint_as_float(((uint32_t)t[e]) << 16);
    v[2 * e + 1] = __uint_as_float(((uint32_t)t[e]) & 0xffff0000u);
  }
}

__device__ __forceinline__ void add_bf16x8(float* w, const i32x4 t) {
  float v[8];
  unpack_bf16x8(t, v);
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] += v[e];
}

// w += 8 consecutive floats at s (16-byte aligned)
__device__ __forceinline__ void add_f32x8(float* w, const float* s) {
  const f32x4 r0 = *(const f32x4*)s, r1 = *(const f32x4*)(s + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    w[e] += r0[e];
    w[4 + e] += r1[e];
  }
}

__device__ __forceinline__ i32x4 pack_bf16x8(const float* w) {
  i32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (int)pack_bf16x2(w[2 * e], w[2 * e + 1]);
  return o;
}

// dact8 with z as loaded (8 packed bf16)
__device__ __forceinline__ void dact_bf16x8(float* w, const i32x4 tz, int dact, float alpha) {
  float z[8];
  unpack_bf16x8(tz, z);
  dact8(w, z, dact, alpha);
}

// dact8 for LRELU / RELU with the factor taken from the activation sign bitmap
// (dvie_conv_desc.zbits): bit k of `bits` is z[k] > 0 of the lane's 8 channels
__device__ __forceinline__ void dact_bits8(float* w, unsigned bits, int dact, float alpha) {
  if (dact == DVIE_ACT_LRELU) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] *= (bits >> k) & 1u ? 1.f : alpha;
  } else if (dact == DVIE_ACT_RELU) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (bits >> k) & 1u ? w[k] : 0.f;
  }
}

// the bitmap byte of 8 packed bf16 results: bit k = (stored value k > 0), what a reader of
// z computes in dact8 (taken from the rounded bf16, not from the fp32 value before the pack)
__device__ __forceinline__ unsigned sign_bits8(const i32x4 packed) {
  float z[8];
  unpack_bf16x8(packed, z);
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) bits |= (z[k] > 0.f ? 1u : 0u) << k;
  return bits;
}

// bf16 epilogue arithmetic from operands already in registers (R residual, B accumulate
// target, Z activation input; an operand whose flag is off is never read): the packed result,
// the store is the kernel's
template <bool R, bool B, bool Z>
__device__ __forceinline__ i32x4 epi8_regs(float* w, const dvie_conv_desc& p, const i32x4* r, const i32x4* b,
                                           const i32x4* z) {
  if constexpr (R) add_bf16x8(w, *r);
  if constexpr (B) add_bf16x8(w, *b);
  act8(w, p.act, p.alpha);
  if constexpr (Z) dact_bf16x8(w, *z, p.dact, p.alpha);
  return pack_bf16x8(w);
}

// epi8_regs with the activation input as its bitmap byte (LRELU / RELU derivative)
template <bool R, bool B>
__device__ __forceinline__ i32x4 epi8_regs_bits(float* w, const dvie_conv_desc& p, const i32x4* r, const i32x4* b,
                                                unsigned bits) {
  if constexpr (R) add_bf16x8(w, *r);
  if constexpr (B) add_bf16x8(w, *b);
  act8(w, p.act, p.alpha);
  dact_bits8(w, bits, p.dact, p.alpha);
  return pack_bf16x8(w);
}

// The whole epilogue of the lane's 8 channels at output pixel pix, channel co, operands read
// from memory: one 16-byte (bf16) or two 16-byte (fp32) stores
template <bool OUTF32>
__device__ __forceinline__ void epi8_mem(float* w, const dvie_conv_desc& p, long long pix, int co) {
  if (p.bias) add_f32x8(w, p.bias + co);
  if constexpr (OUTF32) {
    float* dst = (float*)p.y + pix * p.y_ld + co;
    if (p.res) add_f32x8(w, (const float*)p.res + pix * p.res_ld + co);
    if (p.beta) add_f32x8(w, dst);
    act8<true>(w, p.act, p.alpha);
    if (p.dact) dact_bf16x8(w, *(const i32x4*)((const bf16_t*)p.z + pix * p.z_ld + co), p.dact, p.alpha);
    *(f32x4*)dst = f32x4{w[0], w[1], w[2], w[3]};
    *(f32x4*)(dst + 4) = f32x4{w[4], w[5], w[6], w[7]};
  } else {
    bf16_t* dst = (bf16_t*)p.y + pix * p.y_ld + co;
    if (p.res) add_bf16x8(w, *(const i32x4*)((const bf16_t*)p.res + pix * p.res_ld + co));
    if (p.beta) add_bf16x8(w, *(const i32x4*)dst);
    act8(w, p.act, p.alpha);
    if (p.dact) dact_bf16x8(w, *(const i32x4*)((const bf16_t*)p.z + pix * p.z_ld + co), p.dact, p.alpha);
    *(i32x4*)dst = pack_bf16x8(w);
  }
}

}  // namespace dvie
