// The two pointwise ends of a device-resident inference forward (synth.py VideoSynthesizer):
//   dvie_synth_load    uint8 RGB frames -> the fp32 NHWC form the HRNet plan reads (and writes:
//                      the shape and strides of its external `rgb` output);
//   dvie_synth_finish  the plan's fp32 rgb / segmentation-logit outputs -> uint8 frames and
//                      uint8 label maps (clamp + quantise, argmax).
// They replace the eager glue of InterTrainer.mini_test (normalize, argmax, one_hot, cat and
// the fp32 20-channel one-hot kept per frame).
//
// Both are HBM-bound byte work, no MFMA, no LDS.  finish reads 128 B and writes 4 B per pixel:
// a lane owns ONE pixel, so its 16-byte loads walk that pixel's row (consecutive lanes are one
// pixel row, rgb_ld / seg_ld floats, apart and every fetched line is consumed by the same
// wave), and the four lanes of a quad then exchange their bytes in registers so that the
// stores are whole dwords of one contiguous run per wave (3 dwords of RGB, 1 of labels per
// quad).  More pixels per lane would widen the stores but spread each load instruction over
// four times the address range; the NCHW pack measured slower that way (profiles/r06/nchw4).
#include <math.h>

#include "common.h"

namespace dvie {

// One thread = 4 output floats of one pixel: the stores of a wave are one contiguous 1 KiB run.
__global__ __launch_bounds__(256) void synth_load_kernel(const dvie_synth_load_desc p, int ldq) {
  const long long e = blockIdx.x * 256LL + threadIdx.x;
  if (e >= p.npix * ldq) return;
  const long long pix = e / ldq;
  const int q = (int)(e - pix * ldq);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (q == 0) {
    const uint8_t* s = p.frames + pix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((float)s[c] / 255.f - 0.5f) / 0.5f;  // = clip.hip's, bit for bit
  }
  *(f32x4*)(p.out + pix * p.out_ld + 4 * q) = v;
}

// t * 127.5 + 127.5 with the multiply and the add rounded separately: an fma changes bits at the
// half-points (43.5 comes out just below and rounds to 43).  HIP's __fmul_rn / __fadd_rn are a
// plain * and +, which the default -ffp-contract=fast fuses, so contraction is switched off here.
__device__ __forceinline__ float scale_unfused(float t) {
#pragma clang fp contract(off)
  const float m = t * 127.5f;
  return m + 127.5f;
}

// kDword: frame and label are 4-byte aligned, so whole quads store dwords; partial quads (the
// last npix % 4 pixels) and unaligned outputs store bytes.
template <bool kDword>
__global__ __launch_bounds__(256) void synth_finish_kernel(const dvie_synth_finish_desc p) {
  const long long pix = blockIdx.x * 256LL + threadIdx.x;
  const bool live = pix < p.npix;
  const long long pp = live ? pix : p.npix - 1;  // (dead lanes stay for the quad exchange; they store nothing)
  uint32_t rgb = 0, lab = 0;
  if (p.frame) {
    const f32x4 v = *(const f32x4*)(p.rgb + pp * p.rgb_ld);  // v[3] is padding: loaded, never used
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = fminf(fmaxf(v[c], -1.f), 1.f);
      const float u = rintf(scale_unfused(t));  // half to even, in [0, 255]
      rgb |= (uint32_t)(int)u << (8 * c);
    }
  }
  if (p.label) {
    const float* s = p.seg + pp * p.seg_ld;
    float best = -INFINITY;  // (an all -inf row keeps index 0, as argmax does)
    int bi = 0;
#pragma unroll 2
    for (int c0 = 0; c0 < p.n_classes; c0 += 4) {
      const f32x4 v = *(const f32x4*)(s + c0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < p.n_classes && v[k] > best) {  // padding channels never compared
          best = v[k];
          bi = c0 + k;
        }
    }
    lab = (uint32_t)bi;
  }
  const int j = threadIdx.x & 3;
  const long long q0 = pix - j;  // first pixel of this lane's quad (a multiple of 4)
  const bool full = kDword && q0 + 3 < p.npix;
  if (kDword) {
    const int l0 = (threadIdx.x & 63) - j;
    if (p.frame) {
      const uint32_t r0 = __shfl(rgb, l0), r1 = __shfl(rgb, l0 + 1), r2 = __shfl(rgb, l0 + 2), r3 = __shfl(rgb, l0 + 3);
      // the quad's 12 bytes [p0.rgb p1.rgb p2.rgb p3.rgb] as three dwords
      const uint32_t d = j == 0 ? (r0 | (r1 << 24)) : (j == 1 ? ((r1 >> 8) | (r2 << 16)) : ((r2 >> 16) | (r3 << 8)));
      if (full && j < 3) ((uint32_t*)(p.frame + 3 * q0))[j] = d;
    }
    if (p.label) {
      uint32_t w = lab << (8 * j);
      w |= __shfl_xor(w, 1);
      w |= __shfl_xor(w, 2);
      if (full && j == 0) *(uint32_t*)(p.label + q0) = w;
    }
  }
  if (!full && live) {
    if (p.frame) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.frame[3 * pix + c] = (uint8_t)(rgb >> (8 * c));
    }
    if (p.label) p.label[pix] = (uint8_t)lab;
  }
}

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_load(const dvie_synth_load_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->frames && d->out && d->npix > 0, "synth_load: frames / out / npix");
  DVIE_CHECK_ARG(d->out_ld >= 4 && d->out_ld % 4 == 0 && (((uintptr_t)d->out) & 15) == 0,
                 "synth_load: out_ld=%d must be a multiple of 4 (>= 4) and out 16-byte aligned", d->out_ld);
  const int ldq = d->out_ld / 4;
  const long long blocks = (d->npix * ldq + 255) / 256;
  DVIE_CHECK_ARG(blocks < (1LL << 31), "synth_load: grid too large");
  DVIE_LAUNCH(synth_load_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *d, ldq);
  DVIE_RETURN_LAUNCH();
}

int dvie_synth_finish(const dvie_synth_finish_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->npix > 0, "synth_finish: npix must be positive");
  DVIE_CHECK_ARG(d->frame || d->label, "synth_finish: at least one of frame / label");
  DVIE_CHECK_ARG(d->rgb_ld % 4 == 0 && d->seg_ld % 4 == 0 && d->rgb_ld >= 0 && d->seg_ld >= 0,
                 "synth_finish: leading dimensions rgb_ld=%d seg_ld=%d must be multiples of 4", d->rgb_ld, d->seg_ld);
  if (d->frame)
    DVIE_CHECK_ARG(d->rgb && d->rgb_ld >= 4 && (((uintptr_t)d->rgb) & 15) == 0,
                   "synth_finish: rgb (16-byte aligned, rgb_ld >= 4) is needed for frame");
  if (d->label) {
    DVIE_CHECK_ARG(d->n_classes > 0 && d->n_classes <= d->seg_ld && d->n_classes <= 256,
                   "synth_finish: n_classes=%d must be in 1..min(seg_ld=%d, 256)", d->n_classes, d->seg_ld);
    DVIE_CHECK_ARG(d->seg && (((uintptr_t)d->seg) & 15) == 0, "synth_finish: seg (16-byte aligned) is needed for label");
  }
  const long long blocks = (d->npix + 255) / 256;
  DVIE_CHECK_ARG(blocks < (1LL << 31), "synth_finish: grid too large");
  const bool dword = ((((uintptr_t)d->frame) | ((uintptr_t)d->label)) & 3) == 0;
  if (dword)
    DVIE_LAUNCH(synth_finish_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *d);
  else
    DVIE_LAUNCH(synth_finish_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
