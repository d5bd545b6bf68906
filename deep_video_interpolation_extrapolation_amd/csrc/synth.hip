// The two pointwise ends of a device-resident inference forward (synth.py VideoSynthesizer):
//   dvie_synth_load    uint8 RGB frames -> the fp32 NHWC form the HRNet plan reads (and writes:
//                      the shape and strides of its external `rgb` output);
//   dvie_synth_finish  the plan's fp32 rgb / segmentation-logit outputs -> uint8 frames and
//                      uint8 label maps (clamp + quantise, argmax);
//   dvie_synth_bridge  between two plans of a two-stage forward: an fp32 image and the coarse
//                      logits -> [clamp(image) | softmax(logits)] in the next plan's input buffer;
//   dvie_synth_load_pad / dvie_synth_finish_crop  load and finish for a frame of any size on a
//                      padded canvas: the replicate padding and the crop happen in these launches.
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
//
// The per-pixel arithmetic (normalise, quantise, argmax, the quad's label store, the canvas
// geometry) is pixel.h's, shared with tile.hip.
#include <math.h>

#include "common.h"
#include "pixel.h"

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
    for (int c = 0; c < 3; ++c) v[c] = px_normalise(s[c]);
  }
  *(f32x4*)(p.out + pix * p.out_ld + 4 * q) = v;
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
    for (int c = 0; c < 3; ++c) rgb |= (uint32_t)px_quantise(v[c]) << (8 * c);
  }
  if (p.label) lab = (uint32_t)argmax_logits(p.seg + pp * p.seg_ld, p.n_classes);
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
    if (p.label) label_quad_store(p.label + q0, lab, full);
  }
  if (!full && live) {
    if (p.frame) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.frame[3 * pix + c] = (uint8_t)(rgb >> (8 * c));
    }
    if (p.label) p.label[pix] = (uint8_t)lab;
  }
}

// The padded-canvas forms of load and finish (dvie.h).  Both launch one block row per canvas row
// (blockIdx.x = image * hp + y, blockIdx.y = the 256-thread chunk of the row), so the canvas
// coordinates cost one 32-bit division per thread and nothing is 64-bit but the addresses.
//
// load_pad: four output floats per thread as in load, a wave's stores one contiguous run of a
// canvas row; the thread that owns a pixel's channels 0-3 also copies its label byte.
__global__ __launch_bounds__(256) void synth_load_pad_kernel(const dvie_synth_load_pad_desc p, int ldq) {
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= p.wp * ldq) return;
  const int x = e / ldq, q = e - x * ldq;
  const canvas_pos cv = canvas_row(p.hp);
  const long long pix = (long long)cv.row * p.wp + x;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (q == 0) {
    const long long src = ((long long)cv.img * p.h + min(cv.y, p.h - 1)) * p.w + min(x, p.w - 1);
    const uint8_t* s = p.frames + src * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = px_normalise(s[c]);
    if (p.labels) p.label_out[pix] = p.labels[src];
  }
  *(f32x4*)(p.out + pix * p.out_ld + 4 * q) = v;
}

// finish_crop: one lane per CANVAS pixel, finish's loads.  wp % 4 == 0, so the four lanes of a
// quad are four pixels of one canvas row and label_canvas keeps finish's dword stores
// (kCanvasDword: label_canvas is 4-byte aligned).  The cropped outputs have rows of w * 3 and w
// bytes at any alignment and are stored bytewise.  A pad pixel loads its logits only for
// label_canvas and its rgb never.
template <bool kCanvasDword>
__global__ __launch_bounds__(256) void synth_finish_crop_kernel(const dvie_synth_finish_crop_desc p) {
  const int x = blockIdx.y * 256 + threadIdx.x;
  if (x >= p.wp) return;  // (whole quads: wp and 256 are multiples of 4)
  const canvas_pos cv = canvas_row(p.hp);
  const bool inside = cv.y < p.h && x < p.w;
  if (!inside && !p.label_canvas) return;  // (no exchange follows without label_canvas)
  const long long pix = (long long)cv.row * p.wp + x;
  const uint32_t lab = (uint32_t)argmax_logits(p.seg + pix * p.seg_ld, p.n_classes);
  if (p.label_canvas) {
    if (kCanvasDword)
      label_quad_store(p.label_canvas + pix, lab);
    else
      p.label_canvas[pix] = (uint8_t)lab;
  }
  if (inside) {
    const long long o = ((long long)cv.img * p.h + cv.y) * p.w + x;
    const f32x4 v = *(const f32x4*)(p.rgb + pix * p.rgb_ld);  // v[3] is padding: loaded, never used
#pragma unroll
    for (int c = 0; c < 3; ++c) p.frame[3 * o + c] = (uint8_t)px_quantise(v[c]);
    p.label[o] = (uint8_t)lab;
  }
}

// dvie_synth_bridge: one lane owns one pixel, as in finish (its 16-byte loads walk the pixel's
// own 12 + 80 bytes of image and logits) and holds the pixel's whole span in registers, so the
// stores are whole 16-byte vectors of one contiguous run per lane (48 .. 160 B); the runs of a
// wave are dst_ld apart (contiguous for `in_x`, whose span is the whole pixel).
// The softmax is softmax_fwd_kernel's (gan.hip), expression for expression: nothing in it is a
// multiply followed by an add, so there is nothing for -ffp-contract=fast to fuse.
template <typename T, int NRGB, int RW, int SW>
__global__ __launch_bounds__(256) void synth_bridge_kernel(const dvie_synth_bridge_desc p) {
  constexpr int NCLS = 20, SPAN = NRGB * RW + SW, VW = 16 / (int)sizeof(T);
  static_assert(SPAN % VW == 0, "the span is a whole number of 16-byte vectors");
  const long long pix = blockIdx.x * 256LL + threadIdx.x;
  if (pix >= p.npix) return;
  float o[SPAN];
#pragma unroll
  for (int k = 0; k < SPAN; ++k) o[k] = 0.f;  // (the padding channels are written, as zeros)
  const f32x4 v = *(const f32x4*)(p.rgb + pix * p.rgb_ld);  // v[3] is padding: loaded, never used
#pragma unroll
  for (int r = 0; r < NRGB; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[r * RW + c] = fminf(fmaxf(v[c], -1.f), 1.f);
  const float* s = p.seg + pix * p.seg_ld;
  float x[NCLS];
#pragma unroll
  for (int c0 = 0; c0 < NCLS; c0 += 4) {
    const f32x4 t = *(const f32x4*)(s + c0);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[c0 + k] = t[k];
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NCLS; ++k) m = fmaxf(m, x[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < NCLS; ++k) sum += expf(x[k] - m);
  const float inv = 1.f / sum;
#pragma unroll
  for (int k = 0; k < NCLS; ++k) o[NRGB * RW + k] = expf(x[k] - m) * inv;
  T* d = (T*)p.dst + pix * p.dst_ld;
#pragma unroll
  for (int k = 0; k < SPAN; k += VW) {
    if constexpr (sizeof(T) == 4) {
      *(f32x4*)(d + k) = f32x4{o[k], o[k + 1], o[k + 2], o[k + 3]};
    } else {
      i32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w[j] = (int)((uint32_t)f2bf(o[k + 2 * j]) | ((uint32_t)f2bf(o[k + 2 * j + 1]) << 16));
      *(i32x4*)(d + k) = w;
    }
  }
}

template <typename T, int NRGB, int RW, int SW>
static void launch_bridge(const dvie_synth_bridge_desc& d, unsigned blocks, hipStream_t s) {
  DVIE_LAUNCH((synth_bridge_kernel<T, NRGB, RW, SW>), dim3(blocks), dim3(256), 0, s, d);
}

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_bridge(const dvie_synth_bridge_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->rgb && d->seg && d->dst, "synth_bridge: rgb / seg / dst must not be null");
  DVIE_CHECK_ARG(d->npix > 0, "synth_bridge: npix must be positive");
  DVIE_CHECK_ARG(d->dtype == DVIE_F32 || d->dtype == DVIE_BF16, "synth_bridge: dtype=%d", d->dtype);
  DVIE_CHECK_ARG(d->n_rgb == 1 || d->n_rgb == 2, "synth_bridge: n_rgb=%d must be 1 or 2", d->n_rgb);
  DVIE_CHECK_ARG(d->rgb_w == 4 || d->rgb_w == 8, "synth_bridge: rgb_w=%d must be 4 or 8", d->rgb_w);
  DVIE_CHECK_ARG(d->seg_w == 20 || d->seg_w == 24, "synth_bridge: seg_w=%d must be 20 or 24", d->seg_w);
  const int span = d->n_rgb * d->rgb_w + d->seg_w, es = d->dtype == DVIE_BF16 ? 2 : 4;
  DVIE_CHECK_ARG(span <= d->dst_ld, "synth_bridge: the span of %d channels does not fit in dst_ld=%d", span, d->dst_ld);
  DVIE_CHECK_ARG(span * es % 16 == 0 && (long long)d->dst_ld * es % 16 == 0 && (((uintptr_t)d->dst) & 15) == 0,
                 "synth_bridge: span=%d and dst_ld=%d must be whole 16-byte vectors of the dtype, dst 16-byte aligned",
                 span, d->dst_ld);
  DVIE_CHECK_ARG(d->rgb_ld >= 4 && d->rgb_ld % 4 == 0 && d->seg_ld >= 20 && d->seg_ld % 4 == 0 &&
                     ((((uintptr_t)d->rgb) | ((uintptr_t)d->seg)) & 15) == 0,
                 "synth_bridge: rgb_ld=%d (>= 4) and seg_ld=%d (>= 20) must be multiples of 4, rgb / seg 16-byte aligned",
                 d->rgb_ld, d->seg_ld);
  const long long blocks = (d->npix + 255) / 256;
  DVIE_CHECK_ARG(blocks < (1LL << 31), "synth_bridge: grid too large");
  const unsigned nb = (unsigned)blocks;
  hipStream_t s = (hipStream_t)stream;
  const int key = (d->n_rgb - 1) * 4 + (d->rgb_w == 8) * 2 + (d->seg_w == 24);
  if (d->dtype == DVIE_F32) {
    switch (key) {
      case 0: launch_bridge<float, 1, 4, 20>(*d, nb, s); break;
      case 1: launch_bridge<float, 1, 4, 24>(*d, nb, s); break;
      case 2: launch_bridge<float, 1, 8, 20>(*d, nb, s); break;
      case 3: launch_bridge<float, 1, 8, 24>(*d, nb, s); break;
      case 4: launch_bridge<float, 2, 4, 20>(*d, nb, s); break;
      case 5: launch_bridge<float, 2, 4, 24>(*d, nb, s); break;
      case 6: launch_bridge<float, 2, 8, 20>(*d, nb, s); break;
      default: launch_bridge<float, 2, 8, 24>(*d, nb, s); break;
    }
  } else {  // (the spans of 28 and 36 channels are no whole bf16 vectors: refused above)
    switch (key) {
      case 0: launch_bridge<bf16_t, 1, 4, 20>(*d, nb, s); break;
      case 3: launch_bridge<bf16_t, 1, 8, 24>(*d, nb, s); break;
      case 5: launch_bridge<bf16_t, 2, 4, 24>(*d, nb, s); break;
      default: launch_bridge<bf16_t, 2, 8, 24>(*d, nb, s); break;
    }
  }
  DVIE_RETURN_LAUNCH();
}

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

int dvie_synth_load_pad(const dvie_synth_load_pad_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->frames && d->out, "synth_load_pad: frames / out must not be null");
  DVIE_CHECK_ARG((d->labels != nullptr) == (d->label_out != nullptr),
                 "synth_load_pad: labels and label_out must be given together");
  DVIE_CHECK_ARG(d->n >= 1, "synth_load_pad: n=%d must be positive", d->n);
  DVIE_CHECK_ARG(d->h >= 1 && d->h <= d->hp, "synth_load_pad: h=%d must be in 1..hp=%d", d->h, d->hp);
  DVIE_CHECK_ARG(d->w >= 1 && d->w <= d->wp, "synth_load_pad: w=%d must be in 1..wp=%d", d->w, d->wp);
  DVIE_CHECK_ARG(d->out_ld >= 4 && d->out_ld % 4 == 0 && (((uintptr_t)d->out) & 15) == 0,
                 "synth_load_pad: out_ld=%d must be a multiple of 4 (>= 4) and out 16-byte aligned", d->out_ld);
  const int ldq = d->out_ld / 4;
  const long long rows = (long long)d->n * d->hp, chunks = ((long long)d->wp * ldq + 255) / 256;
  DVIE_CHECK_ARG(rows < (1LL << 31) && chunks <= 65535, "synth_load_pad: grid too large");
  DVIE_LAUNCH(synth_load_pad_kernel, dim3((unsigned)rows, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, *d, ldq);
  DVIE_RETURN_LAUNCH();
}

int dvie_synth_finish_crop(const dvie_synth_finish_crop_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->rgb && d->seg && d->frame && d->label,
                 "synth_finish_crop: rgb / seg / frame / label must not be null");
  DVIE_CHECK_ARG(d->n >= 1, "synth_finish_crop: n=%d must be positive", d->n);
  DVIE_CHECK_ARG(d->h >= 1 && d->h <= d->hp, "synth_finish_crop: h=%d must be in 1..hp=%d", d->h, d->hp);
  DVIE_CHECK_ARG(d->w >= 1 && d->w <= d->wp, "synth_finish_crop: w=%d must be in 1..wp=%d", d->w, d->wp);
  DVIE_CHECK_ARG(d->wp % 4 == 0, "synth_finish_crop: wp=%d must be a multiple of 4", d->wp);
  DVIE_CHECK_ARG(d->rgb_ld % 4 == 0 && d->seg_ld % 4 == 0 && d->rgb_ld >= 4 && d->seg_ld >= 4,
                 "synth_finish_crop: leading dimensions rgb_ld=%d seg_ld=%d must be multiples of 4 (>= 4)", d->rgb_ld,
                 d->seg_ld);
  DVIE_CHECK_ARG(((((uintptr_t)d->rgb) | ((uintptr_t)d->seg)) & 15) == 0,
                 "synth_finish_crop: rgb / seg must be 16-byte aligned");
  DVIE_CHECK_ARG(d->n_classes > 0 && d->n_classes <= d->seg_ld && d->n_classes <= 256,
                 "synth_finish_crop: n_classes=%d must be in 1..min(seg_ld=%d, 256)", d->n_classes, d->seg_ld);
  const long long rows = (long long)d->n * d->hp, chunks = ((long long)d->wp + 255) / 256;
  DVIE_CHECK_ARG(rows < (1LL << 31) && chunks <= 65535, "synth_finish_crop: grid too large");
  const dim3 grid((unsigned)rows, (unsigned)chunks);
  if ((((uintptr_t)d->label_canvas) & 3) == 0)
    DVIE_LAUNCH(synth_finish_crop_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *d);
  else
    DVIE_LAUNCH(synth_finish_crop_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
