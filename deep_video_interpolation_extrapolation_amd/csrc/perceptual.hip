// Per-frame VGG19 feature-cosine score of uint8 frames (synth.PerceptualScorer; include/dvie.h
// has the semantics).  Two ends of the VGG scoring plan:
//
//   dvie_synth_vgg_load  uint8 RGB frame pairs -> the plan's NHWC input buffer (2n, h16, w16, 8)
//                        in the plan dtype, images [pred_0 .. pred_{n-1} | gt_0 .. gt_{n-1}]
//                        (or, chunk by chunk, a part of such a batch).
//   dvie_cosfeat         mode 0: per-image cosine partials of one feature tap (a plan op after the
//                        tap's conv); mode 1: the finalize launch, the plan's last op.
//
// vgg_load_kernel: one pixel per thread, blockIdx.y the destination image.  The normalisation
// (byte / 255 - mean_c) / std_c is a 3 x 256 table the host rounded once (float64 -> fp32, and
// for a bf16 plan fp32 -> bf16 nearest even): the block copies it into LDS, a pixel is three
// byte loads (no alignment assumed, as synth_load) and three LDS lookups, no division and no
// rounding on the device.  A pixel is stored as whole 16-byte vectors, channels 3..7 zero: one
// vector in bf16, two in fp32, so a wave writes one contiguous 1 KiB / 2 KiB run.  The crop to
// (h16, w16) is read in place through the source row pitch 3 * w.
//
// cosfeat_kernel: L = min(64, C / V) lanes own one pixel (V = 8 bf16 / 4 fp32 channels per 16-byte
// load); a wave's load is 64 / L consecutive pixels, one contiguous run where the channel pitch
// equals C.  dot, |a|^2 and |b|^2 are summed in fp32 per lane, across the L lanes by xor
// shuffles, and the pixel's cosine dot / (sqrtf(saa) * sqrtf(sbb)) (cosnhwc_kernel's expression,
// 0/0 = NaN included) is added in float64 by the pixel's first lane.  A block of 256 threads
// walks COS_IT passes of 256 / L pixels of ONE image (blockIdx.y), sums its 256 float64 values
// through the fixed LDS tree of common.h and writes one partial: no atomics, the same bits every run.
//
// cosfeat_finalize_kernel: one block per image; per tap the partials are summed in index order
// per thread and through the same fixed tree, divided by the tap's pixel count, and the taps'
// means are averaged into one float64.
#include <type_traits>

#include "common.h"

namespace dvie {

namespace {

constexpr int COS_TB = 256;  // threads of a block
constexpr int COS_IT = 16;   // passes of a block over its image

struct cos_geom {
  int vec;  // channels of a 16-byte load
  int nv;   // 16-byte vectors of a pixel
  int L;    // lanes of a pixel
  int ppb;  // pixels of a block
};

__host__ __device__ __forceinline__ cos_geom cos_geom_of(int c, int dtype) {
  cos_geom g;
  g.vec = dtype == DVIE_BF16 ? 8 : 4;
  g.nv = c / g.vec;
  g.L = g.nv < 64 ? g.nv : 64;
  g.ppb = g.L > 0 ? COS_TB / g.L * COS_IT : 0;
  return g;
}

__device__ __forceinline__ void cos_fma8(const i32x4 a, const i32x4 b, float& dot, float& saa, float& sbb) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a0 = __uint_as_float(((uint32_t)a[k]) << 16), a1 = __uint_as_float(((uint32_t)a[k]) & 0xffff0000u);
    const float b0 = __uint_as_float(((uint32_t)b[k]) << 16), b1 = __uint_as_float(((uint32_t)b[k]) & 0xffff0000u);
    dot += a0 * b0;
    saa += a0 * a0;
    sbb += b0 * b0;
    dot += a1 * b1;
    saa += a1 * a1;
    sbb += b1 * b1;
  }
}

__device__ __forceinline__ void cos_fma4(const f32x4 a, const f32x4 b, float& dot, float& saa, float& sbb) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    dot += a[k] * b[k];
    saa += a[k] * a[k];
    sbb += b[k] * b[k];
  }
}

}  // namespace

template <bool kBf16>
__global__ __launch_bounds__(256) void vgg_load_kernel(const dvie_synth_vgg_load_desc p) {
  typedef typename std::conditional<kBf16, uint16_t, float>::type E;
  __shared__ E s_lut[3 * 256];
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) s_lut[c * 256 + t] = ((const E*)p.lut)[c * 256 + t];
  __syncthreads();
  const int n = p.n0 * p.n1;
  const int src_img = blockIdx.y;  // [pred_0 .. pred_{n-1} | gt_0 .. gt_{n-1}] of this call
  const int f = src_img < n ? src_img : src_img - n;
  const int img = p.img0 + f + (src_img < n ? 0 : p.n_out);  // its place among the 2 * n_out images
  const int i0 = f / p.n1, i1 = f - i0 * p.n1;
  const uint8_t* src = src_img < n ? p.pred + i0 * p.pred_s0 + i1 * p.pred_s1 : p.gt + i0 * p.gt_s0 + i1 * p.gt_s1;
  const int npx = p.h16 * p.w16;
  const int px = blockIdx.x * 256 + t;
  if (px >= npx) return;
  const int y = px / p.w16, x = px - y * p.w16;
  const uint8_t* s = src + ((long long)y * p.w + x) * 3;
  const E v0 = s_lut[s[0]], v1 = s_lut[256 + s[1]], v2 = s_lut[512 + s[2]];
  const long long o = ((long long)img * npx + px) * 8;
  if constexpr (kBf16) {
    i32x4 r = {(int)((uint32_t)v0 | ((uint32_t)v1 << 16)), (int)(uint32_t)v2, 0, 0};
    *(i32x4*)((uint16_t*)p.out + o) = r;
  } else {
    float* d = (float*)p.out + o;
    *(f32x4*)d = f32x4{v0, v1, v2, 0.f};
    *(f32x4*)(d + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <bool kBf16>
__global__ __launch_bounds__(COS_TB) void cosfeat_kernel(const dvie_cosfeat_desc p) {
  __shared__ double s_d[COS_TB];
  const cos_geom g = cos_geom_of(p.c, p.dtype);
  const int t = threadIdx.x, sub = t & (g.L - 1), grp = t / g.L, per_pass = COS_TB / g.L;
  const int npx = p.h * p.w, img = blockIdx.y;
  const int es = kBf16 ? 2 : 4;
  const long long img_bytes = (long long)npx * p.ld * es;
  const char* a = (const char*)p.feat + img * img_bytes;
  const char* b = (const char*)p.feat + (long long)(p.n + img) * img_bytes;
  const int px0 = blockIdx.x * g.ppb;
  double acc = 0.0;
  for (int it = 0; it < COS_IT; ++it) {
    const int base = px0 + it * per_pass;
    if (base >= npx) break;  // (uniform over the block)
    const int px = base + grp;
    const bool live = px < npx;
    float dot = 0.f, saa = 0.f, sbb = 0.f;
    if (live) {
      const long long o = (long long)px * p.ld * es;
      for (int k = sub; k < g.nv; k += g.L) {
        if constexpr (kBf16)
          cos_fma8(*(const i32x4*)(a + o + 16LL * k), *(const i32x4*)(b + o + 16LL * k), dot, saa, sbb);
        else
          cos_fma4(*(const f32x4*)(a + o + 16LL * k), *(const f32x4*)(b + o + 16LL * k), dot, saa, sbb);
      }
    }
    for (int s = 1; s < g.L; s <<= 1) {
      dot += __shfl_xor(dot, s, 64);
      saa += __shfl_xor(saa, s, 64);
      sbb += __shfl_xor(sbb, s, 64);
    }
    if (live && sub == 0) acc += (double)(dot / (sqrtf(saa) * sqrtf(sbb)));
  }
  lds_tree_sum<COS_TB>(acc, s_d);
  if (t == 0) p.ws[((long long)p.tap * p.n + img) * p.ws_blocks + blockIdx.x] = s_d[0];
}

__global__ __launch_bounds__(COS_TB) void cosfeat_finalize_kernel(const dvie_cosfeat_desc p) {
  __shared__ double s_d[COS_TB];
  const int t = threadIdx.x, img = blockIdx.x;
  double total = 0.0;
  for (int tap = 0; tap < p.n_taps; ++tap) {
    const double* w = p.ws + ((long long)tap * p.n + img) * p.ws_blocks;
    double s = 0.0;
    for (int j = t; j < p.blocks[tap]; j += COS_TB) s += w[j];
    lds_tree_sum<COS_TB>(s, s_d);
    const double v = s_d[0];
    __syncthreads();  // (s_d[0] is read by every thread before the next tap writes it)
    total += v / (double)p.px[tap];
  }
  if (t == 0) p.out[img] = total / (double)p.n_taps;
}

// 0: the sizes are invalid (dvie_cosfeat then says why)
static int cosfeat_blocks_of(const dvie_cosfeat_desc* d) {
  if (!d || d->h < 1 || d->w < 1 || (long long)d->h * d->w > 0x3fffffffLL || d->c < 1) return 0;
  if (d->dtype != DVIE_F32 && d->dtype != DVIE_BF16) return 0;
  const cos_geom g = cos_geom_of(d->c, d->dtype);
  if (g.nv < 1 || g.nv * g.vec != d->c || (g.nv & (g.nv - 1))) return 0;
  return cdiv((long long)d->h * d->w, g.ppb);
}

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_vgg_load(const dvie_synth_vgg_load_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->pred && d->gt && d->out && d->lut, "synth_vgg_load: pred / gt / out / lut must not be null");
  DVIE_CHECK_ARG(d->dtype == DVIE_F32 || d->dtype == DVIE_BF16, "synth_vgg_load: dtype=%d", d->dtype);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n1 >= 1 && (long long)d->n0 * d->n1 <= 32767,
                 "synth_vgg_load: n0=%d x n1=%d frame pairs must be in 1..32767", d->n0, d->n1);
  DVIE_CHECK_ARG(d->img0 >= 0 && d->n_out <= 32767 && (long long)d->img0 + (long long)d->n0 * d->n1 <= d->n_out,
                 "synth_vgg_load: pairs img0=%d .. +%d must lie inside n_out=%d (<= 32767)", d->img0, d->n0 * d->n1, d->n_out);
  DVIE_CHECK_ARG(d->h16 >= 1 && d->w16 >= 1 && d->h16 <= d->h && d->w16 <= d->w,
                 "synth_vgg_load: the region %dx%d must lie inside the %dx%d frame", d->h16, d->w16, d->h, d->w);
  DVIE_CHECK_ARG((long long)d->h16 * d->w16 <= 0x7fffffffLL - 256 && d->w <= (1 << 29),
                 "synth_vgg_load: region %dx%d too large", d->h16, d->w16);
  DVIE_CHECK_ARG(((uintptr_t)d->out & 15) == 0 && ((uintptr_t)d->lut & 3) == 0,
                 "synth_vgg_load: out must be 16-byte aligned and lut 4-byte aligned");
  const dim3 grid((unsigned)cdiv((long long)d->h16 * d->w16, 256), (unsigned)(2 * d->n0 * d->n1));
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == DVIE_BF16)
    DVIE_LAUNCH(vgg_load_kernel<true>, grid, dim3(256), 0, s, *d);
  else
    DVIE_LAUNCH(vgg_load_kernel<false>, grid, dim3(256), 0, s, *d);
  DVIE_RETURN_LAUNCH();
}

int dvie_cosfeat_blocks(const dvie_cosfeat_desc* d) { return cosfeat_blocks_of(d); }

int dvie_cosfeat(const dvie_cosfeat_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->ws, "cosfeat: the partial workspace is missing");
  DVIE_CHECK_ARG(((uintptr_t)d->ws & 7) == 0, "cosfeat: ws must be 8-byte aligned");
  DVIE_CHECK_ARG(d->n >= 1 && d->n <= 32767, "cosfeat: n=%d image pairs must be in 1..32767", d->n);
  DVIE_CHECK_ARG(d->n_taps >= 1 && d->n_taps <= DVIE_COSFEAT_MAX_TAPS, "cosfeat: n_taps=%d must be in 1..%d", d->n_taps,
                 DVIE_COSFEAT_MAX_TAPS);
  DVIE_CHECK_ARG(d->ws_blocks >= 1, "cosfeat: ws_blocks=%d must be at least 1", d->ws_blocks);
  hipStream_t s = (hipStream_t)stream;
  if (d->mode == 1) {
    DVIE_CHECK_ARG(d->out && ((uintptr_t)d->out & 7) == 0, "cosfeat: out must not be null and 8-byte aligned");
    for (int t = 0; t < d->n_taps; ++t)
      DVIE_CHECK_ARG(d->blocks[t] >= 1 && d->blocks[t] <= d->ws_blocks && d->px[t] >= 1,
                     "cosfeat: tap %d has blocks=%d (ws_blocks=%d) px=%d", t, d->blocks[t], d->ws_blocks, d->px[t]);
    DVIE_LAUNCH(cosfeat_finalize_kernel, dim3((unsigned)d->n), dim3(COS_TB), 0, s, *d);
    DVIE_RETURN_LAUNCH();
  }
  DVIE_CHECK_ARG(d->mode == 0, "cosfeat: mode=%d must be 0 (tap partials) or 1 (finalize)", d->mode);
  DVIE_CHECK_ARG(d->feat, "cosfeat: feat must not be null");
  DVIE_CHECK_ARG(d->tap >= 0 && d->tap < d->n_taps, "cosfeat: tap=%d outside 0..%d", d->tap, d->n_taps - 1);
  const int blocks = cosfeat_blocks_of(d);
  DVIE_CHECK_ARG(blocks > 0,
                 "cosfeat: h=%d w=%d c=%d dtype=%d: c must be a power-of-two number of 16-byte vectors, h*w < 2^30", d->h,
                 d->w, d->c, d->dtype);
  DVIE_CHECK_ARG(blocks <= d->ws_blocks, "cosfeat: tap needs %d blocks per image, ws_blocks=%d", blocks, d->ws_blocks);
  const int es = d->dtype == DVIE_BF16 ? 2 : 4;
  DVIE_CHECK_ARG(d->ld >= d->c && ((uintptr_t)d->feat & 15) == 0 && (d->ld * es) % 16 == 0,
                 "cosfeat: feat must be 16-byte aligned and the channel pitch ld=%lld (>= c=%d) a whole number of "
                 "16-byte vectors", d->ld, d->c);
  const dim3 grid((unsigned)blocks, (unsigned)d->n);
  if (d->dtype == DVIE_BF16)
    DVIE_LAUNCH(cosfeat_kernel<true>, grid, dim3(COS_TB), 0, s, *d);
  else
    DVIE_LAUNCH(cosfeat_kernel<false>, grid, dim3(COS_TB), 0, s, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
