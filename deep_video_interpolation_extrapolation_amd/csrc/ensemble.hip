// dvie_synth_flip / dvie_synth_ens_acc: the two passes a self-ensemble adds around a forward
// (include/dvie.h has both contracts; DESIGN.md "Self-ensemble" the members, the sum order and the
// measurements).
//
// Both are pure streaming kernels: plain 16-byte loads and stores, no LDS, no atomics, no cross-lane
// traffic, and every output byte has exactly one owning lane, so nothing is read-modify-written
// (the accumulators are read and written by the same lane at the same address).
//
// synth_flip_kernel: one flat grid.  The first `fblocks` blocks mirror the fp32 images: a lane owns
// one 16-byte vector (4 channels) of one destination pixel and fetches it from the mirrored column
// of the source, so consecutive lanes write consecutive vectors and read whole pixels of a row
// backwards.  The other blocks mirror the label maps: a lane owns the 4 destination bytes
// [4k, 4k + 4) of one row.  When all 4 exist and both the destination bytes and the 4 source bytes
// they come from (columns w - 4k - 4 .. w - 4k - 1) sit on a dword boundary, the lane loads the
// dword, reverses its bytes and stores it; every other group -- the tail of a width that is no
// multiple of 4, and any row whose base is unaligned on either side -- moves byte by byte.
//
// synth_ens_acc_kernel: a lane owns one 16-byte vector of one accumulator pixel: the first
// rgb_ld / 4 vectors of a pixel's work are its image channels, the other seg_ld / 4 its logits.  A
// vector wholly inside the padding channels loads nothing and stores zeros.
#include "common.h"

namespace dvie {

namespace {

constexpr int ENS_T = 256;

__global__ __launch_bounds__(ENS_T) void synth_flip_kernel(const dvie_synth_flip_desc p, const unsigned fblocks,
                                                           const long long nvec, const int groups, const long long ngroups) {
  if (blockIdx.x < fblocks) {
    const long long idx = (long long)blockIdx.x * ENS_T + threadIdx.x;
    if (idx >= nvec) return;
    const int vpp = p.ld >> 2;
    const int v = (int)(idx % vpp);
    const long long pix = idx / vpp;
    const int x = (int)(pix % p.w);
    const long long row = pix / p.w;  // i * h + y
    const int y = (int)(row % p.h);
    const long long i = row / p.h;
    const float* s = p.src + i * p.src_stride + ((long long)y * p.w + (p.w - 1 - x)) * p.ld + 4 * v;
    V4<float>::store(p.dst + pix * p.ld + 4 * v, V4<float>::load(s));
    return;
  }
  const long long idx = (long long)(blockIdx.x - fblocks) * ENS_T + threadIdx.x;
  if (idx >= ngroups) return;
  const int x0 = 4 * (int)(idx % groups);
  const long long row = idx / groups;
  const int y = (int)(row % p.h);
  const long long i = row / p.h;
  uint8_t* d = p.ldst + row * p.w + x0;
  const uint8_t* srow = p.lsrc + i * p.lsrc_stride + (long long)y * p.w;
  const int nx = min(4, p.w - x0);
  const uint8_t* s4 = srow + (p.w - x0 - 4);  // the 4 source bytes of a whole group, ascending
  if (nx == 4 && ((((uintptr_t)d) | ((uintptr_t)s4)) & 3) == 0) {
    *(uint32_t*)d = __builtin_bswap32(*(const uint32_t*)s4);
    return;
  }
  for (int k = 0; k < nx; ++k) d[k] = srow[p.w - 1 - x0 - k];
}

__global__ __launch_bounds__(ENS_T) void synth_ens_acc_kernel(const dvie_synth_ens_acc_desc p, const long long nvec,
                                                              const float scale) {
  const long long idx = (long long)blockIdx.x * ENS_T + threadIdx.x;
  if (idx >= nvec) return;
  const int rv = p.rgb_ld >> 2, vpp = rv + (p.seg_ld >> 2);
  const int v = (int)(idx % vpp);
  const long long pix = idx / vpp;
  const bool img = v < rv;
  const int c0 = 4 * (img ? v : v - rv), lim = img ? 3 : p.n_classes, ld = img ? p.rgb_ld : p.seg_ld;
  float* acc = (img ? p.rgb_acc : p.seg_acc) + pix * ld + c0;
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (c0 < lim) {
    long long spix = pix;
    if (p.flip) {
      const int x = (int)(pix % p.w);
      spix = pix - x + (p.w - 1 - x);
    }
    const f32x4 m = V4<float>::load((img ? p.rgb : p.seg) + spix * ld + c0);
    f32x4 a = m;
    if (!p.first) a = V4<float>::load(acc) + m;
    if (p.last_m) a = a * scale;  // (a second rounding: a sum and a product do not contract)
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = c0 + j < lim ? a[j] : 0.f;
  }
  V4<float>::store(acc, r);
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void* a, long long na, const void* b, long long nb) {
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
  return ua < ub + (uintptr_t)nb && ub < ua + (uintptr_t)na;
}

}  // namespace

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_flip(const dvie_synth_flip_desc* d, void* stream) {
  DVIE_CHECK_ARG(d, "synth_flip: the descriptor must not be null");
  DVIE_CHECK_ARG(d->src && d->dst, "synth_flip: src / dst must not be null");
  DVIE_CHECK_ARG((d->lsrc != nullptr) == (d->ldst != nullptr), "synth_flip: lsrc and ldst must be given both or neither");
  DVIE_CHECK_ARG(d->n >= 1 && d->h >= 1 && d->w >= 1, "synth_flip: n=%d h=%d w=%d must be positive", d->n, d->h, d->w);
  DVIE_CHECK_ARG(d->ld >= 4 && d->ld % 4 == 0, "synth_flip: ld=%d must be a positive multiple of 4", d->ld);
  const long long img = (long long)d->h * d->w * d->ld, limg = (long long)d->h * d->w;
  DVIE_CHECK_ARG(d->src_stride % 4 == 0 && (d->n == 1 || d->src_stride >= img),
                 "synth_flip: src_stride=%lld must be a multiple of 4 and at least one image (%lld floats)", d->src_stride, img);
  DVIE_CHECK_ARG((((uintptr_t)d->src | (uintptr_t)d->dst) & 15) == 0, "synth_flip: src / dst must be 16-byte aligned");
  DVIE_CHECK_ARG((const float*)d->dst != d->src, "synth_flip: src == dst: the mirror is not done in place");
  const long long span = ((long long)(d->n - 1) * d->src_stride + img) * 4;
  DVIE_CHECK_ARG(!overlaps(d->src, span, d->dst, (long long)d->n * img * 4), "synth_flip: the src and dst ranges overlap");
  if (d->lsrc) {
    DVIE_CHECK_ARG(d->n == 1 || d->lsrc_stride >= limg, "synth_flip: lsrc_stride=%lld must be at least one label map (%lld bytes)",
                   d->lsrc_stride, limg);
    DVIE_CHECK_ARG((const uint8_t*)d->ldst != d->lsrc, "synth_flip: lsrc == ldst: the mirror is not done in place");
    DVIE_CHECK_ARG(!overlaps(d->lsrc, (long long)(d->n - 1) * d->lsrc_stride + limg, d->ldst, (long long)d->n * limg),
                   "synth_flip: the lsrc and ldst ranges overlap");
  }
  const long long nvec = (long long)d->n * limg * (d->ld / 4);
  const int groups = (d->w + 3) / 4;
  const long long ngroups = d->lsrc ? (long long)d->n * d->h * groups : 0;
  const long long fblocks = (nvec + ENS_T - 1) / ENS_T, lblocks = (ngroups + ENS_T - 1) / ENS_T;
  DVIE_CHECK_ARG(fblocks + lblocks <= 0x7fffffffLL, "synth_flip: grid too large (n=%d h=%d w=%d ld=%d)", d->n, d->h, d->w, d->ld);
  DVIE_LAUNCH(synth_flip_kernel, dim3((unsigned)(fblocks + lblocks)), dim3(ENS_T), 0, (hipStream_t)stream, *d,
              (unsigned)fblocks, nvec, groups, ngroups);
  DVIE_RETURN_LAUNCH();
}

int dvie_synth_ens_acc(const dvie_synth_ens_acc_desc* d, void* stream) {
  DVIE_CHECK_ARG(d, "synth_ens_acc: the descriptor must not be null");
  DVIE_CHECK_ARG(d->rgb && d->seg && d->rgb_acc && d->seg_acc, "synth_ens_acc: rgb / seg / rgb_acc / seg_acc must not be null");
  DVIE_CHECK_ARG(d->n >= 1 && d->h >= 1 && d->w >= 1, "synth_ens_acc: n=%d h=%d w=%d must be positive", d->n, d->h, d->w);
  DVIE_CHECK_ARG(d->rgb_ld >= 4 && d->rgb_ld % 4 == 0 && d->seg_ld >= 4 && d->seg_ld % 4 == 0,
                 "synth_ens_acc: leading dimensions rgb_ld=%d seg_ld=%d must be positive multiples of 4", d->rgb_ld, d->seg_ld);
  DVIE_CHECK_ARG(d->n_classes >= 1 && d->n_classes <= d->seg_ld, "synth_ens_acc: n_classes=%d must be in 1..seg_ld=%d",
                 d->n_classes, d->seg_ld);
  DVIE_CHECK_ARG(d->last_m == 0 || d->last_m == 2 || d->last_m == 4, "synth_ens_acc: last_m=%d must be 0, 2 or 4", d->last_m);
  DVIE_CHECK_ARG((d->flip == 0 || d->flip == 1) && (d->first == 0 || d->first == 1),
                 "synth_ens_acc: flip=%d and first=%d must be 0 or 1", d->flip, d->first);
  DVIE_CHECK_ARG((((uintptr_t)d->rgb | (uintptr_t)d->seg | (uintptr_t)d->rgb_acc | (uintptr_t)d->seg_acc) & 15) == 0,
                 "synth_ens_acc: rgb / seg / rgb_acc / seg_acc must be 16-byte aligned");
  const long long npix = (long long)d->n * d->h * d->w;
  const long long rb = npix * d->rgb_ld * 4, sb = npix * d->seg_ld * 4;
  const void* ptr[4] = {d->rgb, d->seg, d->rgb_acc, d->seg_acc};
  const long long len[4] = {rb, sb, rb, sb};
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      DVIE_CHECK_ARG(!overlaps(ptr[a], len[a], ptr[b], len[b]), "synth_ens_acc: the member and the accumulators overlap "
                     "(a member is added from its own buffers, not in place)");
  const long long nvec = npix * ((d->rgb_ld + d->seg_ld) / 4);
  const long long blocks = (nvec + ENS_T - 1) / ENS_T;
  DVIE_CHECK_ARG(blocks <= 0x7fffffffLL, "synth_ens_acc: grid too large (n=%d h=%d w=%d)", d->n, d->h, d->w);
  const float scale = d->last_m ? 1.f / (float)d->last_m : 1.f;
  DVIE_LAUNCH(synth_ens_acc_kernel, dim3((unsigned)blocks), dim3(ENS_T), 0, (hipStream_t)stream, *d, nvec, scale);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
