// dvie_synth_msssim: per-frame multi-scale SSIM of uint8 frames against the originals
// (include/dvie.h has the semantics; DESIGN.md "Multi-scale SSIM" the measurements).
//
// msssim_pyramid_kernel (K >= 2): a workgroup of 256 threads owns a 16-row x 64-pixel tile of one
// frame pair -- aligned to 2^(K-1) <= 16 in both directions, so every block of every level lies
// inside one tile.  It reads the tile's bytes of both frames once (byte loads, no alignment
// assumed) into LDS as uint16 and folds them 2x2 -> 2x2 ... between two LDS buffers, writing
// level 1 .. K-1 of both frames to the workspace as uint16 block SUMS (<= 255 * 4^4 = 65280:
// exact).  Integer arithmetic only.  A level's pixel (i, j) exists iff its whole block lies in the
// image ((i + 1) << s <= h), so no written value depends on a sample outside it.
//
// msssim_level_kernel: the row walk of ssim_walk.h (a workgroup of 192 threads, a 64-pixel strip
// of a 32-row segment, thread t one (pixel, channel) item) over ONE LEVEL of one pair.  Samples
// are the bytes of the frames at level 0 and the uint16 sums of the workspace above it; C1, C2
// come per level, scaled by (255 * 4^s)^2.  The grid's x dimension runs over the blocks of all K
// levels (level 0 first), so the small coarse levels fill the tail of the large one instead of
// being launches of a few blocks each.  A block sums cs, on the last level l * cs, and leaves one
// float64 partial through the fixed LDS tree of common.h.
//
// msssim_finalize_kernel: one block of five waves per pair; wave s sums the partials of level s in
// a fixed order and divides by 3 * h_s * w_s -> parts and its power (float64 pow); thread 0
// multiplies the K powers in order -> msssim.
#include "common.h"
#include "ssim_walk.h"

#include <algorithm>

namespace dvie {

namespace {

constexpr int MS_MAXK = 5;
constexpr int MS_WIN = 11;
constexpr int PY_ROWS = 16, PY_PX = 64, PY_IT = 3 * PY_PX, PY_THREADS = 256;

struct ms_level {
  long long src;   // uint16 elements from the start of the pyramid area to this level (s >= 1)
  double c1, c2;
  int h, w, strips, blk0;  // size, 64-pixel strips per row of blocks, first block of the level
};

struct ms_plan {
  ms_level lv[MS_MAXK];
  double wt[MS_MAXK];
  long long blocks;      // level-pass blocks of one pair, all levels
  long long pyr_bytes;   // bytes of the pyramid area (after the N * blocks float64 partials)
  int K, N;
};

// false: the sizes are invalid (dvie_synth_msssim then says why)
bool ms_plan_of(const dvie_synth_msssim_desc* d, ms_plan* q) {
  if (!d || d->scales < 1 || d->scales > MS_MAXK || d->h < 1 || d->w < 1 || d->h > (1 << 19) || d->w > (1 << 19) ||
      d->n0 < 1 || d->n1 < 1 || (long long)d->n0 * d->n1 > 65535)
    return false;
  const int K = d->scales;
  if ((std::min(d->h, d->w) >> (K - 1)) < MS_WIN) return false;
  static const double W5[MS_MAXK] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  double wsum = 0.0;
  for (int s = 0; s < K; ++s) wsum += W5[s];
  q->K = K;
  q->N = d->n0 * d->n1;
  long long blk = 0, src = 0;
  for (int s = 0; s < MS_MAXK; ++s) {
    ms_level& l = q->lv[s];
    l = ms_level{0, 0.0, 0.0, 0, 0, 0, 0};
    q->wt[s] = 0.0;
    if (s >= K) continue;
    const double scale = 255.0 * (double)(1 << (2 * s));
    l.c1 = (0.01 * scale) * (0.01 * scale);
    l.c2 = (0.03 * scale) * (0.03 * scale);
    l.h = d->h >> s;
    l.w = d->w >> s;
    l.strips = (l.w + SW_PX - 1) / SW_PX;
    l.blk0 = (int)blk;
    blk += (long long)l.strips * ((l.h + SW_SEG - 1) / SW_SEG);
    l.src = src;
    if (s >= 1) src += ((2LL * q->N * l.h * l.w * 3 + 3) / 4) * 4;  // (levels start 8-byte aligned)
    q->wt[s] = W5[s] / wsum;
  }
  q->blocks = blk;  // <= 1.34 * 2^14 * 2^13
  q->pyr_bytes = 2 * src;
  return true;
}

__device__ __forceinline__ uint16_t* ms_pyramid(void* ws, const ms_plan& q) {
  return (uint16_t*)((double*)ws + (long long)q.N * q.blocks);
}

__device__ __forceinline__ const uint8_t* ms_frame(const uint8_t* base, long long s0, long long s1, int f, int n1) {
  const int i0 = f / n1, i1 = f - i0 * n1;
  return base + i0 * s0 + i1 * s1;
}

// level S of a tile from level S - 1 in LDS (`lo`, [image][32 >> S][384 >> S]) into `hi`
// ([image][16 >> S][192 >> S]) and, where the level has the pixel, into the workspace
template <int S>
__device__ __forceinline__ void ms_fold(const uint16_t* lo, uint16_t* hi, uint16_t* pyr, const ms_level& lv, int f,
                                        int y0, int x0, int t) {
  constexpr int rows = PY_ROWS >> S, items = PY_IT >> S;  // items = 3 * (64 >> S)
  constexpr int prow = 2 * items;                         // items of a row of the level below
  const int gy0 = y0 >> S, gx0 = x0 >> S;
#pragma unroll
  for (int idx0 = 0; idx0 < 2 * rows * items; idx0 += PY_THREADS) {
    const int idx = idx0 + t;
    if (idx < 2 * rows * items) {
      const int img = idx / (rows * items), rem = idx - img * (rows * items);
      const int i = rem / items, jc = rem - i * items;
      const int j = jc / 3, c = jc - 3 * j;
      const uint16_t* b = lo + (img * 2 * rows + 2 * i) * prow + 6 * j + c;
      const unsigned v = (unsigned)b[0] + b[3] + b[prow] + b[prow + 3];
      hi[idx] = (uint16_t)v;
      const int gy = gy0 + i, gx = gx0 + j;
      if (gy < lv.h && gx < lv.w) pyr[lv.src + (((long long)(2 * f + img) * lv.h + gy) * lv.w + gx) * 3 + c] = (uint16_t)v;
    }
  }
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(PY_THREADS) void msssim_pyramid_kernel(const dvie_synth_msssim_desc p, const ms_plan q) {
  // level s of the tile sits in s_even / s_odd by the parity of s, as [image][16 >> s][192 >> s]
  __shared__ uint16_t s_even[2 * PY_ROWS * PY_IT];
  __shared__ uint16_t s_odd[2 * (PY_ROWS / 2) * (PY_IT / 2)];
  const int t = threadIdx.x, f = blockIdx.z;
  const int x0 = blockIdx.x * PY_PX, y0 = blockIdx.y * PY_ROWS;
  const long long rowb = 3LL * p.w;
  const uint8_t* pa = ms_frame(p.pred, p.pred_s0, p.pred_s1, f, p.n1);
  const uint8_t* pb = ms_frame(p.gt, p.gt_s0, p.gt_s1, f, p.n1);

  // all of a thread's byte loads are issued before the first is used
  constexpr int PY_LOADS = 2 * PY_ROWS * PY_IT / PY_THREADS;
  static_assert(PY_LOADS % 2 == 0 && PY_LOADS / 2 * PY_THREADS == PY_ROWS * PY_IT,
                "an image's tile is a whole number of loads per thread");
  uint8_t v[PY_LOADS];
#pragma unroll
  for (int k = 0; k < PY_LOADS; ++k) {
    const int rem = t + (k % (PY_LOADS / 2)) * PY_THREADS;  // loads 0 .. 11: pred, 12 .. 23: gt
    const int y = rem / PY_IT, x = rem - y * PY_IT;
    const long long col = 3LL * x0 + x;
    const int gy = y0 + y;
    v[k] = (gy < p.h && col < rowb) ? (k < PY_LOADS / 2 ? pa : pb)[gy * rowb + col] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < PY_LOADS; ++k) s_even[t + k * PY_THREADS] = v[k];
  __syncthreads();

  uint16_t* pyr = ms_pyramid(p.ws, q);
  ms_fold<1>(s_even, s_odd, pyr, q.lv[1], f, y0, x0, t);
  if (q.K > 2) ms_fold<2>(s_odd, s_even, pyr, q.lv[2], f, y0, x0, t);
  if (q.K > 3) ms_fold<3>(s_even, s_odd, pyr, q.lv[3], f, y0, x0, t);
  if (q.K > 4) ms_fold<4>(s_odd, s_even, pyr, q.lv[4], f, y0, x0, t);
}

namespace {

struct ms_row {
  uint32_t a, b, ha, hb;  // centre sample of both images, halo sample of both
};

}  // namespace

__global__ __launch_bounds__(SW_IT) void msssim_level_kernel(const dvie_synth_msssim_desc p, const ms_plan q) {
  __shared__ double s_red[SW_IT];

  const int t = threadIdx.x, f = blockIdx.y;
  const int bid = (int)blockIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 1; k < MS_MAXK; ++k)
    if (k < q.K && bid >= q.lv[k].blk0) s = k;
  const ms_level lv = q.lv[s];
  const int local = bid - lv.blk0;
  const int seg = local / lv.strips, strip = local - seg * lv.strips;
  const int x0 = strip * SW_PX, y0 = seg * SW_SEG;
  const int y1 = min(y0 + SW_SEG, lv.h);
  const long long rowb = 3LL * lv.w;
  const bool wide = s > 0;  // uint16 sums of the workspace; level 0: the frames' bytes
  const long long img = (long long)lv.h * rowb;
  const uint16_t* wa = ms_pyramid(p.ws, q) + lv.src + 2LL * f * img;
  const uint16_t* wb = wa + img;
  const uint8_t* pa = ms_frame(p.pred, p.pred_s0, p.pred_s1, f, p.n1);
  const uint8_t* pb = ms_frame(p.gt, p.gt_s0, p.gt_s1, f, p.n1);
  const bool last = s == q.K - 1;  // the luminance factor multiplies in on the last level only

  const ssim_cols c = ssim_cols_of(x0, rowb);
  auto fetch = [&](int r) {
    ms_row v = {0, 0, 0, 0};
    if (r >= 0 && r < lv.h) {
      const long long o = r * rowb;
      if (wide) {
        if (c.colok) {
          v.a = wa[o + c.col];
          v.b = wb[o + c.col];
        }
        if (c.hok) {
          v.ha = wa[o + c.hcol];
          v.hb = wb[o + c.hcol];
        }
      } else {
        if (c.colok) {
          v.a = pa[o + c.col];
          v.b = pb[o + c.col];
        }
        if (c.hok) {
          v.ha = pa[o + c.hcol];
          v.hb = pb[o + c.hcol];
        }
      }
    }
    return v;
  };
  const double acc = ssim_walk(c, y0, y1, lv.h, lv.c1, lv.c2, last, fetch, [](int, const ms_row&) {});

  lds_tree_sum<SW_IT>(acc, s_red);
  if (t == 0) ((double*)p.ws)[(long long)f * q.blocks + bid] = s_red[0];
}

__global__ __launch_bounds__(64 * MS_MAXK) void msssim_finalize_kernel(const dvie_synth_msssim_desc p, const ms_plan q) {
  // wave s sums level s: every lane a fixed strided subset in order, then a fixed tree
  __shared__ double s_d[MS_MAXK][64];
  __shared__ double s_pow[MS_MAXK];
  const int t = threadIdx.x, f = blockIdx.x, s = t >> 6, lane = t & 63;
  const double* part = (const double*)p.ws + (long long)f * q.blocks;
  double sum = 0.0;
  if (s < q.K) {
    const long long b1 = s + 1 < q.K ? (long long)q.lv[s + 1].blk0 : q.blocks;
    for (long long j = q.lv[s].blk0 + lane; j < b1; j += 64) sum += part[j];
  }
  s_d[s][lane] = sum;
  __syncthreads();
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    if (lane < k) s_d[s][lane] += s_d[s][lane + k];
    __syncthreads();
  }
  if (lane == 0 && s < q.K) {
    const double m = s_d[s][0] / (3.0 * (double)q.lv[s].h * (double)q.lv[s].w);
    p.parts[(long long)f * q.K + s] = m;
    s_pow[s] = pow(fmax(m, 0.0), q.wt[s]);
  }
  __syncthreads();
  if (t == 0) {
    double prod = 1.0;
    for (int k = 0; k < q.K; ++k) prod *= s_pow[k];
    p.msssim[f] = prod;
  }
}

}  // namespace dvie

using namespace dvie;

extern "C" {

size_t dvie_synth_msssim_ws_bytes(const dvie_synth_msssim_desc* d) {
  ms_plan q;
  if (!ms_plan_of(d, &q)) return 0;
  return (size_t)(8LL * q.N * q.blocks + q.pyr_bytes);
}

int dvie_synth_msssim(const dvie_synth_msssim_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->pred && d->gt, "synth_msssim: pred / gt frames must not be null");
  DVIE_CHECK_ARG(d->scales >= 1 && d->scales <= MS_MAXK, "synth_msssim: scales=%d must be in 1..%d", d->scales, MS_MAXK);
  DVIE_CHECK_ARG(d->h >= 1 && d->w >= 1 && d->h <= (1 << 19) && d->w <= (1 << 19),
                 "synth_msssim: h=%d and w=%d must be in 1..%d", d->h, d->w, 1 << 19);
  int fit = 0;
  while (fit < MS_MAXK && (std::min(d->h, d->w) >> fit) >= MS_WIN) ++fit;
  DVIE_CHECK_ARG(d->scales <= fit,
                 "synth_msssim: %d scales need min(h, w) >> %d >= %d; %dx%d frames take at most %d scales", d->scales,
                 d->scales - 1, MS_WIN, d->h, d->w, fit);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n1 >= 1 && (long long)d->n0 * d->n1 <= 65535,
                 "synth_msssim: n0=%d x n1=%d frames must be in 1..65535", d->n0, d->n1);
  DVIE_CHECK_ARG(d->msssim && d->parts, "synth_msssim: msssim / parts outputs must not be null");
  DVIE_CHECK_ARG(d->ws, "synth_msssim: workspace is missing (dvie_synth_msssim_ws_bytes bytes)");
  const uintptr_t al = (uintptr_t)d->ws | (uintptr_t)d->msssim | (uintptr_t)d->parts;
  DVIE_CHECK_ARG((al & 7) == 0, "synth_msssim: ws and the outputs must be 8-byte aligned");
  ms_plan q;
  DVIE_CHECK_ARG(ms_plan_of(d, &q), "synth_msssim: invalid sizes");
  hipStream_t s = (hipStream_t)stream;
  if (q.K > 1) {
    // tiles that hold a whole level-1 block: rows < h & ~1, columns < w & ~1
    const dim3 grid((unsigned)(((d->w & ~1) + PY_PX - 1) / PY_PX), (unsigned)(((d->h & ~1) + PY_ROWS - 1) / PY_ROWS),
                    (unsigned)q.N);
    DVIE_LAUNCH(msssim_pyramid_kernel, grid, dim3(PY_THREADS), 0, s, *d, q);
  }
  DVIE_LAUNCH(msssim_level_kernel, dim3((unsigned)q.blocks, (unsigned)q.N), dim3(SW_IT), 0, s, *d, q);
  DVIE_LAUNCH(msssim_finalize_kernel, dim3((unsigned)q.N), dim3(64 * MS_MAXK), 0, s, *d, q);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
