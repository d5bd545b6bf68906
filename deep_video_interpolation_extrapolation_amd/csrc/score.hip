// dvie_synth_score: PSNR / SSIM / label agreement of synthesised uint8 frames against the
// held-out originals, per frame, in one pass over the 8 B per pixel of the four inputs
// (include/dvie.h has the semantics).  It replaces, on the 8-bit frames the synthesiser writes,
// the reference's losses.py:18-48 and 63-87 (gaussian, create_window, _ssim, SSIM), 103-116
// (PSNR) and 122-131 (IoU), which on the training side run on fp32 [0,1] NCHW tensors.
//
// synth_score_kernel: a workgroup of 192 threads owns a 64-pixel column strip of a 32-row
// segment of one frame; thread t owns byte t of the strip's 192-byte row piece, one
// (pixel, channel) item.  It walks input rows y0-5 .. y1+4 top-down.  Per row:
//   * the 222-byte span (15 bytes = 5 pixels of halo each side) of both frames goes, converted
//     to float64, into one of two LDS row buffers (byte loads: no alignment is assumed; samples
//     outside the image are 0); the next row's bytes are fetched before this row is consumed;
//   * each thread forms the five horizontal 11-tap sums (a, b, a^2, b^2, ab) of its item and
//     keeps the last 11 rows of them in REGISTERS (55 doubles; the row loop is unrolled by 11 so
//     that every ring index is a constant) -- no intermediate goes to LDS or HBM;
//   * from the ring it finishes output row r-5: the five vertical sums and the SSIM term;
//   * on the segment's own rows the same bytes give the squared error, and threads 0..63 compare
//     the label bytes of their pixel (class counts through integer LDS atomics).
// All SSIM arithmetic is float64 on the byte values (C1, C2 scaled by 255^2): DESIGN.md
// "Scoring" has why (E[a^2] - mu^2 of a flat image cancels to ~1e-7 of a^2 against C2 = 9e-4).
// Vertical re-read 42/32 = 1.31x, horizontal 222/192 = 1.16x.
//
// Widths: a thread's squared-error sum is <= 32 * 65025 and the block's <= 192 times that
// (3.995e8) in uint32; label counts per block <= 2048; the workspace holds the squared error as
// int64 and the counts as uint32 per block; the per-frame sums (finalize) are int64.
//
// synth_score_finalize_kernel: one block per frame sums that frame's block partials, each
// thread a fixed strided subset in order, then a fixed LDS tree -- the same bits every run.
#include "common.h"
#include "gauss11.h"

namespace dvie {

namespace {

constexpr int SC_PX = 64;              // pixels of a strip
constexpr int SC_IT = 3 * SC_PX;       // items (= threads) of a block
constexpr int SC_SEG = 32;             // output rows of a segment
constexpr int SC_HALO = 15;            // bytes of halo on each side (5 pixels)
constexpr int SC_SPAN = SC_IT + 2 * SC_HALO;
constexpr int SC_MAXC = 32;

struct sc_row {
  uint32_t a, b, ha, hb, lp, lg;  // centre byte of both frames, halo byte of both, the two labels
};

struct sc_ws {
  double* ssim;
  long long* sse;
  uint32_t* cnt;  // [2 + 2 * n_classes][blocks]: agree, valid, inter[c], uni[c]
};

__host__ __device__ __forceinline__ sc_ws sc_ws_of(void* ws, long long blocks) {
  sc_ws r;
  r.ssim = (double*)ws;
  r.sse = (long long*)(r.ssim + blocks);
  r.cnt = (uint32_t*)(r.sse + blocks);
  return r;
}

}  // namespace

__global__ __launch_bounds__(SC_IT) void synth_score_kernel(const dvie_synth_score_desc p) {
  __shared__ double s_row[2][2][SC_SPAN];
  __shared__ double s_red[SC_IT];
  __shared__ unsigned s_cls[2][SC_MAXC];
  __shared__ unsigned s_int[3];

  const int t = threadIdx.x;
  const int f = blockIdx.z, i0 = f / p.n1, i1 = f - i0 * p.n1;
  const int x0 = blockIdx.x * SC_PX, y0 = blockIdx.y * SC_SEG;
  const int y1 = min(y0 + SC_SEG, p.h), rend = y1 + 5;
  const long long rowb = 3LL * p.w;
  const uint8_t* pa = p.pred + i0 * p.pred_s0 + i1 * p.pred_s1;
  const uint8_t* pb = p.gt + i0 * p.gt_s0 + i1 * p.gt_s1;
  const bool labels = p.pred_label != nullptr;
  const uint8_t* la = labels ? p.pred_label + i0 * p.pred_label_s0 + i1 * p.pred_label_s1 : nullptr;
  const uint8_t* lb = labels ? p.gt_label + i0 * p.gt_label_s0 + i1 * p.gt_label_s1 : nullptr;

  const long long col = 3LL * x0 + t;  // this thread's byte within the image row
  const bool colok = col < rowb;
  // threads 0..29 also fetch one halo byte: span positions 0..14 and 207..221
  const int hpos = t < SC_HALO ? t : SC_IT + t;
  const long long hcol = 3LL * x0 - SC_HALO + hpos;
  const bool hok = t < 2 * SC_HALO && hcol >= 0 && hcol < rowb;
  const int lx = x0 + t;
  const bool lok = labels && t < SC_PX && lx < p.w;
  const unsigned nc = (unsigned)p.n_classes;

  if (t < 2 * SC_MAXC) (&s_cls[0][0])[t] = 0;
  if (t < 3) s_int[t] = 0;

  auto fetch = [&](int r) {
    sc_row q = {0, 0, 0, 0, 0, 0};
    if (r >= 0 && r < p.h) {
      const long long o = r * rowb;
      if (colok) {
        q.a = pa[o + col];
        q.b = pb[o + col];
      }
      if (hok) {
        q.ha = pa[o + hcol];
        q.hb = pb[o + hcol];
      }
      if (lok && r >= y0 && r < y1) {
        q.lp = la[(long long)r * p.w + lx];
        q.lg = lb[(long long)r * p.w + lx];
      }
    }
    return q;
  };

  double ring[11][5];
#pragma unroll
  for (int s = 0; s < 11; ++s)
#pragma unroll
    for (int q = 0; q < 5; ++q) ring[s][q] = 0.0;
  const double C1 = 0.01 * 0.01 * 65025.0, C2 = 0.03 * 0.03 * 65025.0;
  double acc = 0.0;
  uint32_t sse = 0, agree = 0, valid = 0;

  sc_row cur = fetch(y0 - 5);
  int it = 0;  // rows consumed: row r = y0 - 5 + it sits in ring slot it % 11
  for (int base = y0 - 5; base < rend; base += 11) {
#pragma unroll
    for (int u = 0; u < 11; ++u) {
      const int r = base + u;
      if (r >= rend) continue;  // (uniform over the block; the tail of the last group of 11)
      const int par = it & 1;
      s_row[par][0][SC_HALO + t] = (double)cur.a;
      s_row[par][1][SC_HALO + t] = (double)cur.b;
      if (t < 2 * SC_HALO) {
        s_row[par][0][hpos] = (double)cur.ha;
        s_row[par][1][hpos] = (double)cur.hb;
      }
      if (r >= y0 && r < y1) {  // the segment's own rows: squared error and labels
        const int d = (int)cur.a - (int)cur.b;  // (0 - 0 outside the image)
        sse += (uint32_t)(d * d);
        if (lok) {
          agree += cur.lp == cur.lg;
          if (cur.lg < nc) {
            ++valid;
            atomicAdd(&s_cls[1][cur.lg], 1u);
            if (cur.lp == cur.lg)
              atomicAdd(&s_cls[0][cur.lg], 1u);
            else if (cur.lp < nc)
              atomicAdd(&s_cls[1][cur.lp], 1u);
          }
        }
      }
      const sc_row nxt = r + 1 < rend ? fetch(r + 1) : sc_row{0, 0, 0, 0, 0, 0};
      // one barrier per row: buffer `par` was last read two rows ago, before the barrier of
      // the row between
      __syncthreads();
      if (r >= 0 && r < p.h) {
        double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double a = s_row[par][0][t + 3 * k], b = s_row[par][1][t + 3 * k];
          const double wa = sc_g(k) * a, wb = sc_g(k) * b;
          h[0] += wa;
          h[1] += wb;
          h[2] = fma(wa, a, h[2]);
          h[3] = fma(wb, b, h[3]);
          h[4] = fma(wa, b, h[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[u][q] = h[q];
      } else {
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[u][q] = 0.0;  // zero padding above and below
      }
      if (it >= 10) {  // output row r - 5: input rows r-10 .. r are slots u+1 .. u+11 (mod 11)
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
          for (int q = 0; q < 5; ++q) v[q] = fma(sc_g(k), ring[(u + 1 + k) % 11][q], v[q]);
        const double m11 = v[0] * v[0], m22 = v[1] * v[1], m12 = v[0] * v[1];
        const double s1 = v[2] - m11, s2 = v[3] - m22, s12 = v[4] - m12;
        const double num = (2.0 * m12 + C1) * (2.0 * s12 + C2);
        const double den = (m11 + m22 + C1) * (s1 + s2 + C2);
        if (colok) acc += num / den;
      }
      cur = nxt;
      ++it;
    }
  }

  // block partials: the float64 sum through a fixed tree, the integers through LDS atomics
  s_red[t] = acc;
  atomicAdd(&s_int[0], sse);
  if (lok) {
    atomicAdd(&s_int[1], agree);
    atomicAdd(&s_int[2], valid);
  }
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s && t + s < SC_IT) s_red[t] += s_red[t + s];
    __syncthreads();
  }
  const long long per_frame = (long long)gridDim.x * gridDim.y;
  const long long blocks = per_frame * gridDim.z;
  const long long bi = f * per_frame + (long long)blockIdx.y * gridDim.x + blockIdx.x;
  const sc_ws ws = sc_ws_of(p.ws, blocks);
  if (t == 0) {
    ws.ssim[bi] = s_red[0];
    ws.sse[bi] = (long long)s_int[0];
  }
  if (labels && t < 2 + 2 * p.n_classes) {
    const unsigned v = t < 2 ? s_int[1 + t] : (t < 2 + p.n_classes ? s_cls[0][t - 2] : s_cls[1][t - 2 - p.n_classes]);
    ws.cnt[t * blocks + bi] = v;
  }
}

__global__ __launch_bounds__(256) void synth_score_finalize_kernel(const dvie_synth_score_desc p, long long per_frame) {
  __shared__ double s_d[256];
  __shared__ long long s_i[256];
  const int t = threadIdx.x, f = blockIdx.x;
  const long long blocks = per_frame * gridDim.x;
  const sc_ws ws = sc_ws_of(p.ws, blocks);
  const long long b0 = f * per_frame;
  {
    double s = 0.0;
    for (long long j = t; j < per_frame; j += 256) s += ws.ssim[b0 + j];
    s_d[t] = s;
    __syncthreads();
#pragma unroll
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) s_d[t] += s_d[t + k];
      __syncthreads();
    }
    if (t == 0) p.ssim[f] = s_d[0] / (3.0 * (double)p.h * (double)p.w);
  }
  const int nq = p.pred_label ? 3 + 2 * p.n_classes : 1;  // sse, agree, valid, inter[c], uni[c]
  for (int q = 0; q < nq; ++q) {
    long long s = 0;
    if (q == 0) {
      for (long long j = t; j < per_frame; j += 256) s += ws.sse[b0 + j];
    } else {
      const uint32_t* c = ws.cnt + (q - 1) * blocks + b0;
      for (long long j = t; j < per_frame; j += 256) s += (long long)c[j];
    }
    s_i[t] = s;
    __syncthreads();
#pragma unroll
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) s_i[t] += s_i[t + k];
      __syncthreads();
    }
    if (t == 0) {
      const long long v = s_i[0];
      if (q == 0)
        p.sse[f] = v;
      else if (q == 1)
        p.agree[f] = v;
      else if (q == 2)
        p.valid[f] = v;
      else if (q < 3 + p.n_classes)
        p.inter[(long long)f * p.n_classes + (q - 3)] = v;
      else
        p.uni[(long long)f * p.n_classes + (q - 3 - p.n_classes)] = v;
    }
    __syncthreads();
  }
}

// 0: the sizes are invalid (dvie_synth_score then says why)
static long long score_blocks_per_frame(const dvie_synth_score_desc* d) {
  if (!d || d->h < 1 || d->w < 1 || d->w > (1 << 29) || d->n0 < 1 || d->n1 < 1 || (long long)d->n0 * d->n1 > 65535)
    return 0;
  const long long segs = ((long long)d->h + SC_SEG - 1) / SC_SEG;
  if (segs > 65535) return 0;
  return segs * ((d->w + SC_PX - 1) / SC_PX);
}

}  // namespace dvie

using namespace dvie;

extern "C" {

size_t dvie_synth_score_ws_bytes(const dvie_synth_score_desc* d) {
  const long long per_frame = score_blocks_per_frame(d);
  if (!per_frame) return 0;
  const bool labels = d->pred_label || d->gt_label;
  if (labels && (d->n_classes < 1 || d->n_classes > SC_MAXC)) return 0;
  const long long blocks = per_frame * d->n0 * d->n1;
  const long long cnt = labels ? 4LL * (2 + 2 * d->n_classes) : 0;
  return (size_t)((blocks * (16 + cnt) + 7) / 8 * 8);
}

int dvie_synth_score(const dvie_synth_score_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->pred && d->gt, "synth_score: pred / gt frames must not be null");
  DVIE_CHECK_ARG((d->pred_label != nullptr) == (d->gt_label != nullptr),
                 "synth_score: pred_label and gt_label must be given together (both or neither)");
  DVIE_CHECK_ARG(d->h >= 1 && d->w >= 1, "synth_score: h=%d and w=%d must be at least 1", d->h, d->w);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n1 >= 1 && (long long)d->n0 * d->n1 <= 65535,
                 "synth_score: n0=%d x n1=%d frames must be in 1..65535", d->n0, d->n1);
  const bool labels = d->pred_label != nullptr;
  if (labels) {
    DVIE_CHECK_ARG(d->n_classes >= 1 && d->n_classes <= SC_MAXC, "synth_score: n_classes=%d must be in 1..%d",
                   d->n_classes, SC_MAXC);
    DVIE_CHECK_ARG(d->agree && d->valid && d->inter && d->uni,
                   "synth_score: agree / valid / inter / uni must not be null with label maps");
  }
  DVIE_CHECK_ARG(d->sse && d->ssim, "synth_score: sse / ssim outputs must not be null");
  const long long per_frame = score_blocks_per_frame(d);
  DVIE_CHECK_ARG(per_frame > 0, "synth_score: h=%d w=%d too large", d->h, d->w);
  DVIE_CHECK_ARG(d->ws, "synth_score: workspace is missing (dvie_synth_score_ws_bytes bytes)");
  const uintptr_t al = (uintptr_t)d->ws | (uintptr_t)d->sse | (uintptr_t)d->ssim | (uintptr_t)d->agree |
                       (uintptr_t)d->valid | (uintptr_t)d->inter | (uintptr_t)d->uni;
  DVIE_CHECK_ARG((al & 7) == 0, "synth_score: ws and the outputs must be 8-byte aligned");
  const int N = d->n0 * d->n1;
  const dim3 grid((unsigned)((d->w + SC_PX - 1) / SC_PX), (unsigned)((d->h + SC_SEG - 1) / SC_SEG), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  DVIE_LAUNCH(synth_score_kernel, grid, dim3(SC_IT), 0, s, *d);
  DVIE_LAUNCH(synth_score_finalize_kernel, dim3((unsigned)N), dim3(256), 0, s, *d, per_frame);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
