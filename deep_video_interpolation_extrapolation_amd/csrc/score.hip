// dvie_synth_score: PSNR / SSIM / label agreement of synthesised uint8 frames against the
// held-out originals, per frame, in one pass over the 8 B per pixel of the four inputs
// (include/dvie.h has the semantics).  It replaces, on the 8-bit frames the synthesiser writes,
// the reference's losses.py:18-48 and 63-87 (gaussian, create_window, _ssim, SSIM), 103-116
// (PSNR) and 122-131 (IoU), which on the training side run on fp32 [0,1] NCHW tensors.
//
// synth_score_kernel: the row walk of ssim_walk.h (a workgroup of 192 threads, a 64-pixel column
// strip of a 32-row segment of one frame, thread t one (pixel, channel) byte) over the frames'
// bytes (byte loads: no alignment is assumed), C1 and C2 scaled by 255^2.  On the segment's own
// rows the same bytes give the squared error, and threads 0..63 compare the label bytes of their
// pixel (class counts through integer LDS atomics).
//
// Widths: a thread's squared-error sum is <= 32 * 65025 and the block's <= 192 times that
// (3.995e8) in uint32; label counts per block <= 2048; the workspace holds the squared error as
// int64 and the counts as uint32 per block; the per-frame sums (finalize) are int64.
//
// synth_score_finalize_kernel: one block per frame sums that frame's block partials, each
// thread a fixed strided subset in order, then the fixed LDS tree of common.h -- the same bits
// every run.
#include "common.h"
#include "ssim_walk.h"

namespace dvie {

namespace {

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

__global__ __launch_bounds__(SW_IT) void synth_score_kernel(const dvie_synth_score_desc p) {
  __shared__ double s_red[SW_IT];
  __shared__ unsigned s_cls[2][SC_MAXC];
  __shared__ unsigned s_int[3];

  const int t = threadIdx.x;
  const int f = blockIdx.z, i0 = f / p.n1, i1 = f - i0 * p.n1;
  const int x0 = blockIdx.x * SW_PX, y0 = blockIdx.y * SW_SEG;
  const int y1 = min(y0 + SW_SEG, p.h);
  const long long rowb = 3LL * p.w;
  const uint8_t* pa = p.pred + i0 * p.pred_s0 + i1 * p.pred_s1;
  const uint8_t* pb = p.gt + i0 * p.gt_s0 + i1 * p.gt_s1;
  const bool labels = p.pred_label != nullptr;
  const uint8_t* la = labels ? p.pred_label + i0 * p.pred_label_s0 + i1 * p.pred_label_s1 : nullptr;
  const uint8_t* lb = labels ? p.gt_label + i0 * p.gt_label_s0 + i1 * p.gt_label_s1 : nullptr;

  const ssim_cols c = ssim_cols_of(x0, rowb);
  const int lx = x0 + t;
  const bool lok = labels && t < SW_PX && lx < p.w;
  const unsigned nc = (unsigned)p.n_classes;

  if (t < 2 * SC_MAXC) (&s_cls[0][0])[t] = 0;
  if (t < 3) s_int[t] = 0;  // (the walk's barriers of rows y0-5 .. y0-1 come before the first atomic)

  auto fetch = [&](int r) {
    sc_row q = {0, 0, 0, 0, 0, 0};
    if (r >= 0 && r < p.h) {
      const long long o = r * rowb;
      if (c.colok) {
        q.a = pa[o + c.col];
        q.b = pb[o + c.col];
      }
      if (c.hok) {
        q.ha = pa[o + c.hcol];
        q.hb = pb[o + c.hcol];
      }
      if (lok && r >= y0 && r < y1) {
        q.lp = la[(long long)r * p.w + lx];
        q.lg = lb[(long long)r * p.w + lx];
      }
    }
    return q;
  };

  uint32_t sse = 0, agree = 0, valid = 0;
  auto own_row = [&](int, const sc_row& cur) {  // squared error and labels
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
  };
  const double C1 = 0.01 * 0.01 * 65025.0, C2 = 0.03 * 0.03 * 65025.0;
  const double acc = ssim_walk(c, y0, y1, p.h, C1, C2, true, fetch, own_row);

  // block partials: the float64 sum through the fixed tree, the integers through LDS atomics
  atomicAdd(&s_int[0], sse);
  if (lok) {
    atomicAdd(&s_int[1], agree);
    atomicAdd(&s_int[2], valid);
  }
  lds_tree_sum<SW_IT>(acc, s_red);
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
    lds_tree_sum<256>(s, s_d);
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
    lds_tree_sum<256>(s, s_i);
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
  const long long segs = ((long long)d->h + SW_SEG - 1) / SW_SEG;
  if (segs > 65535) return 0;
  return segs * ((d->w + SW_PX - 1) / SW_PX);
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
  const dim3 grid((unsigned)((d->w + SW_PX - 1) / SW_PX), (unsigned)((d->h + SW_SEG - 1) / SW_SEG), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  DVIE_LAUNCH(synth_score_kernel, grid, dim3(SW_IT), 0, s, *d);
  DVIE_LAUNCH(synth_score_finalize_kernel, dim3((unsigned)N), dim3(256), 0, s, *d, per_frame);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
