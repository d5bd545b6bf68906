// dvie_synth_tile_blend: the per-tile outputs of a tiled forward -> the uint8 frame, the label map,
// the label canvas and the kept fp32 form of the whole canvas, in one launch (include/dvie.h has the
// blend rule, tests/tile_ref.py its numpy restatement; DESIGN.md "Tiled synthesis" the numbers).
//
// A gather: one lane owns one CANVAS pixel (pixel.h's canvas_row: blockIdx.x = image * hp + y;
// blockIdx.y = the 256-pixel chunk of the row) and reads the tiles that cover it, so every output
// byte has one owner, nothing is accumulated in memory and the result cannot depend on the launch
// geometry.  The row is uniform over a block, hence so are the tile rows that cover it (a scalar
// scan of ys); the covering tile columns are found per lane by a scan of xs with a uniform index
// (the start arrays live in the kernel arguments and are only ever read at a uniform index).
//
// Two paths.  Exactly one covering tile (most of the canvas): the lane copies that tile's pixel --
// 16-byte loads and pixel.h's argmax_logits, nothing is multiplied.  Otherwise the lane walks the
// covering tiles in ascending tile index: the image once, the logits four channels at a time (a
// walk per channel group, so the accumulators are one f32x4 whatever n_classes is; argmax_step
// compares the blended group and moves on, no blended logit is stored anywhere).  Only waves that
// touch a seam diverge; both paths meet again before the quad exchange of the label canvas.  The
// quantisation, the argmax and the label store are pixel.h's, shared with synth.hip, so the tiled
// path equals the untiled one where one tile covers a pixel.
//
// Streaming, HBM-bound, no LDS: 16-byte loads of a pixel's own 32 + 96 bytes as in finish (the
// lanes of a wave are one pixel row apart and consume every fetched line), dword stores of the
// label canvas, 16-byte stores of the kept fp32 form.  All offsets are 64-bit.
#include <math.h>

#include "common.h"
#include "pixel.h"

namespace dvie {

// acc + w * v per channel, the multiply and the add rounded separately (-ffp-contract=fast would
// fuse the plain expression into an fma)
__device__ __forceinline__ f32x4 tile_acc(f32x4 acc, float w, f32x4 v) {
#pragma clang fp contract(off)
  const f32x4 m = v * w;
  return acc + m;
}

// the integer weight of a tile (start s, extent e) on an axis of size S at coordinate c
__device__ __forceinline__ int tile_axis_w(int c, int s, int e, int S, int ov) {
  const int a = s > 0 ? c - s + 1 : ov + 1;
  const int b = s + e < S ? s + e - c : ov + 1;
  return min(min(a, b), ov + 1);
}

// kDword: wp % 4 == 0 and label_canvas is 4-byte aligned, so a quad of lanes is four pixels of one
// canvas row and stores one dword of labels (label_quad_store); bytes otherwise.
template <bool kDword>
__global__ __launch_bounds__(256) void synth_tile_blend_kernel(const dvie_synth_tile_blend_desc p) {
  const int x = blockIdx.y * 256 + threadIdx.x;
  if (x >= p.wp) return;  // (kDword: whole quads)
  const canvas_pos cv = canvas_row(p.hp);
  const int row = cv.row, img = cv.img, y = cv.y;
  const bool inside = y < p.h && x < p.w;
  const bool want_seg = inside || p.label_canvas != nullptr;
  const bool want_rgb = inside || p.rgb_out != nullptr;
  if (!want_seg && !want_rgb) return;  // (label_canvas given: nobody leaves here, the exchange is whole)
  const int ov = p.overlap;
  // the tile rows that cover y: a contiguous run of ys, uniform over the block
  int iy0 = 0, ny = 0, ys0 = 0;
  for (int i = 0; i < p.nty; ++i) {
    const int s = p.ys[i];
    if (s <= y && y < s + p.th) {
      if (ny == 0) iy0 = i, ys0 = s;
      ++ny;
    }
  }
  // the tile columns that cover x, per lane
  int ix0 = 0, nx = 0, xs0 = 0;
  for (int i = 0; i < p.ntx; ++i) {
    const int s = p.xs[i];
    if (s <= x && x < s + p.tw) {
      if (nx == 0) ix0 = i, xs0 = s;
      ++nx;
    }
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  uint32_t lab = 0;
  if (ny == 1 && nx == 1) {
    // ---- one covering tile: its values as they are ----
    const long long src = ((((long long)iy0 * p.ntx + ix0) * p.n + img) * p.th + (y - ys0)) * p.tw + (x - xs0);
    if (want_rgb) c = *(const f32x4*)(p.rgb_tiles + src * p.rgb_ld);  // c[3] is padding: loaded, never used
    if (want_seg) lab = (uint32_t)argmax_logits(p.seg_tiles + src * p.seg_ld, p.n_classes);
  } else {
    // ---- a seam: the weighted mean over the covering tiles, ascending tile index ----
    int wsum = 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int iy = iy0; iy < iy0 + ny; ++iy) {
      const int sy = p.ys[iy], wy = tile_axis_w(y, sy, p.th, p.hp, ov);
      for (int ix = 0; ix < p.ntx; ++ix) {
        const int sx = p.xs[ix];
        if (sx <= x && x < sx + p.tw) {
          const int w = wy * tile_axis_w(x, sx, p.tw, p.wp, ov);
          wsum += w;
          if (want_rgb) {
            const long long src = ((((long long)iy * p.ntx + ix) * p.n + img) * p.th + (y - sy)) * p.tw + (x - sx);
            acc = tile_acc(acc, (float)w, *(const f32x4*)(p.rgb_tiles + src * p.rgb_ld));
          }
        }
      }
    }
    const float fs = (float)wsum;
    c = acc / fs;  // (IEEE division: the build has no fast-math)
    if (want_seg) {
      float best = -INFINITY;
      int bi = 0;
      for (int c0 = 0; c0 < p.n_classes; c0 += 4) {
        f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
        for (int iy = iy0; iy < iy0 + ny; ++iy) {
          const int sy = p.ys[iy], wy = tile_axis_w(y, sy, p.th, p.hp, ov);
          for (int ix = 0; ix < p.ntx; ++ix) {
            const int sx = p.xs[ix];
            if (sx <= x && x < sx + p.tw) {
              const int w = wy * tile_axis_w(x, sx, p.tw, p.wp, ov);
              const long long src = ((((long long)iy * p.ntx + ix) * p.n + img) * p.th + (y - sy)) * p.tw + (x - sx);
              a4 = tile_acc(a4, (float)w, *(const f32x4*)(p.seg_tiles + src * p.seg_ld + c0));
            }
          }
        }
        argmax_step(a4 / fs, c0, p.n_classes, best, bi);
      }
      lab = (uint32_t)bi;
    }
  }
  const long long pix = (long long)row * p.wp + x;
  if (p.rgb_out) {
    float* o = p.rgb_out + pix * p.rgb_ld;
    *(f32x4*)o = f32x4{c[0], c[1], c[2], 0.f};
    for (int k = 4; k < p.rgb_ld; k += 4) *(f32x4*)(o + k) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (p.label_canvas) {
    if (kDword)
      label_quad_store(p.label_canvas + pix, lab);
    else
      p.label_canvas[pix] = (uint8_t)lab;
  }
  if (inside) {
    const long long o = ((long long)img * p.h + y) * p.w + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.frame[3 * o + k] = (uint8_t)px_quantise(c[k]);
    p.label[o] = (uint8_t)lab;
  }
}

// starts[0..nt) of tiles of extent e on an axis of size S: increasing, inside, covering
static const char* tile_axis_error(const int* starts, int nt, int e, int S) {
  if (starts[0] != 0) return "tiles do not cover the canvas (the first start is not 0)";
  for (int i = 0; i < nt; ++i) {
    if (i > 0 && starts[i] <= starts[i - 1]) return "tile starts must increase";
    if (starts[i] < 0 || (long long)starts[i] + e > S) return "a tile leaves the canvas";
    if (i > 0 && starts[i] > starts[i - 1] + e) return "tiles do not cover the canvas (a gap between neighbours)";
  }
  if (starts[nt - 1] + e != S) return "tiles do not cover the canvas (the last tile ends before its edge)";
  return nullptr;
}

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_tile_blend(const dvie_synth_tile_blend_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->rgb_tiles && d->seg_tiles && d->frame && d->label,
                 "synth_tile_blend: rgb_tiles / seg_tiles / frame / label must not be null");
  DVIE_CHECK_ARG(d->n >= 1, "synth_tile_blend: n=%d must be positive", d->n);
  DVIE_CHECK_ARG(d->th >= 1 && d->tw >= 1 && d->hp >= 1 && d->wp >= 1, "synth_tile_blend: tile %dx%d and canvas %dx%d must be positive",
                 d->th, d->tw, d->hp, d->wp);
  DVIE_CHECK_ARG(d->h >= 1 && d->h <= d->hp, "synth_tile_blend: h=%d must be in 1..hp=%d", d->h, d->hp);
  DVIE_CHECK_ARG(d->w >= 1 && d->w <= d->wp, "synth_tile_blend: w=%d must be in 1..wp=%d", d->w, d->wp);
  DVIE_CHECK_ARG(d->rgb_ld % 4 == 0 && d->seg_ld % 4 == 0 && d->rgb_ld >= 4 && d->seg_ld >= 4,
                 "synth_tile_blend: leading dimensions rgb_ld=%d seg_ld=%d must be multiples of 4 (>= 4)", d->rgb_ld,
                 d->seg_ld);
  DVIE_CHECK_ARG(((((uintptr_t)d->rgb_tiles) | ((uintptr_t)d->seg_tiles) | ((uintptr_t)d->rgb_out)) & 15) == 0,
                 "synth_tile_blend: rgb_tiles / seg_tiles / rgb_out must be 16-byte aligned");
  DVIE_CHECK_ARG(d->n_classes > 0 && d->n_classes <= d->seg_ld && d->n_classes <= 256,
                 "synth_tile_blend: n_classes=%d must be in 1..min(seg_ld=%d, 256)", d->n_classes, d->seg_ld);
  DVIE_CHECK_ARG(d->overlap >= 0 && d->overlap <= 256, "synth_tile_blend: overlap=%d must be in 0..256", d->overlap);
  DVIE_CHECK_ARG(d->nty >= 1 && d->nty <= DVIE_TILE_MAX && d->ntx >= 1 && d->ntx <= DVIE_TILE_MAX,
                 "synth_tile_blend: nty=%d and ntx=%d tiles per axis must be in 1..%d", d->nty, d->ntx, DVIE_TILE_MAX);
  const char* bad = tile_axis_error(d->ys, d->nty, d->th, d->hp);
  DVIE_CHECK_ARG(!bad, "synth_tile_blend: rows: %s (th=%d, hp=%d)", bad, d->th, d->hp);
  bad = tile_axis_error(d->xs, d->ntx, d->tw, d->wp);
  DVIE_CHECK_ARG(!bad, "synth_tile_blend: columns: %s (tw=%d, wp=%d)", bad, d->tw, d->wp);
  const long long rows = (long long)d->n * d->hp, chunks = ((long long)d->wp + 255) / 256;
  DVIE_CHECK_ARG(rows < (1LL << 31) && chunks <= 65535, "synth_tile_blend: grid too large");
  const dim3 grid((unsigned)rows, (unsigned)chunks);
  if (d->wp % 4 == 0 && (((uintptr_t)d->label_canvas) & 3) == 0)
    DVIE_LAUNCH(synth_tile_blend_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *d);
  else
    DVIE_LAUNCH(synth_tile_blend_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
