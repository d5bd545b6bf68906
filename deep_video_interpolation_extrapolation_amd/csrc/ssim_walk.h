// The float64 SSIM row walk of the video scores, once: synth_score_kernel (score.hip) runs it over
// the bytes of two frames, msssim_level_kernel (msssim.hip) over one level of two pyramids.
//
// A workgroup of SW_IT = 192 threads owns a 64-pixel column strip of a segment of up to 32 rows,
// y0 .. y1 - 1, of an image pair of height h; thread t owns sample t of the strip's 192-sample
// row piece, one (pixel, channel) item.  The walk takes input rows y0-5 .. y1+4 top-down.  Per row:
//   * the 222-sample span (15 samples = 5 pixels of halo each side) of both images goes, converted
//     to float64, into one of two LDS row buffers (samples outside the image are 0); the next
//     row's samples are fetched before this row is consumed;
//   * each thread forms the five horizontal 11-tap sums (a, b, a^2, b^2, ab) of its item and
//     keeps the last 11 rows of them in REGISTERS (55 doubles; the row loop is unrolled by 11 so
//     that every ring index is a constant) -- no intermediate goes to LDS or HBM;
//   * from the ring it finishes output row r-5: the five vertical sums and the SSIM term.
// All arithmetic is float64 on the sample values, C1 and C2 scaled to their range: DESIGN.md
// "Scoring" has why (E[a^2] - mu^2 of a flat image cancels to ~1e-7 of a^2 against C2 = 9e-4).
// Vertical re-read 42/32 = 1.31x, horizontal 222/192 = 1.16x.
//
// (The SSIM of the training loss, losses.hip, is fp32 and LDS-tiled: another algorithm.)
#pragma once
#include "common.h"

namespace dvie {

constexpr int SW_PX = 64;              // pixels of a strip
constexpr int SW_IT = 3 * SW_PX;       // items (= threads) of a block
constexpr int SW_SEG = 32;             // output rows of a segment
constexpr int SW_HALO = 15;            // samples of halo on each side (5 pixels)
constexpr int SW_SPAN = SW_IT + 2 * SW_HALO;

// The 11-tap gaussian window (sigma 1.5): exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, in float64
// (losses.py:18-20 under a float64 default)
__host__ __device__ __forceinline__ constexpr double sc_g(int k) {
  const int d = k < 5 ? 5 - k : k - 5;
  return d == 0 ? 0.26601172486179436
       : d == 1 ? 0.2130055377112537
       : d == 2 ? 0.10936068950970002
       : d == 3 ? 0.03600077212843083
       : d == 4 ? 0.007598758135239185
                : 0.00102838008447911;
}

// What a thread fetches of a row of rowb samples in the strip that starts at pixel x0: its own
// sample `col`, and threads 0..29 also one halo sample `hcol`: span positions 0..14 and 207..221.
struct ssim_cols {
  long long col, hcol;
  int hpos;
  bool colok, hok;
};

__device__ __forceinline__ ssim_cols ssim_cols_of(int x0, long long rowb) {
  const int t = threadIdx.x;
  ssim_cols c;
  c.col = 3LL * x0 + t;
  c.colok = c.col < rowb;
  c.hpos = t < SW_HALO ? t : SW_IT + t;
  c.hcol = 3LL * x0 - SW_HALO + c.hpos;
  c.hok = t < 2 * SW_HALO && c.hcol >= 0 && c.hcol < rowb;
  return c;
}

// The walk.  fetch(r) returns the thread's record of row r: an aggregate of integers whose members
// a, b, ha, hb are the samples at c.col and c.hcol of both images (0 outside the image; further
// members are the caller's own, and {} is the record of no row).  own_row(r, cur) is called on the
// segment's own rows, after the LDS stores of the row and before the next row's fetch.  `full`
// (uniform over the block) multiplies the luminance factor in: l * cs as one quotient; cs alone
// otherwise.  Returns the thread's sum of the terms of its item (0 where c.colok is false).
template <typename Fetch, typename OwnRow>
__device__ __forceinline__ double ssim_walk(const ssim_cols& c, int y0, int y1, int h, double C1, double C2, bool full,
                                            Fetch fetch, OwnRow own_row) {
  __shared__ double s_row[2][2][SW_SPAN];
  typedef decltype(fetch(0)) row_t;
  const int t = threadIdx.x, rend = y1 + 5;

  double ring[11][5];
#pragma unroll
  for (int s = 0; s < 11; ++s)
#pragma unroll
    for (int q = 0; q < 5; ++q) ring[s][q] = 0.0;
  double acc = 0.0;

  row_t cur = fetch(y0 - 5);
  int it = 0;  // rows consumed: row r = y0 - 5 + it sits in ring slot it % 11
  for (int base = y0 - 5; base < rend; base += 11) {
#pragma unroll
    for (int u = 0; u < 11; ++u) {
      const int r = base + u;
      if (r >= rend) continue;  // (uniform over the block; the tail of the last group of 11)
      const int par = it & 1;
      s_row[par][0][SW_HALO + t] = (double)cur.a;
      s_row[par][1][SW_HALO + t] = (double)cur.b;
      if (t < 2 * SW_HALO) {
        s_row[par][0][c.hpos] = (double)cur.ha;
        s_row[par][1][c.hpos] = (double)cur.hb;
      }
      if (r >= y0 && r < y1) own_row(r, cur);
      const row_t nxt = r + 1 < rend ? fetch(r + 1) : row_t{};
      // one barrier per row: buffer `par` was last read two rows ago, before the barrier of
      // the row between
      __syncthreads();
      if (r >= 0 && r < h) {
        double hs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double a = s_row[par][0][t + 3 * k], b = s_row[par][1][t + 3 * k];
          const double wa = sc_g(k) * a, wb = sc_g(k) * b;
          hs[0] += wa;
          hs[1] += wb;
          hs[2] = fma(wa, a, hs[2]);
          hs[3] = fma(wb, b, hs[3]);
          hs[4] = fma(wa, b, hs[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[u][q] = hs[q];
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
        double num = 2.0 * s12 + C2, den = s1 + s2 + C2;
        if (full) {
          num *= 2.0 * m12 + C1;
          // m11 + m22 is a sum of two products, of which contraction fuses one and rounds the
          // other; which one, the compiler decides by an operand order that it is free to swap
          // (and did, with this code in a header).  Written out: m11 is the fused one.
          den *= fma(v[0], v[0], m22) + C1;
        }
        if (c.colok) acc += num / den;
      }
      cur = nxt;
      ++it;
    }
  }
  return acc;
}

}  // namespace dvie
