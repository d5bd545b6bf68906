// dvie_synth_retime: the output frames of a frame-rate conversion, gathered or blended from the
// slots of an interpolated clip (include/dvie.h has the row rule; DESIGN.md "Frame-rate conversion"
// the clock, the exact division and the measurements).
//
// synth_retime_kernel: grid (pieces of a row, output rows, clips).  A block reads its row's five
// integers and, when flags are given, its pair's flag (both uniform over the block), resolves the
// rule to (source a, source b or none, weight n) and moves its piece of the row: 16 KB, one 16-byte
// vector per thread and step.  A skipped row's blocks leave before they touch a byte.
//
// Alignment: the row's bytes are moved as 16-byte vectors when the destination and every source that
// is read have the SAME offset from a 16-byte boundary: then the first `head` = (-dst) & 15 bytes go
// one by one, the aligned middle as vectors and the rest one by one again.  Piece p covers the bytes
// [head + p * 16 KB, head + (p + 1) * 16 KB) of the row, piece 0 the head as well, so every middle
// piece is whole vectors and only the first and the last piece move single bytes.  When the offsets
// differ (a frame size that is no multiple of 16 bytes puts every slot at another offset) the whole
// row goes byte by byte.  Nothing outside [0, nbytes) of a row is read or written.
//
// Blend: out = (a * (P - n) + b * n + P / 2) / P per byte, P = den <= 4096, 0 < n < P.  The divide
// is a multiply: with k = 4096 / P (integer) and P' = k * P, 2048 < P' <= 4096, the quotient is
// unchanged when numerator and denominator are both scaled by k,
//   x = a * wa + b * wb + r,   wa = (P - n) * k, wb = n * k, r = (P / 2) * k,
//   x <= 255 * P' + P' / 2 < 2^20,   out = x / P',
// and with M = ceil(2^32 / P') = (2^32 + e) / P', 0 <= e < P':
//   x * M / 2^32 = x / P' + x * e / (P' * 2^32),   0 <= x * e / (P' * 2^32) < 2^20 / 2^32 = 2^-12.
// The fractional part of x / P' is at most 1 - 1 / P' <= 1 - 2^-12, so adding less than 2^-12 never
// reaches the next integer: floor(x * M / 2^32) == x / P' for every byte pair and every n.  All of
// wa, wb, r (< 2^13), the bytes, x (< 2^20) and M (<= 2^32 / 2049 + 1 < 2^21) fit 24 bits, so the
// two multiplies and the multiply-high are the full-rate 24-bit forms (v_mul_u32_u24,
// v_mul_hi_u32_u24); no integer divide and no 32 x 32 multiply runs per byte.
#include "common.h"

namespace dvie {

namespace {

constexpr int RT_T = 256;
constexpr int RT_PIECE = RT_T * 16 * 4;  // bytes of a row one block moves

struct rt_weights {
  uint32_t wa, wb, r, m;
};

__device__ __forceinline__ uint32_t rt_blend1(uint32_t a, uint32_t b, const rt_weights w) {
  // (the masks change no value: they tell the compiler that every operand fits 24 bits)
  const uint32_t x = ((a & 255u) * (w.wa & 0x1fffu) + (b & 255u) * (w.wb & 0x1fffu) + (w.r & 0x1fffu)) & 0xfffffu;
  return (uint32_t)(((uint64_t)x * (uint64_t)(w.m & 0x1fffffu)) >> 32);
}

__device__ __forceinline__ uint32_t rt_blend4(uint32_t a, uint32_t b, const rt_weights w) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) o |= rt_blend1((a >> (8 * i)) & 255u, (b >> (8 * i)) & 255u, w) << (8 * i);
  return o;
}

__global__ __launch_bounds__(RT_T) void synth_retime_kernel(const dvie_synth_retime_desc p, const uint32_t scale,
                                                            const uint32_t magic) {
  const int k = blockIdx.y, bi = blockIdx.z;
  const int32_t* row = p.rows_dev + 5LL * k;
  int lo = row[0], hi = row[1], n = row[2];
  const int pair = row[3];
  if (p.cut && pair >= 0 && p.cut[(long long)bi * p.n_pairs + pair]) {
    lo = row[4];
    n = 0;
  }
  if (lo < 0) return;  // (uniform over the block)
  const uint8_t* clip = p.slots + (long long)bi * p.slot_s0;
  const uint8_t* a = clip + (long long)lo * p.slot_s1;
  const uint8_t* b = n ? clip + (long long)hi * p.slot_s1 : a;
  uint8_t* dst = p.out + (long long)bi * p.out_s0 + (long long)k * p.out_s1;

  const uint32_t mis = (uint32_t)((uintptr_t)dst & 15);
  const bool vec = ((uintptr_t)a & 15) == mis && ((uintptr_t)b & 15) == mis;
  const long long head = vec ? min((long long)((16 - mis) & 15), p.nbytes) : 0;
  const long long start = blockIdx.x ? head + (long long)blockIdx.x * RT_PIECE : 0;
  const long long end = min(head + ((long long)blockIdx.x + 1) * RT_PIECE, p.nbytes);
  if (start >= end) return;
  // [start, vs) and [ve, end) byte by byte, [vs, ve) as 16-byte vectors
  long long vs = end, ve = end;
  if (vec) {
    vs = min(max(start, head), end);
    ve = vs + (end - vs) / 16 * 16;
  }
  const int t = threadIdx.x;
  if (n == 0) {
    for (long long o = vs + 16LL * t; o < ve; o += 16LL * RT_T) *(uint4*)(dst + o) = *(const uint4*)(a + o);
    for (long long o = start + t; o < vs; o += RT_T) dst[o] = a[o];
    for (long long o = ve + t; o < end; o += RT_T) dst[o] = a[o];
    return;
  }
  rt_weights w;
  w.wa = (uint32_t)(p.den - n) * scale;
  w.wb = (uint32_t)n * scale;
  w.r = (uint32_t)(p.den / 2) * scale;
  w.m = magic;
  for (long long o = vs + 16LL * t; o < ve; o += 16LL * RT_T) {
    const uint4 x = *(const uint4*)(a + o), y = *(const uint4*)(b + o);
    uint4 z;
    z.x = rt_blend4(x.x, y.x, w);
    z.y = rt_blend4(x.y, y.y, w);
    z.z = rt_blend4(x.z, y.z, w);
    z.w = rt_blend4(x.w, y.w, w);
    *(uint4*)(dst + o) = z;
  }
  for (long long o = start + t; o < vs; o += RT_T) dst[o] = (uint8_t)rt_blend1(a[o], b[o], w);
  for (long long o = ve + t; o < end; o += RT_T) dst[o] = (uint8_t)rt_blend1(a[o], b[o], w);
}

}  // namespace

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_retime(const dvie_synth_retime_desc* d, void* stream) {
  DVIE_CHECK_ARG(d, "synth_retime: the descriptor must not be null");
  DVIE_CHECK_ARG(d->n_rows >= 0 && d->n_rows <= 65535, "synth_retime: n_rows=%d must be in 0..65535", d->n_rows);
  DVIE_CHECK_ARG(d->den >= 1 && d->den <= 4096, "synth_retime: den=%d must be in 1..4096", d->den);
  DVIE_CHECK_ARG(d->nbytes >= 1, "synth_retime: empty rows, nbytes=%lld must be positive", d->nbytes);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n0 <= 65535, "synth_retime: n0=%d clips must be in 1..65535", d->n0);
  DVIE_CHECK_ARG(d->n_slots >= 1, "synth_retime: n_slots=%d must be positive", d->n_slots);
  DVIE_CHECK_ARG(d->n_pairs >= 0, "synth_retime: n_pairs=%d must not be negative", d->n_pairs);
  if (d->n_rows == 0) return DVIE_OK;  // no output: nothing is launched
  DVIE_CHECK_ARG(d->slots && d->out, "synth_retime: slots / out must not be null");
  DVIE_CHECK_ARG(d->rows && d->rows_dev, "synth_retime: rows (host) / rows_dev (device) must not be null");
  const long long a1 = d->slot_s1 < 0 ? -d->slot_s1 : d->slot_s1, o1 = d->out_s1 < 0 ? -d->out_s1 : d->out_s1;
  DVIE_CHECK_ARG(d->n_slots == 1 || a1 >= d->nbytes, "synth_retime: slot stride %lld lets slots of %lld bytes overlap",
                 d->slot_s1, d->nbytes);
  DVIE_CHECK_ARG(d->n_rows == 1 || o1 >= d->nbytes, "synth_retime: output stride %lld lets rows of %lld bytes overlap",
                 d->out_s1, d->nbytes);
  for (int k = 0; k < d->n_rows; ++k) {
    const int32_t* r = d->rows + 5LL * k;
    const int lo = r[0], hi = r[1], n = r[2], pair = r[3], hold = r[4];
    DVIE_CHECK_ARG(n >= 0 && n < d->den, "synth_retime: row %d has weight n=%d outside 0..den-1=%d", k, n, d->den - 1);
    DVIE_CHECK_ARG(lo >= -1 && lo < d->n_slots, "synth_retime: row %d reads slot lo=%d outside the %d slots (-1 skips)", k,
                   lo, d->n_slots);
    DVIE_CHECK_ARG(lo < 0 || n == 0 || (hi >= 0 && hi < d->n_slots), "synth_retime: row %d blends slot hi=%d outside the %d slots",
                   k, hi, d->n_slots);
    DVIE_CHECK_ARG(pair >= -1, "synth_retime: row %d has pair=%d (-1: none)", k, pair);
    if (d->cut && pair >= 0) {
      DVIE_CHECK_ARG(pair < d->n_pairs, "synth_retime: row %d has pair=%d outside the %d flags of a clip", k, pair, d->n_pairs);
      DVIE_CHECK_ARG(hold >= 0 && hold < d->n_slots, "synth_retime: row %d holds slot %d outside the %d slots", k, hold,
                     d->n_slots);
    }
  }
  const long long pieces = (d->nbytes + 15 + RT_PIECE - 1) / RT_PIECE;  // (up to 15 head bytes shift the pieces)
  DVIE_CHECK_ARG(pieces <= 0x7fffffffLL, "synth_retime: nbytes=%lld too large", d->nbytes);
  const uint32_t scale = 4096u / (uint32_t)d->den, pp = scale * (uint32_t)d->den;  // 2048 < pp <= 4096
  const uint32_t magic = (uint32_t)(((1ULL << 32) + pp - 1) / pp);                // ceil(2^32 / pp) < 2^21
  DVIE_LAUNCH(synth_retime_kernel, dim3((unsigned)pieces, (unsigned)d->n_rows, (unsigned)d->n0), dim3(RT_T), 0,
              (hipStream_t)stream, *d, scale, magic);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
