// dvie_synth_scene / dvie_synth_cutfill: scene-cut detection on the uint8 frames of a clip and the
// frame hold that replaces the blend across a cut (include/dvie.h has the integer statistic and the
// fill rule; DESIGN.md "Scene cuts" the traffic and the measurements).
//
// synth_scene_kernel: a workgroup of 256 threads owns a tile of 2048 pixels of ONE clip and walks
// its frames t = 0 .. n1-1; thread i owns the run of 8 pixels (24 bytes) i of the tile.  Per frame
// the run's bytes are loaded, the 8 lumas are formed and packed four to a dword, and
//   * the SAD against the previous frame's lumas, which stayed in two registers, and
//   * the counts of luma >> 3 in this wave's own 32-bin histogram in LDS (integer LDS atomics)
// come out of the one read: every frame byte is fetched once per call.  The bytes of the next two
// frames are requested before this frame's are consumed.  Per frame the block writes its 32 bin
// counts and, from the second frame on, its SAD to the workspace; nothing is accumulated into global
// memory.  The LDS histograms and SAD slots are double-buffered by frame parity: the threads that
// read a buffer out clear it, and the one barrier of the next frame separates that from its reuse.
//
// Loads: the runs of a frame start at multiples of 24 bytes from the frame's base, so the base's low
// three bits m are the misalignment of every run of that frame.  m == 0: three 8-byte loads.  m != 0:
// the four aligned 8-byte vectors that cover the run, shifted by m bytes in registers -- taken only
// when they lie inside the frame's own bytes, so nothing outside the frame is ever read.  The first
// and last run of such a frame, and the last run of a frame whose size is no multiple of 8 pixels,
// move the bytes that exist one by one.
//
// Widths: a thread's SAD of a frame pair is <= 8 * 255 = 2040 and the block's <= 256 times that
// (522 240) in uint32; a bin count of a block is <= 2048 in uint32; the workspace holds both as
// uint32 per block; the per-pair sums (finalize) are int64 (65536 x 65536 pixels: sad < 1.1e12,
// a bin <= 2^32).
//
// synth_scene_finalize_kernel: one block of 1024 threads per neighbouring pair sums the SAD partials
// of the pair and the bin partials of its two frames (the loads in independent batches: few blocks
// run it, so its time is latency), forms hdiff and, when `cut` is given, the flag.  All sums are
// integer: the same bits every run.
//
// synth_cutfill_kernel: grid (pieces of a slot, interior slots of all pairs, clips).  A block reads
// its pair's flag and leaves when it is 0 (no byte of an unflagged pair is read or written);
// otherwise it copies its piece of the nearer input slot over the interior slot: 16-byte moves when
// both slot bases are 16-byte aligned, bytes otherwise and for the tail.
#include "common.h"
#include "pixel.h"

namespace dvie {

namespace {

constexpr int SN_T = 256;               // threads of a block
constexpr int SN_RUN = 8;               // pixels of a thread's run
constexpr int SN_RB = 3 * SN_RUN;       // bytes of a run
constexpr int SN_TILE = SN_T * SN_RUN;  // pixels of a block's tile
constexpr int SN_BINS = 32;
constexpr int SN_WAVES = SN_T / 64;
constexpr int FIN_T = 1024;             // threads of a finalize block: 32 groups of 32 bins
constexpr int FIN_U = 8;                // block partials of a bin a finalize thread loads at once

constexpr int CF_T = 256;
constexpr int CF_PIECE = CF_T * 16 * 4;  // bytes of a slot one block copies

struct sn_ws {
  uint32_t* hist;  // [n0][n1][blocks][32]
  uint32_t* sad;   // [n0][n1 - 1][blocks]
};

__host__ __device__ __forceinline__ sn_ws sn_ws_of(void* ws, long long n0, long long n1, long long blocks) {
  sn_ws r;
  r.hist = (uint32_t*)ws;
  r.sad = r.hist + n0 * n1 * blocks * SN_BINS;
  return r;
}

struct sn_raw {
  uint2 v[4];
};

// how this thread fetches its run of a frame: 0 nothing (no pixel), 1 bytes, 2 aligned, 3 shifted
__device__ __forceinline__ int sn_mode(const uint8_t* frame, long long fbytes, long long off, int nx) {
  if (nx <= 0) return 0;
  if (nx < SN_RUN) return 1;
  const uintptr_t a = (uintptr_t)(frame + off);
  const int m = (int)(a & 7);
  if (m == 0) return 2;
  const uintptr_t lo = a - m;
  return (lo >= (uintptr_t)frame && lo + 32 <= (uintptr_t)frame + (uintptr_t)fbytes) ? 3 : 1;
}

__device__ __forceinline__ sn_raw sn_fetch(const uint8_t* frame, long long off, int mode) {
  sn_raw r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.v[k] = make_uint2(0, 0);
  if (mode == 2) {
    const uint2* q = (const uint2*)(frame + off);
    r.v[0] = q[0], r.v[1] = q[1], r.v[2] = q[2];
  } else if (mode == 3) {
    const uint2* q = (const uint2*)(((uintptr_t)(frame + off)) & ~(uintptr_t)7);
    r.v[0] = q[0], r.v[1] = q[1], r.v[2] = q[2], r.v[3] = q[3];
  }
  return r;
}

// the 6 dwords of the run, little-endian, from what sn_fetch got (mode 1: loaded here, bytewise)
__device__ __forceinline__ void sn_words(const sn_raw& r, const uint8_t* frame, long long off, int mode, int nx,
                                         uint32_t* w) {
  if (mode == 1) {
#pragma unroll
    for (int k = 0; k < SN_RB / 4; ++k) w[k] = 0;
    const uint8_t* q = frame + off;
#pragma unroll
    for (int k = 0; k < SN_RB; ++k)
      if (k < 3 * nx) w[k >> 2] |= (uint32_t)q[k] << (8 * (k & 3));
    return;
  }
  if (mode != 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) w[2 * k] = r.v[k].x, w[2 * k + 1] = r.v[k].y;
    return;
  }
  // the four 8-byte vectors as one 32-byte number, shifted right by m bytes (1 <= m <= 7; m is the
  // same for every run of the frame)
  const int sh = 8 * (int)(((uintptr_t)(frame + off)) & 7);
  unsigned long long a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = ((unsigned long long)r.v[k].y << 32) | r.v[k].x;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned long long o = (a[k] >> sh) | (a[k + 1] << (64 - sh));
    w[2 * k] = (uint32_t)o, w[2 * k + 1] = (uint32_t)(o >> 32);
  }
}

__device__ __forceinline__ uint32_t sn_absdiff4(uint32_t a, uint32_t b) {  // sum of |a_k - b_k| over the four bytes
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
    s += (uint32_t)(d < 0 ? -d : d);
  }
  return s;
}

}  // namespace

__global__ __launch_bounds__(SN_T) void synth_scene_kernel(const dvie_synth_scene_desc p) {
  __shared__ unsigned s_hist[2][SN_WAVES][SN_BINS];
  __shared__ unsigned s_sad[2][SN_WAVES];

  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int i0 = blockIdx.y;
  const long long blocks = gridDim.x, bx = blockIdx.x;
  const long long npix = (long long)p.h * p.w, fbytes = 3 * npix;
  const long long px0 = bx * SN_TILE + (long long)t * SN_RUN;
  const int nx = (int)max(0LL, min((long long)SN_RUN, npix - px0));
  const long long off = 3 * px0;
  const uint8_t* clip = p.frames + i0 * p.s0;
  const sn_ws ws = sn_ws_of(p.ws, gridDim.y, p.n1, blocks);

  static_assert(2 * SN_WAVES * SN_BINS == SN_T, "one thread clears one LDS counter");
  (&s_hist[0][0][0])[t] = 0;
  __syncthreads();

  uint32_t prev[2] = {0, 0};
  int mode = sn_mode(clip, fbytes, off, nx);
  sn_raw raw = sn_fetch(clip, off, mode);
  int mode1 = sn_mode(clip + p.s1, fbytes, off, nx);  // (n1 >= 2)
  sn_raw raw1 = sn_fetch(clip + p.s1, off, mode1);
  for (int f = 0; f < p.n1; ++f) {
    const uint8_t* frame = clip + f * p.s1;
    const uint8_t* fnext = frame + 2 * p.s1;
    const int mnext = f + 2 < p.n1 ? sn_mode(fnext, fbytes, off, nx) : 0;
    const sn_raw rnext = sn_fetch(fnext, off, mnext);  // (mode 0 fetches nothing)
    const int par = f & 1;

    uint32_t w[6];
    sn_words(raw, frame, off, mode, nx, w);
    uint32_t cur[2] = {0, 0};
#pragma unroll
    for (int g = 0; g < 2; ++g) {  // 4 pixels = 3 dwords
      const uint32_t* s = w + 3 * g;
      const uint32_t q[4] = {s[0] & 0xffffffu, ((s[0] >> 24) | (s[1] << 8)) & 0xffffffu,
                             ((s[1] >> 16) | (s[2] << 16)) & 0xffffffu, s[2] >> 8};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t y = px_luma(q[k]);
        if (4 * g + k < nx) {
          cur[g] |= y << (8 * k);
          atomicAdd(&s_hist[par][wave][y >> 3], 1u);
        }
      }
    }
    if (f > 0) {  // (a pixel that does not exist is 0 in both frames)
      uint32_t sad = 0;
#pragma unroll
      for (int g = 0; g < 2; ++g) sad += sn_absdiff4(cur[g], prev[g]);
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) sad += __shfl_down(sad, s, 64);
      if (lane == 0) s_sad[par][wave] = sad;
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) prev[g] = cur[g];
    __syncthreads();
    const long long fi = (long long)i0 * p.n1 + f;
    if (t < SN_BINS) {  // (buffer `par` is next written two frames on, after the next frame's barrier)
      unsigned c = 0;
#pragma unroll
      for (int v = 0; v < SN_WAVES; ++v) {
        c += s_hist[par][v][t];
        s_hist[par][v][t] = 0;
      }
      ws.hist[(fi * blocks + bx) * SN_BINS + t] = c;
    }
    if (t == SN_BINS && f > 0) {
      unsigned c = 0;
#pragma unroll
      for (int v = 0; v < SN_WAVES; ++v) c += s_sad[par][v];
      ws.sad[((long long)i0 * (p.n1 - 1) + (f - 1)) * blocks + bx] = c;
    }
    raw = raw1, mode = mode1;
    raw1 = rnext, mode1 = mnext;
  }
}

__global__ __launch_bounds__(FIN_T) void synth_scene_finalize_kernel(const dvie_synth_scene_desc p, long long blocks) {
  __shared__ long long s_a[FIN_T];
  __shared__ long long s_b[FIN_T];
  const int t = threadIdx.x, pr = blockIdx.x, i0 = blockIdx.y;
  const sn_ws ws = sn_ws_of(p.ws, gridDim.y, p.n1, blocks);
  constexpr int GROUPS = FIN_T / SN_BINS;
  const int bin = t & (SN_BINS - 1), grp = t >> 5;
  const uint32_t* ha = ws.hist + ((long long)i0 * p.n1 + pr) * blocks * SN_BINS;
  const uint32_t* hb = ha + blocks * SN_BINS;
  long long a = 0, b = 0, sad = 0;
  // few blocks run this kernel, so its time is the latency of these loads: they are issued in
  // batches of 2 x FIN_U independent loads before any is consumed
  for (long long j0 = grp; j0 < blocks; j0 += GROUPS * FIN_U) {
    uint32_t va[FIN_U], vb[FIN_U];
#pragma unroll
    for (int u = 0; u < FIN_U; ++u) {
      const long long j = j0 + (long long)u * GROUPS;
      const bool ok = j < blocks;
      va[u] = ok ? ha[j * SN_BINS + bin] : 0u;
      vb[u] = ok ? hb[j * SN_BINS + bin] : 0u;
    }
#pragma unroll
    for (int u = 0; u < FIN_U; ++u) a += (long long)va[u], b += (long long)vb[u];
  }
  const uint32_t* sp = ws.sad + ((long long)i0 * (p.n1 - 1) + pr) * blocks;
  for (long long j = t; j < blocks; j += FIN_T) sad += (long long)sp[j];
  s_a[t] = a;
  s_b[t] = b;
  __syncthreads();
  long long hd = 0;
  if (t < SN_BINS) {  // (the first half of wave 0: one bin each)
    long long x = 0, y = 0;
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) x += s_a[g * SN_BINS + t], y += s_b[g * SN_BINS + t];
    hd = x < y ? y - x : x - y;
  }
  // wave sums through shuffles, then thread 0 adds the 16 waves' SADs
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    sad += __shfl_down(sad, k, 64);
    hd += __shfl_down(hd, k, 64);
  }
  __syncthreads();  // (s_b was read above)
  if ((t & 63) == 0) s_b[t >> 6] = sad;
  __syncthreads();
  if (t == 0) {
    long long total = 0;
#pragma unroll
    for (int v = 0; v < FIN_T / 64; ++v) total += s_b[v];
    const long long o = (long long)i0 * (p.n1 - 1) + pr;
    p.hdiff[o] = hd;
    p.sad[o] = total;
    if (p.cut) p.cut[o] = (uint8_t)(total >= p.sad_min && hd >= p.hist_min);
  }
}

__global__ __launch_bounds__(CF_T) void synth_cutfill_kernel(const dvie_synth_cutfill_desc p) {
  const int step = 1 << p.levels;
  const int pr = blockIdx.y / (step - 1), j = 1 + blockIdx.y % (step - 1), b = blockIdx.z;
  if (!p.cut[(long long)b * (p.n1 - 1) + pr]) return;  // (uniform over the block)
  uint8_t* clip = p.slots + b * p.s0;
  const uint8_t* src = clip + (long long)(j <= step / 2 ? pr : pr + 1) * step * p.s1;
  uint8_t* dst = clip + ((long long)pr * step + j) * p.s1;
  const long long lo = (long long)blockIdx.x * CF_PIECE, hi = min(lo + CF_PIECE, p.nbytes);
  const int t = threadIdx.x;
  if (((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0) {
    const long long vend = lo + (hi - lo) / 16 * 16;
    for (long long o = lo + 16LL * t; o < vend; o += 16LL * CF_T) *(uint4*)(dst + o) = *(const uint4*)(src + o);
    for (long long o = vend + t; o < hi; o += CF_T) dst[o] = src[o];
  } else {
    for (long long o = lo + t; o < hi; o += CF_T) dst[o] = src[o];
  }
}

// blocks of a clip; 0: the sizes are invalid (dvie_synth_scene then says why)
static long long scene_blocks(const dvie_synth_scene_desc* d) {
  if (!d || d->h < 1 || d->w < 1 || d->h > (1 << 16) || d->w > (1 << 16) || d->n0 < 1 || d->n0 > 65535 || d->n1 < 2 ||
      d->n1 > 65535)
    return 0;
  return ((long long)d->h * d->w + SN_TILE - 1) / SN_TILE;
}

}  // namespace dvie

using namespace dvie;

extern "C" {

size_t dvie_synth_scene_ws_bytes(const dvie_synth_scene_desc* d) {
  const long long blocks = scene_blocks(d);
  if (!blocks) return 0;
  return (size_t)(4 * blocks * ((long long)d->n0 * d->n1 * SN_BINS + (long long)d->n0 * (d->n1 - 1)) + 7) / 8 * 8;
}

int dvie_synth_scene(const dvie_synth_scene_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->frames, "synth_scene: frames must not be null");
  DVIE_CHECK_ARG(d->sad && d->hdiff, "synth_scene: sad / hdiff outputs must not be null");
  DVIE_CHECK_ARG(d->h >= 1 && d->w >= 1 && d->h <= (1 << 16) && d->w <= (1 << 16),
                 "synth_scene: h=%d and w=%d must be in 1..%d", d->h, d->w, 1 << 16);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n0 <= 65535, "synth_scene: n0=%d clips must be in 1..65535", d->n0);
  DVIE_CHECK_ARG(d->n1 >= 2 && d->n1 <= 65535, "synth_scene: n1=%d frames must be in 2..65535 (a pair needs two)",
                 d->n1);
  if (d->cut)
    DVIE_CHECK_ARG(d->sad_min >= 0 && d->hist_min >= 0, "synth_scene: sad_min=%lld and hist_min=%lld must not be negative",
                   d->sad_min, d->hist_min);
  DVIE_CHECK_ARG(d->ws, "synth_scene: workspace is missing (dvie_synth_scene_ws_bytes bytes)");
  DVIE_CHECK_ARG(((((uintptr_t)d->ws) | ((uintptr_t)d->sad) | ((uintptr_t)d->hdiff)) & 7) == 0,
                 "synth_scene: ws, sad and hdiff must be 8-byte aligned");
  const long long blocks = scene_blocks(d);
  hipStream_t s = (hipStream_t)stream;
  DVIE_LAUNCH(synth_scene_kernel, dim3((unsigned)blocks, (unsigned)d->n0), dim3(SN_T), 0, s, *d);
  DVIE_LAUNCH(synth_scene_finalize_kernel, dim3((unsigned)(d->n1 - 1), (unsigned)d->n0), dim3(FIN_T), 0, s, *d, blocks);
  DVIE_RETURN_LAUNCH();
}

int dvie_synth_cutfill(const dvie_synth_cutfill_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->slots && d->cut, "synth_cutfill: slots / cut must not be null");
  DVIE_CHECK_ARG(d->nbytes >= 1, "synth_cutfill: nbytes=%lld must be positive", d->nbytes);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n0 <= 65535, "synth_cutfill: n0=%d clips must be in 1..65535", d->n0);
  DVIE_CHECK_ARG(d->n1 >= 2, "synth_cutfill: n1=%d input frames must be at least 2", d->n1);
  DVIE_CHECK_ARG(d->levels >= 0 && d->levels <= 8, "synth_cutfill: levels=%d must be in 0..8", d->levels);
  const long long a1 = d->s1 < 0 ? -d->s1 : d->s1;
  DVIE_CHECK_ARG(a1 >= d->nbytes, "synth_cutfill: slot stride %lld lets slots of %lld bytes overlap", d->s1, d->nbytes);
  if (d->levels == 0) return DVIE_OK;  // nothing lies between two inputs
  const long long inner = (long long)(d->n1 - 1) * ((1 << d->levels) - 1);
  DVIE_CHECK_ARG(inner <= 65535, "synth_cutfill: %lld interior slots are too many for one launch (65535)", inner);
  const long long pieces = (d->nbytes + CF_PIECE - 1) / CF_PIECE;
  DVIE_CHECK_ARG(pieces <= 0x7fffffffLL, "synth_cutfill: nbytes=%lld too large", d->nbytes);
  DVIE_LAUNCH(synth_cutfill_kernel, dim3((unsigned)pieces, (unsigned)inner, (unsigned)d->n0), dim3(CF_T), 0,
              (hipStream_t)stream, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
