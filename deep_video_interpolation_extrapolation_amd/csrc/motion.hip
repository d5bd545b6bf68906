// dvie_synth_motion: full-search block matching on luma between pairs of uint8 frames
// (include/dvie.h has the integer definition; DESIGN.md "Motion statistics" the traffic and the
// measurements).
//
// motion_plane_kernel (two launches, cur and ref): turns the RGB frames into uint8 luma planes at
// scale s in the workspace.  A thread makes four neighbouring samples (one dword) of a plane that
// is stored WITH its clamped margins, so the matcher has no bounds logic:
//   cur plane: 16*bh rows of 64*groups bytes, sample (y, x) at [y][x]
//   ref plane: 16*bh + 2R rows of PP bytes, sample (y, x) at [y + R][x + R]
// (groups = ceil(bw / 4); PP = 64*groups + 2R rounded up to 4, plus 4).  A stored sample outside
// the plane is the clamped one, P~.  Every source index is clamped into the frame before it is
// used, so no byte outside a frame is read.
//
// motion_match_kernel: grid (groups, bh, pairs), 256 threads.  The workgroup stages the search
// window of its four neighbouring blocks -- 16 + 2R rows of LP = 64 + 2R (+ pad) bytes of the ref
// plane, whole dwords from a dword-aligned start -- in LDS; wave g owns block 4*jg + g.  A wave
// keeps its 16x16 current block in 64 registers (every lane the same values) and spreads the
// (2R+1)^2 candidates over its lanes in groups of four neighbouring dx of one dy, group c = lane +
// 64*k, dy-major.  The rows of a group's four candidates are 16 bytes at byte offsets 0 .. 3 of the
// same five aligned dwords (a block's window columns start at a multiple of 4): the five are read
// from LDS once per row, three v_alignbyte_b32 per dword shift them, and sixteen v_sad_u8 add the
// four candidates' row SADs -- 1.25 LDS dwords and 7 VALU instructions per 16 absolute differences.
// LP / 4 is odd, so the rows a wave touches in one read fall on different banks.  Each lane keeps
// one packed key
//   cost << 26 | (dy*dy + dx*dx) << 14 | (dy + R) << 7 | (dx + R)
// (cost < 2^18, d2 <= 2048 < 2^12, dy + R and dx + R <= 64 < 2^7), the wave takes the minimum
// with shuffles -- the lexicographic order of the definition, whatever the schedule -- and lane 0
// writes the block's four values (and mv / bsad) to the workspace.
//
// motion_finalize_kernel: one workgroup of 1024 threads per pair sums the block values in int64.
#include "common.h"
#include "pixel.h"

namespace dvie {

namespace {

constexpr int MO_T = 256;                 // threads of a block of the plane and match kernels
constexpr int MO_FIN_T = 1024;            // of the finalize kernel: few blocks run it, so its time is load latency
constexpr int MO_G = 4;                   // blocks (waves) of a matcher workgroup
constexpr int MO_B = 16;                  // samples of a block side
constexpr int MO_RMAX = 32;
constexpr int MO_LDS = (MO_B + 2 * MO_RMAX) * ((MO_G * MO_B + 2 * MO_RMAX) / 4 + 1);  // dwords

struct mo_geom {
  int hs, ws, bh, bw, groups;
  int ch, ph;        // rows of a cur / ref plane
  long long cp, pp;  // bytes of a row of a cur / ref plane (multiples of 4)
  int lp;            // bytes of a row of the LDS window (a multiple of 4, lp / 4 odd)
  int wr;            // rows of the LDS window
};

__host__ __device__ __forceinline__ mo_geom mo_geom_of(int h, int w, int R, int s) {
  mo_geom g;
  g.hs = h >> s, g.ws = w >> s;
  g.bh = (g.hs + MO_B - 1) / MO_B, g.bw = (g.ws + MO_B - 1) / MO_B;
  g.groups = (g.bw + MO_G - 1) / MO_G;
  g.ch = MO_B * g.bh, g.ph = g.ch + 2 * R;
  g.cp = (long long)MO_G * MO_B * g.groups;
  g.pp = ((g.cp + 2 * R + 3) & ~3LL) + 4;
  g.lp = ((MO_G * MO_B + 2 * R + 3) & ~3) + 4;  // the last window's rows end at pp exactly
  g.wr = MO_B + 2 * R;
  return g;
}

struct mo_ws {
  uint32_t* cur;   // [pairs][ch][cp / 4]
  uint32_t* ref;   // [pairs][ph][pp / 4]
  uint32_t* part;  // [pairs][bh][bw][4]: d2, sad, sad0, border
};

__host__ __device__ __forceinline__ long long mo_up16(long long x) { return (x + 15) & ~15LL; }

__host__ __device__ __forceinline__ mo_ws mo_ws_of(void* ws, const mo_geom& g, long long pairs) {
  mo_ws r;
  uint8_t* b = (uint8_t*)ws;
  r.cur = (uint32_t*)b;
  b += mo_up16(pairs * g.ch * g.cp);
  r.ref = (uint32_t*)b;
  b += mo_up16(pairs * g.ph * g.pp);
  r.part = (uint32_t*)b;
  return r;
}

}  // namespace

// which: 0 the cur planes, 1 the ref planes.  grid (rows * chunks, pairs)
__global__ __launch_bounds__(MO_T) void motion_plane_kernel(const dvie_synth_motion_desc p, int which) {
  const mo_geom g = mo_geom_of(p.h, p.w, p.radius, p.scale);
  const int rows = which ? g.ph : g.ch, margin = which ? p.radius : 0;
  const long long pd = (which ? g.pp : g.cp) / 4;
  const long long chunks = (pd + MO_T - 1) / MO_T;
  const long long row = blockIdx.x / chunks, cd = (blockIdx.x % chunks) * MO_T + threadIdx.x;
  if (cd >= pd) return;  // (row < rows by the grid)
  const long long f = blockIdx.y;
  const long long i0 = f / p.n1, i1 = f % p.n1;
  const uint8_t* src = which ? p.ref + i0 * p.ref_s0 + i1 * p.ref_s1 : p.cur + i0 * p.cur_s0 + i1 * p.cur_s1;
  const int s = p.scale, n = 1 << s;
  const long long sy = min(max(row - margin, 0LL), (long long)g.hs - 1);
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long sx = min(max(4 * cd + k - margin, 0LL), (long long)g.ws - 1);
    // rows (sy << s) .. + n - 1 <= (hs << s) - 1 <= h - 1, and the same for the columns
    const uint8_t* q = src + (((sy << s) * p.w) + (sx << s)) * 3;
    uint32_t v;
    if (s == 0) {
      v = px_luma(q);
    } else {
      uint32_t sum = 0;
      for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) sum += px_luma(q + ((long long)a * p.w + b) * 3);
      v = (sum + (1u << (2 * s - 1))) >> (2 * s);
    }
    out |= v << (8 * k);
  }
  mo_ws ws = mo_ws_of(p.ws, g, (long long)p.n0 * p.n1);
  (which ? ws.ref : ws.cur)[(f * rows + row) * pd + cd] = out;
}

__global__ __launch_bounds__(MO_T) void motion_match_kernel(const dvie_synth_motion_desc p) {
  __shared__ uint32_t s_win[MO_LDS];

  const mo_geom g = mo_geom_of(p.h, p.w, p.radius, p.scale);
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int jg = blockIdx.x, i = blockIdx.y;
  const long long f = blockIdx.z;
  const mo_ws ws = mo_ws_of(p.ws, g, (long long)p.n0 * p.n1);
  const int R = p.radius, lpd = g.lp / 4;
  const long long ppd = g.pp / 4, cpd = g.cp / 4;

  // the window: ref-plane rows 16 i .. 16 i + wr - 1, bytes 64 jg .. 64 jg + lp - 1 of each
  const uint32_t* rp = ws.ref + (f * g.ph + (long long)MO_B * i) * ppd + (long long)(MO_G * MO_B / 4) * jg;
  for (int k = t; k < g.wr * lpd; k += MO_T) {
    const int r = k / lpd, c = k - r * lpd;
    s_win[k] = rp[r * ppd + c];
  }
  __syncthreads();

  const int j = MO_G * jg + wave;
  if (j >= g.bw) return;  // (no barrier follows)

  uint32_t cur[MO_B * 4];
  const uint32_t* cp = ws.cur + (f * g.ch + (long long)MO_B * i) * cpd + (MO_B / 4) * j;
#pragma unroll
  for (int u = 0; u < MO_B; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) cur[4 * u + v] = cp[u * cpd + v];

  // a lane takes the four candidates dx + R = 4 q .. 4 q + 3 of one dy together: their rows lie in the
  // same five dwords (the block's window columns start at a multiple of 4), shifted by 0 .. 3 bytes
  const int D = 2 * R + 1, DQ = (D + 3) / 4, ngroups = D * DQ;
  unsigned long long best = ~0ULL;
  uint32_t sad0 = 0;
  for (int c = lane; c < ngroups; c += 64) {
    const int dyi = c / DQ, dq = c - dyi * DQ;
    // bytes 16 wave + 4 dq .. + 19 of a window row: at most 2R + 67 < lp
    const uint32_t* q = s_win + dyi * lpd + (MO_B / 4) * wave + dq;
    uint32_t sad[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < MO_B; ++u) {
      uint32_t w[5];
#pragma unroll
      for (int v = 0; v < 5; ++v) w[v] = q[u * lpd + v];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t a = cur[4 * u + v];
        sad[0] = __builtin_amdgcn_sad_u8(a, w[v], sad[0]);
        sad[1] = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(w[v + 1], w[v], 1), sad[1]);
        sad[2] = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(w[v + 1], w[v], 2), sad[2]);
        sad[3] = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(w[v + 1], w[v], 3), sad[3]);
      }
    }
    const int dy = dyi - R;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int dxi = 4 * dq + e, dx = dxi - R;
      if (dxi < D) {  // (the last group of a dy is partial: D is odd)
        const uint32_t cost = sad[e] + (uint32_t)p.penalty * (uint32_t)(abs(dy) + abs(dx));
        const unsigned long long key = ((unsigned long long)cost << 26) | ((unsigned long long)(dy * dy + dx * dx) << 14) |
                                       ((unsigned long long)dyi << 7) | (unsigned long long)dxi;
        best = key < best ? key : best;
        if (dy == 0 && dx == 0) sad0 = sad[e];
      }
    }
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    const unsigned long long o = __shfl_xor(best, k, 64);
    best = o < best ? o : best;
    sad0 += __shfl_xor(sad0, k, 64);  // (one lane holds it, the others 0)
  }
  if (lane == 0) {
    const int dy = (int)((best >> 7) & 127) - R, dx = (int)(best & 127) - R;
    const uint32_t d2 = (uint32_t)((best >> 14) & 4095);
    const uint32_t sad = (uint32_t)(best >> 26) - (uint32_t)p.penalty * (uint32_t)(abs(dy) + abs(dx));
    const uint32_t border = max(abs(dy), abs(dx)) == R;
    const long long o = (f * g.bh + i) * g.bw + j;
    *(uint4*)(ws.part + 4 * o) = make_uint4(d2, sad, sad0, border);
    if (p.mv) {
      p.mv[2 * o] = (int16_t)dy, p.mv[2 * o + 1] = (int16_t)dx;
      p.bsad[2 * o] = sad, p.bsad[2 * o + 1] = sad0;
    }
  }
}

__global__ __launch_bounds__(MO_FIN_T) void motion_finalize_kernel(const dvie_synth_motion_desc p) {
  __shared__ long long s_sum[MO_FIN_T / 64][4];
  const mo_geom g = mo_geom_of(p.h, p.w, p.radius, p.scale);
  const mo_ws ws = mo_ws_of(p.ws, g, (long long)p.n0 * p.n1);
  const int t = threadIdx.x;
  const long long f = blockIdx.x, nb = (long long)g.bh * g.bw;
  const uint4* part = (const uint4*)ws.part + f * nb;
  long long a[4] = {0, 0, 0, 0};
  for (long long k = t; k < nb; k += MO_FIN_T) {
    const uint4 v = part[k];
    a[0] += v.x, a[1] += v.y, a[2] += v.z, a[3] += v.w;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) a[q] += __shfl_down(a[q], k, 64);
    if ((t & 63) == 0) s_sum[t >> 6][q] = a[q];
  }
  __syncthreads();
  if (t < 4) {
    long long total = 0;
#pragma unroll
    for (int v = 0; v < MO_FIN_T / 64; ++v) total += s_sum[v][t];
    (t == 0 ? p.d2 : t == 1 ? p.sad : t == 2 ? p.sad0 : p.border)[f] = total;
  }
}

// the sizes of a descriptor are valid (dvie_synth_motion says why when they are not)
static bool motion_sizes_ok(const dvie_synth_motion_desc* d) {
  return d && d->radius >= 1 && d->radius <= MO_RMAX && d->scale >= 0 && d->scale <= 3 && d->h >= (1 << d->scale) &&
         d->w >= (1 << d->scale) && d->h <= (1 << 16) && d->w <= (1 << 16) && d->n0 >= 1 && d->n1 >= 1 &&
         (long long)d->n0 * d->n1 <= 65535;
}

}  // namespace dvie

using namespace dvie;

extern "C" {

size_t dvie_synth_motion_ws_bytes(const dvie_synth_motion_desc* d) {
  if (!motion_sizes_ok(d)) return 0;
  const mo_geom g = mo_geom_of(d->h, d->w, d->radius, d->scale);
  const long long pairs = (long long)d->n0 * d->n1;
  return (size_t)(mo_up16(pairs * g.ch * g.cp) + mo_up16(pairs * g.ph * g.pp) + 16 * pairs * g.bh * g.bw);
}

int dvie_synth_motion(const dvie_synth_motion_desc* d, void* stream) {
  DVIE_CHECK_ARG(d && d->cur && d->ref, "synth_motion: cur / ref must not be null");
  DVIE_CHECK_ARG(d->d2 && d->sad && d->sad0 && d->border, "synth_motion: d2 / sad / sad0 / border outputs must not be null");
  DVIE_CHECK_ARG(d->radius >= 1 && d->radius <= MO_RMAX, "synth_motion: radius=%d must be in 1..%d", d->radius, MO_RMAX);
  DVIE_CHECK_ARG(d->scale >= 0 && d->scale <= 3, "synth_motion: scale=%d must be in 0..3", d->scale);
  DVIE_CHECK_ARG(d->penalty >= 0 && d->penalty <= 1024, "synth_motion: penalty=%d must be in 0..1024", d->penalty);
  DVIE_CHECK_ARG(d->h >= (1 << d->scale) && d->w >= (1 << d->scale) && d->h <= (1 << 16) && d->w <= (1 << 16),
                 "synth_motion: h=%d and w=%d must be in %d..%d at scale=%d", d->h, d->w, 1 << d->scale, 1 << 16, d->scale);
  DVIE_CHECK_ARG(d->n0 >= 1 && d->n1 >= 1 && (long long)d->n0 * d->n1 <= 65535,
                 "synth_motion: n0=%d times n1=%d pairs must be in 1..65535", d->n0, d->n1);
  DVIE_CHECK_ARG((d->mv != nullptr) == (d->bsad != nullptr), "synth_motion: mv and bsad must be given together");
  DVIE_CHECK_ARG(d->ws, "synth_motion: workspace is missing (dvie_synth_motion_ws_bytes bytes)");
  DVIE_CHECK_ARG((((uintptr_t)d->ws) & 15) == 0, "synth_motion: ws must be 16-byte aligned");
  DVIE_CHECK_ARG(((((uintptr_t)d->d2) | ((uintptr_t)d->sad) | ((uintptr_t)d->sad0) | ((uintptr_t)d->border)) & 7) == 0,
                 "synth_motion: d2, sad, sad0 and border must be 8-byte aligned");
  DVIE_CHECK_ARG(((((uintptr_t)d->mv) & 1) | (((uintptr_t)d->bsad) & 3)) == 0,
                 "synth_motion: mv must be 2-byte and bsad 4-byte aligned");
  const mo_geom g = mo_geom_of(d->h, d->w, d->radius, d->scale);
  const unsigned pairs = (unsigned)(d->n0 * d->n1);
  hipStream_t s = (hipStream_t)stream;
  for (int which = 0; which < 2; ++which) {
    const long long rows = which ? g.ph : g.ch, pd = (which ? g.pp : g.cp) / 4;
    const long long blocks = rows * ((pd + MO_T - 1) / MO_T);  // <= 65600 * 65
    DVIE_LAUNCH(motion_plane_kernel, dim3((unsigned)blocks, pairs), dim3(MO_T), 0, s, *d, which);
  }
  DVIE_LAUNCH(motion_match_kernel, dim3((unsigned)g.groups, (unsigned)g.bh, pairs), dim3(MO_T), 0, s, *d);
  DVIE_LAUNCH(motion_finalize_kernel, dim3(pairs), dim3(MO_FIN_T), 0, s, *d);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
