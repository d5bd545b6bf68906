// dvie_synth_yuv2rgb / dvie_synth_rgb2yuv: packed planar 8-bit Y'CbCr frames (as a YUV4MPEG2 file
// holds them) <-> uint8 RGB frames (include/dvie.h has the integer formulas; DESIGN.md "Streaming
// and Y4M" the measurements).
//
// Both are pure streaming byte work (4:2:0: 1.5 B of one side and 3 B of the other per pixel), no
// LDS, no cross-lane traffic.  A lane owns a run of 8 pixels of one row (4:4:4) or of the two rows
// of a chroma row (4:2:0), so a chroma sample is loaded once and serves its whole 2x2 block: per
// run 2 x 8 B of Y, 4 B of U and of V, and 2 x 24 B of RGB.  Consecutive lanes are consecutive
// runs of one row, so the 8-byte accesses of a wave cover one contiguous span of that row.
//
// Alignment is decided per lane and per side.  A whole run (8 pixels, both rows present) whose
// addresses are 8-byte aligned (the 4 chroma bytes of a 4:2:0 run: 4-byte) moves as whole vectors;
// every other run -- the last columns of a width that is no multiple of 8, the odd last row, and
// any row or frame whose base is not aligned (a packed frame of odd size starts anywhere) -- moves
// the bytes that exist one by one.  The arithmetic between the two is the same code.  Every byte
// of the outputs has exactly one owner, so nothing is read-modify-written.
#include "common.h"

namespace dvie {

namespace {

constexpr int YUV_RUN = 8;

struct yuv_geom {
  long long uoff, voff;  // bytes from the start of a packed frame to its U and V planes
  int cw;                // width of a chroma row
  int runs, rowsets;     // runs per row, row sets (pairs for 4:2:0) per frame
  int total;             // lanes with work
};

__device__ __forceinline__ bool aligned8(const void* a, const void* b) {
  return ((((uintptr_t)a) | ((uintptr_t)b)) & 7) == 0;
}

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// where this lane's run lives
template <bool k420>
struct yuv_run {
  static constexpr int ROWS = k420 ? 2 : 1;
  static constexpr int CN = k420 ? YUV_RUN / 2 : YUV_RUN;  // chroma samples of a whole run
  uint8_t *yp, *up, *vp, *rp;
  int nx, ny, nc;  // pixels per row, rows and chroma samples of the run that exist
  bool full, yuv_vec, rgb_vec;

  __device__ __forceinline__ yuv_run(const dvie_synth_yuv_desc& p, const yuv_geom& g, int idx) {
    const int run = idx % g.runs, t = idx / g.runs;
    const int rs = t % g.rowsets, f = t / g.rowsets;
    const int x0 = run * YUV_RUN, y0 = rs * ROWS;
    nx = min(YUV_RUN, p.w - x0);
    ny = min(ROWS, p.h - y0);
    nc = k420 ? (nx + 1) / 2 : nx;
    uint8_t* frame = p.yuv + f * p.yuv_stride;
    yp = frame + (long long)y0 * p.w + x0;
    up = frame + g.uoff + (long long)rs * g.cw + (k420 ? x0 / 2 : x0);
    vp = up + (g.voff - g.uoff);
    rp = p.rgb + f * p.rgb_stride + y0 * p.rgb_row_stride + 3 * x0;
    full = nx == YUV_RUN && ny == ROWS;
    const bool c_ok = k420 ? ((((uintptr_t)up) | ((uintptr_t)vp)) & 3) == 0 : aligned8(up, vp);
    yuv_vec = full && aligned8(yp, ROWS == 2 ? yp + p.w : yp) && c_ok;
    rgb_vec = full && aligned8(rp, ROWS == 2 ? rp + p.rgb_row_stride : rp);
  }
};

// byte k of the 8 bytes held little-endian in w[0], w[1]
__device__ __forceinline__ int byte_of(const uint32_t* w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

}  // namespace

template <bool k420>
__global__ __launch_bounds__(256) void synth_yuv2rgb_kernel(const dvie_synth_yuv_desc p, const yuv_geom g) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.total) return;
  const yuv_run<k420> r(p, g, idx);
  constexpr int ROWS = yuv_run<k420>::ROWS;

  // ---- load: the run's Y bytes of each row and its chroma bytes, little-endian in dwords ----
  uint32_t yw[ROWS][2], uw[2] = {0, 0}, vw[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < ROWS; ++j) yw[j][0] = yw[j][1] = 0;
  if (r.yuv_vec) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const uint2 t = *(const uint2*)(r.yp + (long long)j * p.w);
      yw[j][0] = t.x;
      yw[j][1] = t.y;
    }
    if (k420) {
      uw[0] = *(const uint32_t*)r.up;
      vw[0] = *(const uint32_t*)r.vp;
    } else {
      const uint2 tu = *(const uint2*)r.up, tv = *(const uint2*)r.vp;
      uw[0] = tu.x, uw[1] = tu.y, vw[0] = tv.x, vw[1] = tv.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int k = 0; k < YUV_RUN; ++k)
        if (j < r.ny && k < r.nx) yw[j][k >> 2] |= (uint32_t)r.yp[(long long)j * p.w + k] << (8 * (k & 3));
#pragma unroll
    for (int k = 0; k < yuv_run<k420>::CN; ++k)
      if (k < r.nc) {
        uw[k >> 2] |= (uint32_t)r.up[k] << (8 * (k & 3));
        vw[k >> 2] |= (uint32_t)r.vp[k] << (8 * (k & 3));
      }
  }

  // ---- convert: px[j][k] = R | G << 8 | B << 16 ----
  const int IY = p.table[0], IRV = p.table[1], IBU = p.table[2], IGU = p.table[3], IGV = p.table[4];
  uint32_t px[ROWS][YUV_RUN];
#pragma unroll
  for (int k = 0; k < YUV_RUN; ++k) {
    const int c = k420 ? k >> 1 : k;
    const int u = byte_of(uw, c) - 128, v = byte_of(vw, c) - 128;
    const int dr = IRV * v + 32768, dg = 32768 - IGU * u - IGV * v, db = IBU * u + 32768;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const int y = IY * (byte_of(yw[j], k) - p.yo);
      px[j][k] = (uint32_t)clip255((y + dr) >> 16) | ((uint32_t)clip255((y + dg) >> 16) << 8) |
                 ((uint32_t)clip255((y + db) >> 16) << 16);
    }
  }

  // ---- store: 24 bytes per row ----
  if (r.rgb_vec) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      uint32_t w[6];
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // 4 pixels = 12 bytes = 3 dwords
        const uint32_t* s = px[j] + 4 * h;
        w[3 * h + 0] = s[0] | (s[1] << 24);
        w[3 * h + 1] = (s[1] >> 8) | (s[2] << 16);
        w[3 * h + 2] = (s[2] >> 16) | (s[3] << 8);
      }
      uint2* q = (uint2*)(r.rp + j * p.rgb_row_stride);
      q[0] = make_uint2(w[0], w[1]);
      q[1] = make_uint2(w[2], w[3]);
      q[2] = make_uint2(w[4], w[5]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int k = 0; k < YUV_RUN; ++k)
        if (j < r.ny && k < r.nx) {
          uint8_t* q = r.rp + j * p.rgb_row_stride + 3 * k;
          q[0] = (uint8_t)px[j][k];
          q[1] = (uint8_t)(px[j][k] >> 8);
          q[2] = (uint8_t)(px[j][k] >> 16);
        }
  }
}

template <bool k420>
__global__ __launch_bounds__(256) void synth_rgb2yuv_kernel(const dvie_synth_yuv_desc p, const yuv_geom g) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.total) return;
  const yuv_run<k420> r(p, g, idx);
  constexpr int ROWS = yuv_run<k420>::ROWS, CN = yuv_run<k420>::CN;

  // ---- load: px[j][k] = R | G << 8 | B << 16; a pixel that does not exist is 0 ----
  uint32_t px[ROWS][YUV_RUN];
  if (r.rgb_vec) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const uint2* q = (const uint2*)(r.rp + j * p.rgb_row_stride);
      const uint2 a = q[0], b = q[1], c = q[2];
      const uint32_t w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t* s = w + 3 * h;
        px[j][4 * h + 0] = s[0] & 0xffffffu;
        px[j][4 * h + 1] = ((s[0] >> 24) | (s[1] << 8)) & 0xffffffu;
        px[j][4 * h + 2] = ((s[1] >> 16) | (s[2] << 16)) & 0xffffffu;
        px[j][4 * h + 3] = s[2] >> 8;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int k = 0; k < YUV_RUN; ++k) {
        px[j][k] = 0;
        if (j < r.ny && k < r.nx) {
          const uint8_t* q = r.rp + j * p.rgb_row_stride + 3 * k;
          px[j][k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
      }
  }

  // ---- convert ----
  const int* FY = p.table;
  const int* FU = p.table + 3;
  const int* FV = p.table + 6;
  uint32_t yw[ROWS][2], uw[2] = {0, 0}, vw[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    yw[j][0] = yw[j][1] = 0;
#pragma unroll
    for (int k = 0; k < YUV_RUN; ++k) {
      const int R = px[j][k] & 255, G = (px[j][k] >> 8) & 255, B = px[j][k] >> 16;
      const int y = clip255(p.yo + ((FY[0] * R + FY[1] * G + FY[2] * B + 32768) >> 16));
      yw[j][k >> 2] |= (uint32_t)y << (8 * (k & 3));
    }
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    // the sums over the block's pixels (absent ones are 0) and 4 / (the number that exist)
    int SR = 0, SG = 0, SB = 0;
    constexpr int BW = k420 ? 2 : 1;
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int i = 0; i < BW; ++i) {
        const uint32_t v = px[j][BW * c + i];
        SR += v & 255, SG += (v >> 8) & 255, SB += v >> 16;
      }
    const int n = k420 ? min(2, r.nx - 2 * c) * r.ny : 1;  // 4, 2, 1 (or <= 0: no such block)
    const int mul = k420 ? (n == 4 ? 1 : (n == 2 ? 2 : 4)) : 4;
    const int u = clip255(128 + (((FU[0] * SR + FU[1] * SG + FU[2] * SB) * mul + 131072) >> 18));
    const int v = clip255(128 + (((FV[0] * SR + FV[1] * SG + FV[2] * SB) * mul + 131072) >> 18));
    uw[c >> 2] |= (uint32_t)u << (8 * (c & 3));
    vw[c >> 2] |= (uint32_t)v << (8 * (c & 3));
  }

  // ---- store ----
  if (r.yuv_vec) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) *(uint2*)(r.yp + (long long)j * p.w) = make_uint2(yw[j][0], yw[j][1]);
    if (k420) {
      *(uint32_t*)r.up = uw[0];
      *(uint32_t*)r.vp = vw[0];
    } else {
      *(uint2*)r.up = make_uint2(uw[0], uw[1]);
      *(uint2*)r.vp = make_uint2(vw[0], vw[1]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int k = 0; k < YUV_RUN; ++k)
        if (j < r.ny && k < r.nx) r.yp[(long long)j * p.w + k] = (uint8_t)byte_of(yw[j], k);
#pragma unroll
    for (int k = 0; k < CN; ++k)
      if (k < r.nc) {
        r.up[k] = (uint8_t)byte_of(uw, k);
        r.vp[k] = (uint8_t)byte_of(vw, k);
      }
  }
}

namespace {

// the checks both directions share; `ntab`: the table entries the direction reads
int yuv_prepare(const dvie_synth_yuv_desc* d, const char* what, int ntab, yuv_geom* g) {
  DVIE_CHECK_ARG(d && d->yuv && d->rgb, "%s: yuv / rgb must not be null", what);
  DVIE_CHECK_ARG(d->layout == DVIE_YUV_420 || d->layout == DVIE_YUV_444, "%s: layout=%d must be %d or %d", what,
                 d->layout, DVIE_YUV_420, DVIE_YUV_444);
  DVIE_CHECK_ARG(d->n >= 1, "%s: n=%d frames must be positive", what, d->n);
  DVIE_CHECK_ARG(d->h >= 1 && d->w >= 1 && d->h <= (1 << 16) && d->w <= (1 << 16),
                 "%s: h=%d and w=%d must be in 1..%d", what, d->h, d->w, 1 << 16);
  DVIE_CHECK_ARG(d->yo >= 0 && d->yo <= 255, "%s: yo=%d must be in 0..255", what, d->yo);
  for (int k = 0; k < ntab; ++k)
    DVIE_CHECK_ARG(d->table[k] >= -(1 << 18) && d->table[k] <= (1 << 18), "%s: table[%d]=%d must be in -2^18..2^18",
                   what, k, d->table[k]);
  const bool s420 = d->layout == DVIE_YUV_420;
  const long long ch = s420 ? (d->h + 1) / 2 : d->h, cw = s420 ? (d->w + 1) / 2 : d->w;
  const long long ybytes = (long long)d->h * d->w, fbytes = ybytes + 2 * ch * cw;
  DVIE_CHECK_ARG(d->rgb_row_stride >= 3LL * d->w, "%s: rgb_row_stride=%lld is less than a row of %lld bytes", what,
                 d->rgb_row_stride, 3LL * d->w);
  if (d->n > 1) {
    DVIE_CHECK_ARG(d->yuv_stride >= fbytes, "%s: yuv_stride=%lld is less than a packed frame of %lld bytes", what,
                   d->yuv_stride, fbytes);
    DVIE_CHECK_ARG(d->rgb_stride >= (d->h - 1) * d->rgb_row_stride + 3LL * d->w,
                   "%s: rgb_stride=%lld lets frames of %d rows of stride %lld overlap", what, d->rgb_stride, d->h,
                   d->rgb_row_stride);
  }
  g->uoff = ybytes;
  g->voff = ybytes + ch * cw;
  g->cw = (int)cw;
  g->runs = (d->w + YUV_RUN - 1) / YUV_RUN;
  g->rowsets = (int)ch;
  const long long total = (long long)d->n * g->rowsets * g->runs;
  DVIE_CHECK_ARG(total <= 0x7fffff00LL, "%s: %d frames of %dx%d are too many for one launch", what, d->n, d->h, d->w);
  g->total = (int)total;
  return DVIE_OK;
}

}  // namespace

}  // namespace dvie

using namespace dvie;

extern "C" {

int dvie_synth_yuv2rgb(const dvie_synth_yuv_desc* d, void* stream) {
  yuv_geom g;
  const int rc = yuv_prepare(d, "synth_yuv2rgb", 5, &g);
  if (rc != DVIE_OK) return rc;
  const dim3 grid((unsigned)((g.total + 255) / 256));
  if (d->layout == DVIE_YUV_420)
    DVIE_LAUNCH(synth_yuv2rgb_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *d, g);
  else
    DVIE_LAUNCH(synth_yuv2rgb_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *d, g);
  DVIE_RETURN_LAUNCH();
}

int dvie_synth_rgb2yuv(const dvie_synth_yuv_desc* d, void* stream) {
  yuv_geom g;
  const int rc = yuv_prepare(d, "synth_rgb2yuv", 9, &g);
  if (rc != DVIE_OK) return rc;
  const dim3 grid((unsigned)((g.total + 255) / 256));
  if (d->layout == DVIE_YUV_420)
    DVIE_LAUNCH(synth_rgb2yuv_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *d, g);
  else
    DVIE_LAUNCH(synth_rgb2yuv_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *d, g);
  DVIE_RETURN_LAUNCH();
}

}  // extern "C"
