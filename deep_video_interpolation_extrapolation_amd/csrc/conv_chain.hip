// Two back-to-back 1x1 convolutions on the same pixels in ONE launch (gfx950, bf16):
//   op a: c <= 64 -> 256 channels, epilogue as conv1x1_kernel<4, 1, ...> (bias, residual, forward
//         activation with the sign bitmap written, or residual + derivative from the bitmap / z)
//   op b: 256 -> 64 channels reading a's output, epilogue as conv1x1_persist_kernel<2, 3, ...>
//         (bias, activation, derivative from a 64-channel z)
// layer1's Bottlenecks (nets/HRNet.py:66-85) chain them in both directions: conv3(N) ->
// conv1(N + 1) forward, the data gradient of conv1(N + 1) -> that of conv3(N) backward.  The
// 256-channel map between them is still stored (residual, weight gradients and bitmap readers
// need it) but not read back: the workgroup that produced a pixel tile of it applies the second
// GEMM from LDS.
//
// A persistent workgroup of 8 waves walks 64-pixel tiles T = b, b + G, ...; both weight matrices
// stay in LDS for the whole launch.  Per tile:
//   top    counted wait for this tile's DMA (x rows, residual rows), barrier; then the NEXT
//          tile's DMA and its register operands (bitmap bytes / z) are issued, so they are in
//          flight for the whole of this tile
//   GEMM 1 wave (wp, wc) of a 2 x 4 grid: 32 pixels x 64 channels, one 64-deep K-step
//   epi 1  residual read from the middle tile M (where the DMA put it), result stored to y
//          (and the bitmap) and written back to the same 16-byte chunk of M
//   GEMM 2 waves 0-3 (2 x 2 grid of 32 x 32): K = 256 from M, 16-deep slices in ascending order
//          into one accumulator -- the MFMA sequence of the 256 -> 64 kernel, so the results are
//          the two-launch results bit for bit
//   epi 2  stored to b's y
// LDS images: x and W1 as 128-byte rows (the swizzle of conv1x1.hip), M and W2 as 512-byte
// rows (pixel / output channel) whose 16-byte chunk index is XORed with row & 15: the 16 rows
// of a ds_read_b128 lane group fall on 16 distinct slots of the 256-byte bank row.
// Every global store is a buffer store that all lanes issue (masked lanes aimed past the
// range), so the per-wave store count the next tile's counted wait relies on is uniform.
#include "conv_epilogue.h"

namespace dvie {

// conv1x1.hip: -1 when that file does not take the launch, else 10 * TMC + NS of the tile shape
// it runs (41: single K-step 128-channel wave tiles, 23: the multi-K-step 64-channel tiles);
// *zb: bit 0 the launch reads the bitmap in place of z, bit 1 it writes it
int conv1x1_route(const dvie_conv_desc& p, int* zb);

#define DVIE_CHAIN_VMCNT(N) __builtin_amdgcn_s_waitcnt(((N) & 15) | (((N) >> 4) << 14) | (7 << 4) | (15 << 8))

struct ChainCfg {
  static constexpr int BP = 64;                    // pixels per tile
  static constexpr int XSZ = BP * 128;             // x tile: 64 rows x 128 B
  static constexpr int W1SZ = 256 * 128;           // W of op a: 256 rows x 128 B
  static constexpr int W2SZ = 64 * 512;            // W of op b: 64 rows x 512 B
  static constexpr int MSZ = BP * 512;             // middle tile: 64 pixel rows x 512 B
  static constexpr int X0 = 0, W1 = 2 * XSZ, W2 = W1 + W1SZ, M0 = W2 + W2SZ;
  static constexpr int SMEM = M0 + 2 * MSZ;        // 144 KB: one workgroup per CU
  static constexpr int GRID = 256;
};

// AM (op a's epilogue): 0 forward, 1 forward + bitmap written, 2 derivative from the bitmap,
// 3 derivative from z.  RES: op a adds a residual.  BZ: op b takes a derivative from its z.
template <int AM, bool RES, bool BZ>
__global__ __launch_bounds__(512) void conv1x1_chain_kernel(const dvie_conv_desc a_in, const dvie_conv_desc b_in, int n_tiles) {
  typedef ChainCfg C;
  // none, ReLU or LeakyReLU (the launcher's check), said so that act8's other arms fold away
  dvie_conv_desc a = a_in, b = b_in;
  a.act = a_in.act == DVIE_ACT_LRELU ? DVIE_ACT_LRELU : a_in.act == DVIE_ACT_RELU ? DVIE_ACT_RELU : DVIE_ACT_NONE;
  b.act = b_in.act == DVIE_ACT_LRELU ? DVIE_ACT_LRELU : b_in.act == DVIE_ACT_RELU ? DVIE_ACT_RELU : DVIE_ACT_NONE;
  a.dact = a_in.dact == DVIE_ACT_LRELU ? DVIE_ACT_LRELU : a_in.dact == DVIE_ACT_RELU ? DVIE_ACT_RELU : DVIE_ACT_NONE;
  b.dact = b_in.dact == DVIE_ACT_LRELU ? DVIE_ACT_LRELU : b_in.dact == DVIE_ACT_RELU ? DVIE_ACT_RELU : DVIE_ACT_NONE;
  __shared__ __attribute__((aligned(1024))) char smem[C::SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, hh = lane >> 5;
  const unsigned OOB = 0xFFFFFFF0u;

  // XCD-contiguous workgroup id, as conv1x1_persist_kernel
  const int G = gridDim.x;
  const int g8 = blockIdx.x & 7, i8 = blockIdx.x >> 3;
  const int q8 = G >> 3, r8 = G & 7;
  const int bid = (g8 < r8 ? g8 * (q8 + 1) : r8 * (q8 + 1) + (g8 - r8) * q8) + i8;
  const int npix = a.n * a.oh * a.ow;
  const int my_tiles = bid < n_tiles ? (n_tiles - 1 - bid) / G + 1 : 0;
  if (my_tiles == 0) return;

  // buffer resources over each tensor's span (the launcher checked them against 32 bits)
  const unsigned long long np1 = (unsigned long long)npix - 1;
  auto rsrc = [](const void* ptr, unsigned long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, ptr ? (int)bytes : 0, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rx = rsrc(a.x, np1 * a.x_ld * 2ull + a.c * 2ull);
  const __amdgpu_buffer_rsrc_t rw1 = rsrc(a.w, 256ull * a.kpad * 2ull);
  const __amdgpu_buffer_rsrc_t rw2 = rsrc(b.w, 64ull * b.kpad * 2ull);
  const __amdgpu_buffer_rsrc_t rres = rsrc(RES ? a.res : nullptr, np1 * a.res_ld * 2ull + 512ull);
  const __amdgpu_buffer_rsrc_t ry = rsrc(a.y, np1 * a.y_ld * 2ull + 512ull);
  const __amdgpu_buffer_rsrc_t rzb = rsrc((AM == 1 || AM == 2) ? a.zbits : nullptr, np1 * a.zbits_ld + 32ull);
  const __amdgpu_buffer_rsrc_t rza = rsrc(AM == 3 ? a.z : nullptr, np1 * a.z_ld * 2ull + 512ull);
  const __amdgpu_buffer_rsrc_t ry2 = rsrc(b.y, np1 * b.y_ld * 2ull + 128ull);
  const __amdgpu_buffer_rsrc_t rz2 = rsrc(BZ ? b.z : nullptr, np1 * b.z_ld * 2ull + 128ull);

  // ---- DMA geometry.  128-byte rows: piece = 8 rows, lane -> row 8 piece + lane / 8, LDS chunk
  // lane % 8 holding source chunk (lane % 8) ^ ((row >> 1) & 7).  512-byte rows: piece = 2 rows,
  // lane -> row 2 piece + lane / 32, LDS chunk lane % 32 holding source chunk (lane % 32) ^ (row & 15).
  const int xrow = wave * 8 + (lane >> 3);
  const int xcs = (lane & 7) ^ ((xrow >> 1) & 7);
  const bool xc_ok = xcs * 8 < a.c;  // (c < 64: channel padding, zeros)
  int mrow[4], mcs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    mrow[q] = (wave + 8 * q) * 2 + (lane >> 5);
    mcs[q] = (lane & 31) ^ (mrow[q] & 15);
  }
  // tile i of this workgroup into buffer i & 1: one x piece per wave, four residual pieces
  auto issue_tile = [&](int i) {
    const int p0 = (bid + i * G) * C::BP;
    const int buf = i & 1;
    lds_dma16(rx, smem + C::X0 + buf * C::XSZ + wave * 1024,
              (xc_ok && p0 + xrow < npix) ? (unsigned)(p0 + xrow) * (unsigned)a.x_ld * 2u + xcs * 16u : OOB);
    if constexpr (RES) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        lds_dma16(rres, smem + C::M0 + buf * C::MSZ + (wave + 8 * q) * 1024,
                  p0 + mrow[q] < npix ? (unsigned)(p0 + mrow[q]) * (unsigned)a.res_ld * 2u + mcs[q] * 16u : OOB);
    }
  };

  // ---- roles.  GEMM 1 / epilogue 1: wave (wp, wc) owns pixels 32 wp + r32, channels 64 wc ..
  // + 63.  GEMM 2 / epilogue 2 (waves 0-3): pixels 32 wp + r32, output channels 32 (wave >> 1) .. + 31.
  const int wp = wave & 1, wc = wave >> 1;
  const int prow = 32 * wp + r32;
  const int psw = prow & 15;
  int xf[4], wf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    xf[s] = prow * 128 + (((2 * s + hh) ^ ((prow >> 1) & 7)) << 4);
    wf[s] = (64 * wc + r32) * 128 + (((2 * s + hh) ^ ((r32 >> 1) & 7)) << 4);
  }
  const int w2row = 32 * (wave >> 1) + r32;  // (waves 0-3)

  // register operands of a tile: the lane's bitmap bytes (its wave's 64 channels: 8 bytes), or
  // its 4 chunks of z; for waves 0-3 the 2 chunks of b's z
  struct Pre {
    i32x2 zb;
    i32x4 za[4], z2[2];
  };
  auto load_pre = [&](int i, Pre& o) {
    const int p0 = (bid + i * G) * C::BP;
    const int pix = p0 + prow;
    const bool ok = pix < npix;
    if constexpr (AM == 2)
      o.zb = __builtin_bit_cast(i32x2, __builtin_amdgcn_raw_buffer_load_b64(
                                           rzb, ok ? (unsigned)pix * (unsigned)a.zbits_ld + 8u * wc : OOB, 0, 0));
    if constexpr (AM == 3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int co = 64 * wc + 16 * k + 8 * hh;
        o.za[k] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                rza, ok ? ((unsigned)pix * (unsigned)a.z_ld + co) * 2u : OOB, 0, 0));
      }
    }
    if constexpr (BZ) {
      if (wave < 4) {
#pragma unroll
        for (int P = 0; P < 2; ++P) {
          const int co = 32 * (wave >> 1) + 16 * P + 8 * hh;
          o.z2[P] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                  rz2, ok ? ((unsigned)pix * (unsigned)b.z_ld + co) * 2u : OOB, 0, 0));
        }
      }
    }
  };

  // ---- prologue: both weight matrices, tile 0
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (wave + 8 * q) * 8 + (lane >> 3);
    const int cs = (lane & 7) ^ ((row >> 1) & 7);
    lds_dma16(rw1, smem + C::W1 + (wave + 8 * q) * 1024, cs * 8 < a.c ? (unsigned)row * (unsigned)a.kpad * 2u + cs * 16u : OOB);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    lds_dma16(rw2, smem + C::W2 + (wave + 8 * q) * 1024, (unsigned)mrow[q] * (unsigned)b.kpad * 2u + mcs[q] * 16u);
  issue_tile(0);
  Pre pre = {}, nxt = {};
  load_pre(0, pre);
  // the biases stay in registers: a load inside the loop would be waited for with everything
  // issued before it, the next tile's DMA included
  float bias_a[4][8], bias_b[2][8];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) bias_a[k][e] = 0.f;
#pragma unroll
  for (int P = 0; P < 2; ++P)
#pragma unroll
    for (int e = 0; e < 8; ++e) bias_b[P][e] = 0.f;
  if (a.bias) {
#pragma unroll
    for (int k = 0; k < 4; ++k) add_f32x8(bias_a[k], a.bias + 64 * wc + 16 * k + 8 * hh);
  }
  if (b.bias && wave < 4) {
#pragma unroll
    for (int P = 0; P < 2; ++P) add_f32x8(bias_b[P], b.bias + 32 * (wave >> 1) + 16 * P + 8 * hh);
  }

  // everything the prologue issued has landed (tile 0's part of the wait below)
  __builtin_amdgcn_s_waitcnt(0);
  for (int i = 0; i < my_tiles; ++i) {
    const int buf = i & 1;
    const int p0 = (bid + i * G) * C::BP;
    // this tile's DMA has landed: this wave's pieces by the counted wait (only the stores of
    // the previous tile -- 4 of y, the bitmap's, waves 0-3 their 2 of b's y -- were issued
    // after them), the other waves' by the barrier.  The barrier also ends every wave's reads
    // of the other x buffer (GEMM 1 of tile i - 1) and of the other M (GEMM 2 of tile i - 1).
    if (i > 0) {
      if (wave < 4)
        DVIE_CHAIN_VMCNT(4 + (AM == 1 ? 1 : 0) + 2);
      else
        DVIE_CHAIN_VMCNT(4 + (AM == 1 ? 1 : 0));
    }
    __builtin_amdgcn_s_barrier();
    if (i + 1 < my_tiles) {
      issue_tile(i + 1);
      load_pre(i + 1, nxt);
    }

    // ---- GEMM 1
    const char* X = smem + C::X0 + buf * C::XSZ;
    const char* W1 = smem + C::W1;
    char* M = smem + C::M0 + buf * C::MSZ;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i32x4 bq = *(const i32x4*)(X + xf[s]);
      i32x4 aq[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) aq[j] = *(const i32x4*)(W1 + wf[s] + j * 32 * 128);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, aq[j]), __builtin_bit_cast(bf16x8, bq),
                                                         acc[j], 0, 0, 0);
    }

    // ---- epilogue 1: lane half h holds channels 64 wc + 32 j + 16 P + 8 h .. + 7 of its pixel
    {
      const int pix = p0 + prow;
      const bool ok = pix < npix;
      unsigned zq = 0;  // (AM 1) byte 2 j + P: the bitmap byte 4 j + 2 P + h of the wave's 8
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v[2][8];
        acc_rows8(acc[j], v);
#pragma unroll
        for (int P = 0; P < 2; ++P) {
          const int co = 64 * wc + 32 * j + 16 * P + 8 * hh;
          char* m = M + prow * 512 + (((co >> 3) ^ psw) << 4);
          float* w = v[P];
          if (a.bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] += bias_a[2 * j + P][e];
          }
          i32x4 o;
          if constexpr (AM == 2) {
            const i32x4 r = RES ? *(const i32x4*)m : i32x4{0, 0, 0, 0};
            o = epi8_regs_bits<RES, false>(w, a, &r, nullptr, ((unsigned)pre.zb[j] >> (8 * (2 * P + hh))) & 0xffu);
          } else {
            const i32x4 r = RES ? *(const i32x4*)m : i32x4{0, 0, 0, 0};
            o = epi8_regs<RES, false, AM == 3>(w, a, &r, nullptr, &pre.za[2 * j + P]);
          }
          *(i32x4*)m = o;
          if constexpr (AM == 1) zq |= sign_bits8(o) << (8 * (2 * j + P));
          __builtin_amdgcn_raw_buffer_store_b128(o, ry, ok ? ((unsigned)pix * (unsigned)a.y_ld + co) * 2u : OOB, 0, 0);
        }
      }
      if constexpr (AM == 1) {
        // the wave's 8 bytes of this pixel: even positions are half 0's, odd ones half 1's;
        // half h stores bytes 4 h .. 4 h + 3 (channels 64 wc + 32 h .. + 31)
        const unsigned other = (unsigned)__shfl_xor((int)zq, 32);
        const unsigned ev = hh ? other : zq, od = hh ? zq : other;
        const unsigned e2 = ev >> (16 * hh), o2 = od >> (16 * hh);
        const unsigned z0 = (e2 & 0xffu) | ((o2 & 0xffu) << 8) | ((e2 & 0xff00u) << 8) | ((o2 & 0xff00u) << 16);
        __builtin_amdgcn_raw_buffer_store_b32(z0, rzb, ok ? (unsigned)pix * (unsigned)a.zbits_ld + 8u * wc + 4u * hh : OOB, 0, 0);
      }
    }
    // every wave's part of M is written: GEMM 2 reads all 256 channels
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();

    // ---- GEMM 2 and epilogue 2 (waves 0-3)
    if (wave < 4) {
      const char* W2 = smem + C::W2;
      f32x16 acc2;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
      const char* mb = M + prow * 512;
      const char* wb = W2 + w2row * 512;
      const int wsw = w2row & 15;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const i32x4 bq = *(const i32x4*)(mb + (((2 * s + hh) ^ psw) << 4));
        const i32x4 aq = *(const i32x4*)(wb + (((2 * s + hh) ^ wsw) << 4));
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, aq), __builtin_bit_cast(bf16x8, bq), acc2,
                                                       0, 0, 0);
      }
      float v[2][8];
      acc_rows8(acc2, v);
      const int pix = p0 + prow;
      const bool ok = pix < npix;
#pragma unroll
      for (int P = 0; P < 2; ++P) {
        const int co = 32 * (wave >> 1) + 16 * P + 8 * hh;
        float* w = v[P];
        if (b.bias) {
#pragma unroll
          for (int e = 0; e < 8; ++e) w[e] += bias_b[P][e];
        }
        const i32x4 o = epi8_regs<false, false, BZ>(w, b, nullptr, nullptr, &pre.z2[P]);
        __builtin_amdgcn_raw_buffer_store_b128(o, ry2, ok ? ((unsigned)pix * (unsigned)b.y_ld + co) * 2u : OOB, 0, 0);
      }
    }
    pre = nxt;
  }
  __builtin_amdgcn_s_waitcnt(0);
}

static bool sign_or_none(int v) { return v == DVIE_ACT_NONE || v == DVIE_ACT_LRELU || v == DVIE_ACT_RELU; }

// [p, p + bytes) of two operands intersect (an absent operand intersects nothing)
static bool overlaps(const void* p, unsigned long long pb, const void* q, unsigned long long qb) {
  if (!p || !q || !pb || !qb) return false;
  const uintptr_t a0 = (uintptr_t)p, b0 = (uintptr_t)q;
  return a0 < b0 + qb && b0 < a0 + pb;
}

struct Span {
  const void* p;
  unsigned long long bytes;
};

// 0: no chained launch; else 1 + (AM | RES << 2 | BZ << 3)
static int chain_variant(const dvie_conv_desc& a, const dvie_conv_desc& b) {
  int za = 0, zb = 0;
  // the kernels the two single launches run: the 128-channel wave tile of one K-step, and the
  // three-stage 64-channel tile (persistent or not: the same arithmetic)
  if (conv1x1_route(a, &za) != 41 || conv1x1_route(b, &zb) != 23) return 0;
  auto plain = [](const dvie_conv_desc& p) {
    return p.x && p.w && p.y && !p.out_f32 && !p.beta && !p.phc && p.osy == 1 && p.osx == 1 && p.ory == 0 && p.orx == 0 &&
           p.yh == p.oh && p.yw == p.ow && p.n > 0 && p.oh > 0 && p.ow > 0 && p.c > 0 && p.c % 8 == 0 &&
           p.kpad % 64 == 0 && p.kpad >= p.c && p.x_ld % 8 == 0 && p.x_ld >= p.c && p.y_ld % 8 == 0 && p.y_ld >= p.cout &&
           ((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.w & 15) == 0 && ((uintptr_t)p.y & 15) == 0 &&
           ((uintptr_t)p.bias & 15) == 0 && sign_or_none(p.act) && sign_or_none(p.dact) && !(p.act && p.dact);
  };
  if (!plain(a) || !plain(b)) return 0;
  if (a.n != b.n || a.oh != b.oh || a.ow != b.ow) return 0;
  if (b.x != a.y || b.x_ld != a.y_ld || a.cout != 256 || b.c != 256 || a.c > 64 || b.cout != 64) return 0;
  if (b.res || dvie_conv_zbits(&b) != 0) return 0;
  const bool a_bits_r = a.dact && (za & 1), a_bits_w = a.act && (za & 2);
  if (a.res && (a.res_ld % 8 != 0 || a.res_ld < 256 || ((uintptr_t)a.res & 15))) return 0;
  if (a.dact && !a_bits_r && (!a.z || a.z_ld % 8 != 0 || a.z_ld < 256 || ((uintptr_t)a.z & 15))) return 0;
  if (b.dact && (!b.z || b.z_ld % 8 != 0 || b.z_ld < 64 || ((uintptr_t)b.z & 15))) return 0;
  if ((a_bits_r || a_bits_w) && a.zbits_ld < 32) return 0;

  // spans, each inside the 32-bit offsets of a buffer resource
  const unsigned long long np1 = (unsigned long long)a.n * a.oh * a.ow - 1;
  const Span ax{a.x, np1 * a.x_ld * 2ull + a.c * 2ull}, aw{a.w, 256ull * a.kpad * 2ull}, ab{a.bias, 256ull * 4ull};
  const Span ar{a.res, np1 * a.res_ld * 2ull + 512ull};
  const Span az{(a.dact && !a_bits_r) ? a.z : nullptr, np1 * a.z_ld * 2ull + 512ull};
  const Span azb{(a_bits_r || a_bits_w) ? a.zbits : nullptr, np1 * a.zbits_ld + 32ull};
  const Span ay{a.y, np1 * a.y_ld * 2ull + 512ull};
  const Span bw{b.w, 64ull * b.kpad * 2ull}, bb{b.bias, 64ull * 4ull};
  const Span bz{b.dact ? b.z : nullptr, np1 * b.z_ld * 2ull + 128ull};
  const Span by{b.y, np1 * b.y_ld * 2ull + 128ull};
  for (const Span& s : {ax, aw, ar, az, azb, ay, bw, bz, by})
    if (s.p && s.bytes >= 0xFFFFFF00ull) return 0;
  // no output of one op meets an operand or output of the other (but a's y as b's x)
  for (const Span& o : {ay, a_bits_w ? azb : Span{nullptr, 0}})
    for (const Span& s : {bw, bb, bz, by})
      if (overlaps(o.p, o.bytes, s.p, s.bytes)) return 0;
  for (const Span& s : {ax, aw, ab, ar, az, azb})
    if (overlaps(by.p, by.bytes, s.p, s.bytes)) return 0;

  const int am = a.dact ? (a_bits_r ? 2 : 3) : (a_bits_w ? 1 : 0);
  return 1 + (am | (a.res ? 4 : 0) | (b.dact ? 8 : 0));
}

}  // namespace dvie

using namespace dvie;

extern "C" int dvie_conv_chain(const dvie_conv_desc* a, const dvie_conv_desc* b) {
  return a && b && chain_variant(*a, *b) != 0;
}

extern "C" int dvie_conv2d_chain(const dvie_conv_desc* a, const dvie_conv_desc* b, void* stream) {
  DVIE_CHECK_ARG(a && b, "conv chain: null descriptor");
  const int v = chain_variant(*a, *b);
  DVIE_CHECK_ARG(v != 0, "conv chain: not a chainable pair (dvie_conv_chain): bf16 1x1 c<=64 -> 256 -> 64 on the "
                         "same pixels, b.x = a.y, beta 0, bf16 outputs, disjoint operands");
  hipStream_t s = (hipStream_t)stream;
  dvie_conv_desc pa = *a;
  if (!((v - 1) & 3)) pa.zbits = nullptr;  // a forward without a bitmap to write
  const int npix = a->n * a->oh * a->ow;
  const int n_tiles = (npix + ChainCfg::BP - 1) / ChainCfg::BP;
  const int G = n_tiles < ChainCfg::GRID ? n_tiles : ChainCfg::GRID;
  switch (v - 1) {
#define DVIE_CHAIN_CASE(V)                                                                                          \
  case V:                                                                                                           \
    DVIE_LAUNCH((conv1x1_chain_kernel<(V) & 3, ((V) & 4) != 0, ((V) & 8) != 0>), dim3(G), dim3(512), 0, s, pa, *b, \
                n_tiles);                                                                                           \
    break;
    DVIE_CHAIN_CASE(0) DVIE_CHAIN_CASE(1) DVIE_CHAIN_CASE(2) DVIE_CHAIN_CASE(3) DVIE_CHAIN_CASE(4) DVIE_CHAIN_CASE(5)
    DVIE_CHAIN_CASE(6) DVIE_CHAIN_CASE(7) DVIE_CHAIN_CASE(8) DVIE_CHAIN_CASE(9) DVIE_CHAIN_CASE(10) DVIE_CHAIN_CASE(11)
    DVIE_CHAIN_CASE(12) DVIE_CHAIN_CASE(13) DVIE_CHAIN_CASE(14) DVIE_CHAIN_CASE(15)
#undef DVIE_CHAIN_CASE
  }
  DVIE_RETURN_LAUNCH();
}
