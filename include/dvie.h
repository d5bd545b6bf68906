/*
 * dvie.h — C ABI of the MI355X-native frame-synthesis hot path
 * (deep_video_interpolation_extrapolation, HIP/CDNA4, gfx950).
 *
 * One shared library (libdvie.so) exports these entry points.  Every entry point takes
 * raw device pointers, plain integer shapes/strides and a hipStream_t (passed as void*),
 * launches asynchronously on that stream, never allocates, and returns an int status
 * (DVIE_OK = 0, DVIE_EINVAL = argument validation failure, otherwise a hipError_t).
 *
 * Activations are NHWC ("channels_last"): element (n, y, x, c) of a tensor with pixel
 * stride `ld` (elements) lives at base[((n*H + y)*W + x)*ld + c].  A channel slice of a
 * wider buffer is addressed by offsetting `base` and keeping the wider `ld`.
 *
 * The reference has no native code: every entry point replaces a PyTorch/cuDNN op that
 * the reference calls from Python.  The reference call site each one replaces is cited
 * next to it (paths relative to the reference repository root).
 */
#ifndef DVIE_H
#define DVIE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVIE_OK 0
#define DVIE_EINVAL 1001

/* element types */
#define DVIE_F32 0
#define DVIE_BF16 1

/* activations (forward) and activation derivatives (backward, computed from the
 * activation's OUTPUT z: lrelu'(z) = z > 0 ? 1 : alpha, elu'(z) = z > 0 ? 1 : z + 1,
 * relu'(z) = z > 0) */
#define DVIE_ACT_NONE 0
#define DVIE_ACT_LRELU 1 /* nn.LeakyReLU(0.2)  nets/HRNet.py:22,59,107 */
#define DVIE_ACT_ELU 2   /* nn.ELU()           nets/HRNet.py:360,362    */
#define DVIE_ACT_RELU 3  /* VGG19 ReLU         nets/vgg.py:11-54         */
#define DVIE_ACT_TANH 4  /* F.tanh RGB head    nets/UNet.py:151, nets/SepUNet.py:65 (tanh'(z) = 1 - z^2) */

/*
 * Implicit-GEMM convolution (forward, and data-gradient as a forward conv over the
 * output gradient with re-packed weights).  Replaces nn.Conv2d forward/backward-data:
 *   3x3 s1 / 3x3 s2 / 1x1 convs of nets/HRNet.py:9-12,52-57,127-129,166-194,367-371,
 *   410-441,444-477; seg encoder nets/HRNet.py:358-364; VGG19 convs nets/vgg.py:11-54.
 *
 * GEMM view: rows = output channels (cout), columns = output pixels of the grid
 * (n, oy, ox) in [0,n)x[0,oh)x[0,ow), reduction over K = taps * c:
 *   acc[co][pix] = sum_{t,ci} w[co][t*c + ci] * x[n][oy*sy + dy(t)][ox*sx + dx(t)][ci]
 * with taps on a th x tw grid, dy(i,j) = dy0 + i*ddy, dx(i,j) = dx0 + j*ddx and
 * t = i*tw + j; out-of-image taps read zero.  w is packed [cout][kpad] (kpad a multiple
 * of 64 elements, zero-filled past taps*c).
 * The result for pixel (n,oy,ox) lands at output position
 *   (n, oy*osy + ory, ox*osx + orx) of a yh x yw image with pixel stride y_ld,
 * which is how the stride-2 data gradient writes its 4 phases.
 * Epilogue, in order: v = acc; v += bias[co]; v += res; v += y_old (beta=1);
 *   v = act(v) (forward activation); v *= act'(z) (dact, derivative from output z);
 *   y = v.
 * Constraints: c % (16/sizeof(elem)) == 0, cout % 4 == 0, every ld % 4 == 0, pointers
 * 16-byte aligned for x/w and 8-byte aligned (bf16) / 16-byte (f32) for y/res/z.
 * Size: one input image and the packed weights must each stay below 4 GiB; a larger
 * batch runs internally as batch chunks whose input span fits (the kernels use 32-bit
 * buffer offsets), so e.g. 448-channel bf16 activations at 1024x2048 work at any n.
 */
typedef struct dvie_conv_desc {
  const void* x;
  const void* w;
  void* y;
  const float* bias; /* [cout] fp32 or NULL */
  const void* res;   /* residual at output placement or NULL (same elem type as y) */
  const void* z;     /* activation output for dact (elem type = dtype) or NULL */
  long long x_ld, y_ld, res_ld, z_ld;
  int n, ih, iw, c;
  int kpad, cout;
  int oh, ow, sy, sx;
  int th, tw, dy0, dx0, ddy, ddx;
  int yh, yw, osy, osx, ory, orx;
  int act, dact, beta, dtype;
  int out_f32; /* 1: y (and res) are fp32, 0: y has elem type dtype */
  float alpha; /* activation slope / parameter */
  int phc;     /* 0, or the stride-2 data gradient of a 3x3 pad-1 conv (nets/HRNet.py:181-194,
                  466-474) in ONE launch: cout = 4*phc output channels are the four output
                  phases, blocks of phc channels in the order (a,b) = (0,0), (1,1), (0,1), (1,0);
                  channel q*phc + ci of grid pixel (oy, ox) lands at channel ci of output pixel
                  (2*oy + a, 2*ox + b) (osy = osx = 2, ory = orx = 0; pixels outside yh x yw are
                  skipped).  Taps 2 x 2 at dy0 = dx0 = 0; tap (i, j) carries weight row
                  kh = a + 1 - 2i, kw = b + 1 - 2j of the forward kernel, so a phase with a = 0
                  (b = 0) has no i = 1 (j = 1) taps: those MFMAs are skipped, not multiplied by
                  zero.  bf16, phc % 32 == 0, no bias / fp32 output. */
  int pad1;
  /* Activation sign bitmap (bf16, act / dact DVIE_ACT_RELU or DVIE_ACT_LRELU; NULL: absent).
     Byte pix * zbits_ld + c / 8, bit c % 8, is set iff the stored bf16 z[pix][c] > 0 (so -0.0,
     +0.0 and NaN give 0); zbits_ld = the buffer's channel count / 8, and a region at channel
     offset c0 (a multiple of 8) passes zbits advanced by c0 / 8.  With act set, a forward kernel
     that knows the bitmap writes it next to y (from the packed bf16 result); with dact set, a
     data-gradient kernel that knows it takes act'(z) from it instead of reading z.  z / z_ld
     stay valid: a kernel that does not know the bitmap reads z (and writes no bitmap), which
     dvie_conv_zbits tells the caller beforehand. */
  void* zbits;
  long long zbits_ld;
} dvie_conv_desc;

int dvie_conv2d_fwd(const dvie_conv_desc* d, void* stream);

/* Nonzero when the kernel dvie_conv2d_fwd chooses for *d honours d->zbits: writes the bitmap
 * (d->act set) or reads it in place of z (d->dact set); 0 when that kernel ignores it.
 * 1: at (nearly) no cost to the launch; 2: a writer that pays for it in its epilogue (the
 * multi-K-step ring 1x1 kernel: +8% on heads.0), for the caller to weigh against its readers. */
int dvie_conv_zbits(const dvie_conv_desc* d);

/* Two back-to-back 1x1 convolutions on the same pixels as ONE launch (conv1x1_chain_kernel;
 * layer1's Bottlenecks, nets/HRNet.py:66-85: conv3(N) -> conv1(N+1) forward, the data gradient
 * of conv1(N+1) -> that of conv3(N) backward).  b reads a's output from on-chip memory; a's
 * output (and bitmap) is still stored.  y, the bitmap and b's y are byte for byte what
 * dvie_conv2d_fwd(a) followed by dvie_conv2d_fwd(b) give.
 * dvie_conv_chain: nonzero iff the pair runs chained.  Both are bf16 1x1 stride-1 convs with
 * identity output placement, bf16 output and beta == 0 on the same n x oh x ow grid;
 * b->x == a->y, b->x_ld == a->y_ld, a->c <= 64 (a multiple of 8), a->cout == b->c == 256,
 * b->cout == 64; act / dact are none, ReLU or LeakyReLU, at most one of them per op (a: bias,
 * residual, activation with the bitmap written when dvie_conv_zbits(a) says so, or residual +
 * derivative from the bitmap or z as the single launch would take it; b: bias, activation or
 * derivative from z, no residual, no bitmap); no output of one op overlaps an operand or output
 * of the other (but a->y as b->x); every tensor's byte span stays below 4 GiB.
 * dvie_conv2d_chain: launches the pair; DVIE_EINVAL (dvie_last_error) when dvie_conv_chain is 0. */
int dvie_conv_chain(const dvie_conv_desc* a, const dvie_conv_desc* b);
int dvie_conv2d_chain(const dvie_conv_desc* a, const dvie_conv_desc* b, void* stream);

/*
 * Weight gradient of the convolution above (replaces nn.Conv2d backward-weight):
 *   part[s][co][t*c + ci] = sum_{pix in split s} g[pix][co] * x[pix + tap t][ci]
 * g is the pre-activation output gradient on the (n, oh, ow) grid (pixel stride g_ld),
 * x the forward input.  The pixel range is cut into `splits` contiguous chunks; fp32
 * partials go to `ws` ([splits][cout][taps*c]).  dvie_wgrad_reduce then sums them.
 */
typedef struct dvie_wgrad_desc {
  const void* g;
  const void* x;
  float* ws;
  long long g_ld, x_ld;
  int n, oh, ow, cout;
  int ih, iw, c, sy;
  int sx, th, tw, dy0;
  int dx0, ddy, ddx, splits;
  int dtype;
  int tmap;   /* with ws_taps > 0: tap t of this launch's th x tw grid (t = i*tw + j) is column
                 block (tmap >> 4t) & 15 of the slab rows */
  float* bws; /* NULL, or the bias-gradient partials: bws[slab][cout] = column sums of g over
                 the slab's pixels (dvie_wgrad_bias_slabs slabs; reduce them with
                 dvie_wgrad_reduce, ws_k = 1).  The halo weight-gradient kernels sum g while
                 they hold it for the MFMAs (no second pass over g); other launches run a
                 column-sum pass.  Replaces the separate nn.Conv2d bias backward. */
  int ws_taps; /* 0: slab rows hold th*tw*c values, tap t at column t*c.  > 0: rows hold
                  ws_taps*c values and this launch writes only its taps' column blocks (tmap),
                  so several launches fill one slab set: the stride-2 weight gradient
                  (nets/HRNet.py:181-194, 466-474) runs as its four input phases, each a
                  stride-1 weight gradient over a phase view of x (x + (a*W + b)*ld, x_ld =
                  2*ld, ih = H/2, iw = W as the row pitch: the halo kernels, which then read
                  only columns < ow, require ow % 64 == 0), into the 9 tap columns of one
                  [splits][cout][9*c] slab set reduced by one dvie_wgrad_reduce. */
  int pad1;
} dvie_wgrad_desc;

int dvie_conv2d_wgrad(const dvie_wgrad_desc* d, void* stream);

/* Number of bias partial slabs dvie_conv2d_wgrad writes to d->bws. */
int dvie_wgrad_bias_slabs(const dvie_wgrad_desc* d);

/* Split count the library prefers for this weight gradient (0: no preference).  bf16
 * stride-1 1x1/3x3 convs with c and cout multiples of 64 run a halo-tile kernel that
 * assigns contiguous ranges of 64-pixel-wide output tiles to splits. */
int dvie_wgrad_splits_hint(const dvie_wgrad_desc* d);

/* Number of partial slabs ([slabs][cout][taps*c] fp32) dvie_conv2d_wgrad writes for d
 * (d->splits, or 4*d->splits for the halo kernel's 1x1 case); size `ws` and pass this as
 * dvie_wreduce_desc.splits. */
int dvie_wgrad_slabs(const dvie_wgrad_desc* d);

/*
 * dw[co][cmap[j]][kh][kw] (+)= sum_s part[s][co_off + co][t*c + j]  for every packed
 * position j in [0, c) whose source channel cmap[j] >= 0 (identity when cmap is NULL),
 * t = kh*kw_n + kw, writing an OIHW fp32 parameter gradient of cout_p x cin_p x kh_n x kw_n.
 * Rows co_off .. ws_rows-1 of the slabs are scanned (ws_rows*ws_k and co_off*ws_k multiples
 * of 4), rows co < cout_p written.  Threads walk the partial slabs in memory order
 * (16-byte coalesced), 8 split-lanes per column.  Also used for bias gradients
 * (kh_n = kw_n = 1, cin_p = 1, c = 1, ws_k = 1).
 */
typedef struct dvie_wreduce_desc {
  const float* ws;
  float* dw;
  const int* cmap;
  int splits, ws_rows, ws_k, co_off;
  int cout_p, cin_p, kh_n, kw_n;
  int c, beta;
} dvie_wreduce_desc;

int dvie_wgrad_reduce(const dvie_wreduce_desc* d, void* stream);

/*
 * Several slab reductions in ONE launch (replaces as many dvie_wgrad_reduce launches; the
 * engine batches the weight lane's reductions, each weight gradient of a batch writing its
 * own slab region).  descs: a HOST array of n descriptors, read at launch time, so the caller
 * may re-point their dw / beta between launches.  A flat grid: each descriptor owns a
 * contiguous block range.  Same results as n dvie_wgrad_reduce calls.
 */
int dvie_wgrad_reduce_multi(const dvie_wreduce_desc* descs, int n, void* stream);
typedef struct dvie_wreduce_multi_desc {
  const dvie_wreduce_desc* descs; /* host array */
  int n, pad;
} dvie_wreduce_multi_desc;

/* Bias gradient partials: part[s][co] = sum_{pix in split s} g[pix][co]. */
typedef struct dvie_colsum_desc {
  const void* g;
  float* ws;
  long long g_ld;
  long long rows;
  int c, splits, dtype, pad0;
} dvie_colsum_desc;

int dvie_colsum(const dvie_colsum_desc* d, void* stream);

/*
 * Weight packing: fp32 OIHW parameter -> packed GEMM operand rows (elem type dtype).
 * mode 0 (forward):   dst[r][t*c + j] = src[r][cmap[j]][kh(t)][kw(t)], r < cout_s
 * mode 1 (transpose): dst[r][t*c + j] = src[j][cmap[r]][kh(t)][kw(t)], j < cout_s
 * with kh(t) = kh0 + (t / tw)*dkh, kw(t) = kw0 + (t % tw)*dkw; entries whose source is
 * out of range (cmap < 0, r/j past the source extent, k >= taps*c) are zero.
 * `n` descriptors are processed by one launch (descs points to DEVICE memory) over a flat
 * grid of `blocks` workgroups: descriptor i owns blocks [blk0_i, blk0_i + nb_i), the blk0
 * increasing with i (the caller fills them; `blocks` is the sum), with nb = rows (mode 0,
 * kpad >= 64 and kpad % 4 == 0, cin_s*kh_s*kw_s <= 8192: one packed row per block),
 * ceil(rows / 8) * ceil(c / 64) (mode 1, the same kpad, kh_s*kw_s <= 16, c % 4 == 0: 8 rows x
 * 64 columns per block), else ceil(rows * kpad / 1024) (1024 elements per block).
 */
typedef struct dvie_pack_desc {
  const float* src;
  void* dst;
  const int* cmap; /* device int array or NULL (identity) */
  int rows, kpad, c, mode;
  int th, tw, kh0, kw0;
  int dkh, dkw, cout_s, cin_s;
  int kh_s, kw_s, dtype, blk0; /* blk0: first flat-grid block of this descriptor */
} dvie_pack_desc;

int dvie_pack_weights(const dvie_pack_desc* descs_dev, int n, int blocks, void* stream);

/* Number of flat-grid blocks dvie_pack_weights gives descriptor d (host memory): the blk0 of
 * the next descriptor is d->blk0 plus this, and `blocks` is the sum over all descriptors. */
int dvie_pack_blocks(const dvie_pack_desc* d);

/*
 * Pointwise NHWC family (4 channels per thread).  op selects:
 *  DVIE_EW_FUSE   y = act( sum_i up_i(src_i) ) — HighResolutionModule fuse sum
 *                 (nets/HRNet.py:212-225) and the final bilinear upsample into the
 *                 448-channel concat (nets/HRNet.py:576-582).  up_i is bilinear from
 *                 (src_h, src_w) to (h, w), identity when equal; align_corners=False, or
 *                 True when `align` is set (nn.Upsample of nets/UNet.py:70).
 *  DVIE_EW_UPT    y = up^T(src_0) — adjoint of the bilinear upsample (gather form,
 *                 deterministic, no atomics); src_0 is the fine grid (src_h x src_w);
 *                 `align` as for FUSE.
 *  DVIE_EW_POOL   y = avgpool2x2(src_0) (nets/vgg.py:9 AvgPool2d(2,2)).
 *  DVIE_EW_POOLT  y = adjoint of avgpool2x2 applied to src_0 (coarse grid).
 *  DVIE_EW_COPY   y = src_0 (same grid).
 *  DVIE_EW_L1SIGN y = scale * sign(src_0 - src_1) (VGG feature-L1 gradient, losses.py:178-179)
 *  DVIE_EW_NCHW   y = ext (fp32, arbitrary NCHW strides sn,sc,sh,sw; channels >= ext_c
 *                 read as zero), optionally (ext - mean[c]) / std[c]
 *                 (preprocess_norm, utils/net_utils.py:11-23).  With src1 set, channels
 *                 [sh1, ext_c) come from the fp32 tensor src1 (channel c - sh1, same
 *                 strides): two frames read in place instead of torch.cat
 *                 (runners/InterTrainer.py:373-374 of the reference).
 *  DVIE_EW_TONCHW ext (+)= channels [0, ext_c) of src_0 as fp32 with NCHW strides,
 *                 divided by std[c] when std is set (adjoint of the normalisation);
 *                 beta selects accumulate; the NHWC epilogue is not applied.  align != 0
 *                 clamps the value to [-scale, scale] first (fminf(fmaxf(v, -scale), scale):
 *                 the +-10 clamp of the two-stage nets' outputs, nets/InterRefineNet.py).
 *  DVIE_EW_MASK   y = src_0 * m or src_0 * (1 - m) (ext_c = 0 / 1), m = ext[n, 0, y, x]
 *                 (fp32, NCHW strides): the fg/bg split of nets/SepUNet.py:45-46 (its own
 *                 adjoint with respect to src_0).
 *  DVIE_EW_IM2COL y[n,y,x][t*ext_c + ch] = src_0[n, y + sh1 + ty*sh2, x + sw1 + tx*sw2][ch]
 *                 for tap t = ty*sw0 + tx of an sh0 x sw0 tap grid; zero outside the (h, w)
 *                 image and for t >= sh0*sw0 (ext_c % 8 == 0).  Lowers a stride-1 conv whose
 *                 input has few channels (the data gradient of HRNet's 3x3 448->3 / 448->20
 *                 heads) to a 1x1 GEMM over K = taps*ext_c instead of taps*64.
 *  DVIE_EW_LABELS y[n,y,x][k] = (lab[n,y,x] == k) for k < ext_c, 0 for ext_c <= k < c: the
 *                 one-hot of a uint8 label map, written in the plan dtype.  lab is read
 *                 through `ext` (reinterpreted as const uint8_t*) with ELEMENT strides sn, sh,
 *                 sw (sc unused).  A label >= ext_c (Cityscapes' 255 "ignore") gives an
 *                 all-zero row, as dvie_clip_prep defines it.  A plan input op: it takes no
 *                 epilogue operand (res / beta / act / dact must be unset).  The values equal
 *                 what DVIE_EW_NCHW writes from the fp32 one-hot, at 1 B read per pixel
 *                 instead of 4 * ext_c.
 * then the shared epilogue: v += res; v += y_old (beta); v = act(v); v *= act'(z); y = v.
 * Channels c % 4 == 0; all lds % 4 == 0.
 */
#define DVIE_EW_FUSE 0
#define DVIE_EW_UPT 1
#define DVIE_EW_POOL 2
#define DVIE_EW_POOLT 3
#define DVIE_EW_COPY 4
#define DVIE_EW_L1SIGN 5
#define DVIE_EW_NCHW 6
#define DVIE_EW_TONCHW 7
#define DVIE_EW_MASK 8
#define DVIE_EW_IM2COL 9
#define DVIE_EW_LABELS 10

typedef struct dvie_ew_desc {
  void* y;
  const void* src0;
  const void* src1;
  const void* src2;
  const void* res;
  const void* z;
  float* ext;
  const float* mean;
  const float* std;
  long long y_ld, src_ld0, src_ld1, src_ld2, res_ld, z_ld;
  long long sn, sc, sh, sw;
  int op, n, h, w;
  int c, nsrc, sh0, sw0;
  int sh1, sw1, sh2, sw2;
  int act, dact, beta, dtype;
  int ext_c, align;
  float alpha, scale;
} dvie_ew_desc;

int dvie_ew(const dvie_ew_desc* d, void* stream);

/*
 * Loss reductions on fp32 NCHW-strided (B, C, H, W) images (pred a, target b).
 * Every loss writes its partial sums to `partial` (double[nblocks]) and the final
 * scalar (fp32) to `out`, and — when `grad` is non-NULL — the gradient of `weight *
 * loss` with respect to a in NCHW-contiguous fp32 layout ([B][C][H][W]), overwritten
 * (beta=0) or accumulated (beta=1).
 *  L1   : mean|a-b|                                   nn.L1Loss (losses.py:224)
 *  GDL  : (mean|dx a - dx b| + mean|dy a - dy b|)/2   GDLLoss (losses.py:137-151)
 *  SSIM : 1 - mean ssim_map (11x11 gaussian, sigma 1.5, zero pad 5, C1=1e-4, C2=9e-4)
 *                                                      SSIM/_ssim (losses.py:18-48,63-87)
 *  MSE  : per-sample mean((a-b)^2) -> out[b] (PSNR, losses.py:103-116)
 *  CE   : mean_pix( logsumexp(a[:,.]) - a[label] ), label = argmax_c b[:, c]
 *         (nn.CrossEntropyLoss(a, argmax(b,1)), runners/InterTrainer.py:75,414)
 */
#define DVIE_LOSS_L1 0
#define DVIE_LOSS_GDL 1
#define DVIE_LOSS_SSIM 2
#define DVIE_LOSS_MSE 3
#define DVIE_LOSS_CE 4
#define DVIE_LOSS_L1NHWC 5 /* mean|a-b| over NHWC tensors of elem type dtype (VGG features) */
/* validation metrics (no gradient; `grad` must be NULL):
 *  COSNHWC    : weight * mean_pix( sum_c a.b / (|a| |b|) ) over (B, C=ch, H, W) tensors of
 *               elem type dtype, channel stride a_sc/b_sc (VGGCosineLoss, losses.py:182-207;
 *               NaN for an all-zero feature vector, as the reference's 0/0)
 *  IOU        : mean_pix( a == b ) of int64 label maps (B, H, W), strides a_sn/a_sh/a_sw
 *               (IoU, losses.py:122-131)
 *  ARGMAX_IOU : IOU of argmax_c a and argmax_c b, fp32 (B, C, H, W) scores (first maximum,
 *               as torch.argmax; InterTrainer.validate, runners/InterTrainer.py:615-624) */
#define DVIE_LOSS_COSNHWC 6
#define DVIE_LOSS_IOU 7
#define DVIE_LOSS_ARGMAX_IOU 8

/*
 * grad (L1, GDL, SSIM, CE): d(weight * loss)/d(a), NCHW-contiguous fp32; beta = 1 adds it
 * to what grad holds (several losses of one prediction write one gradient buffer).
 * out: the loss value times out_scale, taken as given (a weight-0 term reports 0; builders
 * set 1.0 for the plain value); out_acc = 1 adds it to *out instead of storing it (the five
 * VGG feature levels into one scalar).  weight scales the gradient only (COSNHWC: the value).
 */
typedef struct dvie_loss_desc {
  const void* a;
  const void* b;
  float* grad;
  float* out;
  double* partial;
  float* ws; /* SSIM gradient scratch: 3*B*C*H*W floats (dvie_loss_ws_floats) */
  long long a_sn, a_sc, a_sh, a_sw;
  long long b_sn, b_sc, b_sh, b_sw;
  int kind, bsz, ch, h;
  int w, beta, dtype, out_acc;
  float weight, out_scale;
} dvie_loss_desc;

int dvie_loss(const dvie_loss_desc* d, void* stream);

/* out[0] = sum of x[0 .. n-1] in index order, one workgroup (the training step's loss_all
 * from its weighted terms; replaces the Python sum at runners/InterTrainer.py:426-430 of
 * the reference) */
int dvie_sum_f32(const float* x, int n, float* out, void* stream);
size_t dvie_loss_partial_count(const dvie_loss_desc* d);
size_t dvie_loss_ws_floats(const dvie_loss_desc* d);

/*
 * Bilinear flow warp (FlowWrapper, utils/net_utils.py:89-114; F.grid_sample bilinear,
 * zeros padding, align_corners=True as in the pinned torch 1.0.1):
 *   gx = linspace(-1,1,W)[x] - flow[n,0,y,x],  gy = linspace(-1,1,H)[y] - flow[n,1,y,x]
 *   out[n,c,y,x] = bilinear(img[n,c], (gx+1)/2*(W-1), (gy+1)/2*(H-1))
 * fp32, NCHW contiguous.  Backward: dimg and dflow (both overwritten), given dout.  Three
 * launches: per sample its source position (ix, iy) into `ws` and dflow; per dimg pixel the
 * samples of a 3x3 window around c minus its displacement (the side chosen by the fractional
 * part) gathered as a plain store, plus the per-sample check that appends samples a corner's
 * window misses to a far list in `ws`; global atomics for the listed samples.  dimg = NULL
 * computes dflow only (ws may be NULL).  `ws` holds dvie_warp_ws_floats(d) floats.
 */
typedef struct dvie_warp_desc {
  const float* img;
  const float* flow;
  float* out;
  const float* dout;
  float* dimg;
  float* dflow;
  float* ws;
  int n, c, h, w;
  int align_corners, pad0;
} dvie_warp_desc;

int dvie_warp_fwd(const dvie_warp_desc* d, void* stream);
int dvie_warp_bwd(const dvie_warp_desc* d, void* stream);
size_t dvie_warp_ws_floats(const dvie_warp_desc* d);

/*
 * Fused Adamax step over a flat fp32 buffer (torch.optim.Adamax semantics,
 * runners/InterTrainer.py:79): m = lerp(m, g, 1-b1); u = max(u*b2, |g|+eps);
 * p -= clr * m / u with clr = lr / (1 - b1^step) (computed by the caller);
 * weight decay applied as g += wd*p first.
 */
int dvie_adamax(float* p, const float* g, float* m, float* u, long long n, float clr,
                float b1, float b2, float eps, float wd, void* stream);

/*
 * Graph-capturable variants (the step count lives on the device, so a captured step
 * replays with the right bias correction): dvie_step_inc adds 1 to *step; dvie_adamax_dev
 * computes clr = lr / (1 - b1^(*step)) on the device in double from the double lr / b1 a
 * host would use, then updates as dvie_adamax (elementwise math in float, as there).
 */
int dvie_step_inc(float* step, void* stream);
int dvie_adamax_dev(float* p, const float* g, float* m, float* u, long long n, double lr, double b1, double b2,
                    double eps, double wd, const float* step, void* stream);

/* scale a flat fp32 buffer in place (used for the 1/W gradient factor) */
int dvie_scale(float* p, long long n, float s, void* stream);

/*
 * Measurement only (bench.py): `blocks` workgroups of 4 waves, each wave issuing
 * 8 * iters back-to-back v_mfma_f32_32x32x16_bf16 on pseudo-random operands in registers
 * (32768 FLOP each); out[blocks * 256] receives per-lane sums.  Its rate is the dense bf16
 * MFMA ceiling at the clock the chip holds under that load on this box.
 */
int dvie_mfma_probe(float* out, int blocks, int iters, void* stream);

/*
 * Measurement only (bench.py): `blocks` workgroups of `threads` threads of an empty kernel --
 * the dispatch / ramp / drain floor of a launch of that shape (the warp forward's grid at
 * 256x512 is a ~7 us launch, where this floor is a large part).
 */
int dvie_launch_probe(int blocks, int threads, void* stream);

/*
 * BatchNorm2d over NHWC rows (rows = N*H*W pixels, c channels), fused with the following
 * activation (nets/FrameDisc.py:45-46, nets/VidDisc.py:45-50, nets/HRNet.py:726-789).
 * training = 1: batch statistics (biased variance for the normalisation; running_mean /
 * running_var, if non-NULL, updated with `momentum` and the unbiased variance, as
 * nn.BatchNorm2d.train()); training = 0: running statistics.
 *   forward : y = act(gamma * (x - mean) * invstd + beta)
 *   backward: g = dL/d(pre-activation output) (the engine applies act' upstream);
 *             dgamma (+)= sum g*xhat, dbeta (+)= sum g (accumulate selects +=);
 *             dx (+)= gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) (beta_dx selects +=).
 * partial: workspace of dvie_bn_partial_doubles(d) doubles = max(splits * 2 * c, 4 * c): the
 * forward and the backward statistics use it as [splits][2][c] (splits =
 * dvie_bn_partial_splits), and the backward then reuses its first 4 * c doubles as four
 * coefficient rows [4][c], which is the larger need when splits is 1.  stats: fp32 [8][c]
 * per-call state written by the forward and read by the backward.
 * Constraints: c % 4 == 0, c <= 1024, lds % 4 == 0.
 */
typedef struct dvie_bn_desc {
  const void* x;
  void* y;
  const void* g;
  void* dx;
  const float* gamma;
  const float* beta;
  float* dgamma;
  float* dbeta;
  float* running_mean;
  float* running_var;
  double* partial;
  float* stats;
  long long x_ld, y_ld, g_ld, dx_ld;
  long long rows;
  int c, splits, act, training;
  int dtype, accumulate, beta_dx, x_f32; /* x_f32: x is fp32 (y, g, dx have elem type dtype) */
  float alpha, eps, momentum, pad1;
} dvie_bn_desc;

int dvie_bn_fwd(const dvie_bn_desc* d, void* stream);
int dvie_bn_bwd(const dvie_bn_desc* d, void* stream);
int dvie_bn_partial_splits(const dvie_bn_desc* d);
size_t dvie_bn_partial_doubles(const dvie_bn_desc* d); /* reads rows and c */

/*
 * Discriminator head: AvgPool2d(pool) of an NHWC (n, h, w, c) map, then
 * view(-1, c).mean(1) over the NCHW-flat pooled tensor (nets/FrameDisc.py:66,74;
 * nets/VidDisc.py:77,83): out[r] = mean(pooled_nchw[r*c : (r+1)*c]), r < n*(h/pool)*(w/pool).
 * pooled: fp32 workspace of n*c*(h/pool)*(w/pool).  Backward: gx (+)= the adjoint applied
 * to gout (pixels past the floor(h/pool)*pool crop get 0).
 */
typedef struct dvie_head_desc {
  const void* x;
  void* gx;
  const float* gout;
  float* out;
  float* pooled;
  long long x_ld, gx_ld;
  int n, h, w, c;
  int pool, dtype, beta, pad0;
} dvie_head_desc;

int dvie_head_fwd(const dvie_head_desc* d, void* stream);
int dvie_head_bwd(const dvie_head_desc* d, void* stream);

/*
 * Channel softmax (F.softmax(seg, dim=1), nets/InterGANNet.py:40), fp32: x with NCHW
 * strides (sn, sc, sh, sw) in elements, y contiguous NCHW.  Backward (gy, y contiguous):
 * gx (+)= y * (gy - sum_c gy*y).
 */
typedef struct dvie_softmax_desc {
  const float* x;
  float* y;
  const float* gy;
  float* gx;
  long long sn, sc, sh, sw;
  int n, c, h, w;
  int beta, pad0;
} dvie_softmax_desc;

int dvie_softmax_fwd(const dvie_softmax_desc* d, void* stream);
int dvie_softmax_bwd(const dvie_softmax_desc* d, void* stream);

/*
 * Fused Adam over a flat fp32 buffer, torch 1.0.1 update form (the discriminator
 * optimizers, runners/InterGANTrainer.py:110-112): m = b1*m + (1-b1)*g;
 * v = b2*v + (1-b2)*g^2; p -= step_size * m / (sqrt(v) + eps) with
 * step_size = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller; weight decay g += wd*p first.
 */
int dvie_adam(float* p, const float* g, float* m, float* v, long long n, float step_size, float b1, float b2,
              float eps, float wd, void* stream);
/* the same with step_size computed on the device from lr and *step (graph-captured steps) */
int dvie_adam_dev(float* p, const float* g, float* m, float* v, long long n, double lr, double b1, double b2,
                  double eps, double wd, const float* step, void* stream);

/*
 * SpectralNorm (reference nets/SpectralNorm.py:10-68), fp32, one workgroup per layer.
 * W_bar is the (h, width) row-major view of the OIHW weight (width = cin*kh*kw).
 * Forward (SpectralNorm._update_u_v, l.23-35), `power_iterations` times:
 *   v = l2normalize(W_bar^T u); u = l2normalize(W_bar v)      (l2normalize: x / (|x| + 1e-12))
 * then sigma = u . (W_bar v) and w_eff = W_bar / sigma.  u and v are updated in place; the
 * values used ([sigma, u(h), v(width)]) are saved at state + state_off for the backward.
 * Backward (autograd of `w / sigma` with sigma = u.dot(W_bar.mv(v))),
 * g_sigma = -sum(g_eff * W_bar) / sigma^2:
 *   g_bar (+)= g_eff / sigma + g_sigma * u v^T
 *   g_u   (+)= g_sigma * (W_bar v),  g_v (+)= g_sigma * (W_bar^T u)   (only if non-null: u and v
 *   become trainable in the reference once set_net_grad(True) ran, nets/InterGANNet.py:81)
 * beta = 1 accumulates into g_bar / g_u / g_v.  u, v here are the values the forward saved.
 * Replaces: SpectralNorm.forward's _update_u_v (l.66-68) and its autograd backward.
 * `n` layers (host array, any count), one workgroup each.
 */
typedef struct dvie_sn_layer {
  const float* w_bar;
  float* u;
  float* v;
  float* w_eff;
  const float* g_eff;
  float* g_bar;
  float* g_u;
  float* g_v;
  long long state_off;
  int h, width, power_iterations, beta;
} dvie_sn_layer;

int dvie_sn_fwd(const dvie_sn_layer* layers, int n, float* state, void* stream);
int dvie_sn_bwd(const dvie_sn_layer* layers, int n, const float* state, void* stream);

/*
 * VAEHRNet reparameterisation (reference nets/HRNet.py:960-966), fp32, n elements:
 *   forward  z = eps * exp(0.5 * logvar) + mu
 *   backward gmu (+)= gz; glogvar (+)= gz * eps * 0.5 * exp(0.5 * logvar)   (beta: accumulate)
 * eps is the caller's standard-normal draw (std.new(std.size()).normal_()).
 */
int dvie_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, long long n, void* stream);
int dvie_reparam_bwd(const float* logvar, const float* eps, const float* gz, float* gmu, float* glogvar, long long n,
                     int beta, void* stream);

/*
 * Local-window attention ops of the second-stage refinement nets (MSResAttnRefine,
 * nets/refine_nets.py:138-399; corrmap l.253-287, weight_neighbors_by_probmap l.313-323,
 * weight_neighbors_by_low_probmap l.289-311).  NHWC tensors of elem type dtype on an
 * (n, h, w) grid; window entry k of a (wh x ww) window (both odd) is the neighbour at
 * offset (k / ww - wh/2, k % ww - ww/2); the window weights of map m occupy channels
 * [m*K, (m+1)*K), K = wh*ww; out-of-image neighbours read zero.
 *   L2NORM      y[p, :c] = a[p, :c] / |a[p, :c]|                          (x / x.norm(dim=1))
 *   L2NORM_BWD  y = (a - b0 <b0, a>) / |b1|      a = dL/dxn, b0 = xn, b1 = x
 *   CORR        y[p, m*K + k] = <a[p, :c], b_m[p + o_k, :c]>, m < nhalf    (b_0 = b0, b_1 = b1;
 *               a NULL map's entries are written as 0)
 *   GATHER      y[p, :c] = sum_m sum_k a[p, (half0+m)*K + k] * b_m[p + o_k, :c]   (m < 1 + !!b1)
 *   GATHER_T    y[q, :c] = sum_k a[q - o_k, half0*K + k] * b0[q - o_k, :c]  (adjoint in b)
 *   SOFTMAX     y[p, :J] = softmax(a[p, :J]), J = nhalf*K
 *   SOFTMAX_BWD y = b0 * (a - <b0, a>)           a = dL/dprob, b0 = prob
 *   WNORM       per map: y = a / sum_k a
 *   WNORM_BWD   per map: y = (a - <a, b0>) / sum_k b1     a = dL/dWn, b0 = Wn, b1 = W
 *   POOL        y[p, :c] = mean of a over the in-image part of the centred (wh x ww) window
 *               (F.avg_pool2d(k=(wh,ww), stride 1, pad (wh/2, ww/2), count_include_pad=False))
 *   POOL_T      adjoint of POOL
 * Then the common epilogue: v += res; v += y_old (beta); v = act(v); v *= act'(z) (dact).
 * Vector ops (GATHER*, POOL*) need c, every ld % 4 == 0.
 */
#define DVIE_ATTN_L2NORM 0
#define DVIE_ATTN_L2NORM_BWD 1
#define DVIE_ATTN_CORR 2
#define DVIE_ATTN_GATHER 3
#define DVIE_ATTN_GATHER_T 4
#define DVIE_ATTN_SOFTMAX 5
#define DVIE_ATTN_SOFTMAX_BWD 6
#define DVIE_ATTN_WNORM 7
#define DVIE_ATTN_WNORM_BWD 8
#define DVIE_ATTN_POOL 9
#define DVIE_ATTN_POOL_T 10

typedef struct dvie_attn_desc {
  const void* a;
  const void* b0;
  const void* b1;
  void* y;
  const void* res;
  const void* z;
  long long a_ld, b_ld, y_ld, res_ld, z_ld;
  int op, n, h, w;
  int c, wh, ww, nhalf;
  int half0, act, dact, beta;
  int dtype, pad0;
  float alpha, pad1;
} dvie_attn_desc;

int dvie_attn(const dvie_attn_desc* d, void* stream);

/*
 * Fused backward of a narrow-output 3x3 stride-1 conv over a LeakyReLU-activated map: the
 * HRNet output heads rgb_layer[2] / seg_layer[2] (448 -> 3 / 448 -> 20, reference
 * nets/HRNet.py:410-442, 584-588), whose backward is nn.Conv2d backward-data + the preceding
 * LeakyReLU's derivative + nn.Conv2d backward-weight.  One pass over the hidden map h:
 *   dh[p][ci]  = act'(h[p][ci]) * sum_{t, o} wd[ci][t * cout + o] * g[p + (dy0 + i_t, dx0 + j_t)][o]
 *   ws[s][o][(8 - t) * c + ci] = sum_{p in split s} g[p + (dy0 + i_t, dx0 + j_t)][o] * h[p][ci]
 * (t = 3 i_t + j_t the data-gradient tap; 8 - t the forward tap of the same weight), so
 * h is read once and the dh map written once; the weight-gradient partial slabs have the
 * dvie_conv2d_wgrad layout (reduce them with dvie_wgrad_reduce, ws_k = 9 * c).
 * g: (n, h, w, cout) bf16 NHWC output gradient (cout 8 or 24, padded channels zero);
 * h: the conv input (bf16 NHWC, c channels, a multiple of 64); wd: the packed data-gradient
 * weights [c][kpad] (dvie_pack_weights mode 1: wd[ci][t * cout + o] = w[o][ci][2 - i_t][2 - j_t]);
 * dh: bf16 NHWC, written (not accumulated); dact: DVIE_ACT_LRELU (alpha) or DVIE_ACT_NONE.
 * splits: weight-gradient slabs (grid = (c / 64) * splits workgroups); bf16 only.
 */
typedef struct dvie_head3_bwd_desc {
  const void* g;
  const void* h;
  const void* wd;
  void* dh;
  float* ws;
  long long g_ld, h_ld, dh_ld;
  int n, hgt, wid, c;
  int cout, kpad, dy0, dx0;
  int splits, dact;
  float alpha, pad0;
} dvie_head3_bwd_desc;

int dvie_head3_bwd(const dvie_head3_bwd_desc* d, void* stream);

/*
 * Fused forward of HRNet's segmentation encoder (reference nets/HRNet.py:358-364, applied at
 * l.533-537): e1 = ELU(conv3x3(in) + b0) (24 -> 32 channels; the 20 classes padded to 24),
 * e2 = ELU(conv3x3(e1) + b2) (32 -> 32), out = conv3x3(e2) + b4 (32 -> 8: the 4 encoder
 * channels + 4 zero-weight pads), stride 1, zero padding, bf16 NHWC.  e1 and e2 are written
 * (the backward reads them); out may be a channel slice of a wider buffer (out_ld).  w0 / w2 /
 * w4: the forward-packed weights [cout][kpad] (dvie_pack_weights mode 0: w[co][t * cin + ci]),
 * b0 / b2 / b4: fp32 biases (32, 32, 8).
 */
typedef struct dvie_segenc_desc {
  const void* in;
  void* e1;
  void* e2;
  void* out;
  const void* w0;
  const void* w2;
  const void* w4;
  const float* b0;
  const float* b2;
  const float* b4;
  long long in_ld, e1_ld, e2_ld, out_ld;
  int n, h, w, kpad0;
  int kpad2, kpad4;
} dvie_segenc_desc;

int dvie_segenc_fwd(const dvie_segenc_desc* d, void* stream);

/*
 * Fused backward of the same encoder (the encoder input needs no gradient): from dout (the
 * gradient of the 8-channel output, bf16 NHWC, e.g. a slice of the stem buffer's gradient)
 * and the forward's e2 / e1 / in, the weight- and bias-gradient partial slabs of the three
 * convs; d_e2 = ELU'(e2) conv4^T(dout) and d_e1 = ELU'(e1) conv2^T(d_e2) stay on chip.
 * w4d / w2d: the packed data-gradient weights of conv4 [32][kpad4 >= 80] and conv2
 * [32][kpad2 >= 288] (dvie_pack_weights mode 1).  Slabs (one per workgroup, `slabs` of them):
 * dw4 [slabs][8][288], dw2 [slabs][32][288], dw0 [slabs][32][216] (dvie_conv2d_wgrad layout,
 * reduce with dvie_wgrad_reduce), db4 [slabs][8], db2 / db0 [slabs][32].
 */
typedef struct dvie_segenc_bwd_desc {
  const void* dout;
  const void* e2;
  const void* e1;
  const void* in;
  const void* w4d;
  const void* w2d;
  float* dw4;
  float* dw2;
  float* dw0;
  float* db4;
  float* db2;
  float* db0;
  long long dout_ld, e2_ld, e1_ld, in_ld;
  int n, h, w, kpad4;
  int kpad2, slabs;
} dvie_segenc_bwd_desc;

int dvie_segenc_bwd(const dvie_segenc_bwd_desc* d, void* stream);

/*
 * Op-list executor: runs n descriptors in order with a single host call (the per-step
 * forward and backward plans of the HRNet / VGG executors).  dvie_op.lane picks the stream:
 *   0     the caller's stream;
 *   1     the weight lane (a library side stream of the current device and host thread):
 *         work off the critical path (weight gradients and their reductions).  A run of
 *         lane-1 ops first waits for everything issued so far on the caller's stream (the
 *         lane-0 ops that produced its inputs), so lane-1 ops read only finished data.
 * The call ends with the caller's stream waiting for the side stream if it was used, so the
 * call as a whole is ordered on the caller's stream and capturable (the wait is a graph
 * edge).  DVIE_OP_LANES=0 runs every op on the caller's stream.
 */
#define DVIE_OP_CONV 1
#define DVIE_OP_WGRAD 2
#define DVIE_OP_WREDUCE 3
#define DVIE_OP_COLSUM 4
#define DVIE_OP_EW 5
#define DVIE_OP_LOSS 6
#define DVIE_OP_PACK 7
#define DVIE_OP_BN_FWD 8
#define DVIE_OP_BN_BWD 9
#define DVIE_OP_HEAD_FWD 10
#define DVIE_OP_HEAD_BWD 11
#define DVIE_OP_ATTN 12
#define DVIE_OP_HEAD3_BWD 13
#define DVIE_OP_SEGENC_FWD 14
#define DVIE_OP_SEGENC_BWD 15
#define DVIE_OP_WREDUCE_MULTI 16
#define DVIE_OP_COSFEAT 17

/*
 * dvie_cosfeat: per-image cosine similarity of VGG feature maps, the reduction behind the
 * per-frame perceptual score (synth.PerceptualScorer; Graph.cosfeat in the plan engine).
 *
 * feat: NHWC feature maps (2n, h, w, c) of element type dtype with channel pitch ld (elements):
 * image i (a prediction) is compared with image n + i (its original).  A score is
 *
 *   out[i] = (1 / n_taps) * sum over taps t of  mean over the tap's pixels of
 *              dot(a, b) / (sqrtf(|a|^2) * sqrtf(|b|^2))          a, b the pixel's c channels
 *
 * with dot, |a|^2, |b|^2 summed in fp32 (DVIE_LOSS_COSNHWC's expression), the cosine formed in
 * fp32 and every sum over pixels, blocks and taps in float64.  A pixel whose vector is all zero
 * on either side is 0/0 = NaN and makes out[i] NaN, and no other image's value.
 *
 * mode 0 (one call per tap, after the tap is written): every block of tap `tap` writes its float64
 *   partial to ws[(tap * n + i) * ws_blocks + block]; a block covers pixels of ONE image.
 *   dvie_cosfeat_blocks(d) (from h, w, c, dtype) is the tap's block count per image, 0 for sizes
 *   the kernel does not take: c must be a power-of-two number of 16-byte vectors (8 bf16 or 4
 *   fp32 channels: 64, 128, 256, 512 ...), h * w < 2^30.  feat 16-byte aligned, ld >= c,
 *   ld * sizeof(element) % 16 == 0: the loads are 16-byte vectors along the channels.
 * mode 1 (once, after every tap): one block per image sums tap t's blocks[t] partials in index
 *   order through a fixed tree, divides by px[t] (the tap's h * w), averages the n_taps taps and
 *   writes out[i].  No atomics anywhere: two runs give the same bits.
 * ws: n_taps * n * ws_blocks doubles, 8-byte aligned, ws_blocks >= every tap's block count; the
 * entries read are all written by the mode-0 calls.  n <= 32767, n_taps <= DVIE_COSFEAT_MAX_TAPS.
 */
#define DVIE_COSFEAT_MAX_TAPS 8

typedef struct dvie_cosfeat_desc {
  const void* feat; /* mode 0 */
  double* ws;
  double* out; /* mode 1: n values */
  long long ld;
  int mode, dtype, n, h, w, c, tap, n_taps, ws_blocks, pad0;
  int blocks[DVIE_COSFEAT_MAX_TAPS]; /* mode 1: per tap, its blocks per image ... */
  int px[DVIE_COSFEAT_MAX_TAPS];     /* ... and its pixels per image */
} dvie_cosfeat_desc;

int dvie_cosfeat_blocks(const dvie_cosfeat_desc* d);
int dvie_cosfeat(const dvie_cosfeat_desc* d, void* stream);

typedef struct dvie_pack_list {
  const dvie_pack_desc* descs_dev;
  int n, blocks; /* dvie_pack_weights arguments */
} dvie_pack_list;

typedef struct dvie_op {
  int kind;
  int lane; /* 0: caller's stream, 1: weight lane (see above) */
  union {
    dvie_conv_desc conv;
    dvie_wgrad_desc wgrad;
    dvie_wreduce_desc wreduce;
    dvie_colsum_desc colsum;
    dvie_ew_desc ew;
    dvie_loss_desc loss;
    dvie_pack_list pack;
    dvie_bn_desc bn;
    dvie_head_desc head;
    dvie_attn_desc attn;
    dvie_head3_bwd_desc head3;
    dvie_segenc_desc segenc;
    dvie_segenc_bwd_desc segenc_bwd;
    dvie_wreduce_multi_desc wreduce_multi;
    dvie_cosfeat_desc cosfeat;
  } u;
} dvie_op;

/*
 * Cityscapes clip preparation on the device (reference folder.py:225-247 train branch and
 * l.248-261 val branch; crop parameters folder.py:125-149, flip l.211).  Replaces the
 * DataLoader worker's PIL flip / crop, to_tensor, normalize((.5,.5,.5),(.5,.5,.5)) and
 * np.eye(20)[seg] one-hot.  For clip b (dataset clip idx[b]) and frame t with
 * params[(b*T+t)*3 + {0,1,2}] = {flip, h1, w1}:
 *   src_x = flip ? W0-1-(w1+x) : w1+x,  src_y = h1+y      (flip the full frame, then crop)
 *   frames[t][b][c][y][x] = (img[idx[b]][t][src_y][src_x][c] / 255 - 0.5) / 0.5   (fp32)
 *   segs[t][b][k][y][x]   = (seg[idx[b]][t][src_y][src_x] == k)                      (fp32)
 * img: uint8 (N, T, H0, W0, 3) RGB as decoded, seg: uint8 (N, T, H0, W0) class ids (NULL:
 * no segs), both HBM-resident.  A label >= n_classes (np.eye raises IndexError there)
 * gives an all-zero one-hot and is counted into *bad (optional, accumulated).  idx = NULL
 * means clip b = b.  Every read must stay inside the frame: h1 + hc <= h0, w1 + wc <= w0
 * (the caller's crop generator guarantees it; not re-checked per pixel).
 */
typedef struct dvie_clip_desc {
  const uint8_t* img;
  const uint8_t* seg;
  const int* idx;
  const int* params;
  float* frames;
  float* segs;
  int* bad;
  int b, t, h0, w0, hc, wc, n_classes, pad0;
} dvie_clip_desc;

int dvie_clip_prep(const dvie_clip_desc* d, void* stream);

/*
 * Device-resident video synthesis (synth.py VideoSynthesizer): the two pointwise ends of an
 * inference forward, uint8 frames in and uint8 frames / label maps out.
 *
 * dvie_synth_load: uint8 RGB frames (npix, 3) -> fp32 (npix, out_ld): channels 0-2 =
 *   (u8 / 255 - 0.5) / 0.5 (the expression of dvie_clip_prep, bit for bit), channels
 *   3 .. out_ld-1 = 0.  out_ld = 8 gives the shape and strides of the HRNet plan's external
 *   `rgb` output, so input frames and predictions feed the next forward as equal-stride
 *   channel views.  out_ld % 4 == 0, out 16-byte aligned.
 *
 * dvie_synth_finish: the fp32 outputs of a forward -> what a viewer wants.
 *   frame[p][c] = rintf(fminf(fmaxf(rgb[p*rgb_ld + c], -1), 1) * 127.5f + 127.5f), c < 3, with
 *     the multiply and the add rounded separately (no fma) and round-half-to-even: the
 *     values of eager (x.clamp(-1, 1) * 127.5 + 127.5).round().
 *   label[p] = the smallest index among the maxima of seg[p*seg_ld + 0 .. n_classes-1]
 *     (ascending scan, strict >: torch.argmax / np.argmax on finite inputs).
 *   Either output may be NULL (rgb / seg is then not read and may be NULL too).  Padding
 *   channels (rgb 3 .. rgb_ld-1, seg n_classes .. seg_ld-1) never reach a result.  Inputs are
 *   finite; NaN handling is not part of the contract.  Leading dimensions % 4 == 0, inputs
 *   16-byte aligned, n_classes <= min(seg_ld, 256).
 */
typedef struct dvie_synth_load_desc {
  const uint8_t* frames;
  float* out;
  long long npix;
  int out_ld, pad0;
} dvie_synth_load_desc;

typedef struct dvie_synth_finish_desc {
  const float* rgb;
  const float* seg;
  uint8_t* frame;
  uint8_t* label;
  long long npix;
  int rgb_ld, seg_ld, n_classes, pad0;
} dvie_synth_finish_desc;

int dvie_synth_load(const dvie_synth_load_desc* d, void* stream);
int dvie_synth_finish(const dvie_synth_finish_desc* d, void* stream);

/*
 * Frames of any size on a padded canvas (VideoSynthesizer(pad="replicate")).  The nets need
 * H and W to be multiples of their coarsest stride; a frame (h, w) sits at the top-left of a
 * canvas (hp, wp) >= (h, w) that the forwards run on, and only the two pointwise ends know the
 * difference.
 *
 * dvie_synth_load_pad: uint8 frames (n, h, w, 3) and, optionally, uint8 label maps (n, h, w)
 *   -> the fp32 canvas out (n, hp, wp, out_ld) and the uint8 label canvas label_out
 *   (n, hp, wp), one launch.  Canvas pixel (y, x) reads source pixel (min(y, h-1), min(x, w-1)):
 *   rows h..hp-1 and columns w..wp-1 repeat the last row and column (a label byte is repeated
 *   whatever its value).  Channels 0-2 are dvie_synth_load's expression, bit for bit, channels
 *   3 .. out_ld-1 are 0.  labels and label_out: both or neither.  out_ld % 4 == 0 (>= 4), out
 *   16-byte aligned; no alignment of the uint8 tensors is assumed.
 *
 * dvie_synth_finish_crop: the fp32 outputs of a forward over the canvas, rgb (n, hp, wp, rgb_ld)
 *   and seg (n, hp, wp, seg_ld) -> the cropped uint8 frame (n, h, w, 3) and label (n, h, w),
 *   both contiguous, of any byte alignment, and, when label_canvas is not NULL, the argmax of
 *   EVERY canvas pixel in label_canvas (n, hp, wp) (what a later forward reads as this frame's
 *   label map).  Quantisation and argmax are dvie_synth_finish's, expression for expression.
 *   rgb of the pad region never reaches a result, and with label_canvas == NULL neither do the
 *   pad region's logits (they are not read).  wp % 4 == 0; otherwise dvie_synth_finish's rules.
 */
typedef struct dvie_synth_load_pad_desc {
  const uint8_t* frames;
  const uint8_t* labels;
  float* out;
  uint8_t* label_out;
  int n, h, w, hp, wp, out_ld;
} dvie_synth_load_pad_desc;

typedef struct dvie_synth_finish_crop_desc {
  const float* rgb;
  const float* seg;
  uint8_t* frame;
  uint8_t* label;
  uint8_t* label_canvas;
  int n, h, w, hp, wp;
  int rgb_ld, seg_ld, n_classes;
  int pad0;
} dvie_synth_finish_crop_desc;

int dvie_synth_load_pad(const dvie_synth_load_pad_desc* d, void* stream);
int dvie_synth_finish_crop(const dvie_synth_finish_crop_desc* d, void* stream);

/*
 * dvie_synth_bridge: the hand-off between two plans of a two-stage inference forward (coarse
 * HRNet -> SRNRefine -> MSResAttnRefine).  Per pixel it reads an fp32 image (3 channels at
 * rgb + p*rgb_ld) and the 20 fp32 coarse segmentation logits (seg + p*seg_ld) and writes one
 * contiguous channel span of the destination plan's NHWC input buffer, in that plan's dtype
 * (DVIE_F32, or DVIE_BF16 rounded to nearest even):
 *
 *   dst[p*dst_ld + ...] = [ n_rgb x (clamp(rgb) 3, zeros rgb_w - 3) | softmax(seg) 20, zeros seg_w - 20 ]
 *
 *   SRNRefine `in_full` [0, 40) of 56: n_rgb 2, rgb_w 8, seg_w 24;
 *   MSResAttnRefine `in_x` (24):       n_rgb 1, rgb_w 4, seg_w 20.
 *
 * clamp(v) = fminf(fmaxf(v, -1), 1).  The softmax is dvie_softmax_fwd's expression: a running
 * fmaxf over the channels in order, s += expf(x - m) in order, expf(x - m) * (1 / s) -- the
 * same bits.  Padding channels inside the span are WRITTEN as zeros (an arena buffer holds
 * whatever ran before); channels outside the span are not touched.
 * n_rgb in {1, 2}, rgb_w in {4, 8}, seg_w in {20, 24}; the span n_rgb*rgb_w + seg_w <= dst_ld
 * and a whole number of 16-byte vectors in the destination dtype; dst, rgb, seg 16-byte
 * aligned, rgb_ld % 4 == 0 (>= 4), seg_ld % 4 == 0 (>= 20), dst_ld * sizeof(element) % 16 == 0.
 */
typedef struct dvie_synth_bridge_desc {
  const float* rgb;
  const float* seg;
  void* dst;
  long long npix;
  int rgb_ld, seg_ld, dst_ld, dtype;
  int n_rgb, rgb_w, seg_w, pad0;
} dvie_synth_bridge_desc;

int dvie_synth_bridge(const dvie_synth_bridge_desc* d, void* stream);

/*
 * dvie_synth_score: per-frame quality of synthesised uint8 frames / label maps against the
 * frames that were really there (synth.frame_scores, VideoSynthesizer.score_interpolation /
 * score_extrapolation).  One fused pass over the 8 B per pixel of two RGB frames and two label
 * maps replaces, on the 8-bit data, the reference's losses.py:18-48 and 63-87 (gaussian,
 * create_window, _ssim, SSIM), 103-116 (PSNR: the squared error it needs) and 122-131 (IoU).
 *
 * Frames: N = n0 * n1 frame pairs, frame (i0, i1) of a tensor at base + i0*s0 + i1*s1 BYTES
 * (strides may be anything, a transposed (B, S) view of slot-major storage included); a frame is
 * a contiguous h*w*3 block of uint8 RGB, a label map a contiguous h*w block of uint8.  No
 * alignment of frame bases or rows is assumed.  pred_label / gt_label: both or neither.
 * Outputs, indexed f = i0*n1 + i1, all written by the call (nothing is accumulated into):
 *   sse[f]    int64   sum over the h*w*3 bytes of (pred - gt)^2, exact.  Width: a thread sums at
 *                     most 32 squares <= 65025 and a block 192 such threads (< 4.0e8) in
 *                     uint32; the per-frame sum over blocks is int64 (4096x8192: 6.6e12).
 *   ssim[f]   float64 mean over pixels and the 3 channels of the reference's SSIM map of x/255:
 *                     11-tap gaussian (sigma 1.5, normalised in float64), zero padding (samples
 *                     outside the image are 0, the window is not renormalised), C1 = 0.01^2,
 *                     C2 = 0.03^2.  Evaluated separably in float64 on the byte values with the
 *                     constants scaled by 255^2.
 *   agree[f]  int64   pixels with pred_label == gt_label (bytes as they are): losses.py IoU,
 *                     a pixel accuracy, times h*w.
 *   valid[f]  int64   pixels with gt_label < n_classes.
 *   inter[f][c], uni[f][c] (c < n_classes, int64): over valid pixels, pred == c && gt == c and
 *                     pred == c || gt == c.  A pred label >= n_classes matches no class.
 * Without label maps only sse and ssim are written (the other four may be NULL).
 * Bitwise reproducible: per-block partials (SSIM float64, counts integer) in the workspace,
 * summed in a fixed order by one finalize launch; no float atomics; no intermediate image.
 * ws: dvie_synth_score_ws_bytes(d) bytes, 8-byte aligned, fully overwritten (0 bytes for a
 * descriptor whose sizes are invalid).  sse .. uni 8-byte aligned.  h, w >= 1, 1 <= n_classes
 * <= 32, n0, n1 >= 1, n0 * n1 <= 65535.
 */
typedef struct dvie_synth_score_desc {
  const uint8_t* pred;
  const uint8_t* gt;
  const uint8_t* pred_label;
  const uint8_t* gt_label;
  long long* sse;
  double* ssim;
  long long* agree;
  long long* valid;
  long long* inter;
  long long* uni;
  void* ws;
  long long pred_s0, pred_s1, gt_s0, gt_s1;                         /* byte strides of (i0, i1) */
  long long pred_label_s0, pred_label_s1, gt_label_s0, gt_label_s1;
  int n0, n1, h, w, n_classes, pad0;
} dvie_synth_score_desc;

size_t dvie_synth_score_ws_bytes(const dvie_synth_score_desc* d);
int dvie_synth_score(const dvie_synth_score_desc* d, void* stream);

/*
 * dvie_synth_vgg_load: uint8 frame pairs -> the input buffer of the VGG19 scoring plan
 * (synth.PerceptualScorer).  Frames are addressed as dvie_synth_score addresses them: N = n0 * n1
 * pairs, frame (i0, i1) at base + i0*s0 + i1*s1 BYTES, a frame a contiguous h*w*3 block of uint8
 * RGB, no alignment assumed.  Only the top-left region (h16, w16) <= (h, w) of every frame is
 * read, in place through the row pitch 3 * w (the plan's 2x2 poolings need multiples of 16:
 * synth.vgg_region).  out: (2N, h16, w16, 8) contiguous, element type dtype, 16-byte aligned,
 * images [pred_0 .. pred_{N-1} | gt_0 .. gt_{N-1}] (img0 = 0, n_out = N).  A call may also fill a
 * part of a larger batch: with n_out > N the buffer holds 2 * n_out images and this call's pair j
 * goes to images img0 + j and n_out + img0 + j (0 <= img0, img0 + N <= n_out).
 *
 *   out[img][y][x][c] = lut[c * 256 + byte]   c < 3
 *                     = 0                      c = 3 .. 7 (written every time)
 *
 * lut: 3 x 256 elements of dtype on the device; the host computes (v / 255 - mean_c) / std_c in
 * float64, rounds it once to fp32 and, for DVIE_BF16, that fp32 once more to bf16 (nearest even),
 * so the device divides and rounds nothing and the result is defined bit for bit.
 * n0 * n1 <= 32767, h16 * w16 < 2^31 - 256.
 */
typedef struct dvie_synth_vgg_load_desc {
  const uint8_t* pred;
  const uint8_t* gt;
  void* out;
  const void* lut;
  long long pred_s0, pred_s1, gt_s0, gt_s1; /* byte strides of (i0, i1) */
  int n0, n1, h, w, h16, w16, dtype;
  int img0, n_out, pad0; /* pair j goes to images img0 + j and n_out + img0 + j of out (2 * n_out images) */
} dvie_synth_vgg_load_desc;

int dvie_synth_vgg_load(const dvie_synth_vgg_load_desc* d, void* stream);

/*
 * dvie_synth_msssim: per-frame multi-scale SSIM (Wang, Simoncelli and Bovik, 2003) of uint8 frames
 * against the originals (synth.frame_msssim).  Frames are addressed as dvie_synth_score addresses
 * them: N = n0 * n1 pairs, frame (i0, i1) at base + i0*s0 + i1*s1 BYTES, a frame a contiguous
 * h*w*3 block of uint8 RGB, no alignment assumed.  K = scales, 1 <= K <= 5.
 *
 * Pyramid: level s (0 <= s < K) has size (h >> s, w >> s); its pixel (i, j, c) is the mean of the
 *   2^s x 2^s block of level 0 whose top-left is (i << s, j << s).  Trailing rows and columns that
 *   do not fill a block are dropped (s applications of a 2x2 average pooling, in exact
 *   arithmetic).  A level is held as the uint16 block SUM (<= 255 * 4^4 = 65280), exactly.
 * Per level: the window and border rule of dvie_synth_score -- 11-tap gaussian, sigma 1.5,
 *   normalised in float64, separable, samples outside the level's image 0, all arithmetic
 *   float64 -- on the sums, with C1 = (0.01 * 255 * 4^s)^2, C2 = (0.03 * 255 * 4^s)^2 (a power-of-
 *   two scaling of working on the means: the same bits):
 *     cs = (2*s12 + C2) / (s1 + s2 + C2)        l = (2*mu1*mu2 + C1) / (mu1^2 + mu2^2 + C1)
 *   parts[f][s] = mean over the level's pixels and the 3 channels of cs (s < K-1), of l * cs
 *   (s = K-1).
 * msssim[f] = prod_s max(parts[f][s], 0) ^ w_s, w the first K of (0.0448, 0.2856, 0.3001, 0.2363,
 *   0.1333) divided by their sum (float64 pow).  With K = 1 this is dvie_synth_score's ssim.
 * Size rule: min(h, w) >> (K - 1) >= 11 (the coarsest level holds a whole window).
 *
 * Launches: a pyramid launch (K >= 2; integer arithmetic only, both frames' bytes read once, levels
 * 1 .. K-1 written to ws), one level-pass launch whose grid covers all K levels, a finalize launch.
 * Bitwise reproducible: float64 block partials in ws, summed in a fixed order; no float atomics;
 * no host synchronisation.
 * ws: dvie_synth_msssim_ws_bytes(d) bytes (0 for a descriptor whose sizes are invalid), 8-byte
 * aligned.  msssim (N float64) and parts (N x scales float64) 8-byte aligned, written by the call.
 * n0, n1 >= 1, n0 * n1 <= 65535, h, w <= 2^19.
 */
typedef struct dvie_synth_msssim_desc {
  const uint8_t* pred;
  const uint8_t* gt;
  double* msssim;
  double* parts;
  void* ws;
  long long pred_s0, pred_s1, gt_s0, gt_s1; /* byte strides of (i0, i1) */
  int n0, n1, h, w, scales, pad0;
} dvie_synth_msssim_desc;

size_t dvie_synth_msssim_ws_bytes(const dvie_synth_msssim_desc* d);
int dvie_synth_msssim(const dvie_synth_msssim_desc* d, void* stream);

/*
 * dvie_synth_yuv2rgb / dvie_synth_rgb2yuv: 8-bit planar Y'CbCr frames, packed as a YUV4MPEG2 file
 * holds them, <-> uint8 RGB frames (synth.yuv_to_rgb / rgb_to_yuv; DESIGN.md "Streaming and Y4M").
 * One launch takes all n frames.  Integer arithmetic only, so that every implementation agrees to
 * the byte; `>>` is the arithmetic shift, clip is to [0, 255].
 *
 * Packed frame f starts at yuv + f*yuv_stride BYTES: the Y plane (h x w), then U and V.  layout
 * DVIE_YUV_420: U and V are (ch x cw) = ((h+1)/2 x (w+1)/2), one sample per 2x2 block (the last
 * block row / column of an odd size is 1 pixel high / wide; chroma siting is not modelled);
 * DVIE_YUV_444: U and V are (h x w).  RGB frame f starts at rgb + f*rgb_stride BYTES, its row y at
 * + y*rgb_row_stride, a row w*3 contiguous bytes.  No alignment is assumed of either side: runs of 8
 * pixels whose addresses are 8-byte aligned move as whole 8-byte vectors, everything else bytewise.
 *
 * yuv2rgb reads table[0..4] = (IY, IRV, IBU, IGU, IGV) and yo (synth.yuv_tables):
 *   y = Y - yo, u = U - 128, v = V - 128 (4:2:0: the block's one sample for each of its pixels)
 *   R = clip((IY*y + IRV*v + 32768) >> 16)
 *   G = clip((IY*y - IGU*u - IGV*v + 32768) >> 16)
 *   B = clip((IY*y + IBU*u + 32768) >> 16)
 * rgb2yuv reads table[0..8] = (FY[3], FU[3], FV[3]) and yo:
 *   Y = clip(yo + ((FY . (R,G,B) + 32768) >> 16))
 *   S = the sums of R, G, B over the n pixels of the chroma block that exist (n = 4, 2 or 1; 4:4:4: 1)
 *   U = clip(128 + (((FU . S) * (4/n) + 131072) >> 18)), V likewise with FV.
 * |table[k]| <= 2^18 and 0 <= yo <= 255 keep every intermediate inside int32.
 * n >= 1, 1 <= h, w <= 2^16; for n > 1 the strides must not let frames overlap
 * (yuv_stride >= the packed frame size, rgb_stride >= (h-1)*rgb_row_stride + 3*w); rgb_row_stride >= 3*w.
 */
#define DVIE_YUV_420 420
#define DVIE_YUV_444 444

typedef struct dvie_synth_yuv_desc {
  uint8_t* yuv;
  uint8_t* rgb;
  long long yuv_stride;                 /* bytes between packed frames */
  long long rgb_stride, rgb_row_stride; /* bytes between RGB frames / rows */
  int n, h, w, layout, yo, pad0;
  int table[12];
} dvie_synth_yuv_desc;

int dvie_synth_yuv2rgb(const dvie_synth_yuv_desc* d, void* stream);
int dvie_synth_rgb2yuv(const dvie_synth_yuv_desc* d, void* stream);

/*
 * dvie_synth_scene: the scene-cut statistic of every neighbouring frame pair of uint8 clips
 * (synth.scene_stats / scene_cuts; DESIGN.md "Scene cuts").  Integer arithmetic only, so that every
 * implementation agrees to the last bit.
 *
 * Frames: n0 clips of n1 frames, frame (i0, i1) at frames + i0*s0 + i1*s1 BYTES (strides may be
 * anything, a transposed view of slot-major storage or a [:, ::2] view included); a frame is a
 * contiguous h*w*3 block of uint8 RGB.  No alignment of frame bases is assumed.
 *   Y        = (77*R + 150*G + 29*B + 128) >> 8 per pixel, in 0..255 (the weights sum to 256)
 *   h_t[k]   = pixels of frame t with Y >> 3 == k, k < 32
 * Outputs, indexed o = i0*(n1-1) + t for the pair (t, t+1), all written by the call (nothing is
 * accumulated into, two calls give the same bits):
 *   sad[o]   int64  sum over the h*w pixels of |Y_t - Y_{t+1}|, in 0 .. 255*h*w.  Width: a thread
 *                   sums 8 differences <= 255 and a block 256 such threads (<= 522 240) in
 *                   uint32; the per-pair sum over blocks is int64 (65536x65536: < 1.1e12).
 *   hdiff[o] int64  sum over the 32 bins of |h_t[k] - h_{t+1}[k]|, in 0 .. 2*h*w.  Width: a block's
 *                   bin count is <= 2048 in uint32; the per-frame bin sums over blocks are int64
 *                   (<= h*w <= 2^32), and so is their difference and its sum over the bins.
 *   cut[o]   uint8  (optional, may be NULL) sad[o] >= sad_min && hdiff[o] >= hist_min, compared in
 *                   int64 by the finalize launch, 1 or 0.  sad_min and hist_min are read only then
 *                   and must not be negative (synth.scene_limits makes them on the host).
 * The pair's value depends on its two frames only.
 * Launches: one pass in which every frame byte is read once (a block walks the frames of its
 * 2048-pixel tile and keeps the previous frame's luma in registers), then a finalize launch that
 * sums the per-block partials; no atomics on global memory, no host synchronisation.
 * ws: dvie_synth_scene_ws_bytes(d) bytes = 4 * ceil(h*w / 2048) * (32*n0*n1 + n0*(n1-1)) rounded up
 * to 8 (0 for a descriptor whose sizes are invalid), 8-byte aligned, fully overwritten.  sad and
 * hdiff 8-byte aligned.  1 <= h, w <= 2^16, 1 <= n0 <= 65535, 2 <= n1 <= 65535.
 */
typedef struct dvie_synth_scene_desc {
  const uint8_t* frames;
  long long* sad;
  long long* hdiff;
  uint8_t* cut;
  void* ws;
  long long s0, s1;            /* byte strides of (i0, i1) */
  long long sad_min, hist_min; /* read when cut is given */
  int n0, n1, h, w;
} dvie_synth_scene_desc;

size_t dvie_synth_scene_ws_bytes(const dvie_synth_scene_desc* d);
int dvie_synth_scene(const dvie_synth_scene_desc* d, void* stream);

/*
 * dvie_synth_cutfill: hold frames across the flagged pairs of interpolated clips, in place
 * (synth.cut_fill).  n0 clips of (n1 - 1) * 2^levels + 1 slots, slot (b, s) the nbytes contiguous
 * bytes at slots + b*s0 + s*s1 BYTES (any strides with |s1| >= nbytes: the transposed view of
 * slot-major storage included); input frame t sits in slot t * 2^levels.  cut: the n0 x (n1 - 1)
 * contiguous uint8 flags of dvie_synth_scene, on the device.  With step = 2^levels, for every pair
 * (b, t) whose flag is not 0 and every 1 <= j < step:
 *   slot t*step + j  <-  slot t*step        when j <= step/2  (the midpoint tie goes to the earlier frame)
 *                    <-  slot (t+1)*step    otherwise
 * byte for byte.  No byte of an unflagged pair, and no input slot, is written.  The unit is bytes,
 * so the same call serves frames (h*w*3), label maps (h*w) and packed Y'CbCr frames.  16-byte moves
 * when both slot bases are 16-byte aligned, bytewise otherwise.  One launch; levels = 0 launches
 * nothing.  nbytes >= 1, 1 <= n0 <= 65535, n1 >= 2, 0 <= levels <= 8, (n1 - 1) * (2^levels - 1) <= 65535.
 */
typedef struct dvie_synth_cutfill_desc {
  uint8_t* slots;
  const uint8_t* cut;
  long long s0, s1; /* byte strides of (clip, slot) */
  long long nbytes; /* bytes of a slot */
  int n0, n1, levels, pad0;
} dvie_synth_cutfill_desc;

int dvie_synth_cutfill(const dvie_synth_cutfill_desc* d, void* stream);

/*
 * dvie_synth_tile_blend: the tile outputs of one tiled forward -> the frame, the label map and the
 * kept fp32 form of a canvas (synth.tile_blend; DESIGN.md "Tiled synthesis").  One launch.
 *
 * The canvas (hp, wp) is covered by nty x ntx tiles of one shape (th, tw): tile t = iy*ntx + ix has
 * its top-left at (ys[iy], xs[ix]).  rgb_tiles (nt, n, th, tw, rgb_ld) and seg_tiles
 * (nt, n, th, tw, seg_ld) are fp32, contiguous and 16-byte aligned: every tile's raw image and
 * logits of the n images of the forward.
 *
 * Weight of tile t at canvas pixel (y, x): wy * wx, with per axis (start s, extent e, size S,
 * coordinate c)
 *   a = s > 0     ? c - s + 1 : overlap + 1
 *   b = s + e < S ? s + e - c : overlap + 1
 *   w = min(a, b, overlap + 1)
 * an integer in 1 .. 257 (a canvas border does not ramp; overlap = 0: every weight is 1).
 * Value of a pixel and channel, over its covering tiles in ascending t:
 *   one tile:  the tile's value, bit for bit
 *   several:   acc = 0.f; acc = acc + (float)w_t * v_t per tile (the multiply and the add rounded
 *              separately, no fma); then acc / (float)(sum of w_t), correctly rounded.
 * Outputs (every byte has one owning lane; no atomics, nothing is read back):
 *   rgb_out      fp32 (n, hp, wp, rgb_ld), optional: channels 0-2 the blend, 3 and up zero
 *   frame        uint8 (n, h, w, 3): the top-left (h, w) of the blend through dvie_synth_finish's
 *                quantisation
 *   label        uint8 (n, h, w): dvie_synth_finish's argmax (lowest index on ties) of the blended
 *                logits of the first n_classes classes
 *   label_canvas uint8 (n, hp, wp), optional: the same argmax over every canvas pixel
 * No blended logit map is written.  EINVAL before any launch: null pointers, leading dimensions
 * that are no multiple of 4 (rgb_ld >= 4), unaligned tiles or rgb_out, nty / ntx outside 1..32,
 * starts that do not increase, a tile that leaves the canvas, tiles that do not cover it (the first
 * start is 0, neighbours leave no gap, the last tile ends at the canvas edge), h > hp or w > wp,
 * n_classes outside 1..min(seg_ld, 256), overlap outside 0..256.  All offsets are 64-bit.
 */
#define DVIE_TILE_MAX 32
typedef struct dvie_synth_tile_blend_desc {
  const float* rgb_tiles;
  const float* seg_tiles;
  float* rgb_out; /* may be NULL */
  uint8_t* frame;
  uint8_t* label;
  uint8_t* label_canvas; /* may be NULL */
  int n, th, tw, hp, wp, h, w;
  int rgb_ld, seg_ld, n_classes, overlap;
  int nty, ntx, pad0;
  int ys[DVIE_TILE_MAX], xs[DVIE_TILE_MAX];
} dvie_synth_tile_blend_desc;

int dvie_synth_tile_blend(const dvie_synth_tile_blend_desc* d, void* stream);

/*
 * dvie_synth_retime: the output frames of a frame-rate conversion, gathered or blended from the
 * slots of interpolated clips (synth.retime_gather; DESIGN.md "Frame-rate conversion").  One launch
 * over all n_rows x n0 output rows; no host synchronisation, the flags are read on the device.
 *
 * Slots: n0 clips of n_slots slots, slot (b, s) the nbytes contiguous bytes at slots + b*slot_s0 +
 * s*slot_s1 BYTES; outputs: row (b, k) the nbytes bytes at out + b*out_s0 + k*out_s1 (any strides
 * with |s1| >= nbytes, the transposed views of slot-major storage included; no alignment is
 * assumed).  rows: n_rows x 5 int32 (lo, hi, n, pair, hold), given twice: `rows` on the host, which
 * the call validates, and `rows_dev`, the same values on the device, which the kernel reads.
 * cut: n0 x n_pairs contiguous uint8 flags on the device (dvie_synth_scene's), or NULL.
 * Output row (b, k), in this order:
 *   1. cut != NULL, pair >= 0 and cut[b*n_pairs + pair] != 0:  a byte copy of slot `hold`
 *   2. lo < 0:   nothing is written
 *   3. n == 0:   a byte copy of slot lo
 *   4. else:     every byte (a*(den - n) + c*n + den/2) / den, a and c the bytes of slots lo and hi,
 *                exact integers (the divide is a multiply by ceil(2^32 / (den * (4096 / den))) after
 *                scaling the weights by 4096 / den; csrc/retime.hip shows why that is exact)
 * The unit is bytes, so the same call serves frames, label maps (rows with n = 0) and packed Y'CbCr
 * frames.  No byte outside the written rows is touched.  16-byte moves where the destination and the
 * sources share their offset from a 16-byte boundary (head and tail bytewise), bytes otherwise.
 * Row bases are 64-bit.  EINVAL before any launch: den outside 1..4096, nbytes < 1, n0 outside
 * 1..65535, n_rows outside 0..65535, n outside 0..den-1, lo outside -1..n_slots-1, hi outside the
 * slots of a row that blends, pair < -1, and with cut: pair >= n_pairs or hold outside the slots;
 * overlapping strides; null pointers.  n_rows == 0 launches nothing.
 */
typedef struct dvie_synth_retime_desc {
  const uint8_t* slots;
  uint8_t* out;
  const int32_t* rows;     /* host */
  const int32_t* rows_dev; /* device */
  const uint8_t* cut;      /* device, may be NULL */
  long long slot_s0, slot_s1, out_s0, out_s1; /* byte strides of (clip, slot) and (clip, row) */
  long long nbytes;                           /* bytes of a slot and of a row */
  int n0, n_slots, n_rows, n_pairs, den, pad0;
} dvie_synth_retime_desc;

int dvie_synth_retime(const dvie_synth_retime_desc* d, void* stream);

/*
 * dvie_synth_flip: the W-mirror of one input of a forward -- a frame's fp32 form and its label map
 * -- for a mirrored member of a self-ensemble (synth.synth_flip; DESIGN.md "Self-ensemble").  One
 * launch for both.
 *
 *   dst[i, y, x, c]  = src[i, y, w-1-x, c]     fp32, c in 0..ld-1 (every channel, bit for bit)
 *   ldst[i, y, x]    = lsrc[i, y, w-1-x]       uint8, when lsrc and ldst are given (both or neither)
 *
 * src is n images of (h, w, ld) floats, each contiguous, image i at src + i*src_stride FLOATS; lsrc
 * n label maps of (h, w) bytes, map i at lsrc + i*lsrc_stride BYTES; dst (n, h, w, ld) and ldst
 * (n, h, w) are contiguous.  src, dst and src_stride are 16-byte aligned (ld % 4 == 0): a lane moves
 * one 16-byte vector of a pixel.  The label maps need no alignment: a group of 4 bytes whose source
 * and destination both sit on a dword boundary is one byte-reversed dword, every other byte (row
 * tails, rows with an unaligned base) moves on its own.  Every output byte has one owning lane; no
 * byte outside dst and ldst is written.  EINVAL before any launch: null src / dst, lsrc without
 * ldst or the reverse, n, h or w < 1, ld no positive multiple of 4, a stride smaller than an image
 * (n > 1) or src_stride % 4 != 0, unaligned src / dst, src == dst or lsrc == ldst (the mirror is not
 * done in place), a source range that overlaps its destination.  All offsets are 64-bit.
 */
typedef struct dvie_synth_flip_desc {
  const float* src;
  float* dst;
  const uint8_t* lsrc; /* may be NULL (then ldst is NULL too) */
  uint8_t* ldst;
  long long src_stride;  /* floats between images of src */
  long long lsrc_stride; /* bytes between maps of lsrc */
  int n, h, w, ld;
} dvie_synth_flip_desc;

int dvie_synth_flip(const dvie_synth_flip_desc* d, void* stream);

/*
 * dvie_synth_ens_acc: one member of a self-ensemble added to the running sums of the raw image and
 * of the coarse logits (synth.synth_ens_acc; DESIGN.md "Self-ensemble").  One launch.
 *
 * rgb (n, h, w, rgb_ld) and seg (n, h, w, seg_ld) are the member's outputs, rgb_acc and seg_acc the
 * accumulators of the same shapes; all fp32, contiguous, 16-byte aligned and disjoint.  With
 * xs = w-1-x when flip is set and xs = x otherwise, per pixel (i, y, x), for the channels c in 0..2
 * of the image and the classes c in 0..n_classes-1 of the logits, in fp32:
 *   m = member[i, y, xs, c]
 *   a = first ? m : acc[i, y, x, c] + m
 *   acc[i, y, x, c] = last_m ? a * (1.f / last_m) : a
 * The add and the multiply are two roundings, as written; last_m is 0, 2 or 4, so 1.f / last_m is
 * exact.  Channels 3..rgb_ld-1 of rgb_acc and classes n_classes..seg_ld-1 of seg_acc are written
 * as 0.f by every call.  A chain of M members in order -- the first with `first`, the last with
 * last_m = M -- therefore leaves (((x0 + x1) + x2) + x3) * (1/M).  (The first member may as well be
 * written into the accumulators by its forward: the sums are the same bits, and the last call
 * zeroes the padding.)  Every output vector has one owning lane, which is also the only reader of
 * that accumulator vector.  EINVAL before any launch: null pointers, n, h or w < 1, a leading
 * dimension that is no positive multiple of 4, n_classes outside 1..seg_ld, last_m outside
 * {0, 2, 4}, flip or first outside {0, 1}, unaligned or overlapping buffers.  All offsets are 64-bit.
 */
typedef struct dvie_synth_ens_acc_desc {
  const float* rgb;
  const float* seg;
  float* rgb_acc;
  float* seg_acc;
  int n, h, w;
  int rgb_ld, seg_ld, n_classes;
  int flip, first, last_m, pad0;
} dvie_synth_ens_acc_desc;

int dvie_synth_ens_acc(const dvie_synth_ens_acc_desc* d, void* stream);

/*
 * dvie_synth_motion: full-search block matching on luma between pairs of uint8 frames
 * (synth.block_motion; DESIGN.md "Motion statistics").  Integer arithmetic only, so that every
 * implementation agrees to the last bit.
 *
 * Frames: n0 * n1 pairs; frame (i0, i1) of `cur` at cur + i0*cur_s0 + i1*cur_s1 BYTES and of `ref`
 * at ref + i0*ref_s0 + i1*ref_s1 BYTES (strides may be anything: the views x[:, 1:] and x[:, :-1]
 * of one tensor, a transposed view of slot-major storage); a frame is a contiguous h*w*3 block of
 * uint8 RGB.  No alignment of frame bases is assumed.
 *   Y        = (77*R + 150*G + 29*B + 128) >> 8 per pixel (dvie_synth_scene's luma)
 *   plane P  of size (hs, ws) = (h >> s, w >> s) at scale s:  s = 0: P = Y;  s >= 1:
 *              P[y][x] = (sum of Y over the 2^s x 2^s block at (y << s, x << s) + 2^(2s-1)) >> 2s;
 *              trailing rows and columns that fill no block are dropped (dvie_synth_msssim's rule)
 *   P~[y][x] = P[clamp(y, 0, hs-1)][clamp(x, 0, ws-1)] for any integers y, x
 *   blocks     bh = ceil(hs / 16), bw = ceil(ws / 16); block (i, j) is ALWAYS the 16 x 16 samples
 *              C~[16i+u][16j+v], u, v < 16, of the cur plane: edge blocks read the extension,
 *              nothing is masked
 *   candidates (dy, dx) in [-R, R]^2 with the ref plane R~:
 *              SAD  = sum over u, v < 16 of |C~[16i+u][16j+v] - R~[16i+u+dy][16j+v+dx]|
 *              cost = SAD + penalty * (|dy| + |dx|)
 *   winner     the candidate with the lexicographically smallest (cost, dy*dy + dx*dx, dy, dx);
 *              no other tie rule (two flat frames give zero vectors everywhere)
 * Outputs, indexed f = i0*n1 + i1, all written by the call (nothing is accumulated into, two
 * calls give the same bits), int64:
 *   d2[f]      sum over the blocks of the winner's dy*dy + dx*dx, in plane units
 *   sad[f]     sum of the winners' SAD
 *   sad0[f]    sum of the SAD at (0, 0)
 *   border[f]  blocks whose winner has max(|dy|, |dx|) == R (the search may have been too small)
 * Optional per-block outputs, both or neither (NULL):
 *   mv         int16  [f][bh][bw][2]: (dy, dx)
 *   bsad       uint32 [f][bh][bw][2]: the winner's SAD, the SAD at (0, 0)
 * Widths: a block SAD is <= 256 * 255 = 65 280; a cost is <= 65 280 + 1024 * 64 < 2^18; d2 of a
 * block is <= 2 * 32^2 = 2048; the per-block values are uint32 and the per-pair sums int64.
 * Limits: radius R in 1..32, scale s in 0..3, penalty in 0..1024, 2^s <= h, w <= 65536,
 * n0 * n1 <= 65535; anything else is DVIE_EINVAL with a message that names the value, before any
 * launch.
 * Launches: two that write the cur and ref luma planes at scale s with their clamped margins into
 * the workspace, the matcher (a workgroup stages the search window of four neighbouring blocks in
 * LDS, a wave owns a block, its lanes share the candidates, v_sad_u8 forms the SADs and a wave
 * minimum over one packed key per lane picks the winner), a finalize launch that sums the block
 * values per pair.  No atomics on global memory, no host synchronisation.
 * ws: dvie_synth_motion_ws_bytes(d) bytes (0 for a descriptor whose sizes are invalid), 16-byte
 * aligned, fully overwritten: with groups = ceil(bw / 4), the cur planes (n0*n1 x 16 bh x
 * 64 groups bytes), the ref planes (n0*n1 x (16 bh + 2R) x (64 groups + 2R rounded up to 4, + 4)
 * bytes), each rounded up to 16, and 16 bytes per block.  d2, sad, sad0, border 8-byte aligned.
 */
typedef struct dvie_synth_motion_desc {
  const uint8_t* cur;
  const uint8_t* ref;
  long long* d2;
  long long* sad;
  long long* sad0;
  long long* border;
  int16_t* mv;
  uint32_t* bsad;
  void* ws;
  long long cur_s0, cur_s1, ref_s0, ref_s1; /* byte strides of (i0, i1) */
  int n0, n1, h, w;
  int radius, scale, penalty, pad0;
} dvie_synth_motion_desc;

size_t dvie_synth_motion_ws_bytes(const dvie_synth_motion_desc* d);
int dvie_synth_motion(const dvie_synth_motion_desc* d, void* stream);

int dvie_run_ops(const dvie_op* ops, int n, void* stream);

/* The pairs of ops dvie_run_ops(ops, n) runs as chained launches (host only, nothing is
 * launched): partner[i] = j and partner[j] = i for a pair, -1 for every other op; returns the
 * number of pairs.  Op i (a conv on lane 0) pairs with the next lane-0 op j when every op
 * between them is a weight-lane op of a known kind (weight gradient, reduction, column sum),
 * dvie_conv_chain(&ops[i].u.conv, &ops[j].u.conv) holds and none of the ops between reads or
 * writes ops[j]'s output.  The executor runs the pair at i's turn on the caller's stream, then
 * the ops between them in their order, and goes on after j.  A pair split across two
 * dvie_run_ops calls runs as two launches, as does every op run one at a time.
 * DVIE_CHAIN=0 (environment, read per call): no pairs. */
int dvie_ops_chain_pairs(const dvie_op* ops, int n, int* partner);

/* ABI self-check: sizeof of each descriptor, indexed by DVIE_OP_* (0 = dvie_op; 100.. the
 * descriptors outside the op list: warp, softmax, sn_layer, clip, synth_load, synth_finish,
 * synth_bridge, synth_score, synth_load_pad, synth_finish_crop, synth_vgg_load, synth_msssim, synth_yuv,
 * synth_scene, synth_cutfill, synth_tile_blend; 116 is unused and answers 0; 117: synth_retime,
 * 118: synth_flip, 119: synth_ens_acc; 120 is unused and answers 0; 121: synth_motion). */
size_t dvie_abi_sizeof(int which);
/* library version string */
const char* dvie_version(void);
/* last error text of the calling thread (argument validation) */
const char* dvie_last_error(void);

/* Diagnostics (tests, profiling): launch trace of the calling thread.  dvie_trace_kernels(1)
 * starts recording the kernels every entry point of this thread launches (0 stops; both clear
 * the record; returns the previous state).  dvie_traced_kernels() returns the demangled names
 * of the kernels launched since the last call, ';'-separated in launch order, and clears the
 * record (the text stays valid until the thread's next call). */
int dvie_trace_kernels(int on);
const char* dvie_traced_kernels(void);

#ifdef __cplusplus
}
#endif

#endif /* DVIE_H */
