"""Device-resident video synthesis: uint8 frames and label maps in, uint8 frames and label maps out.

`VideoSynthesizer` runs a trained InterNet / ExtraNet (HRNet coarse model), or one of the
two-stage nets over it (Inter/ExtraRefineNet, Inter/ExtraStage3Net), as a product path:

* every frame lives on the device in two forms: its uint8 RGB / label map (what the caller
  gave or gets) and, while a later forward still reads it, the fp32 (B, H, W, 8) form the
  HRNet plan reads -- for an input frame written by `dvie_synth_load`, for a prediction the
  plan's own raw `rgb` output (unclamped, not re-quantised: what InterTrainer.mini_test
  feeds back).  Both have the strides of the plan's external output, so any two of them go
  into the next forward as channel views, in place;
* the segmentations enter the plan as uint8 label maps (DVIE_EW_LABELS, 1 byte per pixel
  instead of the 80 of an fp32 one-hot);
* the plans are forward-only, label-input and arena-allocated (engine.assign_offsets);
* `dvie_synth_finish` turns a forward's outputs into the uint8 frame and the argmax label;
* nothing is copied to the host.

A two-stage forward is a chain of plans on one stream: the coarse HRNet plan (stem export
on), `dvie_synth_bridge`, the SRNRefine inference plan and, for the stage-3 nets, a second
bridge and the MSResAttnRefine inference plan.  A bridge writes [clamp(image, -1, 1) |
softmax(coarse logits)] straight into the next plan's input buffer (the module forward's
clamp, channel softmax, casts and NCHW input ops in one launch); stage 3 reads the two input
frames in place and their label maps.  The predicted image -- returned quantised, fed back
raw -- is the finest output of the LAST stage with that stage's [-10, 10] clamp (out[2][-1]
of the refine nets' forward, out[3][-1] of the stage-3 nets'); the label is the argmax of
the COARSE logits (the refinement stages predict no segmentation).

Storage is slot-major -- (slots, B, H, W, ...) -- so that one time slot of a chunk of clips is
one contiguous block: a forward reads slots `left` and `right` of clips b0:b1 and writes slot
`out` of the same clips, with no gather or scatter.  All (left, right, out) pairs of a level
form one batch, cut into chunks of at most `max_batch` (VideoSynthesizer.chunks): a chunk that
stays inside one triple runs on those views; where the clips of a triple do not fill a chunk
(a single video), a chunk spans several triples, whose frames are gathered into contiguous
blocks first and whose outputs are scattered back (128 B per pixel and pair, against the
several KB per pixel the forward itself moves).

Frames of any size (pad="replicate"): the fp32 forms and the label maps the forwards read are
canvases of canvas_size(H, W, multiple), the frame at the top-left.  `dvie_synth_load_pad`
writes both canvases of an input slot (its last row and column repeated), and
`dvie_synth_finish_crop` writes the cropped uint8 frame and label of a forward and, for a slot
a later forward reads, the argmax over the whole canvas.  A prediction's pad region is the
network's own output; the uint8 storage the caller gets stays (H, W).

Frames larger than one forward (tile=(th, tw), opt-in): a canvas larger than the tile is cut into
overlapping tiles of one shape (`tile_starts` per axis), the forward above runs per tile on crops of
the input canvases, and `dvie_synth_tile_blend` cross-fades the tiles' raw images and coarse logits
over the overlaps, writing the frame, the label, the label canvas and the kept fp32 form in one
launch (`tile_blend`; include/dvie.h has the weights and the order of the sums).  `max_pixels` is
the largest forward the conv kernels' 32-bit buffer range admits; a larger one is refused on the
host (FrameSizeError) before anything is launched.

Scoring: `frame_scores` (PSNR, SSIM, label agreement: dvie_synth_score) and, opt-in,
`PerceptualScorer`, the per-frame VGG19 feature cosine: `dvie_synth_vgg_load` fills the input
buffer of my_vgg's forward-only, arena-allocated scoring plan from the uint8 frames, and the
plan's own cosfeat ops reduce the five feature maps to one float64 per frame; and
`frame_msssim`, the per-frame multi-scale SSIM over an exact integer pyramid (dvie_synth_msssim).
Motion (opt-in, `MotionSearch`): `block_motion`, full-search block matching on luma between pairs of
frames in exact integers (dvie_synth_motion), gives the held-out scores their motion axis and a
temporal residual across every scored slot (`MotionScores`).

Scene cuts (opt-in, `SceneCuts`): `scene_stats` reduces every neighbouring pair of input frames to
two integers (luma SAD, 32-bin luma histogram distance: dvie_synth_scene), `scene_cuts` compares
them with two integer limits on the device, and after the unchanged rollout `cut_fill`
(dvie_synth_cutfill) overwrites the slots between a flagged pair with copies of the nearer input
frame and label map.  The flags never visit the host on the way.

Frame-rate conversion (opt-in, `Retime`): a ratio P:Q lays an output clock over the dyadic grid of
`levels` doublings.  `retime_plan` maps every output to one or two grid slots on the host, prunes
the midpoint tree to the forwards those slots need and numbers the surviving slots compactly; the
unchanged `_roll` runs that schedule, and `retime_gather` (dvie_synth_retime) copies or blends the
slots into the output frames in one launch, holding frames across flagged pairs from the flags on
the device.

Self-ensemble (opt-in, `ensemble=`): inside one forward (`_run`) the net runs once per member of
`ensemble_members` -- the two inputs in exchanged roles, mirrored along W (`dvie_synth_flip`), or
both -- and `dvie_synth_ens_acc` sums the members' raw images and coarse logits, mirrored back, into
their fp32 means in place, so the finish, the tile stash and every layer above read the means as they
read a single forward's outputs.
"""
import ctypes

import torch

from . import _lib as L
from . import engine as E

_PLAN_FLAGS = ("labels", "alias")


def midpoint_schedule(T, levels):
    """Recursive interpolation of T frames by `levels` doublings: per level the (left, right,
    out) slot triples, slots numbered 0 .. (T - 1) * 2**levels with the input frames at the
    multiples of 2**levels.  Level 1 fills the midpoints of the inputs, level j the midpoints
    of the neighbours at the previous spacing; every other slot is written exactly once."""
    assert T >= 2 and levels >= 0, (T, levels)
    last = (T - 1) << levels
    out = []
    for j in range(1, levels + 1):
        s = 1 << (levels - j + 1)
        out.append([(a, a + s, a + s // 2) for a in range(0, last, s)])
    return out


def heldout_slots(T, levels):
    """Held-out scoring of a T-frame clip by `levels` doublings: frames 0, 2**levels, ... are
    the inputs of the interpolation, every other time index is synthesised and scored against
    the original -> those indices, ascending.  Needs (T - 1) % 2**levels == 0 and T > 2**levels
    (ValueError otherwise)."""
    step = 1 << max(levels, 1)
    if levels < 1 or T <= step or (T - 1) % step:
        raise ValueError(f"held-out interpolation of T={T} frames by levels={levels} needs levels >= 1, "
                         f"(T - 1) % 2**levels == 0 and T > 2**levels")
    return [t for t in range(T) if t % step]


def synth_load(frames, out):
    """uint8 RGB frames (..., 3), contiguous -> fp32 `out` (..., ld) (dvie_synth_load)."""
    L.require_gpu(frames)
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[-1] == 3
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[:-1] == frames.shape[:-1]
    d = L.SynthLoadDesc()
    d.frames, d.out, d.npix, d.out_ld = frames.data_ptr(), out.data_ptr(), frames.numel() // 3, out.shape[-1]
    L.check(L.load().dvie_synth_load(ctypes.byref(d), L.stream_ptr(frames.device)), "synth load")
    return out


def synth_bridge(rgb, seg, dst):
    """fp32 image `rgb` (..., rgb_ld) and coarse logits `seg` (..., seg_ld), contiguous -> the
    channel span `dst`, an (n, H, W, c) view of an NHWC fp32 / bf16 buffer (Plan.input_view):
    c = 40: SRNRefine's [rgb 8 | rgb 8 | softmax 24], c = 24: MSResAttnRefine's [rgb 4 |
    softmax 20] (dvie_synth_bridge)."""
    L.require_gpu(rgb)
    assert rgb.dtype == torch.float32 and rgb.is_contiguous() and seg.dtype == torch.float32 and seg.is_contiguous()
    assert rgb.shape[:-1] == seg.shape[:-1] == dst.shape[:-1] and dst.dim() == 4, (rgb.shape, seg.shape, dst.shape)
    n, H, W, c = dst.shape
    ld = dst.stride(2)
    assert dst.stride() == (H * W * ld, W * ld, ld, 1) and c in (24, 40), (dst.shape, dst.stride())
    d = L.SynthBridgeDesc()
    d.rgb, d.seg, d.dst, d.npix = rgb.data_ptr(), seg.data_ptr(), dst.data_ptr(), n * H * W
    d.rgb_ld, d.seg_ld, d.dst_ld, d.dtype = rgb.shape[-1], seg.shape[-1], ld, E.dv_dtype(dst.dtype)
    d.n_rgb, d.rgb_w, d.seg_w = (2, 8, 24) if c == 40 else (1, 4, 20)
    L.check(L.load().dvie_synth_bridge(ctypes.byref(d), L.stream_ptr(rgb.device)), "synth bridge")


def synth_finish(rgb=None, seg=None, frame=None, label=None, n_classes=20):
    """fp32 `rgb` (..., rgb_ld) -> uint8 `frame` (..., 3) and / or fp32 logits `seg` (..., seg_ld)
    -> uint8 `label` (...) (dvie_synth_finish; all contiguous, either output may be None)."""
    d = L.SynthFinishDesc()
    ref = rgb if frame is not None else seg
    L.require_gpu(ref)
    if frame is not None:
        assert rgb.dtype == torch.float32 and rgb.is_contiguous() and frame.dtype == torch.uint8
        assert frame.is_contiguous() and frame.shape == rgb.shape[:-1] + (3,), (frame.shape, rgb.shape)
        d.rgb, d.frame, d.rgb_ld = rgb.data_ptr(), frame.data_ptr(), rgb.shape[-1]
    if label is not None:
        assert seg.dtype == torch.float32 and seg.is_contiguous() and label.dtype == torch.uint8
        assert label.is_contiguous() and label.shape == seg.shape[:-1], (label.shape, seg.shape)
        d.seg, d.label, d.seg_ld, d.n_classes = seg.data_ptr(), label.data_ptr(), seg.shape[-1], n_classes
    d.npix = ref.numel() // ref.shape[-1]
    L.check(L.load().dvie_synth_finish(ctypes.byref(d), L.stream_ptr(ref.device)), "synth finish")


def canvas_size(H, W, m):
    """the padded canvas of an (H, W) frame: both rounded up to multiples of m"""
    return -(-H // m) * m, -(-W // m) * m


def synth_load_pad(frames, labels, out, label_out):
    """uint8 frames (n, H, W, 3) and label maps (n, H, W) -> the fp32 canvas `out` (n, Hp, Wp, ld)
    and the uint8 label canvas `label_out` (n, Hp, Wp), the last row and column repeated over the
    pad region (dvie_synth_load_pad; all contiguous; labels and label_out both or neither None)."""
    L.require_gpu(frames)
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4 and frames.shape[-1] == 3
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and out.shape[0] == frames.shape[0]
    d = L.SynthLoadPadDesc()
    d.frames, d.out = frames.data_ptr(), out.data_ptr()
    d.n, d.h, d.w = frames.shape[:3]
    d.hp, d.wp, d.out_ld = out.shape[1:]
    if labels is not None or label_out is not None:
        assert labels.dtype == torch.uint8 and labels.is_contiguous() and labels.shape == frames.shape[:3], labels.shape
        assert label_out.dtype == torch.uint8 and label_out.is_contiguous() and label_out.shape == out.shape[:3]
        d.labels, d.label_out = labels.data_ptr(), label_out.data_ptr()
    L.check(L.load().dvie_synth_load_pad(ctypes.byref(d), L.stream_ptr(frames.device)), "synth load_pad")
    return out


def synth_finish_crop(rgb, seg, frame, label, label_canvas=None, n_classes=20):
    """fp32 `rgb` (n, Hp, Wp, rgb_ld) and logits `seg` (n, Hp, Wp, seg_ld) over the canvas -> the
    cropped uint8 `frame` (n, H, W, 3) and `label` (n, H, W) and, when given, the argmax of every
    canvas pixel in `label_canvas` (n, Hp, Wp) (dvie_synth_finish_crop; all contiguous)."""
    L.require_gpu(rgb)
    assert rgb.dtype == torch.float32 and rgb.is_contiguous() and seg.dtype == torch.float32 and seg.is_contiguous()
    assert rgb.dim() == 4 and rgb.shape[:3] == seg.shape[:3], (rgb.shape, seg.shape)
    assert frame.dtype == torch.uint8 and frame.is_contiguous() and label.dtype == torch.uint8 and label.is_contiguous()
    assert frame.dim() == 4 and frame.shape[0] == rgb.shape[0] and frame.shape[3] == 3 and label.shape == frame.shape[:3]
    d = L.SynthFinishCropDesc()
    d.rgb, d.seg, d.frame, d.label = rgb.data_ptr(), seg.data_ptr(), frame.data_ptr(), label.data_ptr()
    d.n, d.h, d.w = frame.shape[:3]
    d.hp, d.wp, d.rgb_ld = rgb.shape[1:]
    d.seg_ld, d.n_classes = seg.shape[3], n_classes
    if label_canvas is not None:
        assert label_canvas.dtype == torch.uint8 and label_canvas.is_contiguous() and label_canvas.shape == rgb.shape[:3]
        d.label_canvas = label_canvas.data_ptr()
    L.check(L.load().dvie_synth_finish_crop(ctypes.byref(d), L.stream_ptr(rgb.device)), "synth finish_crop")


ENSEMBLES = (None, "time", "flip", "time+flip")


def ensemble_members(ensemble):
    """The members (swap, flip) of a self-ensemble, in the order their outputs are summed.  swap:
    the two input frames and their label maps exchange roles (the midpoint of (a, b) is the midpoint
    of (b, a)); flip: the four inputs are mirrored along W and the member's outputs mirrored back.
    None: [(0, 0)], the plain forward.  Anything else: ValueError naming the choices."""
    if ensemble is None:
        return [(0, 0)]
    table = {"time": [(0, 0), (1, 0)], "flip": [(0, 0), (0, 1)], "time+flip": [(0, 0), (1, 0), (0, 1), (1, 1)]}
    if not isinstance(ensemble, str) or ensemble not in table:
        raise ValueError(f'ensemble must be None, "time", "flip" or "time+flip", got {ensemble!r}')
    return list(table[ensemble])


def synth_flip(src, lsrc, dst, ldst):
    """The W-mirror of one input of a forward (dvie_synth_flip, one launch): fp32 `src` (n, H, W, ld),
    its images contiguous and strided over n -> contiguous `dst`; uint8 label maps `lsrc` (n, H, W),
    strided over n -> contiguous `ldst` (lsrc and ldst both or neither None)."""
    L.require_gpu(src)
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.dim() == 4 and dst.shape == src.shape
    n, H, W, ld = src.shape
    assert dst.is_contiguous() and src.stride()[1:] == (W * ld, ld, 1), (src.shape, src.stride())
    d = L.SynthFlipDesc()
    d.src, d.dst, d.src_stride = src.data_ptr(), dst.data_ptr(), src.stride(0)
    d.n, d.h, d.w, d.ld = n, H, W, ld
    if lsrc is not None or ldst is not None:
        assert lsrc.dtype == torch.uint8 and ldst.dtype == torch.uint8 and tuple(lsrc.shape) == tuple(ldst.shape) == (n, H, W)
        assert ldst.is_contiguous() and lsrc.stride()[1:] == (W, 1), (lsrc.shape, lsrc.stride())
        d.lsrc, d.ldst, d.lsrc_stride = lsrc.data_ptr(), ldst.data_ptr(), lsrc.stride(0)
    L.check(L.load().dvie_synth_flip(ctypes.byref(d), L.stream_ptr(src.device)), "synth flip")
    return dst


def synth_ens_acc(rgb, seg, rgb_acc, seg_acc, flip=False, first=False, last_m=0, n_classes=20):
    """One ensemble member's raw image `rgb` (n, H, W, rgb_ld) and coarse logits `seg` (n, H, W,
    seg_ld) into the accumulators of the same shapes (dvie_synth_ens_acc, one launch; all fp32 and
    contiguous): acc = member (first) or acc + member, the member read at the mirrored column with
    flip, then times 1 / last_m when last_m is 2 or 4; the padding channels are written as 0."""
    L.require_gpu(rgb)
    for t, a in ((rgb, rgb_acc), (seg, seg_acc)):
        assert t.dtype == torch.float32 and a.dtype == torch.float32 and t.is_contiguous() and a.is_contiguous()
        assert t.dim() == 4 and t.shape == a.shape, (t.shape, a.shape)
    assert rgb.shape[:3] == seg.shape[:3], (rgb.shape, seg.shape)
    d = L.SynthEnsAccDesc()
    d.rgb, d.seg, d.rgb_acc, d.seg_acc = rgb.data_ptr(), seg.data_ptr(), rgb_acc.data_ptr(), seg_acc.data_ptr()
    d.n, d.h, d.w, d.rgb_ld = rgb.shape
    d.seg_ld, d.n_classes = seg.shape[3], n_classes
    d.flip, d.first, d.last_m = int(bool(flip)), int(bool(first)), int(last_m)
    L.check(L.load().dvie_synth_ens_acc(ctypes.byref(d), L.stream_ptr(rgb.device)), "synth ens_acc")


TILE_MAX = L.TILE_MAX  # tiles per axis
TILE_MAX_OVERLAP = 256


def tile_starts(size, tile, overlap, m):
    """The tiles of one canvas axis -> (starts, extent).  size: the padded canvas size, a multiple of
    m.  size <= tile: ([0], size), the axis is not tiled.  Otherwise n = ceil((size - overlap) /
    (tile - overlap)) tiles of extent `tile` at starts[i] = (i * (size - tile) // (n - 1)) // m * m:
    strictly increasing multiples of m from 0 to size - tile, neighbours overlapping by at least
    `overlap`, at most three tiles over a coordinate.  tile % m == 0, overlap % m == 0, 0 <= overlap
    <= min(tile // 2, 256), at most 32 tiles: ValueError naming the argument otherwise."""
    for name, v in (("size", size), ("tile", tile), ("overlap", overlap), ("m", m)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"tile_starts: {name}={v!r} must be an int")
    if m < 1:
        raise ValueError(f"tile_starts: m={m} must be at least 1")
    if size < 1 or size % m:
        raise ValueError(f"tile_starts: size={size} must be a positive multiple of m={m}")
    if tile < 1 or tile % m:
        raise ValueError(f"tile_starts: tile={tile} must be a positive multiple of m={m}")
    if overlap < 0 or overlap % m or overlap > tile // 2 or overlap > TILE_MAX_OVERLAP:
        raise ValueError(f"tile_starts: overlap={overlap} must be a multiple of m={m} in 0..min(tile // 2, "
                         f"{TILE_MAX_OVERLAP}) = {min(tile // 2, TILE_MAX_OVERLAP)}")
    if size <= tile:
        return [0], size
    n = -(-(size - overlap) // (tile - overlap))
    if n > TILE_MAX:
        raise ValueError(f"tile_starts: tile={tile} cuts size={size} into {n} tiles, at most {TILE_MAX} per axis")
    return [(i * (size - tile) // (n - 1)) // m * m for i in range(n)], tile


def tile_blend(rgb_tiles, seg_tiles, ys, xs, overlap, frame, label, rgb_out=None, label_canvas=None, n_classes=20):
    """The tile outputs of one tiled forward -> the blended canvas (dvie_synth_tile_blend, one
    launch).  rgb_tiles (nt, n, th, tw, rgb_ld) and seg_tiles (nt, n, th, tw, seg_ld): fp32,
    contiguous, tile iy * len(xs) + ix at (ys[iy], xs[ix]) of the canvas (ys[-1] + th, xs[-1] + tw).
    frame uint8 (n, h, w, 3) and label uint8 (n, h, w) get the top-left (h, w) of the blend (the
    quantisation and the argmax of synth_finish); rgb_out, fp32 (n, hp, wp, rgb_ld), the blend in
    channels 0-2 and zeros above; label_canvas, uint8 (n, hp, wp), the argmax of every canvas pixel.
    include/dvie.h states the weights and the order of the sums."""
    L.require_gpu(rgb_tiles)
    ys, xs = list(ys), list(xs)
    f32 = torch.float32
    assert rgb_tiles.dtype == f32 and rgb_tiles.is_contiguous() and seg_tiles.dtype == f32 and seg_tiles.is_contiguous()
    assert rgb_tiles.dim() == 5 and rgb_tiles.shape[:4] == seg_tiles.shape[:4], (rgb_tiles.shape, seg_tiles.shape)
    nt, n, th, tw, rgb_ld = rgb_tiles.shape
    if not 1 <= len(ys) <= TILE_MAX or not 1 <= len(xs) <= TILE_MAX or nt != len(ys) * len(xs):
        raise ValueError(f"tile_blend: {len(ys)} x {len(xs)} starts (1..{TILE_MAX} per axis) for {nt} tiles")
    hp, wp = ys[-1] + th, xs[-1] + tw
    assert frame.dtype == torch.uint8 and frame.is_contiguous() and label.dtype == torch.uint8 and label.is_contiguous()
    assert frame.dim() == 4 and frame.shape[0] == n and frame.shape[3] == 3 and label.shape == frame.shape[:3]
    d = L.SynthTileBlendDesc()
    d.rgb_tiles, d.seg_tiles, d.frame, d.label = rgb_tiles.data_ptr(), seg_tiles.data_ptr(), frame.data_ptr(), label.data_ptr()
    d.n, d.th, d.tw, d.hp, d.wp = n, th, tw, hp, wp
    d.h, d.w = frame.shape[1:3]
    d.rgb_ld, d.seg_ld, d.n_classes, d.overlap = rgb_ld, seg_tiles.shape[4], n_classes, overlap
    d.nty, d.ntx = len(ys), len(xs)
    for k, v in enumerate(ys):
        d.ys[k] = v
    for k, v in enumerate(xs):
        d.xs[k] = v
    if rgb_out is not None:
        assert rgb_out.dtype == f32 and rgb_out.is_contiguous() and tuple(rgb_out.shape) == (n, hp, wp, rgb_ld), rgb_out.shape
        d.rgb_out = rgb_out.data_ptr()
    if label_canvas is not None:
        assert label_canvas.dtype == torch.uint8 and label_canvas.is_contiguous() and tuple(label_canvas.shape) == (n, hp, wp)
        d.label_canvas = label_canvas.data_ptr()
    L.check(L.load().dvie_synth_tile_blend(ctypes.byref(d), L.stream_ptr(rgb_tiles.device)), "synth tile_blend")


class FrameScores:
    """Per-frame scores of uint8 frames against the originals (frame_scores): device tensors
    shaped like the leading dimensions of the frames -- sse (int64), ssim (float64) and, with
    label maps, agree, valid (int64), inter, uni (int64, a trailing class dimension); None
    without.  psnr / acc / miou are derived on the device in float64."""
    FIELDS = ("sse", "ssim", "agree", "valid", "inter", "uni", "msssim", "vgg")

    def __init__(self, H, W, sse, ssim, agree=None, valid=None, inter=None, uni=None, vgg=None, msssim=None):
        self.H, self.W = H, W
        self.sse, self.ssim, self.agree, self.valid, self.inter, self.uni = sse, ssim, agree, valid, inter, uni
        self.vgg = vgg  # float64 VGG19 feature cosine per frame (frame_scores(..., perceptual=)), or None
        self.msssim = msssim  # float64 multi-scale SSIM per frame (frame_scores(..., msssim=K)), or None

    @property
    def psnr(self):
        """10 log10(255^2 / mse) per frame; +inf where the frames are equal (losses.py:103-116)"""
        return 10.0 * torch.log10((255.0 ** 2 * 3 * self.H * self.W) / self.sse.double())

    @property
    def acc(self):
        """pixel accuracy: the reference's `IoU` (losses.py:122-131)"""
        if self.agree is None:
            return None
        # (a tensor divisor: torch turns a division by a Python scalar into a multiplication)
        return self.agree.double() / torch.full_like(self.agree, self.H * self.W, dtype=torch.float64)

    @property
    def miou(self):
        """mean of inter / uni over the classes with uni > 0 (NaN for a frame without a valid pixel)"""
        if self.uni is None:
            return None
        seen = self.uni > 0
        iou = torch.where(seen, self.inter.double() / self.uni.clamp(min=1).double(), torch.zeros((), dtype=torch.float64,
                                                                                                  device=self.uni.device))
        return iou.sum(-1) / seen.sum(-1).double()

    def map(self, fn):
        """the same scores with fn applied to every tensor (the class dimension stays last)"""
        return FrameScores(self.H, self.W, **{k: None if getattr(self, k) is None else fn(getattr(self, k))
                                              for k in self.FIELDS})


def _lead_of(t, tail, what):
    """(n0, n1, s0, s1) of `t` (..., *tail): up to two leading dimensions of any strides (in
    elements = bytes), the trailing `tail` dimensions contiguous"""
    k = len(tail)
    if t.dtype != torch.uint8 or t.dim() < k or t.dim() > k + 2 or tuple(t.shape[t.dim() - k:]) != tuple(tail):
        raise ValueError(f"{what}: uint8 (..., {', '.join(map(str, tail))}) with at most two leading dimensions, got "
                         f"{tuple(t.shape)} {t.dtype}")
    want = 1
    for d in range(t.dim() - 1, t.dim() - k - 1, -1):
        if t.shape[d] != 1 and t.stride(d) != want:
            raise ValueError(f"{what}: the {k} frame-level dimensions must be contiguous, got strides {t.stride()}")
        want *= t.shape[d]
    lead = [(t.shape[d], t.stride(d)) for d in range(t.dim() - k)]
    (n0, s0), (n1, s1) = ([(1, 0)] * (2 - len(lead)) + lead)
    return n0, n1, s0, s1


def vgg_region(H, W):
    """The top-left region (H // 16 * 16, W // 16 * 16) of an (H, W) frame that the perceptual
    score is taken on: the VGG plan's four 2x2 poolings need even sizes at every level.  When H
    and W are multiples of 16 this is the whole frame; otherwise up to 15 trailing rows and
    columns are not seen.  A side below 16 raises ValueError."""
    if H < 16 or W < 16:
        raise ValueError(f"the perceptual score needs frames of at least 16x16, got {H}x{W}")
    return H // 16 * 16, W // 16 * 16


def vgg_lut(dtype=torch.float32):
    """The (3, 256) table of dvie_synth_vgg_load (a CPU tensor): lut[c][v] = (v / 255 - mean_c) /
    std_c with the ImageNet constants, computed in float64 and rounded once to fp32; for
    torch.bfloat16 that fp32 value rounded once more, to nearest even."""
    import numpy as np
    v = np.arange(256, dtype=np.float64)
    t = torch.from_numpy(np.stack([np.float32((v / 255.0 - m) / s) for m, s in zip(E._IMAGENET_MEAN, E._IMAGENET_STD)]))
    return t.bfloat16() if dtype == torch.bfloat16 else t


def _vgg_load_call(pred, gt, n0, n1, strides, H, W, region, out, lut, img0, n_out):
    d = L.SynthVggLoadDesc()
    d.pred, d.gt, d.out, d.lut = pred, gt, out.data_ptr(), lut.data_ptr()
    d.pred_s0, d.pred_s1, d.gt_s0, d.gt_s1 = strides
    d.n0, d.n1, d.h, d.w = n0, n1, H, W
    (d.h16, d.w16), d.dtype, d.img0, d.n_out = region, E.dv_dtype(out.dtype), img0, n_out
    L.check(L.load().dvie_synth_vgg_load(ctypes.byref(d), L.stream_ptr(out.device)), "synth vgg_load")


def _pairs_of(pred, gt):
    """the checks frame_scores makes on its frames -> (lead, H, W, n0, n1, byte strides of pred and gt)"""
    L.require_gpu(pred)
    if pred.dim() < 3 or pred.shape[-1] != 3:
        raise ValueError(f"pred: uint8 (..., H, W, 3), got {tuple(pred.shape)}")
    lead, (H, W) = tuple(pred.shape[:-3]), pred.shape[-3:-1]
    if H < 1 or W < 1 or any(n < 1 for n in lead):
        raise ValueError(f"pred: empty dimensions in {tuple(pred.shape)}")
    n0, n1, ps0, ps1 = _lead_of(pred, (H, W, 3), "pred")
    if not isinstance(gt, torch.Tensor) or gt.device != pred.device or tuple(gt.shape[:gt.dim() - 3]) != lead:
        raise ValueError(f"gt: a tensor on {pred.device} with the leading dimensions {lead} of pred")
    _, _, gs0, gs1 = _lead_of(gt, (H, W, 3), "gt")
    return lead, H, W, n0, n1, (ps0, ps1, gs0, gs1)


def vgg_load(pred, gt, out, lut):
    """uint8 frames `pred`, `gt` (..., H, W, 3) (up to two leading dimensions of any strides, as
    frame_scores takes them) -> `out` (2n, h16, w16, 8), fp32 or bf16, contiguous: the images
    [pred_0 .. pred_{n-1} | gt_0 .. gt_{n-1}] over the region vgg_region(H, W), channels 0-2
    looked up in `lut` (vgg_lut(out.dtype) on the device), channels 3-7 zero (dvie_synth_vgg_load)."""
    lead, H, W, n0, n1, strides = _pairs_of(pred, gt)
    region = vgg_region(H, W)
    assert out.is_contiguous() and tuple(out.shape) == (2 * n0 * n1,) + region + (8,), (out.shape, n0, n1, region)
    assert lut.dtype == out.dtype and lut.is_contiguous() and tuple(lut.shape) == (3, 256) and lut.device == out.device
    _vgg_load_call(pred.data_ptr(), gt.data_ptr(), n0, n1, strides, H, W, region, out, lut, 0, n0 * n1)
    return out


class PerceptualScorer:
    """Per-frame VGG19 perceptual score of uint8 device frames: the reference's `vgg` validation
    metric (losses.VGGCosineLoss -- the cosine between the five my_vgg feature maps relu1_2 ..
    relu5_4 of a frame and of its original, averaged over pixels, then over the five maps), one
    float64 per frame, higher is better, 1 for equal frames, with nothing leaving the device.

    scorer(pred, gt): uint8 (..., H, W, 3) with up to two leading dimensions of any strides (what
    frame_scores takes) -> a float64 device tensor shaped like the leading dimensions.  A pixel
    whose feature vector is all zero on either side makes its frame's score NaN (the reference's
    0/0) and no other frame's.

    The score is taken on the top-left region vgg_region(H, W) = (H // 16 * 16, W // 16 * 16) of
    both frames, read in place (no cropped copy): with H and W multiples of 16 it is the
    reference's value on the whole frame; otherwise up to 15 trailing rows and columns are not
    seen.  A side below 16 raises ValueError.

    vgg_net: a nets.vgg.my_vgg already on the device (a trainer's, so that the weights are
    shared); None builds one from vgg19_features() (DVIE_VGG19_WEIGHTS, or the seeded synthetic
    weights) and moves it to the frames' device at the first call.  The VGG runs in the net's
    precision (precision_of()).  max_batch: frame pairs per VGG forward.  The pairs are cut, in
    order, into chunks of at most max_batch; every chunk size takes a pooled, arena-allocated
    plan of its own, so a last smaller chunk compiles (once) a second plan.

    Per chunk: dvie_synth_vgg_load writes the plan's input buffer, the plan runs its convs and
    poolings with one cosine reduction per feature map, and its last op writes the chunk's
    scores.  Everything runs on the caller's current stream and nothing synchronises with the
    host; the partial workspace and the output are allocated per call on that stream, the
    256-entry normalisation table once per device."""

    def __init__(self, vgg_net=None, max_batch=8):
        from .nets.vgg import my_vgg, vgg19_features
        if vgg_net is not None and not isinstance(vgg_net, my_vgg):
            raise ValueError(f"vgg_net: a nets.vgg.my_vgg, got {type(vgg_net).__name__}")
        if max_batch < 1:
            raise ValueError(f"max_batch={max_batch} must be at least 1")
        self._own = vgg_net is None
        self.net = my_vgg(vgg19_features()) if self._own else vgg_net
        self.max_batch = int(max_batch)
        self._lut = {}  # (device, dtype) -> the table on the device

    @property
    def weights_name(self):
        """which weights the score was taken with: the basename of DVIE_VGG19_WEIGHTS or
        "synthetic-seed19" (what scores.json records as vgg_weights)"""
        import os
        from .nets.vgg import SYNTH_SEED
        path = os.environ.get("DVIE_VGG19_WEIGHTS")
        return os.path.basename(path) if path else f"synthetic-seed{SYNTH_SEED}"

    def _table(self, dev):
        key = (dev, self.net.dtype)
        if key not in self._lut:
            self._lut[key] = vgg_lut(self.net.dtype).to(dev)
        return self._lut[key]

    def __call__(self, pred, gt):
        lead, H, W, n0, n1, (ps0, ps1, gs0, gs1) = _pairs_of(pred, gt)
        region = vgg_region(H, W)
        dev = pred.device
        if next(self.net.parameters()).device != dev:
            if not self._own:
                raise ValueError(f"vgg_net is on {next(self.net.parameters()).device}, the frames on {dev}")
            self.net.to(dev)
        if n1 == 1:  # (B, 1) views: one run of B pairs instead of B rows of one
            n0, n1, ps0, ps1, gs0, gs1 = 1, n0, 0, ps0, 0, gs0
        N = n0 * n1
        lut = self._table(dev)
        out = torch.empty((N,), dtype=torch.float64, device=dev)
        with torch.no_grad():
            for f0 in range(0, N, self.max_batch):
                f1 = min(N, f0 + self.max_batch)
                plan = self.net.score_plan(f1 - f0, region[0], region[1], dev)
                view = plan.input_view("vgg_in")
                f = f0
                while f < f1:  # the chunk's pairs, row by row of the (n0, n1) frame grid
                    i0, a = divmod(f, n1)
                    b = min(n1, a + f1 - f)
                    _vgg_load_call(pred.data_ptr() + i0 * ps0 + a * ps1, gt.data_ptr() + i0 * gs0 + a * gs1, 1, b - a,
                                   (0, ps1, 0, gs1), H, W, region, view, lut, f - f0, f1 - f0)
                    f += b - a
                ws = torch.empty((plan.cosfeat_ws_doubles,), dtype=torch.float64, device=dev)
                plan.set_cosfeat(ws, out[f0:f1])
                plan.run_forward()
        return out.reshape(lead)


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # Wang, Simoncelli and Bovik (2003)


def msssim_weights(K):
    """the exponents of a K-scale MS-SSIM: the first K published weights divided by their sum"""
    if not 1 <= K <= len(MSSSIM_WEIGHTS):
        raise ValueError(f"msssim: scales={K} must be in 1..{len(MSSSIM_WEIGHTS)}")
    total = sum(MSSSIM_WEIGHTS[:K])
    return tuple(w / total for w in MSSSIM_WEIGHTS[:K])


def msssim_max_scales(H, W):
    """the largest K with min(H, W) >> (K - 1) >= 11, at most 5 (the coarsest level must hold a
    whole 11-tap window); 0 for a side below 11.  Five scales need a shorter side of 176."""
    K = 0
    while K < len(MSSSIM_WEIGHTS) and (min(H, W) >> K) >= 11:
        K += 1
    return K


def msssim_check(H, W, scales):
    """ValueError unless (H, W) frames take `scales` MS-SSIM scales (the message names the largest
    number that fits)"""
    if not isinstance(scales, int) or isinstance(scales, bool) or not 1 <= scales <= len(MSSSIM_WEIGHTS):
        raise ValueError(f"msssim: scales={scales!r} must be an int in 1..{len(MSSSIM_WEIGHTS)}")
    fit = msssim_max_scales(H, W)
    if scales > fit:
        raise ValueError(f"msssim: {scales} scales need min(H, W) >> {scales - 1} >= 11; {H}x{W} frames take at most "
                         f"{fit} scales")


def frame_msssim(pred, gt, scales=5):
    """Multi-scale SSIM of uint8 device frames `pred` (..., H, W, 3) against `gt` (what frame_scores
    takes: up to two leading dimensions of any strides) -> (msssim, parts): float64 device tensors
    shaped like the leading dimensions and like them + (scales,) (dvie_synth_msssim: a pyramid
    launch, one level pass, a finalize launch; no host synchronisation).

    Level s of the pyramid is (H >> s, W >> s): the mean of the 2**s x 2**s blocks of the frame,
    trailing rows and columns dropped.  parts[..., s] is the mean of the contrast-structure map cs
    of level s, for the last level of l * cs, with dvie_synth_score's window and border rule;
    msssim = prod max(parts, 0) ** msssim_weights(scales).  scales=1 is frame_scores' ssim.
    min(H, W) >> (scales - 1) must be at least 11 (ValueError naming msssim_max_scales(H, W))."""
    lead, H, W, n0, n1, strides = _pairs_of(pred, gt)
    msssim_check(H, W, scales)
    dev = pred.device
    d = L.SynthMsssimDesc()
    d.pred, d.gt, d.n0, d.n1, d.h, d.w, d.scales = pred.data_ptr(), gt.data_ptr(), n0, n1, H, W, scales
    d.pred_s0, d.pred_s1, d.gt_s0, d.gt_s1 = strides
    out = torch.empty(lead, dtype=torch.float64, device=dev)
    parts = torch.empty(lead + (scales,), dtype=torch.float64, device=dev)
    lib = L.load()
    ws = torch.empty((lib.dvie_synth_msssim_ws_bytes(ctypes.byref(d)),), dtype=torch.uint8, device=dev)
    d.msssim, d.parts, d.ws = out.data_ptr(), parts.data_ptr(), ws.data_ptr()
    L.check(lib.dvie_synth_msssim(ctypes.byref(d), L.stream_ptr(dev)), "synth msssim")
    return out, parts


YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}  # (Kr, Kb)


def yuv_tables(matrix="bt601", full_range=False):
    """The integer tables of dvie_synth_yuv2rgb / dvie_synth_rgb2yuv -> (inverse, forward, yo):
    inverse = (IY, IRV, IBU, IGU, IGV), forward = (FY[3], FU[3], FV[3]) flattened, every entry
    round(65536 * x) as a Python int, yo the luma offset.  Kr, Kb from the matrix ("bt601",
    "bt709"), Kg = 1 - Kr - Kb; limited range sy = 219/255, sc = 224/255, yo = 16, full range
    sy = sc = 1, yo = 0.  The only place the floats become integers (include/dvie.h has the
    formulas the integers enter)."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix {matrix!r} must be one of {', '.join(YUV_MATRICES)}")
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)
    q = lambda x: int(round(65536.0 * x))  # noqa: E731
    inverse = (q(1.0 / sy), q(2.0 * (1.0 - kr) / sc), q(2.0 * (1.0 - kb) / sc),
               q(2.0 * kb * (1.0 - kb) / (kg * sc)), q(2.0 * kr * (1.0 - kr) / (kg * sc)))
    fu, fv = sc / (2.0 * (1.0 - kb)), sc / (2.0 * (1.0 - kr))
    forward = (q(sy * kr), q(sy * kg), q(sy * kb),
               q(-kr * fu), q(-kg * fu), q((1.0 - kb) * fu),
               q((1.0 - kr) * fv), q(-kg * fv), q(-kb * fv))
    return inverse, forward, yo


def _yuv_layout(colourspace, what):
    """DVIE_YUV_420 / DVIE_YUV_444 of a Y4M colourspace tag (Cmono has no chroma to convert)"""
    from .video_io import layout_of
    lay = layout_of(colourspace)
    if lay == "mono":
        raise ValueError(f"{what}: {colourspace} has no chroma; its Y plane is the first H * W bytes of a frame")
    return L.YUV_420 if lay == "420" else L.YUV_444


def _yuv_call(fn, what, yuv, yuv_stride, rgb_ptr, rgb_stride, n, H, W, layout, table, yo, dev):
    d = L.SynthYuvDesc()
    d.yuv, d.rgb, d.yuv_stride, d.rgb_stride, d.rgb_row_stride = yuv, rgb_ptr, yuv_stride, rgb_stride, 3 * W
    d.n, d.h, d.w, d.layout, d.yo = n, H, W, layout, yo
    for k, v in enumerate(table):
        d.table[k] = v
    L.check(fn(ctypes.byref(d), L.stream_ptr(dev)), what)


def _packed_check(t, fb, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != fb or t.shape[0] < 1 \
            or (t.stride(1) != 1 and fb != 1) or (t.shape[0] > 1 and t.stride(0) < fb):
        raise ValueError(f"{what}: uint8 (N, {fb}) packed frames with contiguous rows, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")


def yuv_to_rgb(packed, H, W, colourspace, matrix="bt601", full_range=False, out=None):
    """Packed Y'CbCr frames `packed` (N, frame_bytes(W, H, colourspace)), uint8 on the device, rows
    contiguous and any row stride -> uint8 RGB (N, H, W, 3) (dvie_synth_yuv2rgb: one launch, integer
    arithmetic, nearest chroma upsampling for the 4:2:0 colourspaces).  out: a contiguous
    (N, H, W, 3) uint8 tensor to write instead of a new one."""
    from .video_io import frame_bytes
    L.require_gpu(packed)
    layout = _yuv_layout(colourspace, "yuv_to_rgb")
    _packed_check(packed, frame_bytes(W, H, colourspace), "packed")
    N = packed.shape[0]
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=packed.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous() or out.device != packed.device:
        raise ValueError(f"out: a contiguous uint8 {(N, H, W, 3)} tensor on {packed.device}")
    inverse, _, yo = yuv_tables(matrix, full_range)
    _yuv_call(L.load().dvie_synth_yuv2rgb, "synth yuv2rgb", packed.data_ptr(), packed.stride(0), out.data_ptr(),
              H * W * 3, N, H, W, layout, inverse, yo, packed.device)
    return out


def rgb_to_yuv(frames, colourspace, matrix="bt601", full_range=False, out=None):
    """uint8 RGB device frames (..., H, W, 3) with up to two leading dimensions of any strides (the
    slot-major views interpolate returns are read in place) -> packed Y'CbCr frames
    (N, frame_bytes(W, H, colourspace)) in the order of the leading dimensions (dvie_synth_rgb2yuv;
    4:2:0 chroma is taken on the sum of each 2x2 block).  out: a uint8 (N, frame_bytes) tensor with
    contiguous rows and any row stride and alignment (a slice of a larger buffer) to write instead.
    One launch when the leading dimensions collapse to one stride, otherwise one per index of the
    shorter of the two."""
    from .video_io import frame_bytes
    L.require_gpu(frames)
    layout = _yuv_layout(colourspace, "rgb_to_yuv")
    if frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError(f"frames: uint8 (..., H, W, 3), got {tuple(frames.shape)}")
    H, W = frames.shape[-3:-1]
    n0, n1, s0, s1 = _lead_of(frames, (H, W, 3), "frames")
    N, fb = n0 * n1, frame_bytes(W, H, colourspace)
    if N < 1:
        raise ValueError(f"frames: empty dimensions in {tuple(frames.shape)}")
    if out is None:
        out = torch.empty((N, fb), dtype=torch.uint8, device=frames.device)
    else:
        _packed_check(out, fb, "out")
        if out.shape[0] != N or out.device != frames.device:
            raise ValueError(f"out: {N} packed frames on {frames.device}, got {tuple(out.shape)} on {out.device}")
    _, forward, yo = yuv_tables(matrix, full_range)
    fn, src, dst, ds = L.load().dvie_synth_rgb2yuv, frames.data_ptr(), out.data_ptr(), out.stride(0)
    args = (H, W, layout, forward, yo, frames.device)
    if n0 == 1 or n1 == 1 or s0 == n1 * s1:  # one run of N frames
        _yuv_call(fn, "synth rgb2yuv", dst, ds, src, s1 if n0 == 1 else (s0 if n1 == 1 else s1), N, *args)
    elif n0 <= n1:  # a launch per row of the (n0, n1) grid
        for i in range(n0):
            _yuv_call(fn, "synth rgb2yuv", dst + i * n1 * ds, ds, src + i * s0, s1, n1, *args)
    else:  # a launch per column
        for j in range(n1):
            _yuv_call(fn, "synth rgb2yuv", dst + j * ds, n1 * ds, src + j * s1, s0, n0, *args)
    return out


def window_plan(T, window):
    """The windows a T-frame clip is interpolated in: [(t0, t1)], inclusive input-frame ranges of at
    most `window` frames that share their boundary frame -- (0, N-1), (N-1, 2N-2), ... -- the last
    one shorter when T - 1 is no multiple of window - 1, never fewer than two frames.  Interpolation
    between two neighbouring inputs depends on those two only, so the windows' results, each without
    its first slot after the first window, concatenate to the whole clip's.  T < 2 or window < 2:
    ValueError."""
    if T < 2 or window < 2:
        raise ValueError(f"window_plan needs T >= 2 frames and window >= 2, got T={T}, window={window}")
    out, t0 = [], 0
    while t0 < T - 1:
        t1 = min(t0 + window - 1, T - 1)
        out.append((t0, t1))
        t0 = t1
    return out


def scene_stats(frames):
    """The scene-cut statistic of uint8 device clips `frames` (B, T, H, W, 3), T >= 2, any strides
    over B and T (the frame-level dimensions contiguous) -> (sad, hdiff), int64 device tensors
    (B, T - 1): per neighbouring pair the sum of |Y_t - Y_t+1| over the pixels and the sum over
    32 bins of |h_t - h_t+1|, Y = (77 R + 150 G + 29 B + 128) >> 8 and h the histogram of Y >> 3
    (dvie_synth_scene: one pass that reads every frame once, a finalize launch; exact integers, no
    host synchronisation)."""
    return _scene_call(frames, None)[:2]


def scene_limits(H, W, mad, hist):
    """The two integer limits a pair of (H, W) frames is compared with -> (sad_min, hist_min) =
    (ceil(mad * H * W), ceil(hist * 2 * H * W)), Python ints: the only place a float becomes an
    integer.  mad: the mean absolute luma difference in 0..255; hist: the histogram distance in
    0..1 (ValueError outside)."""
    import math
    if not 0 <= mad <= 255 or not 0 <= hist <= 1:
        raise ValueError(f"scene_limits: mad={mad} must be in 0..255 and hist={hist} in 0..1")
    if H < 1 or W < 1:
        raise ValueError(f"scene_limits: H={H} and W={W} must be at least 1")
    return int(math.ceil(mad * H * W)), int(math.ceil(hist * 2 * H * W))


def _scene_call(frames, limits):
    """scene_stats, and with limits = (sad_min, hist_min) the flags of the finalize launch too ->
    (sad, hdiff, cut or None)"""
    L.require_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or frames.shape[1] < 2 or \
            min(frames.shape) < 1:
        raise ValueError(f"frames: uint8 (B, T, H, W, 3) with T >= 2, got {tuple(frames.shape)} {frames.dtype}")
    B, T, H, W, _ = frames.shape
    d = L.SynthSceneDesc()
    d.n0, d.n1, d.s0, d.s1 = _lead_of(frames, (H, W, 3), "frames")
    d.frames, d.h, d.w = frames.data_ptr(), H, W
    dev = frames.device
    sad = torch.empty((B, T - 1), dtype=torch.int64, device=dev)
    hdiff = torch.empty((B, T - 1), dtype=torch.int64, device=dev)
    cut = None
    if limits is not None:
        cut = torch.empty((B, T - 1), dtype=torch.bool, device=dev)  # (the kernel writes bytes 0 and 1)
        d.cut, d.sad_min, d.hist_min = cut.data_ptr(), limits[0], limits[1]
    lib = L.load()
    ws = torch.empty((lib.dvie_synth_scene_ws_bytes(ctypes.byref(d)),), dtype=torch.uint8, device=dev)
    d.sad, d.hdiff, d.ws = sad.data_ptr(), hdiff.data_ptr(), ws.data_ptr()
    L.check(lib.dvie_synth_scene(ctypes.byref(d), L.stream_ptr(dev)), "synth scene")
    return sad, hdiff, cut


def scene_cuts(frames, mad, hist):
    """Which neighbouring pairs of the uint8 device clips `frames` (B, T, H, W, 3) are scene cuts ->
    a bool device tensor (B, T - 1): sad >= sad_min and hdiff >= hist_min with scene_stats' two sums
    and scene_limits' two integers, compared in int64 by the statistic's finalize launch.  A pair's
    flag depends on its two frames only."""
    if frames.dim() != 5:
        raise ValueError(f"frames: uint8 (B, T, H, W, 3), got {tuple(frames.shape)}")
    return _scene_call(frames, scene_limits(frames.shape[2], frames.shape[3], mad, hist))[2]


def cut_sources(levels):
    """Which input frame fills the 2**levels - 1 slots between a flagged pair, in slot order: 0 the
    left one, 1 the right one -- the nearest in time, the midpoint going to the left."""
    if levels < 0:
        raise ValueError(f"cut_sources: levels={levels} must not be negative")
    step = 1 << levels
    return [0 if j <= step // 2 else 1 for j in range(1, step)]


def cut_fill(slots, cuts, levels):
    """Hold frames across the flagged pairs, in place: `slots` uint8 (B, (T - 1) * 2**levels + 1,
    ...) on the device, any strides over the two leading dimensions and the others contiguous
    (frames, label maps or packed Y'CbCr frames; the transposed views interpolate returns are
    taken as they are), `cuts` bool or uint8 (B, T - 1) on the device.  The slots between the two
    inputs of a flagged pair become byte copies of the nearer input slot (cut_sources); nothing
    else is written (dvie_synth_cutfill: one launch that reads the flags on the device).  -> slots"""
    L.require_gpu(slots)
    if slots.dtype != torch.uint8 or slots.dim() < 2:
        raise ValueError(f"slots: uint8 (B, S, ...), got {tuple(slots.shape)} {slots.dtype}")
    if cuts.dtype not in (torch.bool, torch.uint8) or cuts.dim() != 2 or cuts.device != slots.device:
        raise ValueError(f"cuts: bool (B, T - 1) on {slots.device}, got {tuple(cuts.shape)} {cuts.dtype}")
    B, S = slots.shape[:2]
    T = cuts.shape[1] + 1
    if levels < 0 or cuts.shape[0] != B or T < 2 or S != ((T - 1) << levels) + 1:
        raise ValueError(f"cut_fill: {tuple(cuts.shape)} flags and levels={levels} need {B} clips of "
                         f"{((T - 1) << max(levels, 0)) + 1} slots, got {tuple(slots.shape[:2])}")
    tail = tuple(slots.shape[2:])
    d = L.SynthCutFillDesc()
    d.n0, _, d.s0, d.s1 = _lead_of(slots, tail, "slots")
    d.n1, d.levels, d.nbytes = T, levels, 1
    for n in tail:
        d.nbytes *= n
    if d.nbytes < 1:
        raise ValueError(f"slots: empty dimensions in {tuple(slots.shape)}")
    cuts = cuts.contiguous()
    d.slots, d.cut = slots.data_ptr(), cuts.data_ptr()
    L.check(L.load().dvie_synth_cutfill(ctypes.byref(d), L.stream_ptr(slots.device)), "synth cutfill")
    return slots


class SceneCuts:
    """The two thresholds of scene-cut detection (interpolate(..., scene=)): a neighbouring pair of
    input frames is a cut when its mean absolute luma difference is at least `mad` (0..255) AND its
    32-bin luma histogram distance at least `hist` (0..1); scene_limits turns them into the integers
    the device compares.  The defaults (30, 0.25) are provisional: they have not been validated on
    real footage."""

    def __init__(self, mad=30.0, hist=0.25):
        if not 0 <= mad <= 255 or not 0 <= hist <= 1:
            raise ValueError(f"SceneCuts: mad={mad} must be in 0..255 and hist={hist} in 0..1")
        self.mad, self.hist = float(mad), float(hist)

    def __repr__(self):
        return f"SceneCuts(mad={self.mad}, hist={self.hist})"


MOTION_BLOCK = 16  # samples of a block side of dvie_synth_motion
MOTION_MAX_RADIUS, MOTION_MAX_SCALE, MOTION_MAX_PENALTY = 32, 3, 1024


class MotionSearch:
    """The parameters of the block matching (block_motion, score_*(..., motion=)): every 16 x 16
    block of the luma plane at `scale` (the frame's luma averaged over 2**scale x 2**scale pixels)
    is searched over (dy, dx) in [-radius, radius]^2 of the reference plane, and a candidate costs
    its SAD + penalty * (|dy| + |dx|).  radius in 1..32 (plane samples: radius * 2**scale frame
    pixels), scale in 0..3, penalty in 0..1024, all integers.  The defaults (16, 0, 16) are
    provisional: they have not been validated on real footage."""

    def __init__(self, radius=16, scale=0, penalty=16):
        for name, v, lo, hi in (("radius", radius, 1, MOTION_MAX_RADIUS), ("scale", scale, 0, MOTION_MAX_SCALE),
                                ("penalty", penalty, 0, MOTION_MAX_PENALTY)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"MotionSearch: {name}={v!r} must be an integer in {lo}..{hi}")
        self.radius, self.scale, self.penalty = radius, scale, penalty

    def __repr__(self):
        return f"MotionSearch(radius={self.radius}, scale={self.scale}, penalty={self.penalty})"


def motion_grid(H, W, scale):
    """(bh, bw): the 16 x 16 blocks of the (H >> scale, W >> scale) plane of an (H, W) frame, edge
    blocks included (ValueError when the frame has no sample at that scale)"""
    if not 0 <= scale <= MOTION_MAX_SCALE:
        raise ValueError(f"motion_grid: scale={scale} must be in 0..{MOTION_MAX_SCALE}")
    if H < (1 << scale) or W < (1 << scale):
        raise ValueError(f"motion_grid: a {H}x{W} frame has no sample at scale={scale}")
    return -(-(H >> scale) // MOTION_BLOCK), -(-(W >> scale) // MOTION_BLOCK)


class MotionStats:
    """What block_motion returns: the int64 device tensors `d2`, `sad`, `sad0`, `border`, shaped like
    the leading dimensions of the frames (per pair the sums over its blocks of the winning
    vector's squared length in plane samples, of the winners' SAD, of the SAD at (0, 0), and the
    number of blocks whose winner lies on the border of the search); `blocks` per pair, `samples`
    = blocks * 256 and `scale`; with vectors=True also `mv`, int16 (..., bh, bw, 2) holding
    (dy, dx), and `bsad`, the winner's and the zero SAD (..., bh, bw, 2) (the device's uint32 in
    an int32 tensor: a block SAD is at most 65 280); None otherwise.  rms, residual, residual0
    and saturated are derived on the device in float64."""

    def __init__(self, d2, sad, sad0, border, blocks, scale, mv=None, bsad=None):
        self.d2, self.sad, self.sad0, self.border = d2, sad, sad0, border
        self.blocks, self.samples, self.scale = blocks, blocks * MOTION_BLOCK * MOTION_BLOCK, scale
        self.mv, self.bsad = mv, bsad

    def _over(self, t, n):  # (a tensor divisor: torch turns a division by a Python scalar into a multiplication)
        return t.double() / torch.full_like(t, n, dtype=torch.float64)

    @property
    def rms(self):
        """sqrt(d2 / blocks) * 2**scale: the RMS block displacement in frame pixels"""
        return torch.sqrt(self._over(self.d2, self.blocks)) * float(1 << self.scale)

    @property
    def residual(self):
        """sad / samples: the mean absolute difference after motion compensation, in grey levels"""
        return self._over(self.sad, self.samples)

    @property
    def residual0(self):
        """sad0 / samples: the same without motion compensation"""
        return self._over(self.sad0, self.samples)

    @property
    def saturated(self):
        """border / blocks: the fraction of blocks for which the search may have been too small"""
        return self._over(self.border, self.blocks)


def block_motion(cur, ref, search=None, vectors=False):
    """Block-matching motion statistics of uint8 device frames `cur` (..., H, W, 3) against `ref`
    (the frames frame_scores takes: up to two leading dimensions of any strides -- x[:, 1:] against
    x[:, :-1] of one clip runs in place -- the frame-level dimensions contiguous) -> MotionStats
    shaped like the leading dimensions.  search: a MotionSearch (None: the defaults).
    dvie_synth_motion: the luma planes, the matcher and a finalize launch; exact integers, no host
    synchronisation; include/dvie.h has the definition."""
    search = MotionSearch() if search is None else search
    if not isinstance(search, MotionSearch):
        raise ValueError(f"search: a MotionSearch, got {search!r}")
    lead, H, W, n0, n1, strides = _pairs_of(cur, ref)
    bh, bw = motion_grid(H, W, search.scale)
    d = L.SynthMotionDesc()
    d.cur, d.ref, d.n0, d.n1, d.h, d.w = cur.data_ptr(), ref.data_ptr(), n0, n1, H, W
    d.cur_s0, d.cur_s1, d.ref_s0, d.ref_s1 = strides
    d.radius, d.scale, d.penalty = search.radius, search.scale, search.penalty
    dev = cur.device
    sums = [torch.empty(lead, dtype=torch.int64, device=dev) for _ in range(4)]
    d.d2, d.sad, d.sad0, d.border = (t.data_ptr() for t in sums)
    mv = bsad = None
    if vectors:
        mv = torch.empty(lead + (bh, bw, 2), dtype=torch.int16, device=dev)
        bsad = torch.empty(lead + (bh, bw, 2), dtype=torch.int32, device=dev)
        d.mv, d.bsad = mv.data_ptr(), bsad.data_ptr()
    lib = L.load()
    ws = torch.empty((lib.dvie_synth_motion_ws_bytes(ctypes.byref(d)),), dtype=torch.uint8, device=dev)
    d.ws = ws.data_ptr()
    L.check(lib.dvie_synth_motion(ctypes.byref(d), L.stream_ptr(dev)), "synth motion")
    return MotionStats(*sums, bh * bw, search.scale, mv, bsad)


class MotionScores:
    """The motion columns of score_interpolation / score_extrapolation(..., motion=): four float64
    device tensors (B, len(slots)).  `motion`: MotionStats.rms of the later against the earlier of
    the two original input frames that bracket the slot (extrapolation: of the second against the
    first input frame, the same value at every step), in pixels per input interval; `saturated`:
    the same pairs' MotionStats.saturated; `tres`: the motion-compensated residual of the
    synthesised video across the slot (interpolation: the mean of the residuals of output frame t
    against output frames t - 1 and t + 1; extrapolation: of prediction k against prediction k - 1,
    for k = 0 against the second input frame); `tres_gt`: the same on the originals.  tres -
    tres_gt is the flicker the synthesis added."""
    FIELDS = ("motion", "saturated", "tres", "tres_gt")

    def __init__(self, motion, saturated, tres, tres_gt):
        self.motion, self.saturated, self.tres, self.tres_gt = motion, saturated, tres, tres_gt


RETIME_MAX = 4096  # the largest P and Q of a Retime (dvie_synth_retime's den)
RETIME_MODES = ("nearest", "blend")


class Retime:
    """A frame-rate conversion by the ratio num:den = P:Q (interpolate(..., rate=)): output frame k has
    time k*Q/P in input-frame units.  24 -> 60 Hz is Retime(5, 2), 25 -> 30 Retime(6, 5), 30 -> 25
    Retime(5, 6).  P and Q are positive ints, reduced by their gcd and then at most 4096 each.  mode:
    "nearest" -- an output is a byte copy of the nearest slot of the dyadic grid of `levels`
    doublings, a tie going to the earlier slot (timing error at most 1 / 2**(levels + 1) of an input
    interval) -- or "blend": the rounded integer cross-fade of the two neighbouring slots
    (dvie_synth_retime).  Neither mode has been judged on trained weights and real footage."""

    def __init__(self, num, den, mode="nearest"):
        import math
        for name, v in (("num", num), ("den", den)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"Retime: {name}={v!r} must be a positive int")
        if mode not in RETIME_MODES:
            raise ValueError(f"Retime: mode {mode!r} must be one of {', '.join(RETIME_MODES)}")
        g = math.gcd(num, den)
        self.num, self.den, self.mode = num // g, den // g, mode
        if max(self.num, self.den) > RETIME_MAX:
            raise ValueError(f"Retime: {self.num}:{self.den} (reduced) must not exceed {RETIME_MAX} on either side")

    def __repr__(self):
        return f"Retime({self.num}, {self.den}, mode={self.mode!r})"

    def __eq__(self, other):
        return isinstance(other, Retime) and (self.num, self.den, self.mode) == (other.num, other.den, other.mode)

    def __hash__(self):
        return hash((self.num, self.den, self.mode))


def _retime_check(levels, rate):
    if not isinstance(rate, Retime):
        raise ValueError(f"rate: a Retime or None, got {type(rate).__name__}")
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 0:
        raise ValueError(f"levels={levels!r} must be a non-negative int")
    if rate.num > rate.den << levels:
        need = levels
        while rate.num > rate.den << need:
            need += 1
        raise ValueError(f"rate {rate.num}:{rate.den} puts more than 2**levels = {1 << levels} outputs into an input "
                         f"interval, so outputs would repeat grid slots: raise levels / --synth_levels to at least {need}")


def retime_count(T, rate):
    """The output frames of a T-frame clip at `rate`: those with time k*Q/P <= T - 1 ->
    (T - 1) * P // Q + 1"""
    if T < 1:
        raise ValueError(f"retime_count: T={T} must be at least 1")
    return (T - 1) * rate.num // rate.den + 1


def retime_fps(fps, rate):
    """The frame rate (num, den) of a clip of rate `fps` = (num, den) after `rate`: (num * P, den * Q)
    reduced by their gcd -- (24000, 1001) at 5:2 is (60000, 1001)"""
    import math
    n, d = int(fps[0]) * rate.num, int(fps[1]) * rate.den
    g = math.gcd(n, d) or 1
    return n // g, d // g


class RetimePlan:
    """retime_plan's result.  With S = len(slots) compact slots and N = count outputs:
      T, levels, rate, t0, first   what was planned
      k0, count        the global index of the first emitted output and how many are emitted
      slots            the dense slots (0 .. (T - 1) * 2**levels, input t at t * 2**levels) that exist,
                       ascending; compact index c stands for dense slot slots[c]
      index            {dense slot: compact index}
      in_slots         the compact indices of the T inputs, in order
      levels_c         the pruned schedule: levels of (left, right, out) compact triples, coarsest
                       spacing first, ascending within a level (midpoint_schedule's order)
      keep             frozenset of the compact slots some forward reads
      rows             per output (lo, hi, n, pair, hold) for the frames (dvie_synth_retime's rows)
      label_rows       the same with `nearest` resolved: (s, s, 0, pair, hold)
      input_rows       rows over the window's T INPUTS (slot t = input t) for data that exists per
                       input only, such as packed Y'CbCr frames: a time-aligned output copies its
                       input, every other output is skipped (lo = -1) unless its pair is flagged, when
                       it copies input `hold`
      aligned          [(j, t)]: emitted output j (window-local) is input frame t (window-local)
      forwards, dense_forwards   the forwards of levels_c and of the full 2**levels schedule"""

    def keep_fn(self, s):
        return s in self.keep


def retime_plan(T, levels, rate, t0=0, first=True):
    """Plan the rate conversion of one window of T >= 2 input frames whose first frame has global
    index t0 -> RetimePlan.  Output k (global) has time k*Q/P and, on the window's dense grid of
    `levels` doublings, the position x = k*Q*2**levels/P - t0*2**levels: lo = floor(x) and the
    weight n = (k*Q*2**levels) mod P over P of slot lo + 1 (Python ints throughout: k is unbounded
    on a long stream).  The window emits the outputs with t0 < time <= t0 + T - 1, and time == t0 as
    well when `first` (interpolate_stream's closed-right convention: a later window's first frame
    was emitted by the window before).  "nearest" reads slot lo when 2n <= P and lo + 1 otherwise;
    "blend" reads lo and, when n > 0, lo + 1, and takes its label map by the nearest rule.  An
    output strictly inside input pair p is held, when p is flagged, as the left input if
    time - p <= 1/2 and the right one otherwise.  Only the slots an output reads, the inputs and
    their midpoint ancestors exist; the schedule holds the forwards that write them.
    P > Q * 2**levels: ValueError (raise levels)."""
    _retime_check(levels, rate)
    if isinstance(T, bool) or not isinstance(T, int) or T < 2:
        raise ValueError(f"retime_plan: T={T!r} must be an int of at least 2")
    if isinstance(t0, bool) or not isinstance(t0, int) or t0 < 0:
        raise ValueError(f"retime_plan: t0={t0!r} must be a non-negative int")
    P, Q, step = rate.num, rate.den, 1 << levels
    k0 = -((-t0 * P) // Q) if first else t0 * P // Q + 1
    k1 = (t0 + T - 1) * P // Q  # the last output of the window, inclusive
    outs = []  # (lo, n, near, pair, hold_slot, aligned input or None), dense window-local slots
    need = set(t * step for t in range(T))
    for k in range(k0, k1 + 1):
        g = k * Q * step - t0 * step * P  # x * P, window-local
        lo, n = divmod(g, P)
        near = lo if 2 * n <= P else lo + 1
        if n == 0 and lo % step == 0:
            pair, hold, at = -1, lo, lo // step
        else:
            pair, at = lo // step, None
            hold = pair * step if 2 * (g - pair * step * P) <= step * P else (pair + 1) * step
        outs.append((lo, n, near, pair, hold, at))
        need.update((near,) if rate.mode == "nearest" else ((lo, lo + 1) if n else (lo,)))
    triples = [[] for _ in range(levels)]
    todo = sorted(s for s in need if s % step)
    while todo:  # the midpoint ancestors: slot s of spacing h = lowest set bit is made from s - h and s + h
        s = todo.pop()
        h = s & -s
        for a in (s - h, s + h):
            if a % step and a not in need:
                need.add(a)
                todo.append(a)
    p = RetimePlan()
    p.T, p.levels, p.rate, p.t0, p.first = T, levels, rate, t0, first
    p.k0, p.count = k0, len(outs)
    p.slots = sorted(need)
    p.index = {s: c for c, s in enumerate(p.slots)}
    ix = p.index
    p.in_slots = [ix[t * step] for t in range(T)]
    for s in p.slots:
        if s % step:
            h = s & -s
            triples[levels - h.bit_length()].append((ix[s - h], ix[s + h], ix[s]))
    p.levels_c = [lv for lv in triples if lv]
    p.keep = frozenset(c for lv in p.levels_c for a, b, _ in lv for c in (a, b))
    p.rows, p.label_rows, p.input_rows, p.aligned = [], [], [], []
    for j, (lo, n, near, pair, hold, at) in enumerate(outs):
        if rate.mode == "nearest":
            p.rows.append((ix[near], ix[near], 0, pair, ix[hold]))
        else:
            p.rows.append((ix[lo], ix[lo + 1] if n else ix[lo], n, pair, ix[hold]))
        p.label_rows.append((ix[near], ix[near], 0, pair, ix[hold]))
        if at is not None:
            p.input_rows.append((at, at, 0, -1, at))
            p.aligned.append((j, at))
        else:
            p.input_rows.append((-1, -1, 0, pair, hold // step))
    p.forwards = sum(len(lv) for lv in p.levels_c)
    p.dense_forwards = (T - 1) * (step - 1)
    return p


def retime_gather(slots, rows, den, out, cuts=None):
    """The output frames of a rate conversion, gathered or blended on the device: `slots` uint8
    (B, S, ...) and `out` uint8 (B, N, ...) on one device, any strides over the two leading
    dimensions and the others contiguous and equal (frames, label maps or packed Y'CbCr frames; the
    transposed views of slot-major storage are taken as they are); `rows`: N rows (lo, hi, n, pair,
    hold) of ints (RetimePlan.rows / label_rows / input_rows), uploaded once; `cuts`: bool or uint8
    (B, pairs) on the device, or None.  Output (b, k), in this order: its pair is flagged -> a byte
    copy of slot hold; lo < 0 -> not written; n == 0 -> a byte copy of slot lo; else every byte
    (a * (den - n) + c * n + den // 2) // den of the bytes a, c of slots lo and hi, exact
    (dvie_synth_retime: one launch, the flags read on the device, no host synchronisation).
    N == 0 launches nothing.  -> out"""
    L.require_gpu(slots)
    if slots.dtype != torch.uint8 or slots.dim() < 2 or out.dtype != torch.uint8 or out.dim() != slots.dim() or \
            out.device != slots.device or out.shape[0] != slots.shape[0] or out.shape[2:] != slots.shape[2:]:
        raise ValueError(f"slots: uint8 (B, S, ...) and out: uint8 (B, N, ...) of the same rows on one device, got "
                         f"{tuple(slots.shape)} {slots.dtype} and {tuple(out.shape)} {out.dtype}")
    B, S = slots.shape[:2]
    N = out.shape[1]
    rows = [tuple(int(v) for v in r) for r in rows]
    if len(rows) != N or any(len(r) != 5 for r in rows):
        raise ValueError(f"rows: {N} rows (lo, hi, n, pair, hold), one per output, got {len(rows)}")
    if N == 0:
        return out
    tail = tuple(slots.shape[2:])
    d = L.SynthRetimeDesc()
    d.n0, d.n_slots, d.slot_s0, d.slot_s1 = _lead_of(slots, tail, "slots")
    _, d.n_rows, d.out_s0, d.out_s1 = _lead_of(out, tail, "out")
    d.nbytes, d.den = 1, den
    for n in tail:
        d.nbytes *= n
    if cuts is not None:
        if cuts.dtype not in (torch.bool, torch.uint8) or cuts.dim() != 2 or cuts.device != slots.device or \
                cuts.shape[0] != B:
            raise ValueError(f"cuts: bool (B, pairs) on {slots.device}, got {tuple(cuts.shape)} {cuts.dtype}")
        cuts = cuts.contiguous()
        d.cut, d.n_pairs = cuts.data_ptr(), cuts.shape[1]
    host = (ctypes.c_int32 * (5 * N))(*[v for r in rows for v in r])
    dev = torch.tensor(rows, dtype=torch.int32).to(slots.device)
    d.slots, d.out, d.rows, d.rows_dev = slots.data_ptr(), out.data_ptr(), ctypes.addressof(host), dev.data_ptr()
    L.check(L.load().dvie_synth_retime(ctypes.byref(d), L.stream_ptr(slots.device)), "synth retime")
    return out


def frame_scores(pred, gt, pred_labels=None, gt_labels=None, n_classes=20, perceptual=None, msssim=None):
    """Score uint8 device frames `pred` (..., H, W, 3) against `gt` and, when both are given,
    label maps `pred_labels` (..., H, W) against `gt_labels` (dvie_synth_score: one fused pass
    and a finalize launch, no host synchronisation) -> FrameScores shaped like the leading
    dimensions.  Up to two leading dimensions, of any strides (the (B, S) views interpolate /
    extrapolate return are scored in place); the frame-level dimensions must be contiguous.
    perceptual: a PerceptualScorer -> the result also has `.vgg`, the per-frame VGG19 feature
    cosine on the region vgg_region(H, W) (up to 15 trailing rows and columns are not seen when
    H or W is no multiple of 16; a side below 16 raises ValueError); None: `.vgg` is None.
    msssim: an int K -> the result also has `.msssim`, frame_msssim(pred, gt, K)[0] (ValueError when
    the frames are too small for K scales); None: `.msssim` is None."""
    L.require_gpu(pred)
    if pred.dim() < 3 or pred.shape[-1] != 3:
        raise ValueError(f"pred: uint8 (..., H, W, 3), got {tuple(pred.shape)}")
    lead, (H, W) = tuple(pred.shape[:-3]), pred.shape[-3:-1]
    if H < 1 or W < 1 or any(n < 1 for n in lead):
        raise ValueError(f"pred: empty dimensions in {tuple(pred.shape)}")
    if (pred_labels is None) != (gt_labels is None):
        raise ValueError("pred_labels and gt_labels must be given together")
    has_labels = pred_labels is not None
    if has_labels and not 1 <= n_classes <= 32:
        raise ValueError(f"n_classes={n_classes} must be in 1..32")
    if perceptual is not None:
        vgg_region(H, W)  # (a frame too small for the perceptual score fails before anything runs)
    if msssim is not None:
        msssim_check(H, W, msssim)
    d = L.SynthScoreDesc()
    d.n0, d.n1, d.pred_s0, d.pred_s1 = _lead_of(pred, (H, W, 3), "pred")
    for t, tail, what in ((gt, (H, W, 3), "gt"),) + (((pred_labels, (H, W), "pred_labels"),
                                                       (gt_labels, (H, W), "gt_labels")) if has_labels else ()):
        if not isinstance(t, torch.Tensor) or t.device != pred.device or tuple(t.shape[:t.dim() - len(tail)]) != lead:
            raise ValueError(f"{what}: a tensor on {pred.device} with the leading dimensions {lead} of pred")
        _, _, s0, s1 = _lead_of(t, tail, what)
        setattr(d, what.replace("labels", "label") + "_s0", s0)
        setattr(d, what.replace("labels", "label") + "_s1", s1)
    d.pred, d.gt, d.h, d.w, d.n_classes = pred.data_ptr(), gt.data_ptr(), H, W, n_classes
    dev = pred.device
    i64 = dict(dtype=torch.int64, device=dev)
    out = FrameScores(H, W, torch.empty(lead, **i64), torch.empty(lead, dtype=torch.float64, device=dev))
    d.sse, d.ssim = out.sse.data_ptr(), out.ssim.data_ptr()
    if has_labels:
        d.pred_label, d.gt_label = pred_labels.data_ptr(), gt_labels.data_ptr()
        out.agree, out.valid = torch.empty(lead, **i64), torch.empty(lead, **i64)
        out.inter, out.uni = torch.empty(lead + (n_classes,), **i64), torch.empty(lead + (n_classes,), **i64)
        d.agree, d.valid, d.inter, d.uni = (t.data_ptr() for t in (out.agree, out.valid, out.inter, out.uni))
    lib = L.load()
    ws = torch.empty((lib.dvie_synth_score_ws_bytes(ctypes.byref(d)),), dtype=torch.uint8, device=dev)
    d.ws = ws.data_ptr()
    L.check(lib.dvie_synth_score(ctypes.byref(d), L.stream_ptr(dev)), "synth score")
    if perceptual is not None:
        out.vgg = perceptual(pred, gt)
    if msssim is not None:
        out.msssim = frame_msssim(pred, gt, msssim)[0]
    return out


def motion_bucket_names(edges):
    """the keys of summarize's per_motion rows for the ascending positive `edges`: "0-e0", "e0-e1",
    ..., "e_last-inf" (ValueError for edges that are not ascending positive numbers)"""
    import math
    edges = [float(e) for e in edges]
    if not edges or any(not math.isfinite(e) or e <= 0 for e in edges) or any(a >= b for a, b in zip(edges, edges[1:])):
        raise ValueError(f"edges={edges} must be ascending positive numbers")
    names = ["0"] + [f"{e:g}" for e in edges] + ["inf"]
    return [f"{a}-{b}" for a, b in zip(names, names[1:])]


def summarize(position, psnr, ssim, acc, miou, vgg=None, msssim=None, motion=None, saturated=None, tres=None,
              tres_gt=None, edges=None):
    """Host-side means of per-frame scores (numpy arrays of one length; `position` an integer
    per frame) -> {"psnr", "ssim", "acc", "miou", "frames", "per_position": {position: the same
    four and "frames"}} as Python floats.  The mean PSNR is the mean of the per-frame PSNRs
    (losses.py:103-116); an infinite value stays infinite.  With `vgg` (the per-frame perceptual
    scores) the result and every per_position row also have "vgg", with `msssim` (the per-frame
    multi-scale SSIM) "msssim".  With the per-frame MotionScores columns `motion`, `saturated`,
    `tres` and `tres_gt` they also have those means, and with both `tres` and `tres_gt`
    "tres_excess" = mean(tres - tres_gt), the flicker the synthesis added.  With `edges` (ascending
    positive floats; needs `motion`) the result also has "per_motion": one row with the columns of
    a per_position row per bucket [0, e0), [e0, e1), ..., [e_last, inf) of the per-frame `motion`,
    keyed by motion_bucket_names ("2-8"); empty buckets are omitted."""
    import numpy as np
    position = np.asarray(position)
    cols = dict(psnr=np.asarray(psnr, dtype=np.float64), ssim=np.asarray(ssim, dtype=np.float64),
                acc=np.asarray(acc, dtype=np.float64), miou=np.asarray(miou, dtype=np.float64))
    if vgg is not None:
        cols["vgg"] = np.asarray(vgg, dtype=np.float64)
    if msssim is not None:
        cols["msssim"] = np.asarray(msssim, dtype=np.float64)
    for k, v in (("motion", motion), ("saturated", saturated), ("tres", tres), ("tres_gt", tres_gt)):
        if v is not None:
            cols[k] = np.asarray(v, dtype=np.float64)
    if tres is not None and tres_gt is not None:
        cols["tres_excess"] = cols["tres"] - cols["tres_gt"]
    if edges is not None and motion is None:
        raise ValueError("summarize: edges needs the per-frame motion")

    def means(sel):
        with np.errstate(invalid="ignore"):
            row = {k: float(np.mean(v[sel])) for k, v in cols.items()}
        row["frames"] = int(np.count_nonzero(sel))
        return row

    out = means(np.ones(position.shape, dtype=bool))
    out["per_position"] = {int(p): means(position == p) for p in sorted(set(position.tolist()))}
    if edges is not None:
        names = motion_bucket_names(edges)
        bucket = np.searchsorted(np.asarray(edges, dtype=np.float64), cols["motion"], side="right")  # e belongs to [e, next)
        out["per_motion"] = {names[b]: means(bucket == b) for b in range(len(names)) if np.any(bucket == b)}
    return out


class SynthScores:
    """What score_interpolation / score_extrapolation return: `slots`, the scored time indices
    (interpolation: indices into the clip; extrapolation: the step index k of original frame
    2 + k); `scores`, the FrameScores of shape (B, len(slots)), whose tensors and derived
    values are also attributes here (sse, ssim, agree, valid, inter, uni, psnr, acc, miou, vgg
    when a PerceptualScorer was passed and msssim when a number of scales was);
    `frames` / `labels`, the synthesised video as interpolate / extrapolate returns it;
    `positions`, per slot the position the summary groups by (slot % 2**levels, or the step);
    `motion`, the MotionScores when a MotionSearch was passed, None otherwise."""

    def __init__(self, slots, positions, scores, frames, labels, motion=None):
        self.slots, self.positions, self.scores, self.frames, self.labels = list(slots), list(positions), scores, frames, labels
        self.motion = motion

    def __getattr__(self, name):
        if name in FrameScores.FIELDS or name in ("psnr", "acc", "miou"):
            return getattr(self.scores, name)
        raise AttributeError(name)

    def host(self, vgg=False, msssim=False, motion=False):
        """psnr, ssim, acc, miou -- with vgg=True also vgg (scored with a PerceptualScorer), with
        msssim=True also msssim (scored with msssim=K), with motion=True also motion, saturated,
        tres and tres_gt (scored with motion=), each after the others -- as float64 numpy
        arrays (B, len(slots)): one copy to the host"""
        s = self.scores
        if motion and self.motion is None:
            raise ValueError("these scores have no motion columns (score_* was called without motion=)")
        if vgg and s.vgg is None:
            raise ValueError("these scores have no vgg column (score_* was called without perceptual=)")
        if msssim and s.msssim is None:
            raise ValueError("these scores have no msssim column (score_* was called without msssim=)")
        return tuple(torch.stack([s.psnr, s.ssim, s.acc, s.miou] + ([s.vgg] if vgg else [])
                                 + ([s.msssim] if msssim else [])
                                 + ([getattr(self.motion, k) for k in MotionScores.FIELDS] if motion else [])).cpu().numpy())

    def summary(self):
        """Means over all scored frames and per position (summarize) as Python floats -- the
        one place that copies to the host.  "vgg", "msssim" and the motion columns (with
        "tres_excess") are included when the scores have them."""
        import numpy as np
        extra = [k for k in ("vgg", "msssim") if getattr(self.scores, k) is not None]
        cols = self.host(**{k: True for k in extra}, motion=self.motion is not None)
        names = extra + (list(MotionScores.FIELDS) if self.motion is not None else [])
        pos = np.broadcast_to(np.asarray(self.positions), cols[0].shape)
        return summarize(pos.ravel(), *[c.ravel() for c in cols[:4]],
                         **{k: c.ravel() for k, c in zip(names, cols[4:])})


class FrameSizeError(ValueError):
    """a frame size that VideoSynthesizer cannot run: no multiple of the net's stride with pad=None,
    or (too_large) a forward of more than max_pixels pixels, which tile= cuts into smaller ones"""
    too_large = False


class _Captured:
    """One forward (every stage of it; with an ensemble every member's, with the flips and the
    accumulates between them) + finish of a fixed (n, H, W) as a hipGraph over static tensors: one
    single-stream chain either way.  With a padded canvas (H, W) is the canvas and `crop` the (h, w) of the frames that
    leave: the static frame and label have the cropped size, and the label canvas is static too."""

    def __init__(self, syn, n, H, W, dev, crop=None):
        f32, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
        h, w = crop or (H, W)
        self.xa, self.xb = torch.zeros((n, H, W, 8), **f32), torch.zeros((n, H, W, 8), **f32)
        self.la, self.lb = torch.zeros((n, H, W), **u8), torch.zeros((n, H, W), **u8)
        self.rgb = torch.empty((n, H, W, 8), **f32)
        self.frame, self.label = torch.empty((n, h, w, 3), **u8), torch.empty((n, h, w), **u8)
        self.lcan = torch.empty((n, H, W), **u8) if crop else None
        self.plans = syn._plans(n, H, W, dev)
        syn._scratch_of(n, H, W, dev)  # (allocated here, on the caller's stream, not in the warm-up)
        for p in self.plans:
            p.busy = True  # the graph holds these plans' pointers: nobody else gets them from the pool
        args = (self.plans, self.xa, self.xb, self.la, self.lb, self.rgb, self.frame, self.label, self.lcan)
        side = torch.cuda.Stream(dev)  # warm-up on a side stream, as stream capture requires
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            syn._run(*args)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):  # a single-stream chain: the forward list, then finish
            syn._run(*args)

    def __call__(self, xa, xb, la, lb, rgb, frame, label, lcan=None):
        for dst, src in ((self.xa, xa), (self.xb, xb), (self.la, la), (self.lb, lb)):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        for dst, src in ((rgb, self.rgb), (frame, self.frame), (label, self.label)) + \
                (((lcan, self.lcan),) if lcan is not None else ()):
            dst.copy_(src, non_blocking=True)


class VideoSynthesizer:
    """interpolate / extrapolate uint8 device video with a trained coarse or two-stage net.

    net: nets.InterNet / ExtraNet, InterRefineNet / ExtraRefineNet (+ SRNRefine) or
    InterStage3Net / ExtraStage3Net (+ SRNRefine + MSResAttnRefine, any n_scales, stage3_prop
    on or off) over HRNet (either highres_large setting), one predicted frame per forward
    (num_pred_once 1, no fix_init_frames / inpaint_mask); it is put in eval mode.  The frame
    returned and fed back is the last stage's finest image (module docstring); the label comes
    from the coarse logits.  GAN and VAE nets and a bare HRNet raise ValueError.  max_batch:
    frame pairs per forward.  graph: replay one captured hipGraph per forward (built per
    (n, H, W) at first use; call reset() after the net's parameters were moved or replaced).
    pad: None -- H and W must be multiples of `multiple` (ValueError otherwise); "replicate" --
    any H, W >= 1: the frames sit at the top-left of a canvas of canvas(H, W), whose other rows
    and columns repeat an input frame's (and its label map's) last row and column.  The canvas
    persists through the rollout: a prediction is the network's raw output over the whole canvas,
    its label canvas the argmax over the whole canvas, and both feed later forwards as they are
    (the pad region is not re-replicated).  What is returned is cropped to (H, W), so the result
    equals padding the uint8 inputs, running pad=None on the canvas and cropping.
    tile: None -- every forward covers the whole canvas; (th, tw), multiples of `multiple` -- a
    canvas larger than that in either direction is cut into overlapping tiles of one shape
    (tile_starts per axis, `tiles`), every forward runs on one tile of the chunk's pairs, and
    tile_blend cross-fades the tiles' raw images and coarse logits over the overlaps into the
    frame, the label and the kept fp32 form (the crop of a padded canvas included).  overlap: the
    least number of rows / columns neighbouring tiles share, a multiple of `multiple` in
    0..min(th, tw) // 2 and at most 256 (64 is provisional: unvalidated on trained weights).  A
    canvas that fits one tile runs exactly as with tile=None.  A tiled frame approximates the
    untiled one: the net's receptive field is wider than any overlap, and a tile's inner borders
    see zero padding.  A forward of more than `max_pixels` pixels raises FrameSizeError before
    anything is launched.
    ensemble: None -- one forward per prediction; "time", "flip" or "time+flip" -- test-time
    self-ensembling: every forward runs once per member of ensemble_members(ensemble) (the inputs
    in exchanged roles, mirrored along W over the extent the forward runs on -- the canvas, the
    tile -- or both), the mirrored outputs are mirrored back, and the raw image and the coarse
    logits become the fp32 means (((x0 + x1) + x2) + x3) * (1 / M); the frame, the label and what
    later levels read come from the means.  M forwards per predicted frame.  An Extra net takes
    only "flip" (ValueError: extrapolation has no time symmetry).  Its effect on quality has not
    been measured on trained weights."""

    def __init__(self, net, max_batch=8, graph=False, pad=None, tile=None, overlap=64, ensemble=None):
        from .nets.ExtraNet import ExtraNet, ExtraRefineNet, ExtraStage3Net
        from .nets.HRNet import HRNet
        from .nets.InterNet import InterNet
        from .nets.InterRefineNet import InterRefineNet, InterStage3Net
        from .nets.refine import MSResAttnRefine, SRNRefine
        n_stages = {InterNet: 0, ExtraNet: 0, InterRefineNet: 1, ExtraRefineNet: 1, InterStage3Net: 2,
                    ExtraStage3Net: 2}.get(type(net))
        if n_stages is None or type(getattr(net, "coarse_model", None)) is not HRNet:
            raise ValueError(f"VideoSynthesizer runs the coarse and two-stage Inter / Extra nets over HRNet, not "
                             f"{type(net).__name__} (GAN and VAE nets are out of scope)")
        if (n_stages >= 1 and type(net.refine_model) is not SRNRefine) or \
                (n_stages == 2 and type(net.stage3_model) is not MSResAttnRefine):
            raise ValueError("VideoSynthesizer runs SRNRefine and MSResAttnRefine as the second and third stage")
        # [SRNRefine][MSResAttnRefine]: the stages after the coarse model
        self.stages = [getattr(net, name) for name in ("refine_model", "stage3_model")[:n_stages]]
        cm = net.coarse_model
        if cm.npo != 1 or cm.fix_init or cm.inpaint_mask or cm.n_frames != 2:
            raise ValueError("VideoSynthesizer needs one predicted frame from two (num_pred_once 1, no "
                             "fix_init_frames / inpaint_mask)")
        assert max_batch >= 1
        if pad not in (None, "replicate"):
            raise ValueError(f'pad must be None or "replicate", got {pad!r}')
        self.pad = pad
        self.members = ensemble_members(ensemble)  # (ValueError for an unknown setting)
        if any(swap for swap, _ in self.members) and isinstance(net, (ExtraNet, ExtraRefineNet, ExtraStage3Net)):
            raise ValueError(f'ensemble={ensemble!r}: extrapolation has no time symmetry (the frame after (a, b) is not '
                             f'the frame after (b, a)); an Extra net takes ensemble=None or "flip"')
        self.ensemble = ensemble
        net.eval()
        self.net, self.cm, self.max_batch, self.graph = net, cm, int(max_batch), bool(graph)
        self._scratch = {}  # (n, H, W, device) -> the scratch tensors of a forward
        self._graphs = {}
        self.retime_last = None  # the RetimePlan of the last interpolate(..., rate=)
        self._tile_scratch = {}  # (n, th, tw, tiles, device) -> the tile inputs and the stash of a tiled forward
        self._max_pixels = None
        self.tile, self.overlap = None, 0
        if tile is not None:
            m = self.multiple
            if not isinstance(tile, (tuple, list)) or len(tile) != 2 or \
                    any(not isinstance(v, int) or isinstance(v, bool) or v < m or v % m for v in tile):
                raise ValueError(f"tile must be None or (th, tw), positive multiples of the net's multiple {m}, got {tile!r}")
            tile_starts(min(tile), min(tile), overlap, m)  # (the overlap rules, for the smaller side)
            self.tile, self.overlap = (int(tile[0]), int(tile[1])), int(overlap)

    def reset(self):
        """drop the captured graphs and scratch (after net.to(...) or a load that re-allocates)"""
        for c in self._graphs.values():
            for p in c.plans:
                p.busy = False
        self._graphs, self._scratch, self._tile_scratch = {}, {}, {}

    @property
    def multiple(self):
        """what H and W of a forward must be multiples of: the net's coarsest stride (HRNet 4, 8
        with highres_large; a refinement stage 4 << (n_scales - 1))"""
        return max([8 if self.cm.highres_large else 4] + [4 << (s.n_scales - 1) for s in self.stages])

    def canvas(self, H, W):
        """(Hp, Wp) of the canvas an (H, W) frame is synthesised on when pad is "replicate": both
        rounded up to `multiple`"""
        return canvas_size(H, W, self.multiple)

    def tile_grid(self, H, W):
        """(ys, xs, th, tw): the tile starts per axis of the canvas of an (H, W) frame and the one
        shape of its tiles; ([0], [0], Hp, Wp) without tile= or when the canvas fits one tile"""
        Hp, Wp = self.canvas(H, W) if self.pad else (H, W)
        if self.tile is None:
            return [0], [0], Hp, Wp
        m = self.multiple
        ys, th = tile_starts(Hp, self.tile[0], self.overlap, m)
        xs, tw = tile_starts(Wp, self.tile[1], self.overlap, m)
        return ys, xs, th, tw

    def tiles(self, H, W):
        """the tiles [(y0, x0, th, tw)] of the canvas of an (H, W) frame in row-major order: one
        shape for all of them (one plan serves them); one tile, the canvas, when it fits"""
        ys, xs, th, tw = self.tile_grid(H, W)
        return [(y0, x0, th, tw) for y0 in ys for x0 in xs]

    RANGE_BYTES = 0xFFFFFF00  # the conv kernels address one image of a map through a 32-bit buffer range

    @property
    def max_pixels(self):
        """The largest Hp * Wp of one forward: one image of the widest activation of the net's
        plans, at the net's precision, must stay below RANGE_BYTES (dvie_conv2d_fwd's rule).  The
        widths come from a dry lowering of every stage at a small size: per buffer its bytes per
        pixel of the full-resolution frame.  HRNet's stacked head buffer is not counted: the
        lowering splits it in two where it would exceed the range (HRNet._heads)."""
        if self._max_pixels is None:
            from fractions import Fraction
            m = self.multiple * 4
            graphs = [self.cm._lower(E.Graph(self.cm.dtype), m, m, dry=True, labels=True)]
            for st in self.stages:
                g = E.Graph(st.dtype)
                st._lower(g, m, m, False, True)
                graphs.append(g)
            widest = Fraction(0)
            for g in graphs:
                for b in g.buffers:
                    if b.name == "heads_hidden":
                        continue
                    es = 2 if (b.dtype or g.dtype) == torch.bfloat16 else 4
                    widest = max(widest, Fraction(b.H * b.W * b.C * es, m * m))
            self._max_pixels = int((self.RANGE_BYTES - 1) / widest)
        return self._max_pixels

    def _check_size(self, H, W):
        """FrameSizeError (too_large) when a forward of an (H, W) frame -- its tile, or the whole
        canvas -- has more than max_pixels pixels"""
        _, _, th, tw = self.tile_grid(H, W)
        if th * tw > self.max_pixels:
            what = f"a tile of {th}x{tw}" if self.tile is not None else f"the {th}x{tw} canvas of a {H}x{W} frame"
            e = FrameSizeError(f"{what} is a forward of {th * tw} pixels, more than max_pixels = {self.max_pixels} (one "
                               f"image of the net's widest activation must stay below {self.RANGE_BYTES:#x} bytes): pass "
                               f"tile=(th, tw) with th * tw <= {self.max_pixels} to synthesise the frame in tiles")
            e.too_large = True
            raise e

    # ---------------- one forward ----------------
    def _plans(self, n, H, W, dev):
        """the plans of an (n, H, W) forward: the coarse HRNet plan (exporting its stem features
        when a refinement stage follows), then the stages' inference plans"""
        coarse = self.cm._pool.acquire((n, H, W, self.cm.dtype, False, dev, False, bool(self.stages), _PLAN_FLAGS))
        return [coarse] + [m.infer_plan(n, H, W, dev) for m in self.stages]

    def _scratch_of(self, n, H, W, dev):
        """the scratch of an (n, H, W) forward: the coarse segmentation logits and, with
        refinement stages, the stem features and the image of every stage but the last"""
        key = (n, H, W, dev)
        if key not in self._scratch:
            f32 = dict(dtype=torch.float32, device=dev)
            sc = {"seg": torch.empty((n, H, W, E.rup(self.cm.seg_out_dim, 8)), **f32)}
            if self.stages:
                sc["stem"] = torch.empty((n, 7 * self.cm.n_frames, H, W), **f32)
                sc["img"] = [torch.empty((n, H, W, 8), **f32) for _ in self.stages]
            if self.ensemble is not None:
                # a later member's raw image and logits (32 + 96 B per pixel and pair) and, for a
                # mirrored member, the mirrors of the four inputs (2 * 32 + 2 B)
                sc["ens_rgb"], sc["ens_seg"] = torch.empty((n, H, W, 8), **f32), torch.empty_like(sc["seg"])
                if any(flip for _, flip in self.members):
                    u8 = dict(dtype=torch.uint8, device=dev)
                    sc["ens_x"] = [torch.empty((n, H, W, 8), **f32) for _ in range(2)]
                    sc["ens_l"] = [torch.empty((n, H, W), **u8) for _ in range(2)]
            self._scratch[key] = sc
        return self._scratch[key]

    def _run(self, plans, xa, xb, la, lb, rgb, frame, label, lcan=None):
        """rgb (fp32, raw), frame, label <- net(xa, xb | la, lb); every tensor a contiguous
        (n, H, W, ...) block (the inputs may be strided over n).  On a padded canvas frame and
        label are (n, h, w, ...), the crop, and lcan (or None) gets the label canvas (n, H, W).
        With an ensemble rgb and the coarse logits are the members' means (_run_members)."""
        n, H, W, _ = rgb.shape
        sc = self._scratch_of(n, H, W, rgb.device)
        seg = sc["seg"]
        if self.ensemble is None:
            self._forward(plans, sc, xa, xb, la, lb, rgb, seg)
        else:
            self._run_members(plans, sc, xa, xb, la, lb, rgb, seg)
        if frame is None:  # (a tile of a tiled forward: tile_blend finishes the canvas)
            return
        if frame.shape[1:3] == (H, W):
            synth_finish(rgb, seg, frame, label, n_classes=self.cm.n_classes)
        else:
            synth_finish_crop(rgb, seg, frame, label, lcan, n_classes=self.cm.n_classes)

    def _run_members(self, plans, sc, xa, xb, la, lb, rgb, seg):
        """The members of the ensemble in order, each a complete forward (its bridges read its own
        coarse image and logits): a swapped member reads the inputs in exchanged roles, a mirrored
        one their synth_flip copies.  Member 0, the plain forward, writes rgb and seg themselves;
        every later one writes the ens_* scratch and synth_ens_acc adds it (read mirrored back),
        the last one scaling by 1 / M and zeroing the padding channels: rgb and seg end as
        (((x0 + x1) + x2) + x3) * (1 / M)."""
        M = len(self.members)
        for m, (swap, flip) in enumerate(self.members):
            a, b, sa, sb = (xb, xa, lb, la) if swap else (xa, xb, la, lb)
            if flip:
                (fa, fb), (fla, flb) = sc["ens_x"], sc["ens_l"]
                a, sa = synth_flip(a, sa, fa, fla), fla
                b, sb = synth_flip(b, sb, fb, flb), flb
            if m == 0:
                assert not swap and not flip
                self._forward(plans, sc, a, b, sa, sb, rgb, seg)
                continue
            self._forward(plans, sc, a, b, sa, sb, sc["ens_rgb"], sc["ens_seg"])
            synth_ens_acc(sc["ens_rgb"], sc["ens_seg"], rgb, seg, flip=flip, last_m=M if m == M - 1 else 0,
                          n_classes=self.cm.n_classes)

    def _forward(self, plans, sc, xa, xb, la, lb, rgb, seg):
        """one forward of every stage: the raw image of the last stage into rgb, the coarse logits
        into seg"""
        imgs = sc.get("img", []) + [rgb]  # the image each plan writes: the last one is the prediction
        xs = [xa.permute(0, 3, 1, 2)[:, :3], xb.permute(0, 3, 1, 2)[:, :3]]
        plan = plans[0]
        plan.set_input_parts("x", xs)
        plan.set_input_labels("seg", [la, lb])
        plan.set_output("rgb", imgs[0])
        plan.set_output("segout", seg)
        if self.stages:
            F, stem = self.cm.n_frames, sc["stem"]
            plan.set_output_nchw("stem_x", stem[:, :3 * F])
            for k in range(F):
                plan.set_output_nchw(f"stem_seg{k}", stem[:, 3 * F + 4 * k:3 * F + 4 * k + 4])
        plan.run_forward()
        for k, plan in enumerate(plans[1:]):
            synth_bridge(imgs[k], seg, plan.input_view("bridge"))
            if k == 0:  # SRNRefine: the stem features [frames, seg_encoder(seg_k)]
                plan.set_input("enc", sc["stem"])
                plan.set_output_nchw("pred", imgs[k + 1].permute(0, 3, 1, 2))
            else:  # MSResAttnRefine: the two input frames and their label maps as neighbours
                plan.set_input_parts("nimg", xs)
                plan.set_input_labels("nseg", [la, lb])
                plan.set_output_nchw("out", imgs[k + 1].permute(0, 3, 1, 2))
            plan.run_forward()

    def _tile_scratch_of(self, n, th, tw, nt, dev):
        """the reused scratch of a tiled forward of n pairs: the tile crops of the four inputs, the
        stash of every tile's raw rgb and coarse logits and, for graph replay, the tile's unused
        uint8 outputs"""
        key = (n, th, tw, nt, dev)
        if key not in self._tile_scratch:
            f32, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
            sc = {"xa": torch.empty((n, th, tw, 8), **f32), "xb": torch.empty((n, th, tw, 8), **f32),
                  "la": torch.empty((n, th, tw), **u8), "lb": torch.empty((n, th, tw), **u8),
                  "rgb": torch.empty((nt, n, th, tw, 8), **f32),
                  "seg": torch.empty((nt, n, th, tw, E.rup(self.cm.seg_out_dim, 8)), **f32)}
            if self.graph:
                sc["frame"], sc["label"] = torch.empty((n, th, tw, 3), **u8), torch.empty((n, th, tw), **u8)
            self._tile_scratch[key] = sc
        return self._tile_scratch[key]

    def _pair(self, xa, xb, la, lb, rgb, frame, label, lcan=None, keep=True):
        """one forward of n pairs over the canvas of `rgb`; keep: a later forward reads rgb (a
        tiled forward writes it only then)"""
        n, H, W, _ = rgb.shape
        if self.tile is not None and (H > self.tile[0] or W > self.tile[1]):
            return self._pair_tiled(xa, xb, la, lb, rgb, frame, label, lcan, keep)
        return self._pair_whole(xa, xb, la, lb, rgb, frame, label, lcan)

    def _pair_tiled(self, xa, xb, la, lb, rgb, frame, label, lcan, keep):
        """the forward per tile on crops of the input canvases, every tile's raw rgb and coarse
        logits collected in the stash, then one tile_blend over the canvas"""
        n, H, W, _ = rgb.shape
        ys, xs, th, tw = self.tile_grid(H, W)  # ((H, W) is the canvas: its own canvas)
        sc = self._tile_scratch_of(n, th, tw, len(ys) * len(xs), rgb.device)
        t = 0
        for y0 in ys:
            for x0 in xs:
                for dst, src in ((sc["xa"], xa), (sc["xb"], xb), (sc["la"], la), (sc["lb"], lb)):
                    dst.copy_(src[:, y0:y0 + th, x0:x0 + tw])
                self._pair_whole(sc["xa"], sc["xb"], sc["la"], sc["lb"], sc["rgb"][t], sc.get("frame"), sc.get("label"))
                sc["seg"][t].copy_(self._scratch_of(n, th, tw, rgb.device)["seg"])
                t += 1
        tile_blend(sc["rgb"], sc["seg"], ys, xs, self.overlap, frame, label, rgb if keep else None, lcan,
                   n_classes=self.cm.n_classes)

    def _pair_whole(self, xa, xb, la, lb, rgb, frame, label, lcan=None):
        n, H, W, _ = rgb.shape
        if not self.graph:
            return self._run(self._plans(n, H, W, rgb.device), xa, xb, la, lb, rgb, frame, label, lcan)
        crop = tuple(frame.shape[1:3]) if frame.shape[1:3] != (H, W) else ()
        key = (n, H, W, rgb.device) + crop
        if key not in self._graphs:
            self._graphs[key] = _Captured(self, n, H, W, rgb.device, crop)
        self._graphs[key](xa, xb, la, lb, rgb, frame, label, lcan)

    # ---------------- clips ----------------
    def _check(self, frames, labels):
        L.require_gpu(frames)
        if frames.dtype != torch.uint8 or labels.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 \
                or labels.shape != frames.shape[:4] or labels.device != frames.device:
            raise ValueError("frames: uint8 (B, T, H, W, 3), labels: uint8 (B, T, H, W), on one device; got "
                             f"{tuple(frames.shape)} {frames.dtype}, {tuple(labels.shape)} {labels.dtype}")
        m = self.multiple
        if self.pad is None and (frames.shape[2] % m or frames.shape[3] % m):
            raise FrameSizeError(f"H and W must be multiples of {m}, got {tuple(frames.shape[2:4])}")
        if frames.shape[2] < 1 or frames.shape[3] < 1:
            raise ValueError(f"H and W must be at least 1, got {tuple(frames.shape[2:4])}")
        self._check_size(frames.shape[2], frames.shape[3])

    def chunks(self, triples, B):
        """The forwards of one level: its pairs (triple, clip), triples in order and the clips
        of a triple together, cut into chunks of at most max_batch.  -> [[(left, right, out,
        b0, b1)]]: a chunk is a list of pieces, one per triple it touches, of clips b0:b1.
        With B >= max_batch (or one triple) every chunk is one piece."""
        if B >= self.max_batch or len(triples) == 1:
            return [[(a, b, o, b0, min(B, b0 + self.max_batch))] for a, b, o in triples
                    for b0 in range(0, B, self.max_batch)]
        out, cur, room = [], [], self.max_batch
        for a, b, o in triples:
            b0 = 0
            while b0 < B:
                n = min(room, B - b0)
                cur.append((a, b, o, b0, b0 + n))
                b0, room = b0 + n, room - n
                if room == 0:
                    out.append(cur)
                    cur, room = [], self.max_batch
        return out + ([cur] if cur else [])

    def _roll(self, frames, labels, n_slots, in_slots, levels, keep):
        """The slot-major state, the input frames placed and loaded, then the levels (lists of
        (left, right, out) triples) run in order.  keep(slot): a later forward reads the slot,
        so its fp32 form is kept (other predictions go through one scratch block).  On a padded
        canvas (pad="replicate", H or W no multiple) the fp32 forms are canvases, a kept slot
        also keeps its label canvas, and the public fr / lb stay (H, W): load_pad fills both
        canvases of an input slot, finish_crop writes the crop and the label canvas."""
        B, _, H, W, _ = frames.shape
        dev = frames.device
        Hp, Wp = self.canvas(H, W) if self.pad else (H, W)
        padded = (Hp, Wp) != (H, W)
        u8 = dict(dtype=torch.uint8, device=dev)
        with torch.no_grad():
            fr = torch.empty((n_slots, B, H, W, 3), **u8)
            lb = torch.empty((n_slots, B, H, W), **u8)
            for t, s in enumerate(in_slots):  # the originals pass through bit for bit
                fr[s].copy_(frames[:, t])
                lb[s].copy_(labels[:, t])
            res = {s: torch.empty((B, Hp, Wp, 8), dtype=torch.float32, device=dev) for s in range(n_slots) if keep(s)}
            # lc[s]: the label map of slot s as a forward reads it -- lb[s] itself, or its canvas
            lc = {s: torch.empty((B, Hp, Wp), **u8) for s in res} if padded else lb
            tmp = torch.empty((self.max_batch, Hp, Wp, 8), dtype=torch.float32, device=dev)
            tfr = tlb = tlc = None
            for s in in_slots:
                if s in res:
                    if padded:
                        synth_load_pad(fr[s], lb[s], res[s], lc[s])
                    else:
                        synth_load(fr[s], res[s])
            for triples in levels:
                for chunk in self.chunks(triples, B):
                    if len(chunk) == 1:  # one triple: its slots are contiguous blocks, used in place
                        a, b, o, b0, b1 = chunk[0]
                        rgb = res[o][b0:b1] if o in res else tmp[:b1 - b0]
                        self._pair(res[a][b0:b1], res[b][b0:b1], lc[a][b0:b1], lc[b][b0:b1], rgb, fr[o, b0:b1],
                                   lb[o, b0:b1], lc[o][b0:b1] if padded and o in res else None, keep=o in res)
                        continue
                    # several triples: gather their frames, run one forward, scatter its outputs
                    n = sum(b1 - b0 for *_, b0, b1 in chunk)
                    if tfr is None:
                        tfr = torch.empty((self.max_batch, H, W, 3), **u8)
                        tlb = torch.empty((self.max_batch, H, W), **u8)
                        tlc = torch.empty((self.max_batch, Hp, Wp), **u8) if padded else None
                    xa = torch.cat([res[a][b0:b1] for a, _, _, b0, b1 in chunk])
                    xb = torch.cat([res[b][b0:b1] for _, b, _, b0, b1 in chunk])
                    la = torch.cat([lc[a][b0:b1] for a, _, _, b0, b1 in chunk])
                    lb2 = torch.cat([lc[b][b0:b1] for _, b, _, b0, b1 in chunk])
                    kept = padded and any(o in res for _, _, o, _, _ in chunk)
                    self._pair(xa, xb, la, lb2, tmp[:n], tfr[:n], tlb[:n], tlc[:n] if kept else None,
                               keep=any(o in res for _, _, o, _, _ in chunk))
                    k = 0
                    for _, _, o, b0, b1 in chunk:
                        m = b1 - b0
                        fr[o, b0:b1].copy_(tfr[k:k + m])
                        lb[o, b0:b1].copy_(tlb[k:k + m])
                        if o in res:
                            res[o][b0:b1].copy_(tmp[k:k + m])
                            if padded:
                                lc[o][b0:b1].copy_(tlc[k:k + m])
                        k += m
        return fr, lb

    def interpolate(self, frames, labels, levels=1, scene=None, rate=None, t0=0, first=True):
        """frames (B, T, H, W, 3), labels (B, T, H, W), uint8 on the device -> frames
        (B, (T - 1) * 2**levels + 1, H, W, 3) and labels of the same length (uint8, views of
        slot-major storage): the inputs unchanged at the multiples of 2**levels, between them
        the predictions of midpoint_schedule(T, levels).  A predicted frame enters the next
        level as the network's raw fp32 output and with its argmax label.

        scene: a SceneCuts -> (frames, labels, cuts): scene_cuts of the (H, W) input frames (never
        of the padded canvas), the same rollout -- the forwards of a flagged pair run like every
        other, so the batches, the captured graphs and the absence of host synchronisation are
        what they are without it -- and then cut_fill of the frames and of the label maps: the
        slots between a flagged pair are byte copies of the nearer input frame and label map, the
        midpoint the left one's.  cuts: bool (B, T - 1) on the device.  None: two results, and
        nothing of the above runs.

        rate: a Retime -> frames (B, N, H, W, 3) and labels (B, N, H, W) at the output clock of
        retime_plan(T, levels, rate, t0, first): the N = plan.count outputs the window emits (t0:
        the global index of frames[:, 0]; first: whether the output at time t0 belongs to it), N = 0
        included.  Only the plan's compact slots are rolled out (plan.forwards forwards instead of
        plan.dense_forwards); two retime_gather launches then write the frames (plan.rows) and the
        label maps (plan.label_rows).  With scene, scene_cuts of the inputs is taken as above and
        the gathers read the flags on the device: an output strictly inside a flagged pair is the
        nearer input's frame and label map (no cut_fill runs), and cuts (B, T - 1) is returned as the
        third result.  The plan of the last such call stays in `retime_last`.  t0 or first without
        rate: ValueError.  None: everything above is what it was."""
        self._check(frames, labels)
        T = frames.shape[1]
        if T < 2 or levels < 0:
            raise ValueError("interpolate needs at least two frames and levels >= 0")
        if rate is None and (t0 != 0 or first is not True):
            raise ValueError("interpolate: t0 and first place a window on the output clock of rate=; without a rate "
                             "they have no meaning")
        if rate is not None:
            return self._interpolate_rate(frames, labels, levels, scene, rate, t0, first)
        if scene is not None:
            if not isinstance(scene, SceneCuts):
                raise ValueError(f"scene: a SceneCuts or None, got {type(scene).__name__}")
            cuts = scene_cuts(frames, scene.mad, scene.hist)
            out_f, out_l = self.interpolate(frames, labels, levels)
            cut_fill(out_f, cuts, levels)
            cut_fill(out_l, cuts, levels)
            return out_f, out_l, cuts
        sched = midpoint_schedule(T, levels)
        step = 1 << levels
        n_slots = (T - 1) * step + 1
        # the last level's predictions (the odd slots) are read by no forward
        fr, lb = self._roll(frames, labels, n_slots, [t * step for t in range(T)], sched,
                            keep=lambda s: levels > 0 and s % 2 == 0)
        return fr.transpose(0, 1), lb.transpose(0, 1)

    def _interpolate_rate(self, frames, labels, levels, scene, rate, t0, first):
        """interpolate(..., rate=): the plan, the flags, the pruned rollout, the two gathers"""
        B, T, H, W, _ = frames.shape
        plan = retime_plan(T, levels, rate, t0, first)
        if scene is not None and not isinstance(scene, SceneCuts):
            raise ValueError(f"scene: a SceneCuts or None, got {type(scene).__name__}")
        cuts = scene_cuts(frames, scene.mad, scene.hist) if scene is not None else None
        self.retime_last = plan
        N = plan.count
        out_f = torch.empty((N, B, H, W, 3), dtype=torch.uint8, device=frames.device).transpose(0, 1)
        out_l = torch.empty((N, B, H, W), dtype=torch.uint8, device=frames.device).transpose(0, 1)
        if N:
            fr, lb = self._roll(frames, labels, len(plan.slots), plan.in_slots, plan.levels_c, keep=plan.keep_fn)
            retime_gather(fr.transpose(0, 1), plan.rows, rate.num, out_f, cuts)
            retime_gather(lb.transpose(0, 1), plan.label_rows, rate.num, out_l, cuts)
        return (out_f, out_l) if scene is None else (out_f, out_l, cuts)

    def interpolate_stream(self, chunks, levels=1, scene=None, rate=None):
        """interpolate() of a clip of any length in bounded memory: a generator over `chunks`, any
        iterable of (frames (B, t, H, W, 3), labels (B, t, H, W)) uint8 device tensors with t >= 1,
        the clip in order.  The last input frame of a chunk (its uint8 frame and label map) is
        carried to the next; whenever carry + chunk holds at least two frames it goes through
        interpolate(), and the result is yielded -- without its first slot when that slot (the
        carried frame) was yielded before.  A first chunk of one frame is held and yields nothing.
        Everything yielded, concatenated, has (T - 1) * 2**levels + 1 slots with the originals bit
        for bit at the multiples of 2**levels, and equals, window by window, interpolate() of the
        windows (window_plan); with max_batch = 1 it equals interpolate() of the whole clip (with a
        larger max_batch the windowing changes which pairs share a forward: `chunks`).  Nothing
        but the carried frame stays on the device between chunks (the plans and scratch of the
        synthesiser aside); what is yielded belongs to the consumer.  Fewer than two frames in
        all: ValueError when the input ends.

        scene: a SceneCuts -> (frames, labels, cuts) per window, interpolate(..., scene=) of carry +
        chunk: cuts (B, t - 1) covers that window's pairs, the one after the carried frame
        included, and the slots are filled before the carried frame's slot is dropped.  A pair's
        flag depends on its two frames only, so the equalities above hold with the flags: the
        streamed triples equal the per-window ones byte for byte, and with max_batch = 1 the
        whole clip's.

        rate: a Retime -> every window goes through interpolate(..., rate=, t0=, first=) with the
        global index of its first frame; a window yields the outputs whose time lies after its first
        frame, up to and including its last (the very first window its first frame's too), so
        nothing is dropped afterwards and a window that holds no output (possible when P < Q) yields
        tensors with zero slots.  Concatenated, the yields are retime_count(T, rate) frames, equal
        window by window to interpolate() of the window with its t0 and, with max_batch = 1, to
        interpolate(..., rate=) of the whole clip."""
        if rate is not None:
            _retime_check(levels, rate)
        carry, emitted, total = None, False, 0
        for frames, labels in chunks:
            self._check(frames, labels)
            t = frames.shape[1]
            if t < 1:
                raise ValueError("interpolate_stream: a chunk needs at least one frame")
            if carry is not None:
                if frames.shape[0] != carry[0].shape[0] or frames.shape[2:] != carry[0].shape[2:] or \
                        frames.device != carry[0].device:
                    raise ValueError(f"interpolate_stream: a chunk of {tuple(frames.shape)} follows one of "
                                     f"{tuple(carry[0].shape)}")
                frames, labels = torch.cat([carry[0], frames], 1), torch.cat([carry[1], labels], 1)
            total += t
            carry = (frames[:, -1:].clone(), labels[:, -1:].clone())
            if frames.shape[1] < 2:
                continue  # (the first chunk was one frame: held)
            if rate is not None:
                out_f, out_l, *cuts = self.interpolate(frames, labels, levels, scene, rate, total - frames.shape[1],
                                                       not emitted)
            else:
                out_f, out_l, *cuts = self.interpolate(frames, labels, levels, scene)
            del frames, labels
            if emitted and rate is None:
                out_f, out_l = out_f[:, 1:], out_l[:, 1:]
            emitted = True
            yield (out_f, out_l, *cuts)
            del out_f, out_l, cuts
        if total < 2:
            raise ValueError(f"interpolate_stream needs at least two frames, got {total}")

    def extrapolate(self, frames, labels, steps=1):
        """frames (B, 2, H, W, 3), labels (B, 2, H, W) -> the `steps` following frames and
        labels: each step predicts from [previous, last] and appends (the num_pred_once == 1
        rule of InterTrainer.mini_test)."""
        self._check(frames, labels)
        if frames.shape[1] != 2 or steps < 1:
            raise ValueError("extrapolate needs exactly two frames and steps >= 1")
        fr, lb = self._roll(frames, labels, 2 + steps, [0, 1], [[(k, k + 1, k + 2)] for k in range(steps)],
                            keep=lambda s: s <= steps)
        return fr[2:].transpose(0, 1), lb[2:].transpose(0, 1)

    # ---------------- held-out scoring ----------------
    def score_interpolation(self, frames, labels, levels=1, perceptual=None, msssim=None, motion=None):
        """Held-out scoring of interpolation: frames (B, T, H, W, 3) and labels (B, T, H, W) of
        real clips with (T - 1) % 2**levels == 0 and T > 2**levels.  Frames 0, 2**levels, ...
        go through interpolate(..., levels); every other slot t is scored against original
        frame and label map t (heldout_slots) -> SynthScores, tensors (B, len(slots)).  The
        slots at one offset inside the period are one strided (B, G) view of the synthesised
        and of the original video, scored in place: 2**levels - 1 scoring calls.
        perceptual: a PerceptualScorer -> the scores also have `.vgg` (frame_scores); msssim: a
        number of scales K -> they also have `.msssim`; motion: a MotionSearch -> the result
        also has `.motion`, the MotionScores of the slots (block_motion: the bracketing inputs'
        motion and the temporal residual across every slot, 4 * (2**levels - 1) + 1 calls)."""
        self._check(frames, labels)
        if motion is not None and not isinstance(motion, MotionSearch):
            raise ValueError(f"motion: a MotionSearch, got {motion!r}")
        if perceptual is not None:
            vgg_region(*frames.shape[2:4])  # (too small a frame fails before the synthesis runs)
        if msssim is not None:
            msssim_check(*frames.shape[2:4], msssim)
        T, step = frames.shape[1], 1 << max(levels, 0)
        slots = heldout_slots(T, levels)
        out_f, out_l = self.interpolate(frames[:, ::step], labels[:, ::step], levels)
        parts = [frame_scores(out_f[:, o::step], frames[:, o::step], out_l[:, o::step], labels[:, o::step],
                              n_classes=self.cm.n_classes, perceptual=perceptual, msssim=msssim)
                 for o in range(1, step)]
        # (B, G) per offset -> (B, G, step - 1) -> (B, G * (step - 1)): ascending slots
        scores = parts[0].map(lambda _: None)
        for k in FrameScores.FIELDS:
            if getattr(parts[0], k) is None:  # (vgg without a scorer, msssim without scales)
                continue
            t = torch.stack([getattr(p, k) for p in parts], dim=2)
            setattr(scores, k, t.reshape((t.shape[0], len(slots)) + tuple(t.shape[3:])))
        ms = None
        if motion is not None:
            G = (T - 1) // step
            br = block_motion(frames[:, step::step], frames[:, :-step:step], motion)  # (B, G): later against earlier

            def per_slot(t):  # (B, G) per pair -> (B, G * (step - 1)): the pair's value at each of its slots
                return t.unsqueeze(2).expand(-1, -1, step - 1).reshape(t.shape[0], len(slots))

            def tres_of(video):  # slot t = g * step + o: the residuals against slots t - 1 and t + 1, averaged
                parts = [(block_motion(video[:, o::step], video[:, o - 1::step][:, :G], motion).residual
                          + block_motion(video[:, o::step], video[:, o + 1::step][:, :G], motion).residual) * 0.5
                         for o in range(1, step)]
                return torch.stack(parts, dim=2).reshape(-1, len(slots))

            ms = MotionScores(per_slot(br.rms), per_slot(br.saturated), tres_of(out_f), tres_of(frames))
        return SynthScores(slots, [t % step for t in slots], scores, out_f, out_l, ms)

    def score_extrapolation(self, frames, labels, perceptual=None, msssim=None, motion=None):
        """Held-out scoring of extrapolation: frames (B, 2 + S, H, W, 3), S >= 1.  The first two
        frames are the inputs of extrapolate(..., steps=S); step k is scored against original
        frame 2 + k -> SynthScores with slots 0 .. S-1, tensors (B, S).
        perceptual: a PerceptualScorer -> the scores also have `.vgg` (frame_scores); msssim: a
        number of scales K -> they also have `.msssim`; motion: a MotionSearch -> the result
        also has `.motion`, the MotionScores of the steps (block_motion, three calls)."""
        self._check(frames, labels)
        if motion is not None and not isinstance(motion, MotionSearch):
            raise ValueError(f"motion: a MotionSearch, got {motion!r}")
        if perceptual is not None:
            vgg_region(*frames.shape[2:4])
        if msssim is not None:
            msssim_check(*frames.shape[2:4], msssim)
        S = frames.shape[1] - 2
        if S < 1:
            raise ValueError("score_extrapolation needs two input frames and at least one frame of truth")
        out_f, out_l = self.extrapolate(frames[:, :2], labels[:, :2], steps=S)
        scores = frame_scores(out_f, frames[:, 2:], out_l, labels[:, 2:], n_classes=self.cm.n_classes,
                              perceptual=perceptual, msssim=msssim)
        ms = None
        if motion is not None:
            br = block_motion(frames[:, 1:2], frames[:, 0:1], motion)  # (B, 1): the second input against the first
            video = torch.cat([frames[:, 1:2], out_f], dim=1)  # the second input, then the predictions
            ms = MotionScores(br.rms.expand(-1, S), br.saturated.expand(-1, S),
                              block_motion(video[:, 1:], video[:, :-1], motion).residual,
                              block_motion(frames[:, 2:], frames[:, 1:-1], motion).residual)
        return SynthScores(range(S), range(S), scores, out_f, out_l, ms)
