"""Command-line options, flag-compatible with the reference options/options.py:5-536.

Same flags / dests / defaults for the global options and the EXTRA and INTER sub-commands
(so reference command lines parse unchanged), plus MI355X-path additions:
  --precision {fp32,bf16}   compute dtype of the HIP plan (fp32 = parity mode)
  --synthetic N             use N synthetic Cityscapes-shaped clips (no dataset on disk)
  --clip_store F.npz        decoded uint8 clip store (imgs (N,3,H0,W0,3), segs (N,3,H0,W0),
                            optional val_imgs / val_segs) kept in HBM and prepared on the GPU
                            by data.DeviceClips (train: flip + pseudo-motion crop to input_h x
                            input_w; val: whole frames)
  --synth_levels K          --split test, INTER: frame-rate doublings of the recursive
                            interpolation (K levels: 2**K - 1 new frames between two inputs)
  --synth_eval              --split test: held-out scoring instead of synthesis.  INTER keeps every
                            2**K-th frame of a clip (K = --synth_levels), synthesises the others and
                            scores them against the originals; EXTRA predicts up to --num_pred_step
                            frames from a clip's first two and scores them against the frames that
                            follow.  Writes <cycgen_load_dir>/synth_eval/scores.json (per clip and slot
                            PSNR, SSIM, label accuracy, mIoU; the mean summary), no PNGs
  --synth_vgg               with --synth_eval: also the per-frame VGG19 perceptual score (the reference's
                            `vgg` validation metric, synth.PerceptualScorer) -> "vgg" per clip and in the
                            summary of scores.json, and "vgg_weights"; taken on the top-left
                            (H // 16 * 16, W // 16 * 16) of the frames, which must be at least 16x16
  --synth_msssim K          with --synth_eval: also the per-frame K-scale MS-SSIM (synth.frame_msssim,
                            1 <= K <= 5; 0 = off) -> "msssim" per clip and in the summary of scores.json,
                            and "msssim_scales"; a clip with min(H, W) >> (K - 1) < 11 ends the run
  --synth_motion            with --synth_eval: also block-matching motion statistics (synth.block_motion,
                            synth.MotionSearch) -> per clip and slot "motion" (the RMS block displacement
                            between the two input frames that bracket the slot, pixels per input
                            interval), "motion_saturated" (the fraction of their blocks whose vector lies
                            on the border of the search), "tres" and "tres_gt" (the motion-compensated
                            residual across the slot in the synthesised and in the original video, grey
                            levels per sample); the summary and its per_position rows gain their means
                            and "tres_excess" = mean(tres - tres_gt), and a "per_motion" table groups
                            the frames by "motion" at --synth_motion_edges; a top-level "motion" names
                            the search.  A clip whose mean saturation exceeds one half is logged once
  --synth_motion_radius R   the search radius in plane samples, 1..32 (default 16)
  --synth_motion_scale S    match on the luma averaged over 2**S x 2**S pixels, 0..3 (default 0): a
                            radius of R then reaches R * 2**S frame pixels
  --synth_motion_edges a,b,c
                            the ascending positive bucket edges of per_motion (default 2,8,32).  The
                            defaults of all three are provisional: they have not been validated on real
                            footage
  --synth_pad {none,replicate}
                            --split test: `none` takes only clips whose height and width are multiples
                            of the net's coarsest stride (4; 8 with --highres_large; 4 << (--n_sc - 1)
                            for the refinement stages); `replicate` takes any size: the clip is
                            synthesised on a canvas rounded up to that multiple, its last row and
                            column repeated, and the PNGs and scores have the clip's own size
  --synth_window N          --split test, INTER: N >= 2 runs every clip in windows of N input frames that
                            share their boundary frame (synth.window_plan, interpolate_stream): the clip
                            is read, synthesised and written window by window, one thread reading the
                            next window and one writing the previous while the device works, so device
                            and host memory depend on N and not on the clip's length.  0 (default): the
                            whole clip at once.  1 or a negative value is an error.  EXTRA ignores it
                            (it reads a clip's last two frames; --num_pred_step bounds its memory)
  --synth_yuv {bt601,bt709} --split test: the matrix of the Y'CbCr <-> RGB conversion of .y4m clips.  A
                            clip is a directory of PNGs under <cycgen_load_dir>/rgb (labels: the same
                            names under seg) or a file rgb/<name>.y4m with its labels in seg/<name>.y4m
                            (YUV4MPEG2: C420*, C444 or Cmono, 8 bit; the labels' Y plane is the class
                            id); a .y4m clip is written as synth/{rgb,seg,vis_seg}/<name>.y4m.  Y4M has
                            no tag for the matrix: bt601 (default) is what swscale writes and assumes
                            for an untagged stream; the range follows the file's XCOLORRANGE tag
  --synth_scd               --split test, INTER: scene-cut detection (synth.SceneCuts; off by default).  A
                            neighbouring pair of input frames is a cut when its mean absolute luma
                            difference reaches --synth_scd_mad AND its 32-bin luma histogram distance
                            reaches --synth_scd_hist; the 2**K - 1 slots between the two frames then hold
                            the nearer input frame and label map (the midpoint the earlier one's) instead
                            of the network's blend -- in a .y4m clip the input's own packed bytes -- and
                            one log line per clip names the input frames the cuts follow.  EXTRA predicts
                            as without it and warns when a clip's last two frames are a cut;
                            --synth_eval ignores it
  --synth_scd_mad F         the mean absolute luma difference of a cut, 0..255 (default 30)
  --synth_scd_hist F        the histogram distance of a cut, 0..1 (default 0.25).  Both defaults are
                            provisional: they have not been validated on real footage
  --synth_tile HxW          --split test (also with --synth_eval): frames whose canvas is larger than H x W
                            are synthesised in overlapping tiles of that one size, blended on the device
                            (synth.VideoSynthesizer(tile=), synth.tile_blend); H and W must be multiples
                            of the net's coarsest stride (see --synth_pad).  Off by default.  One forward
                            takes at most VideoSynthesizer.max_pixels pixels (4 793 489 for the bf16
                            coarse net, half of that in fp32): a larger frame, 2160x3840 for one, needs
                            this flag.  One log line per clip gives the tile grid
  --synth_tile_overlap N    the least overlap of neighbouring tiles in pixels: a multiple of the net's
                            coarsest stride, at most half the smaller tile side and at most 256 (default
                            64, provisional: not validated on trained weights and real footage)
  --synth_rate P:Q          --split test, INTER: frame-rate conversion by the ratio P:Q (synth.Retime): output
                            frame k has the time k*Q/P in input frames, so 5:2 turns 24 Hz into 60 Hz, 6:5
                            25 into 30 and 5:6 30 into 25.  The output clock is laid over the grid of
                            --synth_levels K doublings, which needs P <= Q * 2**K (raise --synth_levels
                            otherwise); only the forwards the outputs need are run, and one log line per
                            clip gives the rate, the output count and "F forwards of D".  P and Q are
                            positive and at most 4096 once reduced.  A .y4m clip is written at its own rate
                            times P/Q; outputs that coincide with an input are the input's own packed
                            bytes.  Works with --synth_window, --synth_scd, --synth_pad and --synth_tile.
                            Off by default; EXTRA and --synth_eval ignore it
  --synth_rate_mode {nearest,blend}
                            with --synth_rate: `nearest` (default) writes the grid frame nearest to each
                            output time, a tie going to the earlier one (timing error at most 1/2**(K+1) of
                            an input interval); `blend` cross-fades the two neighbouring grid frames, which
                            are 1/2**K of an input interval apart, with exact integer rounding.  Neither
                            has been judged on trained weights and real footage
  --synth_ensemble {none,time,flip,time+flip}
                            --split test (also with --synth_eval): test-time self-ensembling
                            (synth.VideoSynthesizer(ensemble=)).  Every predicted frame is the fp32 mean of
                            M forwards: `time` (M = 2) adds the forward with the two input frames in
                            exchanged roles, `flip` (M = 2) the forward on the horizontally mirrored inputs,
                            mirrored back, `time+flip` (M = 4) all four; the label is the argmax of the mean
                            logits.  One log line per run names the ensemble and M.  EXTRA takes only
                            `flip`: extrapolation has no time symmetry, and `time` ends the run.  Default
                            `none`; whether the M-fold cost pays off on given weights is what --synth_eval
                            with and without the flag tells -- it has not been measured on trained weights
"""
import argparse

_ADAMAX = ["adamax", "adam", "sgd"]


def _window(text):
    """--synth_window: 0 (off) or a window of at least two input frames"""
    n = int(text)
    if n == 1 or n < 0:
        raise argparse.ArgumentTypeError(f"--synth_window {n}: a window holds at least 2 input frames (0 = the whole clip)")
    return n


def _tile(text):
    """--synth_tile: HxW, two positive integers"""
    import re
    m = re.fullmatch(r"([1-9][0-9]*)x([1-9][0-9]*)", text)
    if not m:
        raise argparse.ArgumentTypeError(f"--synth_tile {text}: expected HxW, two positive integers (576x1024)")
    return int(m.group(1)), int(m.group(2))


def _overlap(text):
    """--synth_tile_overlap: a non-negative integer"""
    import re
    if not re.fullmatch(r"[0-9]+", text):
        raise argparse.ArgumentTypeError(f"--synth_tile_overlap {text}: expected a non-negative integer")
    return int(text)


def _rate(text):
    """--synth_rate: P:Q, two positive integers, each at most 4096 once reduced by their gcd -> (P, Q) reduced"""
    import math
    import re
    m = re.fullmatch(r"([0-9]+):([0-9]+)", text)
    if not m:
        raise argparse.ArgumentTypeError(f"--synth_rate {text}: expected P:Q, two positive integers (5:2 for 24 -> 60 Hz)")
    p, q = int(m.group(1)), int(m.group(2))
    if p < 1 or q < 1:
        raise argparse.ArgumentTypeError(f"--synth_rate {text}: P and Q must be at least 1")
    g = math.gcd(p, q)
    p, q = p // g, q // g
    if max(p, q) > 4096:
        raise argparse.ArgumentTypeError(f"--synth_rate {text}: P and Q must not exceed 4096 once reduced "
                                         f"({p}:{q}); use a nearby ratio of smaller terms")
    return p, q


def _int_range(flag, lo, hi):
    """an integer option in lo..hi"""
    def parse(text):
        import re
        if not re.fullmatch(r"[0-9]+", text) or not lo <= int(text) <= hi:
            raise argparse.ArgumentTypeError(f"{flag} {text}: must be an integer in {lo}..{hi}")
        return int(text)
    return parse


def _edges(text):
    """--synth_motion_edges: ascending positive numbers separated by commas -> a tuple of floats"""
    import math
    try:
        v = tuple(float(x) for x in text.split(","))
    except ValueError:
        v = ()
    if not v or any(not math.isfinite(e) or e <= 0 for e in v) or any(a >= b for a, b in zip(v, v[1:])):
        raise argparse.ArgumentTypeError(f"--synth_motion_edges {text}: expected ascending positive numbers (2,8,32)")
    return v


def _unit_range(flag, hi):
    """a float option in 0..hi"""
    def parse(text):
        v = float(text)
        if not 0 <= v <= hi:  # (NaN fails too)
            raise argparse.ArgumentTypeError(f"{flag} {text}: must be in 0..{hi}")
        return v
    return parse


# (flag, dest, kind, default, choices)  kind: str/int/float/bool(store_true)
GLOBAL = [
    ("--dataset", "dataset", str, "cityscape", ["cityscape", "ucf101", "vimeo", "synthetic"]),
    ("--split", "split", str, "train", ["train", "val", "test", "cycgen", "mycycgen"]),
    ("--img_dir", "img_dir", str, None, None),
    ("--seg_dir", "seg_dir", str, None, None),
    ("--cycgen_load_dir", "cycgen_load_dir", str, None, None),
    ("--input_h", "input_h", int, 128, None),
    ("--input_w", "input_w", int, 256, None),
    ("--syn_type", "syn_type", str, "extra", ["inter", "extra"]),
    ("--mode", "mode", str, "xs2xs", ["xs2xs", "xx2x"]),
    ("--bs", "batch_size", int, 1, None),
    ("--epochs", "epochs", int, 20, None),
    ("--interval", "interval", float, 1, None),
    ("--nw", "num_workers", int, 4, None),
    ("--port", "port", int, None, None),
    ("--seed", "seed", int, 1024, None),
    ("--start_epoch", "start_epoch", int, 1, None),
    ("--disp_interval", "disp_interval", int, 10, None),
    ("--lr_decay_step", "lr_decay_step", int, 5, None),
    ("--lr_decay_gamma", "lr_decay_gamma", float, 1, None),
    ("--save_dir", "save_dir", str, "log", None),
    ("--one_hot_seg", "one_hot_seg", bool, False, None),
    ("--ef", "effec_flow", bool, False, None),
    ("--s", "session", int, 0, None),
    ("--r", "resume", bool, False, None),
    ("--checksession", "checksession", int, 1, None),
    ("--checkepoch", "checkepoch", int, 1, None),
    ("--checkepoch_range", "checkepoch_range", bool, False, None),
    ("--checkepoch_low", "checkepoch_low", int, 1, None),
    ("--checkepoch_up", "checkepoch_up", int, 20, None),
    ("--checkpoint", "checkpoint", int, 0, None),
    ("--load_dir", "load_dir", str, "models", None),
    ("--l1_w", "l1_weight", float, 80, None),
    ("--gdl_w", "gdl_weight", float, 80, None),
    ("--vgg_w", "vgg_weight", float, 20, None),
    ("--ce_w", "ce_weight", float, 30, None),
    ("--ssim_w", "ssim_weight", float, 20, None),
    ("--kld_w", "kld_weight", float, 20, None),
    ("--track_obj_loss", "track_obj_loss", bool, False, None),
    ("--track_obj_w", "track_obj_weight", float, 80, None),
    ("--vid_len", "vid_length", int, 1, None),
    ("--n_track", "num_track_per_img", int, 4, None),
    ("--highres_large", "highres_large", bool, False, None),
    # MI355X-path additions
    ("--precision", "precision", str, "fp32", ["fp32", "bf16"]),
    ("--synthetic", "synthetic", int, 0, None),
    ("--clip_store", "clip_store", str, None, None),
    ("--synth_levels", "synth_levels", int, 1, None),
    ("--synth_eval", "synth_eval", bool, False, None),
    ("--synth_vgg", "synth_vgg", bool, False, None),
    ("--synth_msssim", "synth_msssim", int, 0, None),
    ("--synth_motion", "synth_motion", bool, False, None),
    ("--synth_motion_radius", "synth_motion_radius", _int_range("--synth_motion_radius", 1, 32), 16, None),
    ("--synth_motion_scale", "synth_motion_scale", _int_range("--synth_motion_scale", 0, 3), 0, None),
    ("--synth_motion_edges", "synth_motion_edges", _edges, (2.0, 8.0, 32.0), None),
    ("--synth_pad", "synth_pad", str, "none", ["none", "replicate"]),
    ("--synth_window", "synth_window", _window, 0, None),
    ("--synth_yuv", "synth_yuv", str, "bt601", ["bt601", "bt709"]),
    ("--synth_scd", "synth_scd", bool, False, None),
    ("--synth_scd_mad", "synth_scd_mad", _unit_range("--synth_scd_mad", 255), 30.0, None),
    ("--synth_scd_hist", "synth_scd_hist", _unit_range("--synth_scd_hist", 1), 0.25, None),
    ("--synth_tile", "synth_tile", _tile, None, None),
    ("--synth_tile_overlap", "synth_tile_overlap", _overlap, 64, None),
    ("--synth_rate", "synth_rate", _rate, None, None),
    ("--synth_rate_mode", "synth_rate_mode", str, "nearest", ["nearest", "blend"]),
    ("--synth_ensemble", "synth_ensemble", str, "none", ["none", "time", "flip", "time+flip"]),
]

# second-stage flags of the reference's INTER sub-command (options/options.py:296-380);
# the EXTRA sub-command takes them too for the build-defined extrapolation two-stage nets
# (nets/ExtraNet.py ExtraRefineNet / ExtraStage3Net, BASELINE config 5)
REFINE = [
    ("--n_sc", "n_scales", int, 1, None),
    ("--refine", "refine", bool, False, None),
    ("--with_gt_seg", "with_gt_seg", bool, False, None),
    ("--refine_model", "refine_model", str, "refineUnet", ["refineUnet", "SRNRefine"]),
    ("--refine_o", "refine_optimizer", str, "adamax", _ADAMAX),
    ("--refine_lr", "refine_learning_rate", float, 0.001, None),
    ("--load_refine", "load_refine", bool, False, None),
    ("--train_refine", "train_refine", bool, False, None),
    ("--refine_l1_w", "refine_l1_weight", float, 80, None),
    ("--refine_gdl_w", "refine_gdl_weight", float, 80, None),
    ("--refine_vgg_w", "refine_vgg_weight", float, 20, None),
    ("--refine_ssim_w", "refine_ssim_weight", float, 20, None),
    ("--stage3", "stage3", bool, False, None),
    ("--train_stage3", "train_stage3", bool, False, None),
    ("--load_stage3", "load_stage3", bool, False, None),
    ("--stage3_model", "stage3_model", str, "MSResAttnRefine",
     ["MSResAttnRefine", "MSResAttnRefineV2", "MSResAttnRefineV2Base", "MSResAttnRefineV3"]),
    ("--stage3_prop", "stage3_prop", bool, False, None),
    ("--stage3_flow_consist_w", "stage3_flow_consist_weight", float, 0, None),
]

_EXTRA_MODELS = ["ExtraNet", "ExtraInpaintNet", "ExtraRefineNet", "ExtraStage3Net"]
EXTRA = [
    ("--model", "model", str, "ExtraNet", _EXTRA_MODELS),
    ("--load_model", "load_model", str, "ExtraNet", _EXTRA_MODELS),
    ("--coarse_model", "coarse_model", str, "HRNet", ["HRNet"]),
    ("--coarse_o", "coarse_optimizer", str, "adamax", _ADAMAX),
    ("--coarse_lr", "coarse_learning_rate", float, 0.001, None),
    ("--load_coarse", "load_coarse", bool, False, None),
    ("--train_coarse", "train_coarse", bool, False, None),
    ("--inpaint", "inpaint", bool, False, None),
    ("--inpaint_mask", "inpaint_mask", bool, False, None),
    ("--inpaint_model", "inpaint_model", str, "InpaintUnet", ["InpaintUnet"]),
    ("--inpaint_o", "inpaint_optimizer", str, "adamax", _ADAMAX),
    ("--inpaint_lr", "inpaint_learning_rate", float, 0.001, None),
    ("--load_inpaint", "load_inpaint", bool, False, None),
    ("--train_inpaint", "train_inpaint", bool, False, None),
    ("--num_pred_once", "num_pred_once", int, 1, None),
    ("--num_pred_step", "num_pred_step", int, 1, None),
    ("--fix_init_frames", "fix_init_frames", bool, False, None),
] + REFINE

_DISC_FRAME = ["FrameDiscriminator", "FrameLocalDiscriminator", "FrameSNDiscriminator", "FrameSNLocalDiscriminator",
               "FrameDetDiscriminator", "FrameSNDetDiscriminator", "FrameLSSNDetDiscriminator"]
_DISC_VIDEO = ["VideoDiscriminator", "VideoLocalDiscriminator", "VideoSNDiscriminator", "VideoSNLocalDiscriminator",
               "VideoDetDiscriminator", "VideoSNDetDiscriminator", "VideoLSSNDetDiscriminator",
               "VideoLocalPatchSNDetDiscriminator", "VideoVecSNDetDiscriminator", "VideoPoolSNDetDiscriminator",
               "VideoGlobalZeroSNDetDiscriminator", "VideoGlobalResSNDetDiscriminator",
               "VideoGlobalMaskSNDetDiscriminator", "VideoGlobalCoordSNDetDiscriminator"]
_INTER_MODELS = ["InterNet", "InterRefineNet", "InterStage3Net", "InterGANNet"]

INTER = [
    ("--model", "model", str, "InterNet", _INTER_MODELS),
    ("--load_model", "load_model", str, "InterNet", _INTER_MODELS),
    ("--gan", "gan", bool, False, None),
    ("--coarse_model", "coarse_model", str, "HRNet", ["HRNet", "VAEHRNet"]),
    ("--coarse_o", "coarse_optimizer", str, "adamax", _ADAMAX),
    ("--coarse_lr", "coarse_learning_rate", float, 0.001, None),
    ("--load_coarse", "load_coarse", bool, False, None),
    ("--train_coarse", "train_coarse", bool, False, None),
    ("--vae", "vae", bool, False, None),
    ("--seg_disc", "seg_disc", bool, False, None),
    ("--track_gen", "track_gen", bool, False, None),
    ("--track_gen_model", "track_gen_model", str, "TrackGen", ["TrackGen", "TrackGenV2"]),
    ("--loc_diff_w", "loc_diff_weight", float, 100, None),
] + REFINE + [
    ("--local_disc", "local_disc", bool, False, None),
]
for _kind, _choices in (("frame_disc", _DISC_FRAME), ("frame_det_disc", _DISC_FRAME),
                        ("video_disc", _DISC_VIDEO), ("video_det_disc", _DISC_VIDEO)):
    _default = "FrameDiscriminator" if _kind.startswith("frame") else "VideoDiscriminator"
    INTER += [
        (f"--{_kind}", _kind, bool, False, None),
        (f"--{_kind}_o", f"{_kind}_optimizer", str, "adamax", _ADAMAX),
        (f"--{_kind}_lr", f"{_kind}_learning_rate", float, 0.001, None),
        (f"--train_{_kind}", f"train_{_kind}", bool, False, None),
        (f"--load_{_kind}", f"load_{_kind}", bool, False, None),
        (f"--load_{_kind}_model", f"load_{_kind}_model", str, _default, _choices),
        (f"--{_kind}_model", f"{_kind}_model", str, _default, _choices),
        (f"--{_kind}_d_w", f"{_kind}_disc_weight", float, 1, None),
        (f"--{_kind}_g_w", f"{_kind}_gen_weight", float, 1, None),
    ]


def _add(parser, table):
    for flag, dest, kind, default, choices in table:
        if kind is bool:
            parser.add_argument(flag, dest=dest, action="store_true")
        else:
            parser.add_argument(flag, dest=dest, type=kind, default=default, choices=choices)


class Options:
    def __init__(self):
        self.parser = argparse.ArgumentParser()
        self.initialized = False

    def initialize(self):
        _add(self.parser, GLOBAL)
        sub = self.parser.add_subparsers(help="sub-command help", dest="runner")
        _add(sub.add_parser("EXTRA", help="use extrapolation"), EXTRA)
        _add(sub.add_parser("INTER", help="use interpolation"), INTER)
        self.initialized = True

    def parse(self, argv=None):
        if not self.initialized:
            self.initialize()
        self.opt = self.parser.parse_args(argv)
        return self.opt


def default_args(runner="INTER", **kw):
    """Namespace with every default (for programmatic use: tests, bench)."""
    a = Options().parse([runner])
    a.__dict__.update(kw)
    return a
