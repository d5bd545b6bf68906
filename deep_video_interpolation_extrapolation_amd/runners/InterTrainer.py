"""InterTrainer on the MI355X path (reference runners/InterTrainer.py).

Surface kept from the reference (main.py:85-119 drives it unchanged): __init__(args),
set_epoch, train, validate, save_checkpoint, load_checkpoint; the loop body of the
reference (l.380-441) is factored into `step(data) -> loss_dict`, the hot path:

  HRNet plan forward (HIP)  ->  RGBLoss: L1 + GDL + SSIM kernels, VGG19 plan (HIP)
  -> CE kernel  ->  loss_all / W backward (HRNet + VGG backward plans, HIP; gradient
  buckets all-reduced over RCCL while the backward still runs)  ->  fused Adamax (HIP).

Differences from the reference, all documented: DDP is replaced by runners.comm.GradSync
(identical gradient scaling, see there); the 6 scalar loss all-reduces are one coalesced
all-reduce issued after the optimizer step (values only); tensorboard image logging is
replaced by scalar JSON lines (tensorboardX is not part of this image).
"""
import json
import os
import time
from collections import OrderedDict

import torch
import torch.distributed as dist

from .. import nets
from ..data import DeviceClipLoader, batch_to, get_dataset, load_clip_store
from .. import _lib as L
from ..losses import IoU, L1Loss, make_tape, PSNR, RGBLoss, SegCrossEntropy, SSIM, VGGCosineLoss
from ..optim import Adamax
from ..utils.net_utils import AverageMeter
from . import comm


def get_model(args):
    return nets.__dict__[args.model](args)


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


class _Log:
    def info(self, msg):
        print(msg, flush=True)


class InterTrainer:
    def __init__(self, args):
        self.args = args
        self.log = getattr(args, "logger", None) or _Log()
        self.rank = getattr(args, "rank", 0)
        self.W = comm.world()
        args.gpus = getattr(args, "gpus", self.W) or self.W
        local = int(os.environ.get("LOCAL_RANK", self.rank % max(1, torch.cuda.device_count() or 1)))
        self.device = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        self.log.info("Initializing trainer")
        model = get_model(args)
        self.refine = bool(getattr(args, "refine", False))
        self.stage3 = self.refine and bool(getattr(args, "stage3", False))
        if not getattr(args, "train_coarse", False):
            for p in model.coarse_model.parameters():
                p.requires_grad = False
        if self.refine and not getattr(args, "train_refine", False):  # reference l.49-51
            for p in model.refine_model.parameters():
                p.requires_grad = False
        self.log.info("coarse params " + str(count_parameters(model.coarse_model)))
        if self.refine:
            self.log.info("refine params " + str(count_parameters(model.refine_model)))
            if self.stage3:
                self.log.info("stage3 params " + str(count_parameters(model.stage3_model)))
        model.to(self.device)
        self.model = comm.GradSync(model)
        self.global_step = 0
        self.epoch = 1
        if args.split in ("train", "val"):
            self.train_set, self.val_set = get_dataset(args)
        if args.split == "train":
            self.RGBLoss = RGBLoss(args).to(self.device)
            if self.refine:
                self.refine_RGBLoss = RGBLoss(args, refine=True).to(self.device)
            self.SegLoss = SegCrossEntropy()
            self.coarse_opt = Adamax(list(self.model.module.coarse_model.parameters()), lr=args.coarse_learning_rate)
            if self.refine:  # reference l.80-83
                self.refine_opt = Adamax(list(self.model.module.refine_model.parameters()),
                                         lr=args.refine_learning_rate)
            if self.stage3:
                self.stage3_opt = Adamax(list(self.model.module.stage3_model.parameters()),
                                         lr=args.refine_learning_rate)
            if getattr(args, "clip_store", None):
                self.train_loader = self._device_loader("train", shuffle=True)
            else:
                sampler = torch.utils.data.distributed.DistributedSampler(self.train_set) if self.W > 1 else None
                self.train_loader = torch.utils.data.DataLoader(
                    self.train_set, batch_size=max(1, args.batch_size // args.gpus), shuffle=False,
                    num_workers=getattr(args, "num_workers", 0), pin_memory=True, sampler=sampler)
        elif args.split == "val":
            self.L1Loss, self.PSNRLoss, self.SSIMLoss = L1Loss(), PSNR(), SSIM()
            self.IoULoss, self.VGGCosLoss = IoU(), VGGCosineLoss().to(self.device)
            if getattr(args, "clip_store", None):
                self.val_loader = self._device_loader("val", shuffle=False)
            else:
                sampler = torch.utils.data.distributed.DistributedSampler(self.val_set) if self.W > 1 else None
                self.val_loader = torch.utils.data.DataLoader(
                    self.val_set, batch_size=max(1, args.batch_size // args.gpus), shuffle=False,
                    num_workers=getattr(args, "num_workers", 0), pin_memory=True, sampler=sampler)
        # reference l.105-106 (a subclass that builds more optimizers loads after them:
        # _defer_load)
        if not getattr(self, "_defer_load", False) and (
                getattr(args, "resume", False) or (args.split != "train" and not getattr(args, "checkepoch_range", False))
                or getattr(args, "load_coarse", False) or getattr(args, "load_refine", False)):
            self.load_checkpoint()

    def _device_loader(self, split, shuffle):
        """--clip_store: the decoded clips stay in HBM and each batch is prepared by one HIP
        launch (data.DeviceClips) instead of CPU DataLoader workers."""
        clips = load_clip_store(self.args.clip_store, split, (self.args.input_h, self.args.input_w), self.device)
        return DeviceClipLoader(clips, self.args.batch_size // self.args.gpus, self.rank, self.W,
                                shuffle=shuffle, seed=getattr(self.args, "seed", 0))

    # ---------------- the hot path ----------------
    def get_input(self, data):
        gt_x = data["frame2"]
        gt_seg = data["seg2"] if self.args.mode == "xs2xs" else None
        if getattr(self.args, "model", "InterNet") == "InterNet":
            # the reference's torch.cat (l.373-374), left to the HRNet plan: its input ops read
            # the frames and segmentations in place (HRNet.forward_split)
            x = [data["frame1"], data["frame3"]]
            seg = [data["seg1"], data["seg3"]] if self.args.mode == "xs2xs" else None
        else:
            x = torch.cat([data["frame1"], data["frame3"]], dim=1)
            seg = torch.cat([data["seg1"], data["seg3"]], dim=1) if self.args.mode == "xs2xs" else None
        return x, seg, gt_x, gt_seg

    def _scale_gt(self, gt_x, i):
        """refine_gt_x of reference l.418-419: gt at scale 1 / 2^(n_scales - i - 1)
        (bilinear, align_corners=True)."""
        n = self.args.n_scales
        if i == n - 1:
            return gt_x
        return torch.nn.functional.interpolate(gt_x, scale_factor=1 / (2 ** (n - i - 1)), mode="bilinear",
                                               align_corners=True)

    def step(self, data):
        """One training step (reference l.389-437).  data: sample dict (any device)."""
        ld = self.forward_backward(data)
        self.apply_gradients()
        return comm.sync_losses(ld, self.W)

    def apply_gradients(self, reduce=True):
        """Gradient all-reduce (+ 1/W) and the optimizer steps.  reduce=False: the 1/W
        scale and the optimizers only (device work: runners/graph.py captures it after an
        eager GradSync.reduce())."""
        a = self.args
        if reduce:
            self.model.finish()
        else:
            self.model.scale()
        if getattr(a, "train_coarse", False):
            self.coarse_opt.step()
        if self.refine and getattr(a, "train_refine", False):
            self.refine_opt.step()
        if self.stage3 and getattr(a, "train_stage3", False):
            self.stage3_opt.step()
        self.global_step += 1

    def forward_backward(self, data):
        """Forward, losses and backward of one step -> detached loss dict (this rank's)."""
        a = self.args
        data = batch_to(data, self.device)
        x, seg, gt_x, gt_seg = self.get_input(data)
        out = self.model(x, seg=seg)
        # reference l.401-431: RGBLoss + 30 CE (+ per-scale refine / stage-3 RGBLoss),
        # loss_all = their sum, loss_all / W backward (losses.LossTape: the kernels write the
        # weighted values and the gradients; no PyTorch kernel in between)
        tape = make_tape(self.device, self.W)
        tape.rgb(self.RGBLoss, out[0], gt_x, False, prefix="coarse")
        if a.mode == "xs2xs":
            tape.loss("coarse_ce_loss", L.LOSS_CE, out[1], gt_seg, a.ce_weight)
        if self.refine:  # reference l.415-425 (per scale: refine, then stage 3)
            for i in range(a.n_scales):
                tag = str(1 / (2 ** (a.n_scales - i - 1)))
                gts = self._scale_gt(gt_x, i)
                tape.rgb(self.refine_RGBLoss, out[2][i], gts, False, prefix="refine_" + tag)
                if self.stage3:
                    tape.rgb(self.refine_RGBLoss, out[3][i], gts, False, prefix="stage3_" + tag)
        loss_dict = tape.loss_dict()
        for o in self._opts():
            o.zero_grad(set_to_none=True)
        tape.backward()
        return OrderedDict((k, v.detach()) for k, v in loss_dict.items())

    def _opts(self):
        return [self.coarse_opt] + ([self.refine_opt] if self.refine else []) + ([self.stage3_opt] if self.stage3
                                                                                 else [])

    # ---------------- loops ----------------
    def set_epoch(self, epoch):
        self.log.info("Start of epoch %d" % (epoch + 1))
        self.epoch = epoch + 1
        sampler = getattr(self.train_loader, "sampler", None)
        if isinstance(sampler, (torch.utils.data.distributed.DistributedSampler, DeviceClipLoader)):
            sampler.set_epoch(epoch)

    def train(self):
        if self.rank == 0:
            self.log.info("Training started")
        self.model.train()
        meters = OrderedDict()
        end = time.time()
        load_time = comp_time = 0.0
        for step, data in enumerate(self.train_loader):
            self.step_idx = step
            load_time += time.time() - end
            end = time.time()
            loss_dict = self.step(data)
            comp_time += time.time() - end
            end = time.time()
            if self.rank == 0:
                bs = data["frame1"].size(0)
                for k, v in loss_dict.items():
                    meters.setdefault(k, AverageMeter()).update(float(v), bs)
                if step % self.args.disp_interval == 0:
                    msg = "Epoch [{}/{}][{}/{}] load [{:.3f}s] comp [{:.3f}s] ".format(
                        self.epoch, self.args.epochs, step + 1, len(self.train_loader), load_time, comp_time)
                    msg += " ".join(f"{k} [{m.avg:.3f}]" for k, m in meters.items())
                    self.log.info(msg)
                    self._scalars("losses", {k: m.avg for k, m in meters.items()})
                    meters = OrderedDict()
                    load_time = comp_time = 0.0

    def normalize(self, img):
        return (img + 1) / 2

    def _predict(self, x, seg, gt_x, gt_seg):
        out = self.model(x, seg=seg)
        return out[0], out[1]

    def validate(self):
        self.log.info("Validation epoch {} started".format(self.epoch))
        self.model.eval()
        crit = ["coarse_l1", "coarse_psnr", "coarse_ssim", "coarse_vgg"] + (["coarse_iou"] if self.args.mode == "xs2xs" else [])
        if self.refine:  # reference l.568-569
            crit += ["refine_l1", "refine_psnr", "refine_ssim", "refine_vgg"]
        meters = {c: AverageMeter() for c in crit}
        with torch.no_grad():
            for i, data in enumerate(self.val_loader):
                data = batch_to(data, self.device)
                x, seg, gt_x, gt_seg = self.get_input(data)
                refine_img = None
                if self.refine:  # reference l.593-598
                    out = self.model(x, seg=seg, gt_seg=gt_seg)
                    coarse_img, coarse_seg, refine_img = out[0], out[1], out[2][-1].clamp(-1, 1)
                else:
                    coarse_img, coarse_seg = self._predict(x, seg, gt_x, gt_seg)
                coarse_img = coarse_img.clamp(-1, 1)
                a, b = self.normalize(coarse_img), self.normalize(gt_x)
                d = OrderedDict()
                d["coarse_l1"] = self.L1Loss(a, b)
                d["coarse_psnr"] = self.PSNRLoss(a, b)
                d["coarse_ssim"] = 1 - self.SSIMLoss(a, b)
                if self.args.mode == "xs2xs":
                    d["coarse_iou"] = self.IoULoss.of_scores(coarse_seg, gt_seg)  # IoU(argmax, argmax), fused
                d["coarse_vgg"] = self.VGGCosLoss(a, b, False)
                if refine_img is not None:  # reference l.625-633
                    r = self.normalize(refine_img)
                    d["refine_l1"] = self.L1Loss(r, b)
                    d["refine_psnr"] = self.PSNRLoss(r, b)
                    d["refine_ssim"] = 1 - self.SSIMLoss(r, b)
                    d["refine_vgg"] = self.VGGCosLoss(r, b, False)
                d = comm.sync_losses(d, self.W)
                if self.rank == 0:
                    for c in crit:
                        meters[c].update(float(d[c]), data["frame1"].size(0) * self.W)
        res = {c: m.avg for c, m in meters.items()}
        if self.rank == 0:
            self.log.info("Epoch [{}] Evaluation: ".format(self.epoch) + " ".join(f"{k} [{v:.3f}]" for k, v in res.items()))
            self._scalars("val/score", res)
        return res

    def mini_test(self, img_list, seg_list):
        """Autoregressive rollout from two [0, 1] frames and their segmentations (one-hot
        (B, 20, H, W) or label (B, H, W)) -> per predicted frame the image in [0, 1] and the
        label map, on the CPU (reference InterTrainer.py:786-856 / ExtraTrainer.py:681-757;
        num_pred_step / num_pred_once default to 1 where the runner's options lack them)."""
        assert len(img_list) == 2 and len(seg_list) == 2
        if seg_list[0].dim() == 3:
            seg_list = [torch.nn.functional.one_hot(s.long(), 20).permute(0, 3, 1, 2).float() for s in seg_list]
        self.model.eval()
        dev = self.device
        a = self.args
        npo, nps = getattr(a, "num_pred_once", 1), getattr(a, "num_pred_step", 1)
        onehot = lambda lab: torch.nn.functional.one_hot(lab, 20).permute(0, 3, 1, 2).float()  # noqa: E731
        pred_img, pred_seg = [], []
        with torch.no_grad():
            i1, i2 = img_list[0].to(dev) * 2 - 1, img_list[1].to(dev) * 2 - 1
            s1, s2 = seg_list[0].to(dev), seg_list[1].to(dev)
            for _ in range(nps):
                out = self.model(torch.cat([i1, i2], 1), seg=torch.cat([s1, s2], 1))
                img, seg = out[0], out[1]
                for j in range(npo):
                    pred_img.append(self.normalize(img[:, 3 * j:3 * j + 3]))
                    pred_seg.append(torch.argmax(seg[:, 20 * j:20 * j + 20], dim=1))
                if npo == 1:
                    i1, i2 = i2, pred_img[-1] * 2 - 1
                    s1, s2 = s2, onehot(pred_seg[-1])
                else:
                    i1, i2 = pred_img[-2] * 2 - 1, pred_img[-1] * 2 - 1
                    s1, s2 = onehot(pred_seg[-2]), onehot(pred_seg[-1])
        return [p.cpu() for p in pred_img], [s.cpu() for s in pred_seg]

    def cycgen(self):
        """--split cycgen (reference InterTrainer.py:691-784 / ExtraTrainer.py:586-679): for
        each clip directory, frames 00.0 and {interval}.0 (rgb/ and seg/ PNGs under
        --cycgen_load_dir) -> mini_test rollout -> the inputs and predictions saved as rgb,
        seg and palette-coloured vis_seg PNGs under
        <path>/cycgen/cityscape/<H>x<W>/extra_int_<interval>_len_<vid_length>_nearest/.
        The clip list: the first 61 clip directories in sorted order (the reference reads it
        from a pickle at an absolute path of its authors' machine, root_clip.pkl 'val'[:61])."""
        import numpy as np
        from PIL import Image
        from ..utils.net_utils import save_image, vis_seg_mask
        a = self.args
        assert self.rank == 0, "cycgen runs on one worker"
        assert a.cycgen_load_dir is not None, "please specify --cycgen_load_dir"
        interval = int(a.interval)
        split = "extra_int_{}_len_{}_nearest".format(interval, a.vid_length)
        root = os.path.join(a.path, "cycgen", "cityscape", "{}x{}".format(a.input_h, a.input_w), split)
        load_img_dir, load_seg_dir = os.path.join(a.cycgen_load_dir, "rgb"), os.path.join(a.cycgen_load_dir, "seg")
        clips = sorted(d for d in os.listdir(load_img_dir) if os.path.isdir(os.path.join(load_img_dir, d)))[:61]
        idx = ["{:0>2d}.0".format(0), "{:0>2d}.0".format(interval)]
        for clip in clips:
            imgs = [torch.from_numpy(np.asarray(Image.open(os.path.join(load_img_dir, clip, i + ".png")).convert("RGB"),
                                                dtype=np.float32) / 255).permute(2, 0, 1).unsqueeze(0) for i in idx]
            labs = [torch.from_numpy(np.asarray(Image.open(os.path.join(load_seg_dir, clip, i + ".png")).convert("L"),
                                                dtype=np.int64)).unsqueeze(0) for i in idx]
            segs = [torch.nn.functional.one_hot(l_, 20).permute(0, 3, 1, 2).float() for l_ in labs]
            p_img, p_seg = self.mini_test(imgs, segs)
            save_img = imgs + p_img
            save_seg = [s.argmax(dim=1) for s in segs] + p_seg
            save_vis = [vis_seg_mask(torch.nn.functional.one_hot(s, 20).permute(0, 3, 1, 2).float(), 20)
                        for s in save_seg]
            names = ["{:0>2d}.0".format(int(i * interval)) for i in range(a.vid_length + 2)]
            for sub, lst in (("rgb", save_img), ("seg", save_seg), ("vis_seg", save_vis)):
                d = os.path.join(root, sub, clip)
                os.makedirs(d, exist_ok=True)
                for k in range(a.vid_length + 2):
                    save_image(lst[k].squeeze(0), os.path.join(d, names[k] + ".png"))
        return root

    def _synthesizer(self):
        """--split test: the VideoSynthesizer of this run (--bs pairs per forward, --synth_pad,
        --synth_tile and --synth_tile_overlap; a tile that is no multiple of the net's stride is
        the constructor's ValueError, which names that multiple; --synth_ensemble, logged once per
        run when it is on: `time` on an extrapolation net is the constructor's ValueError too)"""
        from ..synth import VideoSynthesizer
        pad = getattr(self.args, "synth_pad", "none")
        ens = getattr(self.args, "synth_ensemble", "none")
        syn = VideoSynthesizer(self.model.module, max_batch=max(1, self.args.batch_size),
                               pad=None if pad == "none" else pad, tile=getattr(self.args, "synth_tile", None),
                               overlap=getattr(self.args, "synth_tile_overlap", 64),
                               ensemble=None if ens == "none" else ens)
        if syn.ensemble is not None:
            self.log.info("synth: self-ensemble {}: {} forwards per predicted frame".format(ens, len(syn.members)))
        return syn

    @staticmethod
    def _size_hint(e):
        """a FrameSizeError with the flag that runs the size: --synth_tile for a forward that is too
        large, --synth_pad replicate for a size that is no multiple of the net's stride"""
        from ..synth import FrameSizeError
        hint = "--synth_tile HxW synthesises larger frames in tiles" if e.too_large else \
            "--synth_pad replicate takes clips of any size"
        out = FrameSizeError(f"{e} ({hint})")
        out.too_large = e.too_large
        return out

    def _log_tiles(self, syn, clip, H, W):
        """one line per clip when --synth_tile is given: the tile grid of its canvas and the overlap"""
        if syn.tile is None:
            return
        ys, xs, th, tw = syn.tile_grid(H, W)
        self.log.info("synth: {}: {}x{} frames in {} x {} tiles of {}x{}, overlap {}".format(
            clip, H, W, len(ys), len(xs), th, tw, syn.overlap if len(ys) * len(xs) > 1 else 0))

    def _on_clip(self, fn, syn, frames, labels, *rest):
        """fn(syn, frames, labels, ...) of one clip; a frame size that --synth_pad none cannot run
        is reported with the flag that can"""
        from ..synth import FrameSizeError
        try:
            self._log_tiles(syn, rest[0] if rest else "", frames.shape[2], frames.shape[3])
            return fn(syn, frames, labels, *rest)
        except FrameSizeError as e:
            raise self._size_hint(e) from None

    def _scene(self):
        """the synth.SceneCuts of --synth_scd (--synth_scd_mad, --synth_scd_hist), or None"""
        from ..synth import SceneCuts
        a = self.args
        if not getattr(a, "synth_scd", False):
            return None
        return SceneCuts(mad=getattr(a, "synth_scd_mad", 30.0), hist=getattr(a, "synth_scd_hist", 0.25))

    def _log_cuts(self, clip, flags):
        """one line per clip: `flags`, the host flags of its neighbouring input pairs in order"""
        at = [t for t, c in enumerate(flags) if c]
        self.log.info("synth: {}: {} scene cut{} after input frame{} {}".format(
            clip, len(at), "" if len(at) == 1 else "s", "" if len(at) == 1 else "s", at))

    def _rate(self):
        """the synth.Retime of --synth_rate and --synth_rate_mode, or None; a ratio the grid of
        --synth_levels cannot carry is a ValueError that names both flags.  Runners that do not
        stream (EXTRA) ignore the flags, with one log line per run."""
        from ..synth import Retime
        a = self.args
        pq = getattr(a, "synth_rate", None)
        if pq is None:
            return None
        if not self._streams:
            if not getattr(self, "_rate_noted", False):
                self.log.info("synth: --synth_rate and --synth_rate_mode are ignored: extrapolation keeps the clip's rate")
                self._rate_noted = True
            return None
        rate, levels = Retime(int(pq[0]), int(pq[1]), getattr(a, "synth_rate_mode", "nearest")), getattr(a, "synth_levels", 1)
        if levels < 0 or rate.num > rate.den << levels:
            need = max(levels, 0)
            while rate.num > rate.den << need:
                need += 1
            raise ValueError(f"--synth_rate {rate.num}:{rate.den} needs more than the {1 << max(levels, 0)} grid frames "
                             f"per input interval of --synth_levels {levels}: pass --synth_levels {need} or more")
        return rate

    def _log_rate(self, clip, rate, T, n_out, forwards, dense):
        """one line per clip under --synth_rate: the rate, the frame counts and the forwards run"""
        self.log.info("synth: {}: rate {}:{} ({}): {} frames from {}, {} forwards of {}".format(
            clip, rate.num, rate.den, rate.mode, n_out, T, forwards, dense))

    def _synthesize(self, syn, frames, labels, clip=""):
        """--split test, interpolation: --synth_levels frame-rate doublings of the whole clip, or with
        --synth_rate its conversion by P:Q; with --synth_scd frames are held across the detected
        cuts, which are logged"""
        scene, rate = self._scene(), self._rate()
        kw = dict(levels=getattr(self.args, "synth_levels", 1))
        if rate is not None:
            kw["rate"] = rate
        if scene is None:
            out_f, out_l = syn.interpolate(frames, labels, **kw)
        else:
            out_f, out_l, cuts = syn.interpolate(frames, labels, scene=scene, **kw)
            self._log_cuts(clip, cuts[0].cpu().tolist())
        if rate is not None:
            plan = syn.retime_last
            self._log_rate(clip, rate, frames.shape[1], plan.count, plan.forwards, plan.dense_forwards)
        return out_f, out_l

    _streams = True  # --synth_window applies: interpolation runs in windows (ExtraTrainer: False)

    def test(self):
        """--split test: for each clip under --cycgen_load_dir/rgb -> synth.VideoSynthesizer on the
        device (INTER: interpolate with --synth_levels; EXTRA: extrapolate --num_pred_step frames
        from the last two).  A clip is a directory of PNGs (labels: the same file names under /seg),
        all PNGs in sorted order -> <cycgen_load_dir>/synth/{rgb,seg,vis_seg}/<clip>/NNNN.png: the
        frames, the label maps and their palette colouring, numbered in output order; or a file
        <clip>.y4m (labels: /seg/<clip>.y4m, the Y plane the class id) ->
        synth/{rgb,seg,vis_seg}/<clip>.y4m (_stream_clip, _whole_y4m).  INTER with --synth_window N
        >= 2 runs every clip in windows of N input frames with overlapped I/O (_stream_clip).  INTER
        with --synth_rate P:Q converts the frame rate by that ratio instead of by 2**synth_levels
        (_rate; both paths, one log line per clip)."""
        import numpy as np
        from PIL import Image
        from ..utils.net_utils import CITYSCAPES_COLORS
        from ..video_io import PngClip, Y4MClip
        a = self.args
        assert self.rank == 0, "test runs on one worker"
        assert a.cycgen_load_dir is not None, "please specify --cycgen_load_dir"
        if getattr(a, "synth_eval", False):
            return self.test_eval()
        self._rate()  # (a rate --synth_levels cannot carry ends the run before a clip is read)
        syn = self._synthesizer()
        img_dir, seg_dir = os.path.join(a.cycgen_load_dir, "rgb"), os.path.join(a.cycgen_load_dir, "seg")
        root = os.path.join(a.cycgen_load_dir, "synth")
        palette = np.array(CITYSCAPES_COLORS, dtype=np.uint8)
        window = getattr(a, "synth_window", 0) if self._streams else 0
        for clip in sorted(d for d in os.listdir(img_dir) if os.path.isdir(os.path.join(img_dir, d))):
            if window >= 2:
                self._stream_clip(syn, PngClip(img_dir, seg_dir, clip), window, root, palette)
                continue
            names = sorted(f for f in os.listdir(os.path.join(img_dir, clip)) if f.lower().endswith(".png"))
            assert len(names) >= 2, f"{clip}: a clip needs at least two frames"
            imgs = np.stack([np.asarray(Image.open(os.path.join(img_dir, clip, f)).convert("RGB")) for f in names])
            labs = np.stack([np.asarray(Image.open(os.path.join(seg_dir, clip, f)).convert("L")) for f in names])
            frames, labels = self._on_clip(self._synthesize, syn, torch.from_numpy(imgs)[None].to(self.device),
                                           torch.from_numpy(labs)[None].to(self.device), clip)
            frames, labels = frames[0].cpu().numpy(), labels[0].cpu().numpy()
            vis = palette[np.minimum(labels, len(palette) - 1)]  # (ids past the classes: "none")
            for sub, arr in (("rgb", frames), ("seg", labels), ("vis_seg", vis)):
                d = os.path.join(root, sub, clip)
                os.makedirs(d, exist_ok=True)
                for k in range(arr.shape[0]):
                    Image.fromarray(np.ascontiguousarray(arr[k])).save(os.path.join(d, "{:04d}.png".format(k)))
        for fname in self._y4m_clips(img_dir):
            src = Y4MClip(img_dir, seg_dir, fname)
            try:
                if self._streams:
                    self._stream_clip(syn, src, window, root, palette)
                else:
                    self._whole_y4m(syn, src, root, palette)
            finally:
                src.close()
        return root

    @staticmethod
    def _y4m_clips(img_dir):
        """the .y4m clip files of a clip directory, sorted"""
        return sorted(f for f in os.listdir(img_dir) if f.lower().endswith(".y4m") and os.path.isfile(os.path.join(img_dir, f)))

    def _upload(self, src, host, originals=None):
        """one chunk of a clip as its reader thread left it -> (frames (1, t, H, W, 3), labels
        (1, t, H, W)) on the device.  PNG: the decoded arrays; Y4M: the packed frames, converted by
        synth.yuv_to_rgb (--synth_yuv, the file's range), and the Y plane of the packed labels;
        `originals` (a deque) gets the packed device frame of every input frame, in order."""
        from ..synth import yuv_to_rgb
        a, b = (torch.from_numpy(x).to(self.device) for x in host)
        if src.kind == "png":
            return a[None], b[None]
        H, W = src.height, src.width
        frames = yuv_to_rgb(a, H, W, src.rgb.colourspace, getattr(self.args, "synth_yuv", "bt601"), src.rgb.full_range)
        if originals is not None:
            originals.extend(a.unbind(0))
        return frames[None], b[:, :H * W].reshape(-1, H, W).contiguous()[None]

    def _pack_y4m(self, src, out_f, out_l, palette, originals=None, first=0, step=0, cuts=None, hold=None):
        """frames (S, H, W, 3) and labels (S, H, W) of one Y4M clip on the device (any stride over S)
        -> what Y4MSink.write takes, on the host: the packed frames in the input's colourspace, the
        label maps, and their palette colouring packed as C444.  step >= 1: slots first, first +
        step, ... are input frames and get their own packed bytes, copied from the deque
        `originals`; only the other slots go through synth.rgb_to_yuv, each residue modulo step
        as one strided run read and written in place.  step 0: every slot is converted.
        cuts: the window's flags (1, t - 1) of interpolate_stream(..., scene=) -> the packed slots
        between a flagged pair are synth.cut_fill's copies of the neighbouring input's own packed
        bytes, not a conversion of the held RGB frame.  The fill needs the window's leading input
        slot: `hold`, a one-element list, carries the packed bytes of the last input frame from one
        window to the next, where they stand in front of the block while it is filled."""
        from ..synth import cut_fill, rgb_to_yuv
        from ..video_io import frame_bytes
        S, H, W = out_l.shape
        cs, full, matrix = src.rgb.colourspace, src.rgb.full_range, getattr(self.args, "synth_yuv", "bt601")
        lead = int(cuts is not None and hold[0] is not None)  # (the window came without its first slot)
        pkx = torch.empty((S + lead, frame_bytes(W, H, cs)), dtype=torch.uint8, device=out_f.device)
        pk = pkx[lead:]
        if lead:
            pkx[0].copy_(hold[0])
        if step:
            for i in range(first, S, step):
                o = originals.popleft()
                pk[i].copy_(o)
                if hold is not None:
                    hold[0] = o
        for r in ([0] if not step else [r for r in range(min(step, S)) if r != first]):
            rgb_to_yuv(out_f[r::max(step, 1)], cs, matrix, full, out=pk[r::max(step, 1)])
        if cuts is not None and step > 1:
            cut_fill(pkx[None], cuts, step.bit_length() - 1)
        vis = palette[out_l.clamp(max=palette.shape[0] - 1).long()]  # (ids past the classes: "none")
        vis = rgb_to_yuv(vis, "C444", matrix, full)
        return pk.cpu().numpy(), out_l.reshape(S, H * W).cpu().numpy(), vis.cpu().numpy()

    def _pack_y4m_rate(self, src, out_f, out_l, palette, originals, plan, cuts=None):
        """_pack_y4m under --synth_rate: the N = plan.count outputs (N, H, W, 3) / (N, H, W) of one window
        of a Y4M clip -> what Y4MSink.write takes.  The deque `originals` holds the packed device frames
        of the window's plan.T inputs; all but the last, which the next window starts with, are taken
        off.  Outputs that coincide with an input (plan.aligned) never go through synth.rgb_to_yuv: one
        synth.retime_gather over the packed inputs (plan.input_rows) copies the input's own bytes
        there and, reading the flags `cuts` on the device, over every output held across a cut; the
        runs of outputs between the aligned ones are converted first, one launch per run."""
        import numpy as np
        from ..synth import retime_gather, rgb_to_yuv
        from ..video_io import frame_bytes
        N, H, W = out_l.shape
        cs, full, matrix = src.rgb.colourspace, src.rgb.full_range, getattr(self.args, "synth_yuv", "bt601")
        assert len(originals) == plan.T, (len(originals), plan.T)
        inputs = torch.stack(list(originals))
        for _ in range(plan.T - 1):
            originals.popleft()
        pk = torch.empty((N, frame_bytes(W, H, cs)), dtype=torch.uint8, device=out_f.device)
        if N == 0:
            return pk.cpu().numpy(), np.empty((0, H * W), np.uint8), np.empty((0, 3 * H * W), np.uint8)
        i = 0
        for j in [j for j, _ in plan.aligned] + [N]:
            if j > i:
                rgb_to_yuv(out_f[i:j], cs, matrix, full, out=pk[i:j])
            i = j + 1
        retime_gather(inputs[None], plan.input_rows, 1, pk[None], cuts)
        vis = palette[out_l.clamp(max=palette.shape[0] - 1).long()]  # (ids past the classes: "none")
        vis = rgb_to_yuv(vis, "C444", matrix, full)
        return pk.cpu().numpy(), out_l.reshape(N, H * W).cpu().numpy(), vis.cpu().numpy()

    def _stream_clip(self, syn, src, window, root, palette):
        """--split test, interpolation, one clip in windows (window 0: a .y4m clip as one window):
        a reader thread prepares the next window (file reads, PNG decoding), this thread copies it
        to the device, runs VideoSynthesizer.interpolate_stream and copies the result back, a
        writer thread encodes and writes it; both queues hold at most two windows.  Every HIP call
        is made here.  Output slots are numbered across windows; for a .y4m clip the slots at the
        multiples of 2**synth_levels are the input's packed bytes, written back untouched.  With
        --synth_scd the windows come with their cut flags: the held slots of a .y4m clip are the
        neighbouring input's packed bytes (_pack_y4m), the flags reach the host with the window's
        other copies, and one log line names the clip's cuts."""
        import collections
        import time
        from ..synth import FrameSizeError, retime_fps
        from ..video_io import BackgroundWriter, PngSink, Prefetcher, Y4MSink
        levels = getattr(self.args, "synth_levels", 1)
        step = 1 << levels
        rate = self._rate()
        if src.kind == "png":
            sink = PngSink(root, src.name, palette)
        else:
            num, den = src.rgb.fps
            sink = Y4MSink(root, src.name, src.width, src.height,
                           (num * step, den) if rate is None else retime_fps((num, den), rate), src.rgb.colourspace,
                           src.rgb.full_range)
            palette = torch.from_numpy(palette).to(self.device)
        originals = collections.deque()
        scene, flags, hold = self._scene(), [], [None]
        t_start, g0 = time.perf_counter(), 0
        n_in = forwards = dense = 0  # (--synth_rate: the clip's input frames and forwards, summed over its windows)
        try:
            with Prefetcher(src.chunks(window)) as reader, BackgroundWriter(sink.write) as writer:
                on_device = (self._upload(src, host, originals if src.kind == "y4m" else None) for host in reader)
                try:
                    for out_f, out_l, *cuts in syn.interpolate_stream(on_device, levels=levels, scene=scene,
                                                                      **({} if rate is None else dict(rate=rate))):
                        S = out_f.shape[1]
                        if g0 == 0 and n_in == 0:
                            self._log_tiles(syn, src.name, out_f.shape[2], out_f.shape[3])
                        if rate is not None:
                            plan = syn.retime_last
                            n_in, forwards, dense = plan.t0 + plan.T, forwards + plan.forwards, dense + plan.dense_forwards
                        if src.kind == "png":
                            writer.put((g0, out_f[0].cpu().numpy(), out_l[0].cpu().numpy()))
                        elif rate is not None:
                            writer.put(self._pack_y4m_rate(src, out_f[0], out_l[0], palette, originals, plan,
                                                           cuts[0] if cuts else None))
                        else:
                            writer.put(self._pack_y4m(src, out_f[0], out_l[0], palette, originals, (-g0) % step, step,
                                                      *((cuts[0], hold) if cuts else ())))
                        if cuts:
                            flags += cuts[0][0].cpu().tolist()
                        g0 += S
                        del out_f, out_l, cuts
                except FrameSizeError as e:
                    raise self._size_hint(e) from None
                torch.cuda.synchronize(self.device)
                t_dev = time.perf_counter()
        finally:
            sink.close()
        t_end = time.perf_counter()
        if scene is not None:
            self._log_cuts(src.name, flags)
        if rate is not None:
            self._log_rate(src.name, rate, n_in, g0, forwards, dense)
        self.log.info("synth: {}: {} slots in {:.3f} s ({:.1f} slots/s); reader busy {:.3f} s, this thread waited for it "
                      "{:.3f} s and for the writer {:.3f} s, writer busy {:.3f} s ({:.3f} s after the last window)".format(
                          src.name, g0, t_end - t_start, g0 / max(t_end - t_start, 1e-9), reader.busy, reader.waited,
                          writer.waited, writer.busy, t_end - t_dev))

    def _whole_y4m(self, syn, src, root, palette):
        """--split test, extrapolation, one .y4m clip: read whole, --num_pred_step frames predicted from
        its last two, every one of them written through synth.rgb_to_yuv at the input's frame rate"""
        from ..video_io import Y4MSink
        host = list(src.chunks(0))
        if not host or host[0][0].shape[0] < 2:
            raise ValueError(f"{src.name}: a clip needs at least two frames")
        frames, labels = self._on_clip(self._synthesize, syn, *self._upload(src, host[0]), src.name)
        sink = Y4MSink(root, src.name, src.width, src.height, src.rgb.fps, src.rgb.colourspace, src.rgb.full_range)
        try:
            sink.write(self._pack_y4m(src, frames[0], labels[0], torch.from_numpy(palette).to(self.device)))
        finally:
            sink.close()

    def _motion(self):
        """the synth.MotionSearch of --synth_motion (--synth_motion_radius, --synth_motion_scale), or None"""
        from ..synth import MotionSearch
        a = self.args
        if not getattr(a, "synth_motion", False):
            return None
        return MotionSearch(radius=getattr(a, "synth_motion_radius", 16), scale=getattr(a, "synth_motion_scale", 0))

    def _score(self, syn, frames, labels, clip, perceptual=None, msssim=None, motion=None):
        """--split test --synth_eval, interpolation: every 2**synth_levels-th frame is kept, the
        others are synthesised and scored (None: the clip is too short); perceptual: the
        PerceptualScorer of --synth_vgg; msssim: the scales of --synth_msssim; motion: the
        MotionSearch of --synth_motion"""
        step = 1 << getattr(self.args, "synth_levels", 1)
        T = frames.shape[1]
        keep = (T - 1) // step * step + 1
        if keep <= step:
            self.log.info(f"synth_eval: skip {clip}: {T} frames, {step + 1} needed for --synth_levels")
            return None
        if keep < T:
            self.log.info(f"synth_eval: {clip}: the last {T - keep} of {T} frames dropped ((T - 1) % {step} != 0)")
        return syn.score_interpolation(frames[:, :keep], labels[:, :keep], levels=getattr(self.args, "synth_levels", 1),
                                       perceptual=perceptual, msssim=msssim, motion=motion)

    def test_eval(self):
        """--split test --synth_eval: the clips of test(), scored instead of written.  Per clip
        VideoSynthesizer.score_interpolation / score_extrapolation (_score) against the clip's own
        held-out frames -> <cycgen_load_dir>/synth_eval/scores.json: {"clips": {clip: {"slots",
        "psnr", "ssim", "acc", "miou"}} (one value per scored slot), "summary": the means over
        every scored frame of every clip and per position (synth.summarize)}; the summary also
        goes to the log.  No PNG is written.  With --synth_vgg one synth.PerceptualScorer scores
        every clip too: "vgg" per clip, in the summary and in every per_position row, and a
        top-level "vgg_weights" naming the VGG19 weights (PerceptualScorer.weights_name); a clip
        whose size is no multiple of 16 is scored on synth.vgg_region of it (logged once per clip).
        With --synth_msssim K every scored frame also gets its K-scale MS-SSIM (synth.frame_msssim):
        "msssim" per clip, in the summary and in every per_position row, and a top-level
        "msssim_scales"; a clip too small for K scales ends the run with a ValueError naming the
        clip (K is never reduced: one scores.json holds one metric).  With --synth_ensemble other than
        `none` the synthesis is the ensemble's and a top-level "ensemble" names it.  With
        --synth_motion every scored slot also gets the synth.MotionScores columns: "motion",
        "motion_saturated", "tres" and "tres_gt" per clip; "motion", "saturated", "tres", "tres_gt"
        and "tres_excess" in the summary and in every per_position row; "per_motion", the same
        columns per bucket of "motion" at --synth_motion_edges; and a top-level "motion" with the
        block size, the search and the edges.  A clip whose mean saturation exceeds one half is
        logged once (a reporting rule, not a tuned threshold).  Without the flag the file is what
        it was."""
        import numpy as np
        from PIL import Image
        from ..synth import MOTION_BLOCK, MotionScores, PerceptualScorer, motion_grid, msssim_check, summarize, vgg_region
        a = self.args
        if getattr(a, "synth_scd", False):
            self.log.info("synth_eval: --synth_scd is ignored: every held-out frame is scored against its original")
        if getattr(a, "synth_rate", None) is not None:
            self.log.info("synth_eval: --synth_rate and --synth_rate_mode are ignored: the held-out frames sit on the "
                          "2**K grid")
        syn = self._synthesizer()
        scorer = PerceptualScorer(max_batch=max(1, a.batch_size)) if getattr(a, "synth_vgg", False) else None
        scales = getattr(a, "synth_msssim", 0) or None
        search = self._motion()
        extra = (("vgg",) if scorer else ()) + (("msssim",) if scales else ())
        moving = MotionScores.FIELDS if search else ()  # (the columns of summarize)
        keys = ("psnr", "ssim", "acc", "miou") + extra + tuple("motion_saturated" if k == "saturated" else k for k in moving)
        img_dir, seg_dir = os.path.join(a.cycgen_load_dir, "rgb"), os.path.join(a.cycgen_load_dir, "seg")
        clips, cols = {}, [[] for _ in range(1 + len(keys))]
        for clip in sorted(d for d in os.listdir(img_dir) if os.path.isdir(os.path.join(img_dir, d))):
            names = sorted(f for f in os.listdir(os.path.join(img_dir, clip)) if f.lower().endswith(".png"))
            if not names:
                self.log.info(f"synth_eval: skip {clip}: no frames")
                continue
            imgs = np.stack([np.asarray(Image.open(os.path.join(img_dir, clip, f)).convert("RGB")) for f in names])
            labs = np.stack([np.asarray(Image.open(os.path.join(seg_dir, clip, f)).convert("L")) for f in names])
            if scorer and vgg_region(*imgs.shape[1:3]) != imgs.shape[1:3]:
                self.log.info("synth_eval: {}: vgg is scored on the top-left {}x{} of the {}x{} frames".format(
                    clip, *vgg_region(*imgs.shape[1:3]), *imgs.shape[1:3]))
            if scales:
                try:
                    msssim_check(*imgs.shape[1:3], scales)
                except ValueError as e:
                    raise ValueError(f"{clip}: {e}") from None
            if search:
                try:
                    motion_grid(*imgs.shape[1:3], search.scale)
                except ValueError as e:
                    raise ValueError(f"{clip}: {e}") from None
            sc = self._on_clip(self._score, syn, torch.from_numpy(imgs)[None].to(self.device),
                               torch.from_numpy(labs)[None].to(self.device), clip, scorer, scales, search)
            if sc is None:
                continue
            # psnr, ssim, acc, miou (, vgg) (, msssim) (, motion, saturated, tres, tres_gt) of the one clip
            vals = [v[0] for v in sc.host(vgg=scorer is not None, msssim=scales is not None, motion=search is not None)]
            if search and float(np.mean(vals[keys.index("motion_saturated")])) > 0.5:
                self.log.info("synth_eval: {}: {:.0%} of the blocks have their vector on the border of the search: "
                              "\"motion\" is a lower bound there; a larger --synth_motion_scale widens the search".format(
                                  clip, float(np.mean(vals[keys.index("motion_saturated")]))))
            clips[clip] = dict(slots=sc.slots, **{k: v.tolist() for k, v in zip(keys, vals)})
            for col, v in zip(cols, [np.asarray(sc.positions)] + vals):
                col.append(v)
        for fname in self._y4m_clips(img_dir):
            self.log.info(f"synth_eval: skip {fname}: .y4m clips are synthesised, not scored")
        cat = [np.concatenate(c) for c in cols] if clips else None
        edges = tuple(getattr(a, "synth_motion_edges", (2.0, 8.0, 32.0)))
        more = dict(edges=edges) if search else {}
        res = dict(clips=clips, summary=summarize(*cat[:5], **dict(zip(extra + moving, cat[5:])), **more) if clips else None)
        if scorer:
            res["vgg_weights"] = scorer.weights_name
        if scales:
            res["msssim_scales"] = scales
        if syn.ensemble is not None:
            res["ensemble"] = syn.ensemble
        if search:
            res["motion"] = dict(block=MOTION_BLOCK, radius=search.radius, scale=search.scale, penalty=search.penalty,
                                 edges=list(edges))
        root = os.path.join(a.cycgen_load_dir, "synth_eval")
        os.makedirs(root, exist_ok=True)
        with open(os.path.join(root, "scores.json"), "w") as f:
            json.dump(res, f, indent=1)
        self.log.info("synth_eval: {} clips, summary {}".format(len(clips), json.dumps(res["summary"])))
        return root

    def _scalars(self, tag, info):
        path = getattr(self.args, "path", None)
        if path:
            with open(os.path.join(path, "scalars.jsonl"), "a") as f:
                f.write(json.dumps(dict(tag=tag, step=self.global_step, **info)) + "\n")

    # ---------------- checkpoints (reference l.867-960) ----------------
    def _ckpt_name(self, model_name, session, epoch, step, root):
        d = "{}_{}_{}_{}".format(model_name, self.args.mode, self.args.syn_type, session)
        return os.path.join(root, "checkpoint", d + "_{}_{}.pth".format(epoch, step))

    def save_checkpoint(self):
        name = self._ckpt_name(self.args.model, self.args.session, self.epoch, getattr(self, "step_idx", 0),
                               self.args.path)
        os.makedirs(os.path.dirname(name), exist_ok=True)
        d = {"session": self.args.session, "epoch": self.epoch + 1,
             "coarse_model": self.model.module.coarse_model.state_dict(),
             "coarse_opt": self.coarse_opt.state_dict()}
        if self.refine:  # reference l.879-884
            d["refine_model"] = self.model.module.refine_model.state_dict()
            d["refine_opt"] = self.refine_opt.state_dict()
            if self.stage3:
                d["stage3_model"] = self.model.module.stage3_model.state_dict()
                d["stage3_opt"] = self.stage3_opt.state_dict()
        torch.save(d, name)
        self.log.info("save model: {}".format(name))
        return name

    def load_checkpoint(self):
        a = self.args
        name = self._ckpt_name(a.load_model, a.checksession, a.checkepoch, a.checkpoint, a.load_dir or ".")
        self.log.info("Loading checkpoint %s" % name)
        ckpt = torch.load(name, map_location="cpu", weights_only=True)
        # weights gated by load_coarse, optimizer state by train_coarse and load_coarse (l.902-936)
        m = self.model.module
        for part in ("coarse", "refine", "stage3"):
            if not getattr(a, "load_" + part, False):
                continue
            assert part == "coarse" or getattr(a, part if part == "stage3" else "refine", False), \
                "--load_%s needs --%s" % (part, part)
            sd = getattr(m, part + "_model").state_dict()
            sd.update(ckpt[part + "_model"])
            getattr(m, part + "_model").load_state_dict(sd)
        if a.split == "train":  # optimizer states (l.929-952)
            for part in ("coarse", "refine", "stage3"):
                if getattr(a, "train_" + part, False) and getattr(a, "load_" + part, False):
                    getattr(self, part + "_opt").load_state_dict(ckpt[part + "_opt"])
        # epoch bookkeeping as the reference (l.953-958): the file's epoch is checkepoch + 1
        if getattr(a, "resume", False):
            assert ckpt["epoch"] - 1 == a.checkepoch, [ckpt["epoch"], a.checkepoch]
            self.epoch = ckpt["epoch"]
        elif a.split != "train":
            assert ckpt["epoch"] - 1 == a.checkepoch, [ckpt["epoch"], a.checkepoch]
            self.epoch = ckpt["epoch"] - 1
        self.log.info("checkpoint loaded")
