"""numpy restatement of scene-cut detection (include/dvie.h, dvie_synth_scene / dvie_synth_cutfill):
the integer statistic of a neighbouring frame pair, the two integer limits, the fill rule -- and
the synthetic clips the end-to-end tests share, whose pairs lie far from the thresholds those
tests use (tests/test_scene_cpu.py asserts the margins).
"""
import math

import numpy as np

MAD, HIST = 40.0, 0.3  # the thresholds of the end-to-end tests


def luma(frames):
    """uint8 (..., 3) -> int64 (...): (77 R + 150 G + 29 B + 128) >> 8"""
    f = frames.astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def histogram(frame):
    """uint8 (H, W, 3) -> int64 (32,): the counts of luma >> 3"""
    return np.bincount((luma(frame) >> 3).ravel(), minlength=32).astype(np.int64)


def stats(frames):
    """uint8 (B, T, H, W, 3) -> (sad, hdiff), int64 (B, T - 1)"""
    B, T = frames.shape[:2]
    sad, hdiff = np.zeros((B, T - 1), np.int64), np.zeros((B, T - 1), np.int64)
    for b in range(B):
        for t in range(T - 1):
            sad[b, t] = np.abs(luma(frames[b, t]) - luma(frames[b, t + 1])).sum()
            hdiff[b, t] = np.abs(histogram(frames[b, t]) - histogram(frames[b, t + 1])).sum()
    return sad, hdiff


def limits(H, W, mad, hist):
    """(sad_min, hist_min) = (ceil(mad H W), ceil(hist 2 H W))"""
    return int(math.ceil(mad * H * W)), int(math.ceil(hist * 2 * H * W))


def cuts(frames, mad, hist):
    """uint8 (B, T, H, W, 3) -> bool (B, T - 1)"""
    sad, hdiff = stats(frames)
    sad_min, hist_min = limits(frames.shape[2], frames.shape[3], mad, hist)
    return (sad >= sad_min) & (hdiff >= hist_min)


def sources(levels):
    """per interior slot j = 1 .. 2**levels - 1 of a pair: 0 the left input, 1 the right one"""
    step = 1 << levels
    return [0 if 2 * j <= step else 1 for j in range(1, step)]


def fill(slots, flags, levels):
    """(B, (T - 1) * 2**levels + 1, ...) and bool (B, T - 1) -> a filled copy"""
    out = slots.copy()
    step = 1 << levels
    for b, t in zip(*np.nonzero(flags)):
        for j, s in zip(range(1, step), sources(levels)):
            out[b, t * step + j] = slots[b, (t + s) * step]
    return out


# ---------------- the shared inputs ----------------
def scene(seed, H=48, W=64):
    """a smooth random picture, uint8 (H, W, 3): noise at 1/8 resolution, upsampled by 8 and
    box-blurred over 8 taps along both axes"""
    rng = np.random.RandomState(seed)
    small = rng.randint(0, 256, (H // 8, W // 8, 3)).astype(np.float64)
    big = np.repeat(np.repeat(small, 8, 0), 8, 1)
    for axis in (0, 1):
        pad = [(0, 0)] * 3
        pad[axis] = (4, 3)
        p = np.pad(big, pad, mode="edge")
        big = sum(np.take(p, range(k, k + big.shape[axis]), axis) for k in range(8)) / 8.0
    return np.clip(np.rint(big), 0, 255).astype(np.uint8)


def crop(pic, t, H, W):
    """frame t of a pan over `pic`: the (H, W) crop at (t, 3 t)"""
    return pic[t:t + H, 3 * t:3 * t + W]


def pan_clip(seeds, T, H, W, cut_at=None):
    """uint8 (T, H, W, 3): a pan of (1, 3) pixels per frame over scene(seeds[0]); from frame cut_at
    on over scene(seeds[1]) scaled by 0.5"""
    a = scene(seeds[0])
    b = (scene(seeds[1]) // 2).astype(np.uint8) if cut_at is not None else None
    return np.stack([crop(a if cut_at is None or t < cut_at else b, t, H, W) for t in range(T)])


def labels_for(frames, seed):
    """label maps (..., H, W) in 0..19 for frames (..., H, W, 3)"""
    return np.random.RandomState(seed).randint(0, 20, frames.shape[:-1]).astype(np.uint8)


SEEDS_A, SEEDS_B = (1, 2), (2, 2)  # (first scene, second scene) of the clip with a cut; of the clip without


def api_clips(H=16, W=32, T=4, cut_at=2):
    """the clips of the interpolate tests: frames (2, T, H, W, 3), clip 0 with a cut before frame
    cut_at, clip 1 without one; labels (2, T, H, W)"""
    frames = np.stack([pan_clip(SEEDS_A, T, H, W, cut_at), pan_clip(SEEDS_B, T, H, W)])
    return frames, labels_for(frames, 91)


def command_clip(H=16, W=32, T=5, cut_at=3):
    """the one clip of the command tests, (1, T, H, W, 3) with a cut before frame cut_at, and labels"""
    frames = pan_clip(SEEDS_A, T, H, W, cut_at)[None]
    return frames, labels_for(frames, 92)
