"""The definition of the project's multi-scale SSIM (include/dvie.h, dvie_synth_msssim), restated
in float64 on the CPU: the truth the tests of synth.frame_msssim compare against.

Level s of the pyramid is the integer sum of the 2**s x 2**s blocks of the uint8 frame (trailing
rows and columns dropped) divided by 255 * 4**s; per level the maps come from F.conv2d with the
oracle's 11-tap window in float64, zero padding; parts[s] is the mean of cs, for the last level
of l * cs; msssim = prod max(parts, 0) ** w."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.losses import gaussian_window

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def block_sums(img, s):
    """uint8 (H, W, 3) -> int64 (H >> s, W >> s, 3): sums of the 2**s x 2**s blocks"""
    H, W = img.shape[0] >> s, img.shape[1] >> s
    x = img[:H << s, :W << s].astype(np.int64)
    return x.reshape(H, 1 << s, W, 1 << s, 3).sum(axis=(1, 3))


def level(img, s):
    """level s of the pyramid as a float64 (1, 3, H >> s, W >> s) tensor in [0, 1]"""
    return torch.from_numpy(block_sums(img, s)).permute(2, 0, 1)[None].double() / (255.0 * 4 ** s)


def _maps(a, b):
    """(l, cs) maps of two float64 (1, 3, h, w) images in [0, 1]"""
    # the window as oracle.losses.ssim_value builds it for float64 images
    w = gaussian_window(11, 1.5, dtype=torch.float64).double().expand(3, 1, 11, 11).contiguous()
    conv = lambda x: F.conv2d(x, w, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1), (2 * s12 + C2) / (s1 + s2 + C2)


def msssim_truth(pred, gt, K):
    """uint8 numpy (H, W, 3) frames -> (parts (K,) float64, msssim float)"""
    assert pred.dtype == np.uint8 and gt.dtype == np.uint8 and pred.shape == gt.shape and pred.shape[2] == 3
    assert 1 <= K <= 5 and (min(pred.shape[:2]) >> (K - 1)) >= 11, (pred.shape, K)
    parts = np.empty((K,), dtype=np.float64)
    for s in range(K):
        l, cs = _maps(level(pred, s), level(gt, s))
        parts[s] = float((l * cs).mean() if s == K - 1 else cs.mean())
    w = np.array(WEIGHTS[:K], dtype=np.float64)
    w = w / w.sum()
    return parts, float(np.prod(np.maximum(parts, 0.0) ** w))
