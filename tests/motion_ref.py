"""numpy restatement of the block-matching motion statistic (include/dvie.h, dvie_synth_motion): the
luma plane at a scale, its clamped extension, the candidates visited in tie-break order with a
strict `<`, the per-pair sums and the float64 values derived from them -- and the pan clips the
tests share, built from scene_ref.scene.
"""
import functools

import numpy as np

from scene_ref import luma, scene

BLOCK = 16


def plane(frame, s):
    """uint8 (H, W, 3) -> int64 (H >> s, W >> s): the luma, averaged over 2**s x 2**s blocks with
    rounding; trailing rows and columns that fill no block are dropped"""
    y = luma(frame)
    if s == 0:
        return y
    n = 1 << s
    hs, ws = y.shape[0] >> s, y.shape[1] >> s
    blocks = y[:hs * n, :ws * n].reshape(hs, n, ws, n).sum(axis=(1, 3))
    return (blocks + (1 << (2 * s - 1))) >> (2 * s)


def grid(H, W, s):
    return -(-(H >> s) // BLOCK), -(-(W >> s) // BLOCK)


def extended(p, y0, y1, x0, x1):
    """P~ over rows y0 .. y1 - 1 and columns x0 .. x1 - 1 (any integers): indices clamped into the plane"""
    ys = np.clip(np.arange(y0, y1), 0, p.shape[0] - 1)
    xs = np.clip(np.arange(x0, x1), 0, p.shape[1] - 1)
    return p[ys][:, xs]


def candidates(R):
    """(dy, dx) of [-R, R]^2 in tie-break order: ascending (dy*dy + dx*dx, dy, dx)"""
    c = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    return sorted(c, key=lambda v: (v[0] * v[0] + v[1] * v[1], v[0], v[1]))


def match(cur, ref, R, s, lam):
    """uint8 frames (H, W, 3) -> (mv int64 (bh, bw, 2) holding (dy, dx), bsad int64 (bh, bw, 2) holding
    the winner's SAD and the SAD at (0, 0)).  Every block is visited by every candidate in
    tie-break order; a candidate replaces the winner only when its cost is strictly smaller."""
    C, Rp = plane(cur, s), plane(ref, s)
    bh, bw = grid(cur.shape[0], cur.shape[1], s)
    Ce = extended(C, 0, BLOCK * bh, 0, BLOCK * bw)
    best_cost = np.full((bh, bw), np.iinfo(np.int64).max)
    mv = np.zeros((bh, bw, 2), np.int64)
    bsad = np.zeros((bh, bw, 2), np.int64)
    for dy, dx in candidates(R):
        Re = extended(Rp, dy, BLOCK * bh + dy, dx, BLOCK * bw + dx)
        sad = np.abs(Ce - Re).reshape(bh, BLOCK, bw, BLOCK).sum(axis=(1, 3))
        if dy == 0 and dx == 0:
            bsad[..., 1] = sad
        cost = sad + lam * (abs(dy) + abs(dx))
        better = cost < best_cost
        best_cost = np.where(better, cost, best_cost)
        mv[better] = (dy, dx)
        bsad[..., 0] = np.where(better, sad, bsad[..., 0])
    return mv, bsad


def stats(cur, ref, R, s, lam):
    """uint8 (..., H, W, 3) with the same leading dimensions -> dict of int64 arrays shaped like them
    (d2, sad, sad0, border) and mv, bsad (..., bh, bw, 2)"""
    lead = cur.shape[:-3]
    bh, bw = grid(cur.shape[-3], cur.shape[-2], s)
    out = {k: np.zeros(lead, np.int64) for k in ("d2", "sad", "sad0", "border")}
    out["mv"], out["bsad"] = np.zeros(lead + (bh, bw, 2), np.int64), np.zeros(lead + (bh, bw, 2), np.int64)
    for idx in np.ndindex(*lead):
        mv, bsad = match(cur[idx], ref[idx], R, s, lam)
        out["mv"][idx], out["bsad"][idx] = mv, bsad
        out["d2"][idx] = (mv ** 2).sum()
        out["sad"][idx], out["sad0"][idx] = bsad[..., 0].sum(), bsad[..., 1].sum()
        out["border"][idx] = (np.abs(mv).max(axis=-1) == R).sum()
    out["blocks"], out["samples"] = bh * bw, bh * bw * BLOCK * BLOCK
    return out


def derived(st, s):
    """the float64 values of MotionStats from the integers of stats()"""
    blocks, samples = np.float64(st["blocks"]), np.float64(st["samples"])
    return dict(rms=np.sqrt(st["d2"].astype(np.float64) / blocks) * np.float64(1 << s),
                residual=st["sad"].astype(np.float64) / samples, residual0=st["sad0"].astype(np.float64) / samples,
                saturated=st["border"].astype(np.float64) / blocks)


# ---------------- the shared inputs ----------------
@functools.lru_cache(maxsize=None)
def _picture():
    return scene(1, 96, 160)


def pan(H, W, vy, vx, T):
    """uint8 (T, H, W, 3): frame t is the (H, W) crop at (vy t, vx t) of scene(1, 96, 160), so frame
    t + 1 shows the content of frame t moved by (-vy, -vx): frame_t[y][x] == frame_t+1[y - vy][x - vx]"""
    pic = _picture()
    assert vy * (T - 1) + H <= pic.shape[0] and vx * (T - 1) + W <= pic.shape[1]
    return np.stack([pic[vy * t:vy * t + H, vx * t:vx * t + W] for t in range(T)])


def whole_blocks(H, W, s, dy, dx):
    """bool (bh, bw): the blocks whose 16 x 16 samples, and the same samples displaced by (dy, dx),
    lie inside the plane (no sample of the extension enters their SAD at that vector)"""
    hs, ws = H >> s, W >> s
    bh, bw = grid(H, W, s)
    i, j = np.arange(bh)[:, None] * BLOCK, np.arange(bw)[None, :] * BLOCK
    return ((i + min(dy, 0) >= 0) & (i + BLOCK - 1 + max(dy, 0) <= hs - 1) &
            (j + min(dx, 0) >= 0) & (j + BLOCK - 1 + max(dx, 0) <= ws - 1))


# (H, W, (vy, vx), R, penalty, s) of the pan cases
PAN_CASES = [(40, 56, (1, 3), 4, 0, 0), (40, 56, (1, 3), 16, 16, 0), (37, 53, (1, 3), 7, 0, 0),
             (72, 104, (2, 6), 5, 0, 1), (16, 32, (2, 6), 8, 16, 0)]
