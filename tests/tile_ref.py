"""numpy restatement of tiled synthesis (synth.tile_starts, synth.tile_blend / dvie_synth_tile_blend):
the tile plan of an axis, the integer weights and the blend in float32 with the multiply and the add
rounded separately, then dvie_synth_finish's quantisation and argmax.  include/dvie.h states the rule;
nothing here is shared with the code under test."""
import numpy as np

F32 = np.float32


def tile_starts(size, tile, overlap, m):
    """(starts, extent) of one axis"""
    if size <= tile:
        return [0], size
    n = -(-(size - overlap) // (tile - overlap))
    return [(i * (size - tile) // (n - 1)) // m * m for i in range(n)], tile


def axis_weights(start, extent, size, overlap):
    """int64 (size,): the weight of the tile at every coordinate of the axis, 0 where it does not cover"""
    c = np.arange(size, dtype=np.int64)
    a = c - start + 1 if start > 0 else np.full(size, overlap + 1, dtype=np.int64)
    b = start + extent - c if start + extent < size else np.full(size, overlap + 1, dtype=np.int64)
    w = np.minimum(np.minimum(a, b), overlap + 1)
    w[(c < start) | (c >= start + extent)] = 0
    return w


def weights(ys, xs, th, tw, overlap):
    """int64 (nt, hp, wp): the pixel weight wy * wx of every tile, 0 outside it; tile iy * len(xs) + ix"""
    hp, wp = ys[-1] + th, xs[-1] + tw
    wy = [axis_weights(s, th, hp, overlap) for s in ys]
    wx = [axis_weights(s, tw, wp, overlap) for s in xs]
    return np.stack([np.outer(a, b) for a in wy for b in wx])


def blend_map(tiles, ys, xs, overlap):
    """tiles float32 (nt, n, th, tw, C) -> float32 (n, hp, wp, C): one covering tile -> its value bit
    for bit; several -> acc = 0; acc = acc + float32(w) * v in ascending tile index (two roundings per
    step), then acc / float32(sum w)"""
    nt, n, th, tw, C = tiles.shape
    w = weights(ys, xs, th, tw, overlap)
    hp, wp = w.shape[1:]
    cover = (w > 0).sum(0)
    assert cover.min() >= 1
    acc = np.zeros((n, hp, wp, C), dtype=F32)
    single = np.zeros((n, hp, wp, C), dtype=F32)
    t = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for y0 in ys:
            for x0 in xs:
                wt = w[t, y0:y0 + th, x0:x0 + tw]  # > 0 all over the tile
                prod = wt.astype(F32)[None, :, :, None] * tiles[t]  # float32 * float32, rounded
                acc[:, y0:y0 + th, x0:x0 + tw] = acc[:, y0:y0 + th, x0:x0 + tw] + prod  # rounded again
                single[:, y0:y0 + th, x0:x0 + tw] = tiles[t]
                t += 1
        mean = acc / w.sum(0).astype(F32)[None, :, :, None]
    return np.where((cover == 1)[None, :, :, None], single, mean)


def quantise(x):
    """dvie_synth_finish's frame: clamp, * 127.5 and + 127.5 rounded separately, half to even"""
    return np.rint(np.clip(x, F32(-1), F32(1)) * F32(127.5) + F32(127.5)).astype(np.uint8)


def blend(rgb_tiles, seg_tiles, ys, xs, overlap, h, w, n_classes=20):
    """-> (rgb_out (n, hp, wp, rgb_ld) float32, frame (n, h, w, 3), label (n, h, w), label_canvas (n, hp, wp))"""
    rgb = blend_map(rgb_tiles[..., :3], ys, xs, overlap)
    out = np.zeros(rgb.shape[:3] + (rgb_tiles.shape[-1],), dtype=F32)
    out[..., :3] = rgb
    canvas = np.argmax(blend_map(seg_tiles[..., :n_classes], ys, xs, overlap), axis=-1).astype(np.uint8)  # lowest index on ties
    return out, quantise(rgb[:, :h, :w]), canvas[:, :h, :w].copy(), canvas
