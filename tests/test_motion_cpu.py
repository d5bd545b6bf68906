"""CPU checks of the block-matching motion statistic: the numpy restatement (tests/motion_ref.py) on
pan clips, flat frames and ties; summarize's motion columns and buckets; MotionSearch and the
--synth_motion flags; the C ABI and its argument checks (no launch is reached)."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.options import Options
import motion_ref as M


# ---------------- the reference ----------------
@pytest.mark.parametrize("H,W,v,R,lam,s", M.PAN_CASES)
def test_pan_clips_give_the_pan(H, W, v, R, lam, s):
    """Frame t against frame t + 1 of a pan by (vy, vx): every block whose samples and displaced
    samples lie inside the plane finds exactly (-vy >> s, -vx >> s) with SAD 0, and the other way
    round (vy >> s, vx >> s).  The 16x32 case has no such block: its vectors are only counted."""
    vy, vx = v
    clip = M.pan(H, W, vy, vx, 3)
    bh, bw = M.grid(H, W, s)
    assert (bh, bw) == synth.motion_grid(H, W, s)
    for cur, ref, want in ((clip[:-1], clip[1:], (-vy >> s, -vx >> s)), (clip[1:], clip[:-1], (vy >> s, vx >> s))):
        st = M.stats(cur, ref, R, s, lam)
        assert st["mv"].shape == (2, bh, bw, 2) and st["blocks"] == bh * bw
        whole = M.whole_blocks(H, W, s, *want)
        assert whole.any() == ((H, W) != (16, 32))
        for t in range(2):
            assert (st["mv"][t][whole] == want).all(), (t, st["mv"][t])
            assert (st["bsad"][t][whole][:, 0] == 0).all()
        assert (st["bsad"][..., 0] <= st["bsad"][..., 1]).all()  # (the winner costs no more than the zero vector)
        assert (np.abs(st["mv"]) <= R).all() and (st["border"] <= bh * bw).all()


def test_small_pan_case_moves_without_saturation():
    """the 16x32 (2, 6) pan at R = 8, penalty 16: both blocks move by the pan (the samples of the
    extension cost little in a smooth picture), so rms == sqrt(40) and nothing is saturated -- the
    value the launcher test of tests/test_gpu_motion.py places its edges around"""
    clip = M.pan(16, 32, 2, 6, 2)
    st = M.stats(clip[1:], clip[:-1], 8, 0, 16)
    d = M.derived(st, 0)
    assert st["mv"][0].reshape(-1, 2).tolist() == [[2, 6], [2, 6]]
    assert d["rms"].tolist() == [math.sqrt(40.0)] and d["saturated"].tolist() == [0.0]


def test_a_pan_beyond_the_radius_saturates():
    """a pan of (5, 7) searched at R = 4: every block ends on the border of the search.  48x64 has whole
    blocks only: a partial block is mostly repeated rows or columns, which any vector matches"""
    clip = M.pan(48, 64, 5, 7, 2)
    st = M.stats(clip[1:], clip[:-1], 4, 0, 0)
    assert M.derived(st, 0)["saturated"].tolist() == [1.0]
    assert (np.abs(st["mv"]).max(axis=-1) == 4).all()


@pytest.mark.parametrize("value", [0, 137, 255])
@pytest.mark.parametrize("lam", [0, 16])
def test_flat_frames_give_zero_vectors(value, lam):
    a = np.full((1, 37, 53, 3), value, np.uint8)
    st = M.stats(a, a.copy(), 7, 0, lam)
    assert not st["mv"].any() and not st["bsad"].any() and st["d2"].tolist() == [0] and st["border"].tolist() == [0]
    b = np.full((1, 37, 53, 3), 255 - value, np.uint8)  # every candidate has the same SAD: still (0, 0)
    st = M.stats(a, b, 7, 0, lam)
    assert not st["mv"].any() and st["sad"].tolist() == st["sad0"].tolist() == [abs(255 - 2 * value) * 3 * 4 * 256]


def test_ties_go_to_the_shortest_then_smallest_vector():
    """a ref of vertical stripes of period 4: the SAD is 0 at every dx = 2 (mod 4) and any dy, so the
    winner is the shortest of those, and of the two shortest, (0, -2) and (0, 2), the smaller dx"""
    x = np.arange(64)
    stripes = np.where((x // 2) % 2 == 0, 40, 200).astype(np.uint8)
    ref = np.broadcast_to(stripes[None, :, None], (32, 64, 3)).copy()
    cur = np.roll(ref, 2, axis=1)
    st = M.stats(cur[None], ref[None], 5, 0, 0)
    inner = st["mv"][0][:, 1:-1]  # (the outermost columns of blocks see the clamped extension)
    assert (inner == (0, -2)).all() and (st["bsad"][0][:, 1:-1, 0] == 0).all()
    assert M.candidates(1) == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]


def test_the_penalty_moves_a_tie():
    """ref[y][x] = h(2 x + y) repeats under (dy, dx) = (2, -1), and cur is ref moved by 3 columns: the
    SAD is 0 at (0, 3), (2, 2), (4, 1), (6, 0), (-2, 4), ...  Without a penalty the tie goes to the
    shortest, (2, 2); any penalty prefers (0, 3), whose |dy| + |dx| is smaller"""
    H, W = 48, 80
    h = np.random.RandomState(4).randint(0, 256, 2 * (W + 3) + H).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ref = np.repeat(h[2 * x + y][..., None], 3, axis=2)
    cur = np.repeat(h[2 * (x + 3) + y][..., None], 3, axis=2)
    free = M.stats(cur[None], ref[None], 6, 0, 0)
    assert (free["mv"][0][1, 1:-1] == (2, 2)).all() and (free["bsad"][0][1, 1:-1, 0] == 0).all()
    held = M.stats(cur[None], ref[None], 6, 0, 1)
    assert (held["mv"][0][1, 1:-1] == (0, 3)).all() and (held["bsad"][0][1, 1:-1, 0] == 0).all()


@pytest.mark.parametrize("s", [1, 2, 3])
def test_plane_drops_trailing_rows_and_rounds(s):
    f = np.random.RandomState(s).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    p = M.plane(f, s)
    n = 1 << s
    assert p.shape == (37 >> s, 53 >> s)
    y = M.luma(f).astype(np.float64)
    want = np.floor(y[:p.shape[0] * n, :p.shape[1] * n].reshape(p.shape[0], n, p.shape[1], n).mean(axis=(1, 3)) + 0.5)
    assert np.array_equal(p, want.astype(np.int64))
    e = M.extended(p, -2, p.shape[0] + 3, -1, p.shape[1] + 2)
    assert e[0, 0] == p[0, 0] and e[-1, -1] == p[-1, -1] and np.array_equal(e[2:-3, 1:-2], p)


# ---------------- summarize ----------------
def _cols(n):
    rng = np.random.RandomState(n)
    return dict(position=np.arange(n) % 3 + 1, psnr=rng.rand(n) * 40, ssim=rng.rand(n), acc=rng.rand(n), miou=rng.rand(n))


def test_summarize_buckets():
    n = 8
    c = _cols(n)
    motion = np.array([0.0, 1.9, 2.0, 7.99, 8.0, 8.0, 40.0, 1e9])
    sat, tres, tres_gt = np.linspace(0, 1, n), np.arange(n) + 1.0, np.arange(n) * 0.5
    out = synth.summarize(**c, motion=motion, saturated=sat, tres=tres, tres_gt=tres_gt, edges=(2, 8, 32))
    assert list(out["per_motion"]) == ["0-2", "2-8", "8-32", "32-inf"] == synth.motion_bucket_names((2, 8, 32))
    assert [r["frames"] for r in out["per_motion"].values()] == [2, 2, 2, 2]
    assert sum(r["frames"] for r in out["per_motion"].values()) == out["frames"] == n
    row = out["per_motion"]["2-8"]  # an edge belongs to the bucket it opens
    assert row["motion"] == (2.0 + 7.99) / 2 and row["psnr"] == float(np.mean(c["psnr"][2:4]))
    assert set(row) == set(out["per_position"][1]) == {"psnr", "ssim", "acc", "miou", "motion", "saturated", "tres",
                                                       "tres_gt", "tres_excess", "frames"}
    assert out["tres_excess"] == float(np.mean(tres - tres_gt)) and out["saturated"] == float(np.mean(sat))
    assert out["per_position"][2]["tres_excess"] == float(np.mean((tres - tres_gt)[c["position"] == 2]))
    # empty buckets are omitted
    out = synth.summarize(**c, motion=np.full(n, 3.0), saturated=sat, tres=tres, tres_gt=tres_gt, edges=(2, 8, 32))
    assert list(out["per_motion"]) == ["2-8"] and out["per_motion"]["2-8"]["frames"] == n
    assert synth.motion_bucket_names((0.5, 2.25)) == ["0-0.5", "0.5-2.25", "2.25-inf"]
    # without edges: the columns, no table
    out = synth.summarize(**c, motion=motion, saturated=sat, tres=tres, tres_gt=tres_gt)
    assert "per_motion" not in out and "motion" in out
    with pytest.raises(ValueError):
        synth.summarize(**c, edges=(2, 8))  # buckets of nothing
    for bad in ((), (0, 1), (2, 2), (8, 2), (1, float("inf")), (-1,)):
        with pytest.raises(ValueError):
            synth.motion_bucket_names(bad)


def test_summarize_without_the_new_arguments_is_what_it_was():
    c = _cols(7)
    vgg, ms = np.linspace(0, 1, 7), np.linspace(1, 0, 7)
    out = synth.summarize(**c, vgg=vgg, msssim=ms)
    assert list(out) == ["psnr", "ssim", "acc", "miou", "vgg", "msssim", "frames", "per_position"]
    assert list(out["per_position"][1]) == ["psnr", "ssim", "acc", "miou", "vgg", "msssim", "frames"]
    assert out["psnr"] == float(np.mean(c["psnr"])) and out["per_position"][3]["vgg"] == float(np.mean(vgg[c["position"] == 3]))
    assert list(synth.summarize(**c)) == ["psnr", "ssim", "acc", "miou", "frames", "per_position"]
    assert synth.FrameScores.FIELDS[-1] == "vgg" and len(synth.FrameScores.FIELDS) == 8


# ---------------- MotionSearch and the flags ----------------
def test_motion_search_validation():
    s = synth.MotionSearch()
    assert (s.radius, s.scale, s.penalty) == (16, 0, 16) and repr(s) == "MotionSearch(radius=16, scale=0, penalty=16)"
    assert repr(synth.MotionSearch(32, 3, 1024)) == "MotionSearch(radius=32, scale=3, penalty=1024)"
    assert synth.MotionSearch(1, 0, 0).penalty == 0
    for kw in (dict(radius=0), dict(radius=33), dict(scale=-1), dict(scale=4), dict(penalty=-1), dict(penalty=1025),
               dict(radius=4.0), dict(scale=True), dict(penalty="16")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            synth.MotionSearch(**kw)
    assert synth.motion_grid(37, 53, 0) == (3, 4) and synth.motion_grid(37, 53, 3) == (1, 1)
    assert synth.motion_grid(1080, 1920, 0) == (68, 120) and synth.motion_grid(8, 8, 3) == (1, 1)
    for H, W, sc in ((7, 8, 3), (8, 7, 3), (1, 1, 1), (16, 16, 4)):
        with pytest.raises(ValueError):
            synth.motion_grid(H, W, sc)
    assert "provisional" in synth.MotionSearch.__doc__


def test_options_synth_motion(capsys):
    a = Options().parse(["INTER"])
    assert a.synth_motion is False and a.synth_motion_radius == 16 and a.synth_motion_scale == 0
    assert a.synth_motion_edges == (2.0, 8.0, 32.0)
    a = Options().parse(["--synth_eval", "--synth_motion", "--synth_motion_radius", "32", "--synth_motion_scale", "3",
                         "--synth_motion_edges", "0.5,4", "EXTRA"])
    assert a.synth_motion is True and (a.synth_motion_radius, a.synth_motion_scale) == (32, 3)
    assert a.synth_motion_edges == (0.5, 4.0)
    assert Options().parse(["--synth_motion_radius", "1", "INTER"]).synth_motion_radius == 1
    for flag, bad in (("--synth_motion_radius", "0"), ("--synth_motion_radius", "33"), ("--synth_motion_radius", "4.5"),
                      ("--synth_motion_scale", "-1"), ("--synth_motion_scale", "4"), ("--synth_motion_scale", "x"),
                      ("--synth_motion_edges", "8,2"), ("--synth_motion_edges", "0,2"), ("--synth_motion_edges", "2,,8"),
                      ("--synth_motion_edges", "a"), ("--synth_motion_edges", "2,2"), ("--synth_motion_edges", "inf")):
        with pytest.raises(SystemExit):
            Options().parse([flag, bad, "INTER"])
        assert flag in capsys.readouterr().err
    with pytest.raises(SystemExit):  # the penalty is API-only
        Options().parse(["--synth_motion_penalty", "4", "INTER"])


# ---------------- C ABI ----------------
def test_symbols_and_descriptor_sizes():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_motion", "dvie_synth_motion_ws_bytes"):
        assert name in exported and name in L.EXPORTS and hasattr(lib, name), name
    assert L._ABI_MORE[121] is L.SynthMotionDesc
    assert lib.dvie_abi_sizeof(121) == ctypes.sizeof(L.SynthMotionDesc) == 9 * 8 + 4 * 8 + 8 * 4


def _desc(**kw):
    """a valid descriptor of 2 x 3 pairs of 37x53 frames (the pointers are never followed)"""
    d = L.SynthMotionDesc()
    n = 37 * 53 * 3
    base = dict(cur=4096 + n, ref=4096, d2=64, sad=128, sad0=192, border=256, mv=512, bsad=1024, ws=8192,
                cur_s0=4 * n, cur_s1=n, ref_s0=4 * n, ref_s1=n, n0=2, n1=3, h=37, w=53, radius=7, scale=0, penalty=16)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(cur=None), b"null"), (dict(ref=None), b"null"), (dict(d2=None), b"null"), (dict(sad=None), b"null"),
    (dict(sad0=None), b"null"), (dict(border=None), b"null"), (dict(ws=None), b"workspace"),
    (dict(radius=0), b"radius=0"), (dict(radius=33), b"radius=33"), (dict(radius=-1), b"radius=-1"),
    (dict(scale=-1), b"scale=-1"), (dict(scale=4), b"scale=4"),
    (dict(penalty=-1), b"penalty=-1"), (dict(penalty=1025), b"penalty=1025"),
    (dict(h=0), b"h=0"), (dict(w=0), b"w=0"), (dict(h=(1 << 16) + 1), b"h=65537"), (dict(w=(1 << 16) + 1), b"w=65537"),
    (dict(h=7, scale=3), b"h=7"), (dict(w=3, scale=2), b"w=3"),
    (dict(n0=0), b"n0=0"), (dict(n1=0), b"n1=0"), (dict(n0=256, n1=256), b"n0=256 times n1=256"),
    (dict(n0=65536, n1=65536), b"n0=65536"),
    (dict(mv=None), b"together"), (dict(bsad=None), b"together"),
    (dict(ws=8200), b"aligned"), (dict(sad=132), b"aligned"), (dict(mv=513), b"aligned"), (dict(bsad=1026), b"aligned"),
])
def test_argument_validation_without_gpu(kw, word):
    lib = L.load()
    assert lib.dvie_synth_motion(ctypes.byref(_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())
    if not {"h", "w", "n0", "n1", "radius", "scale"}.isdisjoint(kw):
        assert lib.dvie_synth_motion_ws_bytes(ctypes.byref(_desc(**kw))) == 0


def test_null_descriptor_and_workspace_size():
    lib = L.load()
    assert lib.dvie_synth_motion(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    assert lib.dvie_synth_motion_ws_bytes(None) == 0

    def size(n0, n1, h, w, R, s):
        hs, ws = h >> s, w >> s
        bh, bw = -(-hs // 16), -(-ws // 16)
        groups = -(-bw // 4)
        up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
        cur = n0 * n1 * 16 * bh * 64 * groups
        ref = n0 * n1 * (16 * bh + 2 * R) * ((64 * groups + 2 * R + 3) // 4 * 4 + 4)
        return up16(cur) + up16(ref) + 16 * n0 * n1 * bh * bw

    for n0, n1, h, w, R, s in ((2, 3, 37, 53, 7, 0), (1, 1, 1, 1, 1, 0), (1, 2, 1080, 1920, 16, 0), (1, 2, 1080, 1920, 32, 1),
                               (1, 1, 8, 8, 3, 3), (255, 257, 20, 130, 5, 1), (1, 1, 1 << 16, 1 << 16, 32, 0)):
        got = lib.dvie_synth_motion_ws_bytes(ctypes.byref(_desc(n0=n0, n1=n1, h=h, w=w, radius=R, scale=s)))
        assert got == size(n0, n1, h, w, R, s) > 0, (n0, n1, h, w, R, s)
    # the outputs, the penalty and the pointers do not enter the size
    assert lib.dvie_synth_motion_ws_bytes(ctypes.byref(_desc(penalty=-5, mv=None, ws=None))) == size(2, 3, 37, 53, 7, 0)
    # a valid descriptor with mv and bsad both absent passes every check up to the launch, which this
    # test does not reach: only the checks are exercised here
    assert lib.dvie_synth_motion(ctypes.byref(_desc(mv=None, bsad=None, ws=None)), None) == L.DVIE_EINVAL
    assert b"workspace" in lib.dvie_last_error()
