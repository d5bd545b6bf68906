"""CPU checks (no launch) of streaming and Y4M: synth.window_plan, the Y4M reader and writer
(video_io), the integer conversion tables against the float64 formulas (tests/yuv_ref.py), the
--synth_window / --synth_yuv options, the two I/O worker threads, and the exports, descriptor size
and argument validation of dvie_synth_yuv2rgb / dvie_synth_rgb2yuv."""
import ctypes
import io
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth, video_io
from deep_video_interpolation_extrapolation_amd.options import Options
from deep_video_interpolation_extrapolation_amd.video_io import Y4MReader, Y4MWriter, frame_bytes, plane_shapes
import yuv_ref as R

COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


# ---------------- window_plan ----------------
@pytest.mark.parametrize("T,window", [(2, 2), (2, 5), (3, 3), (4, 3), (5, 3), (7, 3), (13, 3), (16, 16), (17, 16),
                                      (65, 16), (6, 2)])
def test_window_plan_covers_the_clip(T, window):
    plan = synth.window_plan(T, window)
    assert plan[0][0] == 0 and plan[-1][1] == T - 1
    for (a0, a1), (b0, b1) in zip(plan, plan[1:]):
        assert b0 == a1  # neighbours share exactly one frame
    for k, (t0, t1) in enumerate(plan):
        assert 2 <= t1 - t0 + 1 <= window
        assert t1 - t0 + 1 == window or k == len(plan) - 1  # only the last window may be shorter
    assert sorted(set(t for t0, t1 in plan for t in range(t0, t1 + 1))) == list(range(T))


def test_window_plan_cases_and_errors():
    assert synth.window_plan(5, 5) == [(0, 4)]  # T = window
    assert synth.window_plan(6, 5) == [(0, 4), (4, 5)]  # T = window + 1: a last window of two frames
    assert synth.window_plan(2, 16) == [(0, 1)]
    assert synth.window_plan(7, 3) == [(0, 2), (2, 4), (4, 6)]
    for T, w in ((1, 3), (0, 3), (5, 1), (5, 0), (5, -2)):
        with pytest.raises(ValueError):
            synth.window_plan(T, w)


# ---------------- Y4M ----------------
class _Pipe(io.RawIOBase):
    """a non-seekable reader that hands out at most 7 bytes per read, as a pipe may"""

    def __init__(self, data):
        self._b = io.BytesIO(data)

    def readable(self):
        return True

    def seekable(self):
        return False

    def seek(self, *a):
        raise io.UnsupportedOperation("seek")

    def tell(self):
        raise io.UnsupportedOperation("tell")

    def read(self, n=-1):
        return self._b.read(min(n, 7) if n is not None and n >= 0 else 7)


def _stream(header, frames, marker=b"FRAME\n"):
    return header + b"".join(marker + bytes(f) for f in frames)


def test_layout_is_computed_in_one_place():
    assert frame_bytes(5, 3, "C420") == 27 and plane_shapes(5, 3, "C420jpeg") == [(3, 5), (2, 3), (2, 3)]
    assert frame_bytes(32, 16, "C420mpeg2") == 768 and frame_bytes(5, 3, "C444") == 45 and frame_bytes(5, 3, "Cmono") == 15
    assert plane_shapes(1, 1, "C420paldv") == [(1, 1), (1, 1), (1, 1)] and plane_shapes(4, 2, "Cmono") == [(2, 4)]
    for tag in ("C422", "C420p10", "C444alpha", "420"):
        with pytest.raises(ValueError, match=tag):
            frame_bytes(4, 4, tag)


@pytest.mark.parametrize("tag", ["C420", "C420jpeg", "C420mpeg2", "C420paldv", "C444", "Cmono", None])
@pytest.mark.parametrize("pipe", [False, True])
def test_header_and_frames_round_trip(tag, pipe):
    W, H = 5, 3
    cs = tag or "C420"
    fb = frame_bytes(W, H, cs)
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, (4, fb)).astype(np.uint8)
    head = b"YUV4MPEG2 W5 H3 F30000:1001 Ip A1:1" + (b" " + tag.encode() if tag else b"") + b" XYSCSS=420JPEG\n"
    data = _stream(head, frames, marker=b"FRAME Ip Xfoo=1\n")  # FRAME parameters are skipped
    r = Y4MReader(_Pipe(data) if pipe else io.BytesIO(data))
    assert (r.width, r.height, r.fps, r.colourspace, r.full_range, r.frame_bytes) == (W, H, (30000, 1001), cs, False, fb)
    got = r.read(3)
    assert got.dtype == np.uint8 and got.shape == (3, fb) and np.array_equal(got, frames[:3])
    assert np.array_equal(r.read(5), frames[3:]) and r.read(2).shape == (0, fb) and r.read(1).shape == (0, fb)
    # and through the writer
    buf = io.BytesIO()
    w = Y4MWriter(buf, W, H, (30000, 1001), cs, False)
    w.write(frames[:1])
    w.write(frames[1:])
    w.close()
    assert b"XCOLORRANGE" not in buf.getvalue().split(b"\n")[0]
    r2 = Y4MReader(io.BytesIO(buf.getvalue()))
    assert (r2.width, r2.height, r2.fps, r2.colourspace, r2.full_range) == (W, H, (30000, 1001), cs, False)
    assert np.array_equal(r2.read(10), frames)


def test_colour_range_tag():
    fb = frame_bytes(4, 2, "C420")
    for tag, full in ((b" XCOLORRANGE=FULL", True), (b" XCOLORRANGE=LIMITED", False), (b"", False)):
        r = Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2 F25:1 I? C420jpeg" + tag + b"\n"))
        assert r.full_range is full and r.frame_bytes == fb and r.read(1).shape == (0, fb)
    buf = io.BytesIO()
    Y4MWriter(buf, 4, 2, (50, 1), "C444", True).close()
    head = buf.getvalue().split(b"\n")[0].split()
    assert head[0] == b"YUV4MPEG2" and b"W4" in head and b"H2" in head and b"F50:1" in head and b"C444" in head
    assert b"XCOLORRANGE=FULL" in head
    assert Y4MReader(io.BytesIO(buf.getvalue())).full_range is True
    with pytest.raises(ValueError):
        Y4MWriter(io.BytesIO(), 4, 2, (25, 1), "C420").write(np.zeros((1, fb + 1), dtype=np.uint8))


def test_reader_refusals():
    for tag in ("C422", "C420p10", "C444alpha"):
        with pytest.raises(ValueError, match=tag):
            Y4MReader(io.BytesIO(f"YUV4MPEG2 W4 H2 F25:1 Ip {tag}\n".encode()))
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=tag):
            Y4MReader(io.BytesIO(f"YUV4MPEG2 W4 H2 F25:1 {tag} C420\n".encode()))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        Y4MReader(io.BytesIO(b"RIFF....AVI \n"))
    with pytest.raises(ValueError):
        Y4MReader(io.BytesIO(b"YUV4MPEG2 H2 F25:1\n"))  # no width


def test_truncated_frame_names_its_index():
    fb = frame_bytes(4, 2, "C420")
    frames = np.arange(3 * fb, dtype=np.uint8).reshape(3, fb)
    data = _stream(b"YUV4MPEG2 W4 H2 F25:1\n", frames)[:-5]
    r = Y4MReader(io.BytesIO(data))
    assert np.array_equal(r.read(2), frames[:2])
    with pytest.raises(ValueError, match=r"frame 2 is truncated"):
        r.read(1)
    r = Y4MReader(io.BytesIO(_stream(b"YUV4MPEG2 W4 H2 F25:1\n", frames[:1]) + b"FRAMF\n" + bytes(fb)))
    with pytest.raises(ValueError, match=r"frame 1.*FRAME"):
        r.read(2)


def test_y4m_clip_chunks_follow_the_window_plan(tmp_path):
    W, H, T = 6, 4, 8
    rng = np.random.RandomState(5)
    rgb = rng.randint(0, 256, (T, frame_bytes(W, H, "C420"))).astype(np.uint8)
    seg = rng.randint(0, 20, (T, frame_bytes(W, H, "Cmono"))).astype(np.uint8)
    for sub, cs, arr in (("rgb", "C420", rgb), ("seg", "Cmono", seg)):
        (tmp_path / sub).mkdir()
        with Y4MWriter(str(tmp_path / sub / "a.y4m"), W, H, (25, 1), cs) as w:
            w.write(arr)
    for window in (3, 8, 9, 0):
        clip = video_io.Y4MClip(str(tmp_path / "rgb"), str(tmp_path / "seg"), "a.y4m")
        chunks = list(clip.chunks(window))
        clip.close()
        plan = synth.window_plan(T, window) if window else [(0, T - 1)]
        assert [c[0].shape[0] for c in chunks] == [t1 - t0 + (k == 0) for k, (t0, t1) in enumerate(plan)]
        assert np.array_equal(np.concatenate([c[0] for c in chunks]), rgb)
        assert np.array_equal(np.concatenate([c[1] for c in chunks]), seg)


# ---------------- the integer tables ----------------
def test_tables_are_the_rounded_coefficients():
    inv, fwd, yo = synth.yuv_tables("bt601", False)
    assert yo == 16 and inv == (76309, 104597, 132201, 25675, 53279)
    assert fwd[:3] == (16829, 33039, 6416) and fwd[5] == fwd[6] == 28784  # 0.5 * 224 / 255 * 65536
    inv, fwd, yo = synth.yuv_tables("bt709", True)
    assert yo == 0 and inv[0] == 65536 and fwd[5] == fwd[6] == 32768
    assert fwd[:3] == (round(65536 * 0.2126), round(65536 * 0.7152), round(65536 * 0.0722))
    for m, fr in COMBOS:
        inv, fwd, yo = synth.yuv_tables(m, fr)
        assert len(inv) == 5 and len(fwd) == 9 and all(isinstance(v, int) and abs(v) <= 1 << 18 for v in inv + fwd)
    with pytest.raises(ValueError):
        synth.yuv_tables("bt2020", False)


def _all_triples(lo):
    """the 2^20 triples (a, b, c) with a in lo .. lo + 15: a (2^20, 3) uint8 array"""
    a, b, c = np.meshgrid(np.arange(lo, lo + 16), np.arange(256), np.arange(256), indexing="ij")
    return np.stack([a.ravel(), b.ravel(), c.ravel()], -1).astype(np.uint8)


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_integer_forms_are_within_one_of_the_float64_forms_exhaustively(matrix, full_range):
    """all 2^24 (Y, U, V) and all 2^24 (R, G, B), in 16 slices: the Q16 coefficients move the real
    value by < 0.01, so the integer result and rint of the float64 one differ only next to a tie"""
    worst = [0, 0]
    for lo in range(0, 256, 16):
        t = _all_triples(lo)
        got = R.yuv2rgb_values(t[:, 0], t[:, 1], t[:, 2], matrix, full_range).astype(np.int64)
        want = np.clip(np.rint(R.yuv2rgb_float(t[:, 0], t[:, 1], t[:, 2], matrix, full_range)), 0, 255).astype(np.int64)
        worst[0] = max(worst[0], int(np.abs(got - want).max()))
        got = R.rgb2yuv_values(t, matrix, full_range).astype(np.int64)
        want = np.clip(np.rint(R.rgb2yuv_float(t, matrix, full_range)), 0, 255).astype(np.int64)
        worst[1] = max(worst[1], int(np.abs(got - want).max()))
    print(f"{matrix} full={full_range}: max |int - rint(float64)| yuv->rgb {worst[0]}, rgb->yuv {worst[1]}")
    assert worst[0] <= 1 and worst[1] <= 1


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_grey_and_primaries(matrix):
    grey = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128]], dtype=np.uint8)
    lim = R.rgb2yuv_values(grey, matrix, False)
    assert lim[:, 0].tolist() == [16, 235, 126] and (lim[:, 1:] == 128).all()
    full = R.rgb2yuv_values(grey, matrix, True)
    assert full[:, 0].tolist() == [0, 255, 128] and (full[:, 1:] == 128).all()
    # and back: black and white exactly
    for fr, y in ((False, (16, 235)), (True, (0, 255))):
        rgb = R.yuv2rgb_values(np.array(y), np.array([128, 128]), np.array([128, 128]), matrix, fr)
        assert rgb.tolist() == [[0, 0, 0], [255, 255, 255]]
    # the primaries land on the extreme chroma values: blue U = 240 (limited) / 255 (full, 128 + 127.5 clipped)
    prim = np.array([[255, 0, 0], [0, 0, 255]], dtype=np.uint8)
    assert R.rgb2yuv_values(prim, matrix, False)[0, 2] == 240 and R.rgb2yuv_values(prim, matrix, False)[1, 1] == 240
    assert R.rgb2yuv_values(prim, matrix, True)[0, 2] == 255 and R.rgb2yuv_values(prim, matrix, True)[1, 1] == 255


def test_packed_references_agree_with_the_per_pixel_form():
    """4:4:4 packed frames are the per-pixel values plane by plane; a 4:2:0 block of equal pixels
    has the per-pixel chroma (the sum over n pixels times 4 / n is 4 times the pixel); odd sizes"""
    rng = np.random.RandomState(7)
    rgb = rng.randint(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    p = R.rgb2yuv_int(rgb, "C444", "bt709", False)
    assert np.array_equal(p.reshape(2, 3, 5, 7).transpose(0, 2, 3, 1), R.rgb2yuv_values(rgb, "bt709", False))
    flat = np.repeat(np.repeat(rgb[:, :3, :4], 2, axis=1), 2, axis=2)[:, :5, :7]  # 2x2 blocks of one colour, cut odd
    p = R.rgb2yuv_int(flat, "C420", "bt601", True)
    Y, U, V = R.split_planes(p, 5, 7, "C420")
    want = R.rgb2yuv_values(rgb[:, :3, :4], "bt601", True)
    assert np.array_equal(U, want[..., 1]) and np.array_equal(V, want[..., 2])
    back = R.yuv2rgb_int(p, 5, 7, "C420", "bt601", True)
    assert back.shape == (2, 5, 7, 3) and np.abs(back.astype(int) - flat).max() <= 2


# ---------------- options ----------------
def test_options_synth_window_and_synth_yuv(capsys):
    assert Options().parse(["INTER"]).synth_window == 0 and Options().parse(["EXTRA"]).synth_yuv == "bt601"
    assert Options().parse(["--synth_window", "0", "INTER"]).synth_window == 0
    assert Options().parse(["--synth_window", "2", "INTER"]).synth_window == 2
    assert Options().parse(["--synth_window", "16", "--synth_yuv", "bt709", "EXTRA"]).synth_yuv == "bt709"
    for bad in ("1", "-3"):
        with pytest.raises(SystemExit):
            Options().parse(["--synth_window", bad, "INTER"])
    assert "at least 2" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        Options().parse(["--synth_yuv", "bt2020", "INTER"])
    # reference command lines still parse
    a = Options().parse(["--dataset", "cityscape", "--split", "val", "--bs", "4", "--syn_type", "inter", "INTER",
                         "--model", "InterNet", "--load_coarse"])
    assert a.batch_size == 4 and a.synth_window == 0 and a.synth_yuv == "bt601"


# ---------------- the worker threads ----------------
def test_prefetcher_keeps_order_and_raises_in_place():
    def gen():
        yield 1
        yield 2
        raise FileNotFoundError("frame 3 is missing")

    with video_io.Prefetcher(gen()) as p:
        it = iter(p)
        assert next(it) == 1 and next(it) == 2
        with pytest.raises(FileNotFoundError, match="frame 3"):
            next(it)
    with video_io.Prefetcher(iter(range(5))) as p:
        assert list(p) == [0, 1, 2, 3, 4]


def test_prefetcher_close_frees_a_worker_blocked_on_a_full_queue():
    made = []

    def gen():
        for k in range(100):
            made.append(k)
            yield k

    p = video_io.Prefetcher(gen())
    assert next(iter(p)) == 0
    p.close()  # (the consumer failed: the worker sits on a full queue)
    assert not p._t.is_alive() and len(made) <= 2 + video_io.QUEUE_DEPTH + 1 and video_io.QUEUE_DEPTH == 2


def test_background_writer_order_and_error():
    seen = []
    with video_io.BackgroundWriter(seen.append) as w:
        for k in range(7):
            w.put(k)
    assert seen == list(range(7))

    def fail(item):
        if item == 2:
            raise OSError("disk full")
        seen.append(item)

    w = video_io.BackgroundWriter(fail)
    with pytest.raises(OSError, match="disk full"):
        for k in range(50):  # far more than the queue holds: put() must not block after the failure
            w.put(k)
        w.close()
    w.close(drop_error=True)
    assert not w._t.is_alive() and threading.active_count() < 50


# ---------------- C ABI ----------------
def _desc(**kw):
    """a valid descriptor of 3 frames of 17x33, 4:2:0 (the pointers are never followed)"""
    d = L.SynthYuvDesc()
    fb = frame_bytes(33, 17, "C420")
    base = dict(yuv=64, rgb=64, yuv_stride=fb, rgb_stride=17 * 33 * 3, rgb_row_stride=33 * 3, n=3, h=17, w=33,
                layout=L.YUV_420, yo=16)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_symbols_and_descriptor_size():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_yuv2rgb", "dvie_synth_rgb2yuv"):
        assert name in exported and name in L.EXPORTS and hasattr(lib, name), name
    assert L._ABI_MORE[112] is L.SynthYuvDesc
    assert lib.dvie_abi_sizeof(112) == ctypes.sizeof(L.SynthYuvDesc) == 112


@pytest.mark.parametrize("fn", ["dvie_synth_yuv2rgb", "dvie_synth_rgb2yuv"])
@pytest.mark.parametrize("kw,word", [
    (dict(yuv=None), b"null"), (dict(rgb=None), b"null"),
    (dict(h=0), b"must be in"), (dict(w=0), b"must be in"), (dict(w=(1 << 16) + 1), b"must be in"),
    (dict(n=0), b"frames"), (dict(layout=422), b"layout"), (dict(layout=0), b"layout"),
    (dict(yo=256), b"yo"), (dict(rgb_row_stride=33 * 3 - 1), b"rgb_row_stride"),
    (dict(yuv_stride=frame_bytes(33, 17, "C420") - 1), b"yuv_stride"), (dict(rgb_stride=17 * 33 * 3 - 1), b"rgb_stride"),
    (dict(n=1 << 20, h=1 << 16, w=1 << 16, yuv_stride=1 << 40, rgb_stride=1 << 40, rgb_row_stride=3 << 16), b"too many"),
])
def test_argument_validation_without_gpu(fn, kw, word):
    lib = L.load()
    assert getattr(lib, fn)(ctypes.byref(_desc(**kw)), None) == L.DVIE_EINVAL, kw
    assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())


def test_null_descriptor_and_table_range():
    lib = L.load()
    assert lib.dvie_synth_yuv2rgb(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    d = _desc()
    d.table[4] = (1 << 18) + 1
    assert lib.dvie_synth_yuv2rgb(ctypes.byref(d), None) == L.DVIE_EINVAL and b"table[4]" in lib.dvie_last_error()
    d.table[4], d.table[8] = 0, -(1 << 18) - 1
    assert lib.dvie_synth_rgb2yuv(ctypes.byref(d), None) == L.DVIE_EINVAL and b"table[8]" in lib.dvie_last_error()


def test_conversions_refuse_cpu_tensors_and_bad_arguments():
    packed = torch.zeros((2, frame_bytes(32, 16, "C420")), dtype=torch.uint8)
    with pytest.raises(L.DvieError):
        synth.yuv_to_rgb(packed, 16, 32, "C420")
    with pytest.raises(L.DvieError):
        synth.rgb_to_yuv(torch.zeros((2, 16, 32, 3), dtype=torch.uint8), "C420", "bt601", False)
