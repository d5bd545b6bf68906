"""Clip I/O on the host: YUV4MPEG2 ("Y4M") files and pipes, and the two worker threads that
overlap a windowed run's file work with the device (synth.VideoSynthesizer.interpolate_stream).

Y4M is a text header line, then per frame a `FRAME` line and the raw planes:

    YUV4MPEG2 W<w> H<h> F<num>:<den> [I<p|?>] [A<n>:<d>] [C<colourspace>] [X<comment>] ...
    FRAME [params]\\n  <Y plane h*w bytes> <U plane> <V plane>

The 8-bit colourspaces are read: C420, C420jpeg, C420mpeg2 and C420paldv (all as 4:2:0 with chroma
planes of ((h+1)//2, (w+1)//2); the three differ only in where the chroma samples sit, which is
ignored here -- chroma is one sample per 2x2 block), C444 and Cmono; no C tag means C420.  Y4M has
no tag for the colour matrix; the range comes from the XCOLORRANGE=FULL|LIMITED comment that ffmpeg
writes (limited when absent).  `frame_bytes` / `plane_shapes` are the one place the layout of a
packed frame is computed; the device-side conversion (synth.yuv_to_rgb / rgb_to_yuv) reads the
same layout.  A label clip is a Y4M whose Y plane holds the class ids (Cmono is the natural form;
the chroma of any other colourspace is ignored).

Nothing here touches the device: `Prefetcher` and `BackgroundWriter` run file reads, decoding and
encoding on one thread each, behind bounded queues; every HIP call stays with the caller."""
import queue
import threading
import time

import numpy as np

MAGIC = b"YUV4MPEG2"
_LAYOUT = {"C420": "420", "C420jpeg": "420", "C420mpeg2": "420", "C420paldv": "420", "C444": "444", "Cmono": "mono"}


def layout_of(colourspace):
    """"420", "444" or "mono" of an accepted colourspace tag; ValueError naming any other tag"""
    try:
        return _LAYOUT[colourspace]
    except KeyError:
        raise ValueError(f"Y4M colourspace {colourspace!r} is not supported (8-bit {', '.join(_LAYOUT)} are)") from None


def plane_shapes(W, H, colourspace):
    """the (rows, columns) of the planes of one packed frame, in file order"""
    if W < 1 or H < 1:
        raise ValueError(f"Y4M frames need W, H >= 1, got {W}x{H}")
    lay = layout_of(colourspace)
    if lay == "mono":
        return [(H, W)]
    c = ((H + 1) // 2, (W + 1) // 2) if lay == "420" else (H, W)
    return [(H, W), c, c]


def frame_bytes(W, H, colourspace):
    """bytes of one packed frame"""
    return sum(h * w for h, w in plane_shapes(W, H, colourspace))


def _read_exact(f, n):
    """up to n bytes of f (fewer only at the end of the file); a pipe may return short reads"""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return b"".join(parts)


def _read_line(f, limit=4096):
    """bytes up to and without the next newline; None at the end of the file (nothing read)"""
    out = bytearray()
    while True:
        b = f.read(1)
        if not b:
            if not out:
                return None
            raise ValueError(f"Y4M: the file ends inside a header line ({bytes(out)[:32]!r}...)")
        if b == b"\n":
            return bytes(out)
        out += b
        if len(out) > limit:
            raise ValueError("Y4M: a header line of more than %d bytes" % limit)


class Y4MReader:
    """Reads a YUV4MPEG2 stream from a path or a binary file object (a pipe works: nothing seeks).

    width, height, fps (num, den), colourspace (the C tag, "C420" when absent), full_range (bool:
    XCOLORRANGE=FULL), interlace, frame_bytes.  read(n) -> up to n frames as one (k, frame_bytes)
    uint8 array; k == 0 at the end of the file."""

    def __init__(self, path_or_file):
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "rb") if self._own else path_or_file
        try:
            self._header()
        except Exception:
            self.close()
            raise
        self.index = 0  # frames read so far

    def _header(self):
        line = _read_line(self._f)
        tokens = (line or b"").decode("ascii", errors="replace").split()
        if not tokens or tokens[0] != MAGIC.decode():
            raise ValueError(f"not a YUV4MPEG2 stream (it starts with {(line or b'')[:16]!r})")
        self.width = self.height = None
        self.fps, self.colourspace, self.full_range, self.interlace = (0, 0), "C420", False, "Ip"
        for t in tokens[1:]:
            key, val = t[0], t[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                num, _, den = val.partition(":")
                self.fps = (int(num), int(den or 1))
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"Y4M interlacing {t!r} is not supported (Ip or I? only)")
                self.interlace = t
            elif key == "C":
                layout_of(t)  # (ValueError naming the tag)
                self.colourspace = t
            elif key == "X" and val.startswith("COLORRANGE="):
                rng = val[len("COLORRANGE="):]
                if rng not in ("FULL", "LIMITED"):
                    raise ValueError(f"Y4M: {t!r} must be XCOLORRANGE=FULL or XCOLORRANGE=LIMITED")
                self.full_range = rng == "FULL"
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise ValueError(f"Y4M header without a valid W and H: {line!r}")
        self.frame_bytes = frame_bytes(self.width, self.height, self.colourspace)

    def read(self, n):
        out = np.empty((max(n, 0), self.frame_bytes), dtype=np.uint8)
        k = 0
        while k < n:
            line = _read_line(self._f)
            if line is None:
                break
            if line != b"FRAME" and not line.startswith(b"FRAME "):  # (parameters after the marker are skipped)
                raise ValueError(f"Y4M frame {self.index}: expected a FRAME marker, got {line[:16]!r}")
            data = _read_exact(self._f, self.frame_bytes)
            if len(data) != self.frame_bytes:
                raise ValueError(f"Y4M frame {self.index} is truncated: {len(data)} of {self.frame_bytes} bytes")
            out[k] = np.frombuffer(data, dtype=np.uint8)
            k += 1
            self.index += 1
        return out[:k]

    def close(self):
        if self._own and self._f is not None:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes a YUV4MPEG2 stream to a path or a binary file object: the header at once (progressive;
    XCOLORRANGE=FULL only for full range), then write(frames (k, frame_bytes) uint8)."""

    def __init__(self, path_or_file, width, height, fps, colourspace="C420", full_range=False):
        self.width, self.height, self.fps = int(width), int(height), (int(fps[0]), int(fps[1]))
        self.colourspace, self.full_range = colourspace, bool(full_range)
        self.frame_bytes = frame_bytes(self.width, self.height, colourspace)
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        head = f"YUV4MPEG2 W{self.width} H{self.height} F{self.fps[0]}:{self.fps[1]} Ip A0:0 {colourspace}"
        if self.full_range:
            head += " XCOLORRANGE=FULL"
        self._f.write(head.encode("ascii") + b"\n")
        self.index = 0

    def write(self, frames):
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != self.frame_bytes:
            raise ValueError(f"Y4MWriter.write: uint8 (k, {self.frame_bytes}), got {frames.shape} {frames.dtype}")
        for k in range(frames.shape[0]):
            self._f.write(b"FRAME\n")
            self._f.write(np.ascontiguousarray(frames[k]).data)
            self.index += 1

    def close(self):
        if self._f is not None:
            self._f.flush()
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------- overlapped I/O ----------------
QUEUE_DEPTH = 2
DECODE_THREADS = 8  # the most threads a window's PNGs are decoded on (fixed: not sized from the CPU count)


class Prefetcher:
    """Iterates `items` (an iterable whose work is file reads and decoding) on one worker thread,
    at most `depth` finished items ahead of the consumer.  An exception in the worker is raised by
    the iteration, in its place in the order; close() (also on leaving a `with`) stops the worker
    wherever it is, so that a consumer that fails never leaves it blocked on a full queue.
    `busy`: seconds the worker spent producing; `waited`: seconds the consumer waited for it."""

    def __init__(self, items, depth=QUEUE_DEPTH):
        self._q = queue.Queue(maxsize=depth)
        self._stop = threading.Event()
        self.busy = self.waited = 0.0
        self._t = threading.Thread(target=self._run, args=(items,), daemon=True, name="dvie-reader")
        self._t.start()

    def _put(self, item):
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _run(self, items):
        try:
            it = iter(items)
            while True:
                t0 = time.perf_counter()
                try:
                    item = next(it)
                except StopIteration:
                    break
                finally:
                    self.busy += time.perf_counter() - t0
                if not self._put(("item", item)):
                    return
            self._put(("end", None))
        except BaseException as e:  # noqa: B902  (handed to the consumer, which raises it)
            self._put(("error", e))

    def __iter__(self):
        while True:
            t0 = time.perf_counter()
            kind, val = self._q.get()
            self.waited += time.perf_counter() - t0
            if kind == "end":
                return
            if kind == "error":
                raise val
            yield val

    def close(self):
        self._stop.set()
        self._t.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BackgroundWriter:
    """Calls fn(item) (encoding and file writes) on one worker thread for every item put(), in
    order, at most `depth` items behind the producer.  After fn raised, the worker drops what
    follows instead of blocking the producer, and the next put() or close() raises the exception
    on the caller's thread.  close() waits for everything put so far.
    `busy`: seconds spent in fn; `waited`: seconds put() waited for room."""

    def __init__(self, fn, depth=QUEUE_DEPTH):
        self._fn, self._q = fn, queue.Queue(maxsize=depth)
        self.error = None
        self.busy = self.waited = 0.0
        self._t = threading.Thread(target=self._run, daemon=True, name="dvie-writer")
        self._t.start()

    def _run(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            if self.error is None:
                t0 = time.perf_counter()
                try:
                    self._fn(item[0])
                except BaseException as e:  # noqa: B902  (raised by put() / close())
                    self.error = e
                self.busy += time.perf_counter() - t0

    def _raise(self):
        if self.error is not None:
            raise self.error

    def put(self, item):
        self._raise()
        t0 = time.perf_counter()
        self._q.put((item,))
        self.waited += time.perf_counter() - t0
        self._raise()

    def close(self, drop_error=False):
        if self._t.is_alive():
            self._q.put(None)
            self._t.join()
        if not drop_error:
            self._raise()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        self.close(drop_error=exc_type is not None)  # (an exception already on its way wins)


# ---------------- clips: where a run's frames come from and go to ----------------
class PngClip:
    """A clip as a directory of PNGs <img_dir>/<clip>/*.png with its label maps under the same names
    in <seg_dir>/<clip>: all PNGs in sorted order."""
    kind = "png"

    def __init__(self, img_dir, seg_dir, clip):
        import os
        self.name = clip
        self.img_dir, self.seg_dir = os.path.join(img_dir, clip), os.path.join(seg_dir, clip)
        self.names = sorted(f for f in os.listdir(self.img_dir) if f.lower().endswith(".png"))
        self.T = len(self.names)

    def _decode(self, name):
        import os
        from PIL import Image
        return (np.asarray(Image.open(os.path.join(self.img_dir, name)).convert("RGB")),
                np.asarray(Image.open(os.path.join(self.seg_dir, name)).convert("L")))

    def chunks(self, window):
        """per window of window_plan(T, window) the frames not read yet -- (imgs (t, H, W, 3), labels
        (t, H, W)) uint8 -- decoded on at most DECODE_THREADS threads"""
        from concurrent.futures import ThreadPoolExecutor
        from .synth import window_plan
        if self.T < 2:
            raise ValueError(f"{self.name}: a clip needs at least two frames")
        with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
            for k, (t0, t1) in enumerate(window_plan(self.T, window)):
                pairs = list(pool.map(self._decode, self.names[t0 + (k > 0):t1 + 1]))
                yield np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


class PngSink:
    """writes <root>/{rgb,seg,vis_seg}/<clip>/NNNN.png, numbered in output order across windows;
    write((first number, frames (S, H, W, 3), labels (S, H, W)))"""

    def __init__(self, root, clip, palette):
        import os
        self.dirs = [os.path.join(root, sub, clip) for sub in ("rgb", "seg", "vis_seg")]
        for d in self.dirs:
            os.makedirs(d, exist_ok=True)
        self.palette = palette

    def write(self, item):
        import os
        from PIL import Image
        g0, frames, labels = item
        vis = self.palette[np.minimum(labels, len(self.palette) - 1)]  # (ids past the classes: "none")
        for d, arr in zip(self.dirs, (frames, labels, vis)):
            for k in range(arr.shape[0]):
                Image.fromarray(np.ascontiguousarray(arr[k])).save(os.path.join(d, "{:04d}.png".format(g0 + k)))

    def close(self):
        pass


class Y4MClip:
    """A clip as a file <img_dir>/<name>.y4m with its label maps in <seg_dir>/<name>.y4m (the Y plane
    is the class id).  Both headers are read at once; the frames stream."""
    kind = "y4m"

    def __init__(self, img_dir, seg_dir, fname):
        import os
        self.name = os.path.splitext(fname)[0]
        self.rgb = Y4MReader(os.path.join(img_dir, fname))
        try:
            if layout_of(self.rgb.colourspace) == "mono":
                raise ValueError(f"{fname}: a Cmono stream has no colour; the frames need C420* or C444")
            self.seg = Y4MReader(os.path.join(seg_dir, fname))
        except Exception:
            self.rgb.close()
            raise
        self.width, self.height = self.rgb.width, self.rgb.height
        if (self.seg.width, self.seg.height) != (self.width, self.height):
            self.close()
            raise ValueError(f"{fname}: the labels are {self.seg.width}x{self.seg.height}, the frames "
                             f"{self.width}x{self.height}")

    def chunks(self, window):
        """the frames not read yet of every window of `window` input frames -- (packed frames
        (t, frame_bytes), packed label frames (t, the label stream's frame_bytes)) -- until the
        file ends; window 0: the whole clip as one chunk"""
        first = True
        while True:
            n = (window if first else window - 1) if window else 64
            parts = [self.rgb.read(n)]
            while not window and parts[-1].shape[0]:
                parts.append(self.rgb.read(n))
            packed = np.concatenate(parts) if len(parts) > 1 else parts[0]
            if not packed.shape[0]:
                return
            labels = self.seg.read(packed.shape[0])
            if labels.shape[0] != packed.shape[0]:
                raise ValueError(f"{self.name}: the label stream ends at frame {self.seg.index}, before the frames do")
            yield packed, labels
            first = False
            if not window:
                return

    def close(self):
        self.rgb.close()
        if getattr(self, "seg", None) is not None:
            self.seg.close()


class Y4MSink:
    """writes <root>/{rgb,seg,vis_seg}/<clip>.y4m: the frames in the input's colourspace and range,
    the labels as Cmono, their colouring as C444; write((packed frames, labels (S, H * W), packed
    colouring))"""

    def __init__(self, root, clip, width, height, fps, colourspace, full_range):
        import os
        self.writers = []
        for sub, cs in (("rgb", colourspace), ("seg", "Cmono"), ("vis_seg", "C444")):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
            self.writers.append(Y4MWriter(os.path.join(root, sub, clip + ".y4m"), width, height, fps, cs,
                                          full_range and sub != "seg"))

    def write(self, item):
        for w, arr in zip(self.writers, item):
            w.write(arr)

    def close(self):
        for w in self.writers:
            w.close()
