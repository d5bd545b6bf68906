"""Frame-rate conversion gather micro-benchmark through the C ABI.

Times dvie_synth_retime on 1080x1920x3 frames, 60 output rows per call, in three cases -- `blend`
(every row the cross-fade of two slots), `nearest` (every row a copy) and `flags` (the blend rows with
cut flags on the device, every third pair flagged) -- and, as the yardstick on the same machine,
dvie_synth_cutfill, the pure-copy kernel, moving the same 60 rows.  HIP-event time per call after a
warm-up, and the rates in bytes/s: output bytes (what a user gets) and traffic (bytes read + written:
3 per output byte for a blend, 2 for a copy).  Descriptors and row tables are built once, so the
window holds launches only.  usage: python tools/retime_micro.py [--reps 200] [--rows 60] [--size HxW]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_video_interpolation_extrapolation_amd import _lib as L  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3  # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rows", type=int, default=60, help="output rows per call (a multiple of 3)")
    ap.add_argument("--size", default="1080x1920")
    a = ap.parse_args()
    H, W = map(int, a.size.split("x"))
    N, nbytes = a.rows, H * W * 3
    assert N % 3 == 0 and N >= 3
    dev = torch.device("cuda:0")
    lib, s = L.load(), L.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    slots = torch.randint(0, 256, (N + 1, nbytes), dtype=torch.uint8, device=dev, generator=g)
    out = torch.empty((N, nbytes), dtype=torch.uint8, device=dev)
    P = 5
    pairs = N // 3
    tables = {
        "blend": [(k, k + 1, 1 + k % (P - 1), k // 3, k) for k in range(N)],
        "nearest": [(k + (k & 1), k, 0, k // 3, k) for k in range(N)],
    }
    tables["flags"] = tables["blend"]
    flags = torch.tensor([[p % 3 == 0 for p in range(pairs)]], dtype=torch.uint8, device=dev)
    res = {"shape": [H, W, 3], "rows": N, "reps": a.reps, "out_bytes": N * nbytes}
    keep = []
    for tag, rows in tables.items():
        host = (ctypes.c_int32 * (5 * N))(*[v for r in rows for v in r])
        rdev = torch.tensor(rows, dtype=torch.int32, device=dev)
        keep += [host, rdev]
        d = L.SynthRetimeDesc()
        d.slots, d.out, d.rows, d.rows_dev = slots.data_ptr(), out.data_ptr(), ctypes.addressof(host), rdev.data_ptr()
        d.slot_s0, d.slot_s1, d.out_s0, d.out_s1, d.nbytes = 0, nbytes, 0, nbytes, nbytes
        d.n0, d.n_slots, d.n_rows, d.den = 1, N + 1, N, P
        if tag == "flags":
            d.cut, d.n_pairs = flags.data_ptr(), pairs
        sec = timed(lambda: L.check(lib.dvie_synth_retime(ctypes.byref(d), s), tag), a.reps)
        if tag == "flags":  # a third of the rows are copies of the held slot
            traffic = nbytes * (2 * (N // 3) + 3 * (N - N // 3))
        else:
            traffic = nbytes * N * (3 if tag == "blend" else 2)
        res[tag] = {"us": sec * 1e6, "out_bytes_per_s": N * nbytes / sec, "traffic_bytes_per_s": traffic / sec}
    # the yardstick: cut_fill over N / 3 flagged pairs at levels 2 copies 3 interior slots per pair = N rows
    T = pairs + 1
    fill = torch.randint(0, 256, (4 * pairs + 1, nbytes), dtype=torch.uint8, device=dev, generator=g)
    every = torch.ones((1, pairs), dtype=torch.uint8, device=dev)
    c = L.SynthCutFillDesc()
    c.slots, c.cut, c.s0, c.s1, c.nbytes = fill.data_ptr(), every.data_ptr(), 0, nbytes, nbytes
    c.n0, c.n1, c.levels = 1, T, 2
    sec = timed(lambda: L.check(lib.dvie_synth_cutfill(ctypes.byref(c), s), "cutfill"), a.reps)
    res["cutfill"] = {"us": sec * 1e6, "out_bytes_per_s": N * nbytes / sec, "traffic_bytes_per_s": 2 * N * nbytes / sec}
    res["blend_traffic_over_copy"] = res["blend"]["traffic_bytes_per_s"] / res["cutfill"]["traffic_bytes_per_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
