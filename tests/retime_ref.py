"""numpy restatement of frame-rate conversion (synth.Retime, retime_plan, retime_gather; include/dvie.h,
dvie_synth_retime), written from the definitions and independent of the product code: the output clock
in exact fractions, the slots an output reads on the dense grid of `levels` doublings, the forwards
those slots need, and the gather rule byte by byte."""
from fractions import Fraction
import math

import numpy as np


def count(T, P, Q):
    """outputs of a T-frame clip: the k with k * Q / P <= T - 1"""
    k = 0
    while Fraction((k + 1) * Q, P) <= T - 1:
        k += 1
    return k + 1


def emitted(T, P, Q, t0=0, first=True):
    """the global output indices a window of T inputs starting at input t0 emits: t0 < time <= t0 + T - 1,
    and time == t0 when first"""
    out, k = [], 0
    while Fraction(k * Q, P) <= t0 + T - 1:
        t = Fraction(k * Q, P)
        if t > t0 or (first and t == t0):
            out.append(k)
        k += 1
    return out


def dense_rows(T, levels, P, Q, mode, t0=0, first=True):
    """per emitted output (lo, hi, n, pair, hold) over the DENSE window-local grid (input t in slot
    t * 2**levels), for the frames; n over P weighs slot hi"""
    step = 1 << levels
    rows = []
    for k in emitted(T, P, Q, t0, first):
        t = Fraction(k * Q, P) - t0  # window-local time
        x = t * step
        lo = math.floor(x)
        w = x - lo  # weight of slot lo + 1, a multiple of 1 / P
        n = int(w * P)
        assert Fraction(n, P) == w and 0 <= n < P
        if t.denominator == 1:
            pair, hold = -1, int(t) * step
        else:
            pair = math.floor(t)
            hold = pair * step if t - pair <= Fraction(1, 2) else (pair + 1) * step
        near = lo if w <= Fraction(1, 2) else lo + 1
        if mode == "nearest" or n == 0:
            s = near if mode == "nearest" else lo
            rows.append((s, s, 0, pair, hold))
        else:
            rows.append((lo, lo + 1, n, pair, hold))
    return rows


def label_rows(T, levels, P, Q, t0=0, first=True):
    """the label maps follow the nearest rule in both modes"""
    return dense_rows(T, levels, P, Q, "nearest", t0, first)


def needed_slots(T, levels, P, Q, mode, t0=0, first=True):
    """the dense slots that must exist: the inputs, what the outputs read, and the midpoint ancestors"""
    step = 1 << levels
    need = {t * step for t in range(T)}
    for lo, hi, n, _, _ in dense_rows(T, levels, P, Q, mode, t0, first):
        need.add(lo)
        if n:
            need.add(hi)

    def parents(s):
        h = 1
        while s % (2 * h) == 0:
            h *= 2
        return s - h, s + h

    grew = True
    while grew:
        grew = False
        for s in sorted(need):
            if s % step:
                for a in parents(s):
                    if a not in need:
                        need.add(a)
                        grew = True
    return sorted(need)


def forwards(T, levels, P, Q, mode, t0=0, first=True):
    """one forward per needed slot that is no input"""
    step = 1 << levels
    return sum(1 for s in needed_slots(T, levels, P, Q, mode, t0, first) if s % step)


def blend_byte(a, b, n, P):
    """(a * (P - n) + b * n + P // 2) // P on integer arrays"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return ((a * (P - n) + b * n + P // 2) // P).astype(np.uint8)


def gather(slots, rows, den, out, cuts=None):
    """slots (B, S, ...) uint8, rows [(lo, hi, n, pair, hold)], out (B, N, ...) uint8 (what the rows
    skip stays), cuts (B, pairs) or None -> a new array"""
    out = out.copy()
    for b in range(slots.shape[0]):
        for k, (lo, hi, n, pair, hold) in enumerate(rows):
            if cuts is not None and pair >= 0 and cuts[b, pair]:
                out[b, k] = slots[b, hold]
            elif lo < 0:
                continue
            elif n == 0:
                out[b, k] = slots[b, lo]
            else:
                out[b, k] = blend_byte(slots[b, lo], slots[b, hi], n, den)
    return out


def convert(dense, levels, P, Q, mode, cuts=None, t0=0, first=True):
    """the dense interpolation result (B, (T - 1) * 2**levels + 1, ...) of a window -> its outputs at
    P:Q (frames with `mode`; pass "nearest" for label maps)"""
    step = 1 << levels
    T = (dense.shape[1] - 1) // step + 1
    rows = dense_rows(T, levels, P, Q, mode, t0, first)
    out = np.zeros((dense.shape[0], len(rows)) + dense.shape[2:], np.uint8)
    return gather(dense, rows, P, out, cuts)
