"""CPU checks of frame-rate conversion: the output clock and the plan of synth.retime_plan against the
numpy restatement (tests/retime_ref.py) and the counts of DESIGN.md "Frame-rate conversion", the plan's
structure, the windows of a stream, every validation error, the option parser and the C entry point's
argument checks (no launch: no GPU here)."""
import ctypes

import pytest

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.options import Options
from deep_video_interpolation_extrapolation_amd.synth import Retime, midpoint_schedule, retime_count, retime_plan, window_plan
import retime_ref as R

RATES = [(5, 2), (6, 5), (5, 6), (2500, 1001)]
# (P, Q, levels, mode) -> (outputs, forwards) of a T = 11 clip; its full schedule at levels 3 has 70 forwards
TABLE = {
    (5, 2, 3, "nearest"): (26, 40), (5, 2, 3, "blend"): (26, 50),
    (6, 5, 3, "nearest"): (13, 26), (6, 5, 3, "blend"): (13, 26),
    (5, 6, 3, "nearest"): (9, 18), (5, 6, 3, "blend"): (9, 21),
    (2500, 1001, 3, "nearest"): (25, 40), (2500, 1001, 3, "blend"): (25, 54),
    (4, 1, 2, "nearest"): (41, 30), (4, 1, 2, "blend"): (41, 30),
}


def _dense_rows(plan, rows):
    """a plan's compact rows in dense slot numbers"""
    return [(plan.slots[lo], plan.slots[hi], n, pair, plan.slots[hold]) for lo, hi, n, pair, hold in rows]


# ---------------- counts ----------------
@pytest.mark.parametrize("key", sorted(TABLE))
def test_counts_of_the_table(key):
    P, Q, levels, mode = key
    outputs, forwards = TABLE[key]
    plan = retime_plan(11, levels, Retime(P, Q, mode))
    assert retime_count(11, Retime(P, Q)) == outputs == plan.count == R.count(11, P, Q)
    assert plan.forwards == forwards == R.forwards(11, levels, P, Q, mode)
    assert plan.dense_forwards == sum(len(lv) for lv in midpoint_schedule(11, levels)) == (70 if levels == 3 else 30)
    assert plan.k0 == 0


def test_count_formula():
    for P, Q in RATES + [(1, 1), (4, 1), (1, 3)]:
        for T in (1, 2, 3, 11, 100):
            assert retime_count(T, Retime(P, Q)) == (T - 1) * P // Q + 1 == R.count(T, P, Q), (P, Q, T)
    assert retime_count(11, Retime(10, 4)) == 26  # reduced
    with pytest.raises(ValueError):
        retime_count(0, Retime(5, 2))


# ---------------- the plan ----------------
@pytest.mark.parametrize("mode", ["nearest", "blend"])
@pytest.mark.parametrize("P,Q", RATES + [(8, 1), (7, 3)])
def test_plan_equals_the_reference_and_is_well_formed(P, Q, mode):
    T, levels = 6, 3
    step = 1 << levels
    plan = retime_plan(T, levels, Retime(P, Q, mode))
    # the slots, ascending and dense in compact numbering
    assert plan.slots == R.needed_slots(T, levels, P, Q, mode) == sorted(set(plan.slots))
    assert plan.index == {s: c for c, s in enumerate(plan.slots)}
    assert plan.in_slots == [plan.index[t * step] for t in range(T)]
    # the rows
    assert _dense_rows(plan, plan.rows) == R.dense_rows(T, levels, P, Q, mode)
    assert _dense_rows(plan, plan.label_rows) == R.label_rows(T, levels, P, Q)
    assert all(r[2] == 0 for r in plan.label_rows)
    want_in = [(h // step, h // step, 0, -1, h // step) if pair < 0 else (-1, -1, 0, pair, h // step)
               for _, _, _, pair, h in R.dense_rows(T, levels, P, Q, mode)]
    assert plan.input_rows == want_in
    assert plan.aligned == [(j, r[0]) for j, r in enumerate(want_in) if r[0] >= 0]
    assert all(plan.rows[j][:2] == (plan.in_slots[t],) * 2 and plan.rows[j][2] == 0 for j, t in plan.aligned)
    # the schedule: inputs of a triple exist before it runs, every other slot is written once
    have, written = set(plan.in_slots), []
    spacing = None
    for lv in plan.levels_c:
        assert lv == sorted(lv)
        gaps = {plan.slots[b] - plan.slots[a] for a, b, _ in lv}
        assert len(gaps) == 1 and (spacing is None or gaps.pop() < spacing)  # coarsest spacing first
        spacing = plan.slots[lv[0][1]] - plan.slots[lv[0][0]]
        for a, b, o in lv:
            assert a in have and b in have and 2 * plan.slots[o] == plan.slots[a] + plan.slots[b]
        have |= {o for _, _, o in lv}
        written += [o for _, _, o in lv]
    assert sorted(written + plan.in_slots) == list(range(len(plan.slots)))
    assert plan.forwards == len(written) == R.forwards(T, levels, P, Q, mode)
    assert plan.keep == {c for lv in plan.levels_c for a, b, _ in lv for c in (a, b)}
    assert all(plan.keep_fn(c) == (c in plan.keep) for c in range(len(plan.slots)))


@pytest.mark.parametrize("mode", ["nearest", "blend"])
def test_power_of_two_rate_is_the_midpoint_schedule(mode):
    T, levels = 5, 2
    plan = retime_plan(T, levels, Retime(4, 1, mode))
    S = (T - 1) * 4 + 1
    assert plan.slots == list(range(S)) and plan.levels_c == midpoint_schedule(T, levels)
    assert [r[:3] for r in plan.rows] == [(k, k, 0) for k in range(S)] == [r[:3] for r in plan.label_rows]
    assert plan.forwards == plan.dense_forwards
    assert plan.keep == {s for s in range(S) if s % 2 == 0}
    # a coarser rate on a finer grid keeps every second slot's subtree only
    plan = retime_plan(T, 3, Retime(4, 1, mode))
    assert [plan.slots[r[0]] for r in plan.rows] == list(range(0, 33, 2)) and plan.forwards == 12


def test_holds_follow_the_nearer_input():
    plan = retime_plan(3, 2, Retime(4, 1))  # outputs on every grid slot: cut_sources' rule
    step = 4
    for k, (_, _, _, pair, hold) in enumerate(plan.rows):
        if k % step == 0:
            assert pair == -1
        else:
            src = synth.cut_sources(2)[k % step - 1]
            assert pair == k // step and plan.slots[hold] == (k // step + src) * step
    # 5:2: times 0.4 (left), 0.8 (right), 1.2 (left), 1.6 (right); 2.0 is aligned
    plan = retime_plan(4, 3, Retime(5, 2))
    assert [(r[3], plan.slots[r[4]] // 8) for r in plan.rows] == [(-1, 0), (0, 0), (0, 1), (1, 1), (1, 2), (-1, 2), (2, 2), (2, 3)]
    # a tie at exactly half an interval goes to the earlier input: 2:1 at time 0.5
    plan = retime_plan(2, 1, Retime(2, 1))
    assert plan.rows[1][3:] == (0, plan.in_slots[0])


# ---------------- windows ----------------
@pytest.mark.parametrize("N", [2, 3, 7])
@pytest.mark.parametrize("P,Q", RATES)
def test_windows_partition_the_outputs(P, Q, N):
    T, levels = 11, 3
    rate = Retime(P, Q, "blend")
    whole = retime_plan(T, levels, rate)
    nxt, empty = 0, 0
    for w, (t0, t1) in enumerate(window_plan(T, N)):
        plan = retime_plan(t1 - t0 + 1, levels, rate, t0=t0, first=w == 0)
        assert list(range(plan.k0, plan.k0 + plan.count)) == R.emitted(t1 - t0 + 1, P, Q, t0, w == 0)
        if plan.count:
            assert plan.k0 == nxt
        else:
            assert plan.rows == [] and plan.forwards == 0 and plan.levels_c == [] and plan.keep == frozenset()
            assert plan.slots == [t * 8 for t in range(t1 - t0 + 1)]
        empty += plan.count == 0
        # a window's rows are the whole clip's, shifted to the window's own slots
        shift = t0 * 8
        mine = _dense_rows(plan, plan.rows)
        ref = _dense_rows(whole, whole.rows)[nxt:nxt + plan.count]
        assert [(lo + shift, hi + shift, n, pair if pair < 0 else pair + t0, hold + shift) for lo, hi, n, pair, hold in mine] == ref
        nxt += plan.count
    assert nxt == retime_count(T, rate)
    if (P, Q, N) == (5, 6, 2):
        assert empty >= 1
    # a later window that starts on an output does not emit it again; a first one does
    assert retime_plan(3, levels, rate, t0=Q, first=False).k0 == P + 1
    assert retime_plan(3, levels, rate, t0=Q, first=True).k0 == P


def test_long_streams_stay_exact():
    t0 = 10 ** 15 + 1
    plan = retime_plan(3, 3, Retime(2500, 1001), t0=t0, first=False)
    assert plan.k0 == t0 * 2500 // 1001 + 1 and plan.count == (t0 + 2) * 2500 // 1001 - plan.k0 + 1
    g = plan.k0 * 1001 * 8 - t0 * 8 * 2500
    blend = retime_plan(3, 3, Retime(2500, 1001, "blend"), t0=t0, first=False)
    lo, hi, n, _, _ = _dense_rows(blend, blend.rows)[0]
    assert (lo, n) == divmod(g, 2500) and blend.k0 == plan.k0


# ---------------- validation ----------------
def test_retime_validation():
    r = Retime(10, 4, "blend")
    assert (r.num, r.den, r.mode) == (5, 2, "blend") and r == Retime(5, 2, "blend") and r != Retime(5, 2)
    assert Retime(8192, 2).num == 4096 and Retime(1, 1).mode == "nearest"
    for bad in ((0, 1), (1, 0), (-5, 2), (2.5, 1), ("5", 2), (True, 2), (4097, 1), (1, 4097), (8193, 4097)):
        with pytest.raises(ValueError):
            Retime(*bad)
    with pytest.raises(ValueError, match="nearest"):
        Retime(5, 2, "linear")


def test_plan_validation():
    with pytest.raises(ValueError, match="--synth_levels"):
        retime_plan(4, 1, Retime(5, 2))
    with pytest.raises(ValueError, match="levels"):
        retime_plan(4, 0, Retime(2, 1))
    retime_plan(4, 0, Retime(1, 1))
    retime_plan(4, 0, Retime(1, 3))
    retime_plan(4, 2, Retime(4, 1))
    for kw in (dict(T=1), dict(T=2.0), dict(levels=-1), dict(t0=-1), dict(rate=(5, 2))):
        args = dict(T=4, levels=3, rate=Retime(5, 2), t0=0)
        args.update(kw)
        with pytest.raises(ValueError):
            retime_plan(args["T"], args["levels"], args["rate"], t0=args["t0"])


def test_y4m_rate_is_reduced():
    assert synth.retime_fps((24000, 1001), Retime(5, 2)) == (60000, 1001)
    assert synth.retime_fps((25, 1), Retime(6, 5)) == (30, 1)
    assert synth.retime_fps((30, 1), Retime(5, 6)) == (25, 1)
    assert synth.retime_fps((24, 1), Retime(2500, 1001)) == (60000, 1001)


def test_option_parser():
    a = Options().parse(["INTER"])
    assert a.synth_rate is None and a.synth_rate_mode == "nearest"
    a = Options().parse(["--synth_rate", "5:2", "--synth_rate_mode", "blend", "INTER"])
    assert a.synth_rate == (5, 2) and a.synth_rate_mode == "blend"
    assert Options().parse(["--synth_rate", "60000:24000", "EXTRA"]).synth_rate == (5, 2)
    assert Options().parse(["--synth_rate", "4096:4095", "INTER"]).synth_rate == (4096, 4095)
    for flag, bad in (("--synth_rate", "5"), ("--synth_rate", "5/2"), ("--synth_rate", "5:0"), ("--synth_rate", "0:2"),
                      ("--synth_rate", "-5:2"), ("--synth_rate", "2.5:1"), ("--synth_rate", "4097:1"),
                      ("--synth_rate", "1:5000"), ("--synth_rate", "5:2:1"), ("--synth_rate_mode", "linear")):
        with pytest.raises(SystemExit):
            Options().parse([flag, bad, "INTER"])


def test_runner_names_the_flag_and_the_fix():
    import logging
    import types
    from deep_video_interpolation_extrapolation_amd.runners.InterTrainer import InterTrainer
    me = types.SimpleNamespace(args=types.SimpleNamespace(synth_rate=(5, 2), synth_rate_mode="blend", synth_levels=1),
                               _streams=True, log=logging.getLogger("t"))
    with pytest.raises(ValueError, match=r"--synth_rate 5:2 .*--synth_levels 2"):
        InterTrainer._rate(me)
    me.args.synth_levels = 2
    assert InterTrainer._rate(me) == Retime(5, 2, "blend")
    me.args.synth_rate = None
    assert InterTrainer._rate(me) is None
    me.args.synth_rate, me._streams = (5, 2), False  # EXTRA
    assert InterTrainer._rate(me) is None


# ---------------- the C entry point ----------------
def _desc(rows, **kw):
    n = len(rows)
    host = (ctypes.c_int32 * max(5 * n, 1))(*[v for r in rows for v in r])
    d = L.SynthRetimeDesc()
    d.slots = d.out = d.rows_dev = 4096
    d.rows = ctypes.addressof(host)
    d.slot_s0, d.slot_s1, d.out_s0, d.out_s1, d.nbytes = 400, 100, 400, 100, 100
    d.n0, d.n_slots, d.n_rows, d.n_pairs, d.den = 1, 4, n, 0, 5
    for k, v in kw.items():
        setattr(d, k, v)
    d._host = host  # (keeps the rows alive)
    return d


def test_entry_point_is_exported_and_sized():
    lib = L.load()
    assert "dvie_synth_retime" in L.EXPORTS and hasattr(lib, "dvie_synth_retime")
    assert L._ABI_MORE[117] is L.SynthRetimeDesc
    assert lib.dvie_abi_sizeof(117) == ctypes.sizeof(L.SynthRetimeDesc) == 104


@pytest.mark.parametrize("rows,kw,word", [
    ([(0, 1, 1, -1, 0)], dict(den=0), "den"),
    ([(0, 1, 1, -1, 0)], dict(den=4097), "den"),
    ([(0, 1, 5, -1, 0)], {}, "n=5"),
    ([(0, 1, -1, -1, 0)], {}, "n=-1"),
    ([(4, 4, 0, -1, 0)], {}, "lo=4"),
    ([(-2, 0, 0, -1, 0)], {}, "lo=-2"),
    ([(0, 4, 2, -1, 0)], {}, "hi=4"),
    ([(0, -1, 2, -1, 0)], {}, "hi=-1"),
    ([(0, 1, 2, -2, 0)], {}, "pair=-2"),
    ([(0, 1, 2, 3, 0)], dict(cut=4096, n_pairs=3), "pair=3"),
    ([(0, 1, 2, 1, 4)], dict(cut=4096, n_pairs=3), "holds slot 4"),
    ([(0, 0, 0, -1, 0)], dict(nbytes=0), "empty rows"),
    ([(0, 0, 0, -1, 0)], dict(n0=0), "n0"),
    ([(0, 0, 0, -1, 0)], dict(n_slots=0), "n_slots"),
    ([(0, 0, 0, -1, 0)], dict(slots=0), "null"),
    ([(0, 0, 0, -1, 0)], dict(rows_dev=0), "null"),
    ([(0, 0, 0, -1, 0)], dict(slot_s1=99), "overlap"),
    ([(0, 0, 0, -1, 0), (1, 1, 0, -1, 0)], dict(out_s1=-99), "overlap"),
])
def test_entry_point_refuses_bad_descriptors_before_any_launch(rows, kw, word):
    lib = L.load()
    assert lib.dvie_synth_retime(ctypes.byref(_desc(rows, **kw)), None) == L.DVIE_EINVAL, (rows, kw)
    assert word.encode() in lib.dvie_last_error(), lib.dvie_last_error()


def test_entry_point_null_and_no_rows():
    lib = L.load()
    assert lib.dvie_synth_retime(None, None) == L.DVIE_EINVAL and b"null" in lib.dvie_last_error()
    assert lib.dvie_synth_retime(ctypes.byref(_desc([])), None) == L.DVIE_OK  # no output: nothing is launched
    assert lib.dvie_synth_retime(ctypes.byref(_desc([], den=0)), None) == L.DVIE_EINVAL
