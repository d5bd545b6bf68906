"""CPU checks of the video-synthesis path: the arena offset assignment (random intervals and
the HRNet forward's own lifetimes), the midpoint schedule, and the argument validation of the
two synth entry points.  Nothing is launched."""
import ctypes
import types

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.synth import midpoint_schedule

ALIGN = 512


def _check_layout(items, offsets, arena):
    """no two items alive at the same time share a byte; offsets aligned; all inside the arena"""
    n = len(items)
    assert len(offsets) == n
    for i in range(n):
        assert offsets[i] % ALIGN == 0 and offsets[i] >= 0
        assert offsets[i] + items[i][0] <= arena
    order = sorted(range(n), key=lambda i: offsets[i])
    for a in range(n):
        i = order[a]
        for b in range(a + 1, n):
            j = order[b]
            if offsets[j] >= offsets[i] + items[i][0]:
                break  # (sorted by offset: nothing further starts inside item i)
            if items[i][1] <= items[j][2] and items[j][1] <= items[i][2]:
                raise AssertionError(f"items {i} {items[i]} @ {offsets[i]} and {j} {items[j]} @ {offsets[j]} overlap")


def test_assign_offsets_random_intervals():
    """200 seeded interval sets.  The arena never exceeds the sum of the sizes rounded to the
    512-byte granule each slot is given (one slot per item is always a valid layout); with
    sizes that are multiples of 512 that is the plain sum."""
    rng = np.random.RandomState(20260)
    for case in range(200):
        n = int(rng.randint(1, 40))
        steps = int(rng.randint(1, 30))
        items = []
        for _ in range(n):
            f = int(rng.randint(0, steps))
            l = int(rng.randint(f, steps))
            size = int(rng.randint(1, 64)) * ALIGN if case % 2 == 0 else int(rng.randint(1, 1 << 16))
            items.append((size, f, l))
        offsets, arena = E.assign_offsets(items)
        _check_layout(items, offsets, arena)
        assert arena <= sum((b + ALIGN - 1) // ALIGN * ALIGN for b, _, _ in items), case
        if case % 2 == 0:
            assert arena <= sum(b for b, _, _ in items), case
        # never below what is alive at one step
        peak = max(sum(b for b, f, l in items if f <= t <= l) for t in range(steps))
        assert arena >= peak


def test_assign_offsets_edge_cases():
    assert E.assign_offsets([]) == ([], 0)
    # closed intervals: [0, 1] and [1, 2] meet at step 1 (an op's input and its output)
    offsets, arena = E.assign_offsets([(1024, 0, 1), (1024, 1, 2), (1024, 2, 3)])
    assert offsets[0] != offsets[1] and offsets[1] != offsets[2] and arena == 2048
    assert offsets[0] == offsets[2]


def _hrnet(**kw):
    a = types.SimpleNamespace(syn_type="inter", highres_large=False, coarse_model="HRNet")
    a.__dict__.update(kw)
    torch.manual_seed(1024)
    return nets.InterNet(a).coarse_model


def _launch_lifetimes(g):
    """This test's own derivation (not the engine's): the graph's ops in order, the three
    convs of each segmentation encoder as ONE launch (the fused bf16 forward), a buffer alive
    from the first launch that touches it to the last."""
    chain_of = {}
    for chain in getattr(g, "segenc", []):
        for op in chain:
            chain_of[id(op)] = id(chain[0])
    launch, index = {}, []
    for op in g.ops:
        k = chain_of.get(id(op), id(op))
        if k not in launch:
            launch[k] = len(launch)
        index.append(launch[k])
    life = {}
    for op, i in zip(g.ops, index):
        regions = list(op.inputs()) + [r for r in (getattr(op, "out", None), getattr(op, "region", None)) if r is not None]
        for r in regions:
            f, l = life.get(id(r.buf), (i, i))
            life[id(r.buf)] = (min(f, i), max(l, i))
    return life, len(launch)


@pytest.mark.parametrize("large,n,H,W", [(False, 2, 16, 32), (False, 8, 256, 512), (True, 8, 256, 512)])
def test_arena_of_hrnet_forward(large, n, H, W):
    """The HRNet forward's arena (bf16, label inputs) against the live-bytes peak this test
    computes from the dry lowering: at most 10 % above it (a condition, not a measurement: a
    greedy-by-size first fit reaches the peak on these graphs) and under half the unaliased
    sum; and the layout is valid for the test's own lifetimes."""
    hr = _hrnet(highres_large=large)
    g = hr._lower(E.Graph(torch.bfloat16), H, W, dry=True, labels=True)
    assert any(isinstance(op, E.LabelInputOp) for op in g.ops)
    offsets, arena, unaliased = E.arena_layout(g, n)
    life, n_launch = _launch_lifetimes(g)
    bufs = [b for b in g.buffers if not b.external]
    nbytes = {id(b): n * b.H * b.W * b.C * (4 if b.dtype == torch.float32 else 2) for b in bufs}
    assert unaliased == sum(nbytes.values())
    assert all(id(b) in life for b in bufs)
    peak = max(sum(nbytes[id(b)] for b in bufs if life[id(b)][0] <= t <= life[id(b)][1]) for t in range(n_launch))
    print(f"HRNet large={large} {n}x{H}x{W}: arena {arena} peak {peak} unaliased {unaliased}")
    assert arena <= 1.10 * peak
    assert arena < 0.5 * unaliased
    _check_layout([(nbytes[id(b)],) + life[id(b)] for b in bufs], [offsets[id(b)] for b in bufs], arena)


def test_alias_plan_compiles_on_cpu_and_refuses_backward():
    hr = _hrnet()
    g = hr._lower(E.Graph(torch.float32), 16, 32, labels=True)
    plan = g.compile(2, torch.device("cpu"), backward=False, alias=True)
    d = plan.describe()
    assert d["arena_bytes"] == plan.arena_bytes and d["unaliased_bytes"] == plan.unaliased_bytes
    assert 0 < plan.arena_bytes < plan.unaliased_bytes
    base = plan.arena.data_ptr()
    for b in g.buffers:
        if not b.external:
            assert base <= b.t.data_ptr() and b.t.data_ptr() + b.t.numel() * b.t.element_size() <= base + plan.arena_bytes
            assert (b.t.data_ptr() - base) % ALIGN == 0
    assert sum(1 for o in plan.fwd if o.kind == L.OP_EW and o.u.ew.op == L.EW_LABELS) == 2
    # the default stays one allocation per buffer
    g2 = hr._lower(E.Graph(torch.float32), 16, 32)
    p2 = g2.compile(2, torch.device("cpu"), backward=False)
    assert p2.arena_bytes is None and p2.unaliased_bytes == plan.unaliased_bytes
    g3 = hr._lower(E.Graph(torch.float32), 16, 32)
    with pytest.raises(AssertionError):
        g3.compile(2, torch.device("cpu"), backward=True, alias=True)


def test_midpoint_schedule():
    assert midpoint_schedule(3, 2) == [[(0, 4, 2), (4, 8, 6)], [(0, 2, 1), (2, 4, 3), (4, 6, 5), (6, 8, 7)]]
    sched = midpoint_schedule(2, 3)
    written = [o for lev in sched for _, _, o in lev]
    assert sorted(written + [0, 8]) == list(range(9))  # 9 slots, each written exactly once
    known = {0, 8}
    for lev in sched:  # a level reads only what the inputs and the earlier levels wrote
        for a, b, o in lev:
            assert a in known and b in known and o == (a + b) // 2
        known |= {o for _, _, o in lev}
    assert midpoint_schedule(4, 0) == []


def test_synth_argument_validation_without_gpu():
    """dvie_synth_finish / dvie_synth_load reject bad descriptors before any launch."""
    lib = L.load()

    def finish(**kw):
        d = L.SynthFinishDesc()
        base = dict(rgb=64, seg=64, frame=64, label=64, npix=70, rgb_ld=8, seg_ld=24, n_classes=20)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.dvie_synth_finish(ctypes.byref(d), None)

    assert finish(npix=0) == L.DVIE_EINVAL and b"npix" in lib.dvie_last_error()
    assert finish(frame=None, label=None) == L.DVIE_EINVAL and b"at least one" in lib.dvie_last_error()
    assert finish(rgb_ld=6) == L.DVIE_EINVAL and b"multiples of 4" in lib.dvie_last_error()
    assert finish(seg_ld=22) == L.DVIE_EINVAL and b"multiples of 4" in lib.dvie_last_error()
    assert finish(n_classes=28) == L.DVIE_EINVAL and b"n_classes" in lib.dvie_last_error()
    assert finish(rgb=None) == L.DVIE_EINVAL
    assert finish(seg=None) == L.DVIE_EINVAL

    def load(**kw):
        d = L.SynthLoadDesc()
        base = dict(frames=64, out=64, npix=70, out_ld=8)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.dvie_synth_load(ctypes.byref(d), None)

    assert load(npix=0) == L.DVIE_EINVAL
    assert load(frames=None) == L.DVIE_EINVAL
    assert load(out_ld=6) == L.DVIE_EINVAL and b"multiple of 4" in lib.dvie_last_error()
    assert load(out=68) == L.DVIE_EINVAL
    # the labels op of the pointwise family: no epilogue operands, at most 256 classes
    e = L.EwDesc()
    e.op, e.n, e.h, e.w, e.c, e.y, e.y_ld, e.ext, e.ext_c = L.EW_LABELS, 1, 4, 4, 24, 64, 24, 64, 20
    e.beta = 1
    assert lib.dvie_ew(ctypes.byref(e), None) == L.DVIE_EINVAL and b"labels" in lib.dvie_last_error()
    e.beta, e.ext_c = 0, 300
    assert lib.dvie_ew(ctypes.byref(e), None) == L.DVIE_EINVAL


def test_synthesizer_refuses_out_of_scope_nets():
    from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer
    a = types.SimpleNamespace(syn_type="extra", highres_large=False, coarse_model="HRNet", num_pred_once=2)
    with pytest.raises(ValueError):
        VideoSynthesizer(nets.ExtraNet(a))
    with pytest.raises(ValueError):
        VideoSynthesizer(_hrnet())  # a bare HRNet is not an InterNet / ExtraNet


def test_level_chunks_cover_every_pair_once():
    """VideoSynthesizer.chunks: every (triple, clip) pair of a level in exactly one chunk, in
    order, no chunk above max_batch; chunks that span triples are full except the last."""
    from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer
    syn = VideoSynthesizer.__new__(VideoSynthesizer)
    for max_batch, B, T, levels in ((2, 3, 3, 2), (3, 1, 4, 2), (3, 2, 3, 1), (4, 3, 3, 1), (8, 2, 6, 1), (1, 2, 3, 1)):
        syn.max_batch = max_batch
        for triples in midpoint_schedule(T, levels):
            chunks = syn.chunks(triples, B)
            pairs = [(a, b, o, i) for ch in chunks for a, b, o, b0, b1 in ch for i in range(b0, b1)]
            assert pairs == [(a, b, o, i) for a, b, o in triples for i in range(B)]
            sizes = [sum(b1 - b0 for *_, b0, b1 in ch) for ch in chunks]
            assert max(sizes) <= max_batch and min(sizes) >= 1
            if B < max_batch and len(triples) > 1:
                assert all(s == max_batch for s in sizes[:-1])
            else:
                assert all(len(ch) == 1 for ch in chunks)
