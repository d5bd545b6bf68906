"""CPU checks (no launch) of two-stage video synthesis: the synthesiser's constructor, the arena
of the refinement nets' inference lowerings, their alias plans compiled on the CPU, and the
argument validation of dvie_synth_bridge."""
import ctypes
import types

import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd import nets
from deep_video_interpolation_extrapolation_amd.synth import VideoSynthesizer

ALIGN = 512
CPU = torch.device("cpu")


def _args(kind="inter", **kw):
    a = types.SimpleNamespace(syn_type=kind, highres_large=False, coarse_model="HRNet", precision="bf16", n_scales=2,
                              stage3_prop=False)
    a.__dict__.update(kw)
    return a


# ---------------- constructor ----------------
@pytest.mark.parametrize("name,kind,n_stages", [("InterRefineNet", "inter", 1), ("ExtraRefineNet", "extra", 1),
                                                ("InterStage3Net", "inter", 2), ("ExtraStage3Net", "extra", 2)])
def test_synthesizer_accepts_two_stage_nets(name, kind, n_stages):
    torch.manual_seed(3)
    net = nets.__dict__[name](_args(kind, n_scales=3))
    net.train()
    syn = VideoSynthesizer(net, max_batch=2)
    assert not net.training and len(syn.stages) == n_stages
    assert syn.stages[0] is net.refine_model and (n_stages == 1 or syn.stages[1] is net.stage3_model)


def test_synthesizer_still_refuses_out_of_scope_nets():
    torch.manual_seed(3)
    with pytest.raises(ValueError):
        VideoSynthesizer(nets.InterGANNet(_args()))
    with pytest.raises(ValueError):
        VideoSynthesizer(nets.ExtraNet(_args("extra", num_pred_once=2)))
    with pytest.raises(ValueError):
        VideoSynthesizer(nets.InterNet(_args()).coarse_model)  # a bare HRNet


# ---------------- arena of the inference lowerings ----------------
def _own_lifetimes(g):
    """This test's own derivation: every graph op is one launch (these graphs hold no fused
    segmentation encoder); a buffer is alive from the first launch that touches it to the
    last; a buffer with a caller-written span is alive from launch 0 (the caller fills it
    before the forward starts)."""
    life = {}
    for i, op in enumerate(g.ops):
        regions = list(op.inputs()) + [r for r in (getattr(op, "out", None), getattr(op, "region", None)) if r is not None]
        for r in regions:
            f, l = life.get(id(r.buf), (i, i))
            life[id(r.buf)] = (min(f, i), max(l, i))
    for r in g.caller_written.values():
        life[id(r.buf)] = (0, life[id(r.buf)][1])
    return life, len(g.ops)


def _check_layout(items, offsets, arena):
    """no two items alive at the same time share a byte; offsets aligned; all inside the arena"""
    n = len(items)
    assert len(offsets) == n
    for i in range(n):
        assert offsets[i] % ALIGN == 0 and offsets[i] >= 0 and offsets[i] + items[i][0] <= arena
    order = sorted(range(n), key=lambda i: offsets[i])
    for a in range(n):
        i = order[a]
        for b in range(a + 1, n):
            j = order[b]
            if offsets[j] >= offsets[i] + items[i][0]:
                break
            if items[i][1] <= items[j][2] and items[j][1] <= items[i][2]:
                raise AssertionError(f"items {i} {items[i]} @ {offsets[i]} and {j} {items[j]} @ {offsets[j]} overlap")


def _infer_graph(which, a, H, W):
    torch.manual_seed(5)
    if which == "srn":
        return nets.SRNRefine(a)._lower(E.Graph(torch.bfloat16), H, W, False, infer=True)
    return nets.MSResAttnRefine(a)._lower(E.Graph(torch.bfloat16), H, W, False, bool(a.stage3_prop), infer=True)


@pytest.mark.parametrize("which", ["srn", "attention"])
@pytest.mark.parametrize("n,H,W,n_scales,prop", [(2, 64, 128, 2, False), (1, 1024, 2048, 3, True)])
def test_arena_of_refine_inference_lowerings(which, n, H, W, n_scales, prop):
    """At most 10 % above the live-bytes peak this test derives from the op order (caller-written
    buffers alive from launch 0), under a quarter of the unaliased sum, and a valid layout for
    the test's own lifetimes."""
    g = _infer_graph(which, _args(n_scales=n_scales, stage3_prop=prop), H, W)
    assert list(g.caller_written) == ["bridge"]
    offsets, arena, unaliased = E.arena_layout(g, n)
    life, n_launch = _own_lifetimes(g)
    bufs = [b for b in g.buffers if not b.external]
    nbytes = {id(b): n * b.H * b.W * b.C * (4 if b.dtype == torch.float32 else 2) for b in bufs}
    assert unaliased == sum(nbytes.values())
    assert all(id(b) in life for b in bufs)
    bridge = g.caller_written["bridge"].buf
    assert life[id(bridge)][0] == 0
    peak = max(sum(nbytes[id(b)] for b in bufs if life[id(b)][0] <= t <= life[id(b)][1]) for t in range(n_launch))
    print(f"{which} {n}x{H}x{W} n_scales={n_scales}: arena {arena} peak {peak} unaliased {unaliased} "
          f"ratio {arena / unaliased:.3f}")
    assert arena <= 1.10 * peak
    assert arena < 0.25 * unaliased
    _check_layout([(nbytes[id(b)],) + life[id(b)] for b in bufs], [offsets[id(b)] for b in bufs], arena)


def test_caller_written_buffer_is_live_from_launch_zero():
    """Without the caller-written rule the attention net's `in_x` would start living at its
    first reader, and an earlier launch's output could be placed in its bytes."""
    g = _infer_graph("attention", _args(), 64, 128)
    x = g.caller_written["bridge"].buf
    first_touch = min(i for i, op in enumerate(g.ops) if any(r.buf is x for r in E._op_regions(op)))
    assert first_touch > 0  # (the neighbour streams' input ops come first)
    assert E.forward_lifetimes(g, 2)[id(x)][0] == 0


# ---------------- alias plans on the CPU ----------------
def _in_arena(plan, t):
    base = plan.arena.data_ptr()
    return base <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= base + plan.arena_bytes


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_srn_inference_plan_compiles_on_cpu(dtype):
    torch.manual_seed(5)
    m = nets.SRNRefine(_args())
    g = m._lower(E.Graph(dtype), 32, 64, False, infer=True)
    plan = g.compile(2, CPU, backward=False, alias=True)
    assert 0 < plan.arena_bytes < plan.unaliased_bytes
    for b in g.buffers:
        assert not b.external and _in_arena(plan, b.t)
    v = plan.input_view("bridge")
    assert v.dtype == dtype and tuple(v.shape) == (2, 32, 64, 40) and v.stride() == (32 * 64 * 56, 64 * 56, 56, 1)
    full = g.caller_written["bridge"].buf
    assert v.data_ptr() == full.t.data_ptr() and full.C == 56
    # the only input op is the stem features', behind the span; one output, the finest image
    ins = [o for o in plan.fwd if o.kind == L.OP_EW and o.u.ew.op == L.EW_NCHW]
    assert len(ins) == 1 and ins[0].u.ew.y == full.t.data_ptr() + 40 * v.element_size() and ins[0].u.ew.ext_c == 14
    assert list(plan.ext_in) == ["enc"]
    outs = [o for o in plan.fwd if o.kind == L.OP_EW and o.u.ew.op == L.EW_TONCHW]
    assert len(outs) == 1 and list(plan.ext_nchw_out) == ["pred"]
    assert (outs[0].u.ew.h, outs[0].u.ew.w, outs[0].u.ew.ext_c) == (32, 64, 8)
    assert outs[0].u.ew.align == 1 and outs[0].u.ew.scale == 10.0  # the nets' clamp of a stage's output


@pytest.mark.parametrize("prop", [False, True])
def test_attention_inference_plan_compiles_on_cpu(prop):
    torch.manual_seed(5)
    m = nets.MSResAttnRefine(_args(stage3_prop=prop))
    g = m._lower(E.Graph(torch.bfloat16), 64, 128, False, prop, infer=True)
    plan = g.compile(2, CPU, backward=False, alias=True)
    assert 0 < plan.arena_bytes < plan.unaliased_bytes
    for b in g.buffers:
        assert not b.external and _in_arena(plan, b.t)
    v = plan.input_view("bridge")
    assert v.dtype == torch.bfloat16 and tuple(v.shape) == (2, 64, 128, 24) and v.stride() == (64 * 128 * 24, 128 * 24, 24, 1)
    lo, hi = v.data_ptr(), v.data_ptr() + v.numel() * 2
    for o in plan.fwd:  # no input op of any kind writes the span the bridge owns
        if o.kind == L.OP_EW and o.u.ew.op in (L.EW_NCHW, L.EW_LABELS):
            assert not lo <= o.u.ew.y < hi
    # the neighbours: two frames through NCHW views, two label maps
    assert sum(1 for o in plan.fwd if o.kind == L.OP_EW and o.u.ew.op == L.EW_NCHW) == 2
    labels = [o for o in plan.fwd if o.kind == L.OP_EW and o.u.ew.op == L.EW_LABELS]
    assert len(labels) == 2 and all(o.u.ew.ext_c == 20 and o.u.ew.c == 20 for o in labels)
    assert sorted(plan.ext_in) == ["nimg", "nseg"]
    assert all(isinstance(op, E.LabelInputOp) for _, op in plan.ext_in["nseg"])
    assert list(plan.ext_nchw_out) == ["out"]
    assert sum(1 for op in g.ops if isinstance(op, E.AttnOp) and op.kind == "pool") == (2 if prop else 0)


def test_training_and_inference_plans_keep_apart_in_the_pool():
    torch.manual_seed(5)
    m = nets.SRNRefine(_args(precision="fp32", n_scales=1))
    inf = m.infer_plan(1, 16, 32, CPU)
    fwd = m._pool.acquire((1, 16, 32, m.dtype, False, CPU))
    assert inf is not fwd and inf.alias and not fwd.alias
    assert "bridge" in inf.g.caller_written and not fwd.g.caller_written
    assert sorted(fwd.ext_in) == ["enc", "rgb", "seg"] and list(fwd.ext_nchw_out) == ["pred0"]
    assert m.infer_plan(1, 16, 32, CPU) is inf and m._pool.acquire((1, 16, 32, m.dtype, False, CPU)) is fwd
    a = nets.MSResAttnRefine(_args(precision="fp32", n_scales=1))
    inf = a.infer_plan(1, 16, 32, CPU)
    fwd = a._pool.acquire((1, 16, 32, a.dtype, False, False, CPU))
    assert inf is not fwd and inf.alias and not fwd.alias and sorted(fwd.ext_in) == ["img", "nimg", "nseg", "seg"]


# ---------------- dvie_synth_bridge: argument validation ----------------
def test_bridge_argument_validation_without_gpu():
    lib = L.load()
    assert "dvie_synth_bridge" in L.EXPORTS and hasattr(lib, "dvie_synth_bridge")
    assert lib.dvie_abi_sizeof(106) == ctypes.sizeof(L.SynthBridgeDesc)

    def bridge(**kw):
        d = L.SynthBridgeDesc()
        base = dict(rgb=64, seg=64, dst=64, npix=70, rgb_ld=8, seg_ld=24, dst_ld=56, dtype=L.BF16, n_rgb=2, rgb_w=8,
                    seg_w=24)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.dvie_synth_bridge(ctypes.byref(d), None)

    for kw, word in ((dict(rgb=None), b"null"), (dict(seg=None), b"null"), (dict(dst=None), b"null"),
                     (dict(npix=0), b"npix"), (dict(npix=-3), b"npix"),
                     (dict(rgb_w=3), b"rgb_w"), (dict(rgb_w=12), b"rgb_w"),
                     (dict(seg_w=16), b"seg_w"), (dict(seg_w=28), b"seg_w"),
                     (dict(n_rgb=0), b"n_rgb"), (dict(n_rgb=3), b"n_rgb"),
                     (dict(dst_ld=32), b"does not fit"),  # SRN's span of 40 in a row of 32
                     (dict(n_rgb=1, rgb_w=4, seg_w=20, dst_ld=16), b"does not fit"),
                     (dict(n_rgb=1, rgb_w=4, seg_w=24), b"16-byte"),  # 28 bf16 channels: no whole vectors
                     (dict(dst_ld=60), b"16-byte"), (dict(dst=72), b"16-byte"),
                     (dict(rgb_ld=6), b"multiples of 4"), (dict(seg_ld=16), b"seg_ld"), (dict(rgb=68), b"aligned"),
                     (dict(dtype=7), b"dtype")):
        assert bridge(**kw) == L.DVIE_EINVAL, kw
        assert word in lib.dvie_last_error(), (kw, lib.dvie_last_error())
