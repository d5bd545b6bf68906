"""CPU checks of the per-frame perceptual score (synth.PerceptualScorer): the region rule, the
normalisation table, summarize with and without the vgg column, the arena of my_vgg's scoring
graph, the --synth_vgg option and the C ABI of the new entry points.  No kernel is launched."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from deep_video_interpolation_extrapolation_amd import _lib as L
from deep_video_interpolation_extrapolation_amd import engine as E
from deep_video_interpolation_extrapolation_amd import synth
from deep_video_interpolation_extrapolation_amd.nets.vgg import my_vgg, vgg19_features

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------- region ----------------
def test_vgg_region():
    assert synth.vgg_region(150, 150) == (144, 144)
    assert synth.vgg_region(256, 512) == (256, 512)
    assert synth.vgg_region(16, 31) == (16, 16)
    with pytest.raises(ValueError):
        synth.vgg_region(15, 64)
    with pytest.raises(ValueError):
        synth.vgg_region(64, 15)


# ---------------- table ----------------
def test_table_is_the_float64_expression_rounded_once():
    v = np.arange(256, dtype=np.float64)
    want = np.stack([np.float32((v / 255 - m) / s) for m, s in zip(MEAN, STD)])
    got = synth.vgg_lut(torch.float32)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 256) and got.is_contiguous()
    assert got.numpy().tobytes() == want.tobytes()
    bf = synth.vgg_lut(torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and tuple(bf.shape) == (3, 256) and bf.is_contiguous()
    assert torch.equal(bf.view(torch.int16), torch.tensor(want).bfloat16().view(torch.int16))


# ---------------- summarize ----------------
POS = [0, 1, 0]
PSNR, SSIM, ACC, MIOU, VGG = [10.0, 20.0, 30.0], [0.5, 0.25, 0.75], [1.0, 0.0, 1.0], [0.5, 0.5, 1.0], [0.25, 1.0, 0.5]


def test_summarize_without_vgg_is_unchanged():
    got = synth.summarize(POS, PSNR, SSIM, ACC, MIOU)
    assert got == {
        "psnr": 20.0, "ssim": 0.5, "acc": 2 / 3, "miou": 2 / 3, "frames": 3,
        "per_position": {0: {"psnr": 20.0, "ssim": 0.625, "acc": 1.0, "miou": 0.75, "frames": 2},
                         1: {"psnr": 20.0, "ssim": 0.25, "acc": 0.0, "miou": 0.5, "frames": 1}}}
    assert list(got) == ["psnr", "ssim", "acc", "miou", "frames", "per_position"]
    for row in got["per_position"].values():
        assert list(row) == ["psnr", "ssim", "acc", "miou", "frames"]


def test_summarize_with_vgg_adds_the_column_to_every_row():
    got = synth.summarize(POS, PSNR, SSIM, ACC, MIOU, vgg=VGG)
    base = synth.summarize(POS, PSNR, SSIM, ACC, MIOU)
    pos, v = np.asarray(POS), np.asarray(VGG, dtype=np.float64)
    assert got["vgg"] == float(np.mean(v)) and isinstance(got["vgg"], float)
    for p, row in got["per_position"].items():
        assert row["vgg"] == float(np.mean(v[pos == p]))
        assert {k: x for k, x in row.items() if k != "vgg"} == base["per_position"][p]
    assert {k: x for k, x in got.items() if k not in ("vgg", "per_position")} == \
        {k: x for k, x in base.items() if k != "per_position"}


def test_frame_scores_fields_carry_vgg():
    assert synth.FrameScores.FIELDS[-1] == "vgg"
    fs = synth.FrameScores(4, 4, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.float64))
    assert fs.vgg is None and fs.map(lambda t: t + 1).vgg is None
    fs.vgg = torch.ones(2, dtype=torch.float64)
    assert torch.equal(fs.map(lambda t: t * 2).vgg, torch.full((2,), 2.0, dtype=torch.float64))


# ---------------- the scoring graph of my_vgg ----------------
@pytest.fixture(scope="module")
def net():
    return my_vgg(vgg19_features())


def _graph(net, dtype, H, W):
    g = E.Graph(dtype)
    feats = net.lower_score(g, H, W)
    return g, feats


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("nf,H,W", [(2, 16, 16), (4, 32, 64), (10, 32, 48)])
def test_scoring_graph_arena(net, dtype, nf, H, W):
    g, feats = _graph(net, dtype, H, W)
    launches = E.forward_launches(g, nf)
    kinds = [type(s[0]) for s in launches]
    assert kinds.count(E.CosFeatOp) == 5 and kinds.count(E.ConvOp) == 16 and kinds.count(E.PoolOp) == 4
    assert E.L1FeatOp not in kinds and E.InputOp not in kinds and list(g.caller_written) == ["vgg_in"]
    assert [f.c for f in feats] == [64, 128, 256, 512, 512]
    assert [(f.H, f.W) for f in feats] == [(H >> k, W >> k) for k in range(5)]
    life = E.forward_lifetimes(g, nf)
    bufs = [b for b in g.buffers if not b.external]
    assert life[id(g.caller_written["vgg_in"].buf)][0] == 0
    # every tap lives at least until its cosfeat, which directly follows the tap's conv
    for i, site in enumerate(launches):
        if isinstance(site[0], E.CosFeatOp):
            tap = site[0].a.buf
            assert tap is feats[site[0].idx].buf and launches[i - 1][0].out.buf is tap
            assert life[id(tap)][0] == i - 1 and life[id(tap)][1] >= i
    items = [(nf * b.H * b.W * b.C * E.elem_size(dtype),) + life[id(b)] for b in bufs]
    offsets, arena = E.assign_offsets(items)
    size = [E.rup(it[0], E.ARENA_ALIGN) for it in items]
    for i in range(len(items)):
        assert offsets[i] % E.ARENA_ALIGN == 0 and offsets[i] + size[i] <= arena
        for j in range(i):
            in_time = items[i][1] <= items[j][2] and items[j][1] <= items[i][2]
            in_bytes = offsets[i] < offsets[j] + size[j] and offsets[j] < offsets[i] + size[i]
            assert not (in_time and in_bytes), (bufs[i], bufs[j])
    peak = max(sum(s for s, it in zip(size, items) if it[1] <= k <= it[2]) for k in range(len(launches)))
    assert arena == peak
    layout = E.arena_layout(g, nf)
    assert layout[1] == arena and layout[2] == sum(it[0] for it in items) and arena < layout[2]


def test_scoring_plan_compiles_on_cpu_under_its_own_pool_key(net):
    cpu = torch.device("cpu")
    plan = net.score_plan(2, 32, 64, cpu)
    assert plan is net.score_plan(2, 32, 64, cpu) and plan is not net.score_plan(2, 32, 64, cpu, alias=False)
    assert plan.nf == 4 and plan.alias and not plan.backward_enabled and plan.static_weights and plan.n_bwd == 0
    assert 0 < plan.arena_bytes < plan.unaliased_bytes
    assert all(k[0] == "score" for k in net._pool.plans)
    kinds = [o.kind for o in plan.fwd]
    assert kinds.count(L.OP_COSFEAT) == 6 and kinds[-1] == L.OP_COSFEAT and L.OP_LOSS not in kinds
    last = plan.fwd[-1].u.cosfeat
    assert last.mode == 1 and last.n == 2 and last.n_taps == 5
    assert list(last.px)[:5] == [32 * 64 >> (2 * k) for k in range(5)]
    assert all(1 <= b <= plan.cos_ws_blocks for b in list(last.blocks)[:5])
    assert plan.cosfeat_ws_doubles == 5 * 2 * plan.cos_ws_blocks
    view = plan.input_view("vgg_in")
    assert tuple(view.shape) == (4, 32, 64, 8) and view.is_contiguous() and view.dtype == net.dtype
    with pytest.raises(AssertionError):
        g = E.Graph(torch.float32)
        net.lower_score(g, 32, 64)
        g.compile(4, cpu, backward=True)


# ---------------- options and ABI ----------------
def test_option_synth_vgg():
    from deep_video_interpolation_extrapolation_amd.options import Options
    base = ["--split", "test", "--synth_eval"]
    assert Options().parse(base + ["INTER"]).synth_vgg is False
    assert Options().parse(base + ["--synth_vgg", "INTER"]).synth_vgg is True
    assert Options().parse(base + ["--synth_vgg", "EXTRA"]).synth_vgg is True


# sizeof of every descriptor before this feature, by dvie_abi_sizeof index
OLD_SIZES = {0: 240, 1: 216, 2: 128, 3: 64, 4: 48, 5: 232, 6: 152, 7: 88, 8: 184, 10: 88, 12: 152, 13: 112, 14: 136,
             15: 152, 16: 16, 100: 80, 101: 88, 102: 88, 103: 88, 104: 32, 105: 56, 106: 64, 107: 176, 108: 56, 109: 80}


def test_new_symbols_and_descriptor_sizes():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvie_[a-z0-9_]+)", out))
    for name in ("dvie_synth_vgg_load", "dvie_cosfeat", "dvie_cosfeat_blocks"):
        assert name in exported and name in L.EXPORTS, name
    assert lib.dvie_abi_sizeof(L.OP_COSFEAT) == ctypes.sizeof(L.CosFeatDesc) and L.OP_COSFEAT == 17
    assert lib.dvie_abi_sizeof(110) == ctypes.sizeof(L.SynthVggLoadDesc)
    assert L._ABI[L.OP_COSFEAT] is L.CosFeatDesc and L._ABI[110] is L.SynthVggLoadDesc
    assert set(L._ABI) == set(OLD_SIZES) | {L.OP_COSFEAT, 110}
    for which, size in OLD_SIZES.items():
        assert lib.dvie_abi_sizeof(which) == ctypes.sizeof(L._ABI[which]) == size, which


def test_argument_validation_without_gpu():
    lib = L.load()
    d = L.CosFeatDesc()
    d.h, d.w, d.dtype = 5, 7, L.BF16
    for c, ok in ((64, True), (128, True), (256, True), (512, True), (96, False), (60, False), (0, False)):
        d.c = c
        assert (lib.dvie_cosfeat_blocks(ctypes.byref(d)) > 0) == ok, c
    d.c, d.ws, d.n, d.n_taps, d.ws_blocks, d.feat, d.ld = 64, 64, 1, 5, 8, 8, 64  # feat not 16-byte aligned
    assert lib.dvie_cosfeat(ctypes.byref(d), None) == L.DVIE_EINVAL and b"16-byte" in lib.dvie_last_error()
    d.feat, d.ld = 64, 68  # the pitch is no whole number of 16-byte vectors
    assert lib.dvie_cosfeat(ctypes.byref(d), None) == L.DVIE_EINVAL and b"16-byte" in lib.dvie_last_error()
    v = L.SynthVggLoadDesc()
    v.pred, v.gt, v.out, v.lut = 1, 1, 64, 64
    v.n0, v.n1, v.h, v.w, v.h16, v.w16, v.dtype, v.n_out = 1, 2, 37, 53, 48, 48, L.F32, 2
    assert lib.dvie_synth_vgg_load(ctypes.byref(v), None) == L.DVIE_EINVAL and b"region" in lib.dvie_last_error()
    v.h16, v.img0 = 32, 1  # pairs 1..2 of a batch of 2
    assert lib.dvie_synth_vgg_load(ctypes.byref(v), None) == L.DVIE_EINVAL and b"n_out" in lib.dvie_last_error()
