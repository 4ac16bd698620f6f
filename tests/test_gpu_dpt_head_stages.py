"""-m gpu: every launch of heads_hip.HipDPTHead at the head's real channel counts under a per-element budget (tests/dpt_stages.py: the
launches are recorded with their inputs, the tape must equal the schedule written from the reference head, and every launch is gated against
the float64 reference of its OWN recorded inputs; test_dpt_stages_host.py proves on the CPU that this checker pins planted defects to their
launch). Three parts: (a) both heads at tiny grids (4x7 patches and the two one-line grids) in bf16 / f16 / f32 with every element
referenced, the two forms of the output stage bit-equal before it and one-frame passes bit-equal to one pass; (b) the point head across the
256-pixel line (19x18 patches, three views: 64 tiles + 32 pixels at level 0) with the dispatch restated and sampled references; (c) the
head's other convolution shapes on the 256-pixel kernels as single calls into guard bands. Budgets are those of kernel_guards.py."""
import importlib

import pytest
import torch

import dpt_stages as ds
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops  # noqa: F401
from test_gpu_edges import DEV, MODES, Slot, _need_gpu, _sync_check  # noqa: F401 (_need_gpu: the autouse fixture)
from test_gpu_head_edges import _expected_conv256

pytestmark = pytest.mark.gpu
WORST, SHARE = {}, {"window": 0.0}
_HEADS, _TOKS = {}, {}

heads = importlib.import_module("omnivggt_official_amd.heads")
heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")


def _note(mode, R):
    for kind, used in R["worst"].items():
        WORST[(kind, mode)] = max(WORST.get((kind, mode), 0.0), used)
    for _, _, share in R["shares"]:
        SHARE["window"] = max(SHARE["window"], share)
    print("worst used budget so far: " + ", ".join("%s/%s %.3f" % (k[0], k[1], v) for k, v in sorted(WORST.items()))
          + "; largest window share %.4f" % SHARE["window"], flush=True)


def _head(which):
    if which not in _HEADS:
        _HEADS[which] = ds.rand_head(heads, which, DEV)
    return _HEADS[which]


def _tokens(grid):
    if grid not in _TOKS:
        _TOKS.clear()
        S, ph, pw = ds.GRIDS[grid]
        toks, images = ds.rand_tokens(S, ph, pw)
        _TOKS[grid] = ([t.to(DEV) for t in toks], images.to(DEV))
    return _TOKS[grid]


def _dispatch(mode, launch):
    a = launch.arg
    n, H, W, cin = a("x").shape
    if mode == "f32" or a("out_f32") or a("w").shape[0] != (max(a("upshuffle"), 1) ** 2) * a("cout"):
        return None
    return _expected_conv256(mode, n, H, W, cin, a("cout"), a("ksize"), a("stride"), a("upshuffle"), a("x").stride(2))


def _record(which, grid, mode, fused):
    toks, images = _tokens(grid)
    S, ph, pw = ds.GRIDS[grid]
    hip = heads_hip.HipDPTHead(_head(which))
    hip.fused_tail = fused
    tape, val, conf = ds.run_recorded(heads_hip, hip, toks, images, MODES[mode])
    torch.cuda.synchronize()
    sched = ds.expected_schedule(ph, pw, ds.HEADS[which][0], fused and mode != "f32")
    ds.assert_schedule(tape, sched)
    return hip, tape, sched, val, conf


# =============================================================================================
# a. tiny grids, every element referenced
# =============================================================================================
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("which", ["depth", "point"])
@pytest.mark.parametrize("grid", ["4x7", "1x6", "6x1"])
def test_every_launch_of_both_heads_at_tiny_grids(grid, which, mode):
    toks, images = _tokens(grid)
    tapes = {}
    for fused in ((True, False) if mode != "f32" else (False,)):
        tag = "%s_%s_%s_%s" % (grid, which, mode, "fused" if fused else "three")
        hip, tape, sched, val, conf = _record(which, grid, mode, fused)
        assert len(tape) == (39 if fused else 41), tag
        for launch, s in zip(tape, sched):
            if launch.op == "conv":
                assert _dispatch(mode, launch) is None, "%s: %s is expected on the 128-pixel kernel" % (tag, s["name"])
        R = ds.check_tape(tape, sched, mode, tag=tag)
        assert max(R["worst"].values()) <= 1.0 and not R["failures"]
        for i, name, share in R["shares"]:
            assert share <= ds.WINDOW_CAP, "%s: the rounding window of launch %d (%s) holds %.1f%% of its map" % (tag, i, name, 100 * share)
        _note(mode, R)
        # one frame per pass: the same bytes as one pass over all frames
        with torch.no_grad():
            v1, c1 = hip(toks, images, 5, frames_chunk_size=1, dtype=MODES[mode])
        torch.cuda.synchronize()
        assert torch.equal(v1, val) and torch.equal(c1, conf), tag + ": frames_chunk_size=1 gives other bytes than one pass"
        kg.STATS["numeric"] += 1
        tapes[fused] = tape
    if len(tapes) == 2:
        for i in range(38):
            assert torch.equal(tapes[True][i].out, tapes[False][i].out), "%s %s %s: launch %d differs between the two forms of the output stage" % (grid, which, mode, i)
        kg.STATS["numeric"] += 1


# =============================================================================================
# b. across the 256-pixel line
# =============================================================================================
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_point_head_across_the_256_pixel_line(mode):
    grid, which = "19x18", "point"
    S, ph, pw = ds.GRIDS[grid]
    assert S * 4 * ph * 4 * pw == 64 * 256 + 32                # level 0: 64 tiles + 32 pixels, two image seams inside tiles
    hip, tape, sched, val, conf = _record(which, grid, mode, True)
    took = {s["name"]: _dispatch(mode, l) for l, s in zip(tape, sched) if l.op == "conv"}
    expect = {"layer1_rn": 256, "refinenet1.rcu1.conv1": 256, "refinenet1.rcu1.conv2": 256, "refinenet1.rcu2.conv1": 256, "refinenet1.rcu2.conv2": 256,
              "refinenet1.out_conv": 256, "output_conv1": 128}
    assert {k: v for k, v in took.items() if v is not None} == expect, took
    R = ds.check_tape(tape, sched, mode, tail_images=[0], tag="%s_%s_%s" % (grid, which, mode))
    assert max(R["worst"].values()) <= 1.0 and not R["failures"]
    assert set(expect) <= set(s[1] for s in R["sampled"])
    for i, name, share in R["shares"]:
        assert share <= ds.WINDOW_CAP, "%s: the rounding window of launch %d (%s) holds %.1f%% of its map" % (mode, i, name, 100 * share)
    _note(mode, R)
    torch.cuda.empty_cache()


# =============================================================================================
# c. the head's other launch shapes on the 256-pixel kernels
# =============================================================================================
#  name: (n, H, W, cin, cout, form); M is the least value over 16384 for the image size, and no multiple of 256
SHAPES = {
    "project_2048to256": (12, 37, 37, 2048, 256, dict(k=1, pos=True)),
    "project_2048to512": (12, 37, 37, 2048, 512, dict(k=1, pos=True)),
    "project_2048to1024": (12, 37, 37, 2048, 1024, dict(k=1, pos=True)),
    "convT4_256": (12, 37, 37, 256, 256, dict(up=4)),                       # 4096 GEMM columns
    "convT2_512": (12, 37, 37, 512, 512, dict(up=2)),                       # 2048 GEMM columns
    "3x3s2_1024": (46, 37, 37, 1024, 1024, dict(k=3, stride=2)),            # 46 x 19 x 19 outputs: images larger than a tile in, 361 pixels out
    "layer2_rn_512to256": (3, 74, 74, 512, 256, dict(k=3, relu=True, bias=False)),
    "layer3_rn_1024to256": (12, 37, 37, 1024, 256, dict(k=3, relu=True, bias=False)),
    "layer4_rn_1024to256": (46, 19, 19, 1024, 256, dict(k=3, relu=True, bias=False)),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_head_conv_shapes_on_the_256_pixel_kernels(mode, shape):
    n, H, W, cin, cout, f = SHAPES[shape]
    dt = MODES[mode]
    k, stride, up, relu, pos, has_bias = f.get("k", 1), f.get("stride", 1), f.get("up", 0), f.get("relu", False), f.get("pos", False), f.get("bias", True)
    s_ = up if up > 1 else 1
    pd = k // 2
    OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
    M = n * OH * OW
    assert M > 16384 and M % 256 != 0 and (n - 1) * OH * OW <= 16384, (shape, M)
    tag = "head_conv256_%s_%s" % (shape, mode)
    assert _expected_conv256(mode, n, H, W, cin, cout, k, stride, up, cin) == 256, tag
    g = torch.Generator(device=DEV).manual_seed(151 + list(SHAPES).index(shape))
    x = torch.randn(n, H, W, cin, device=DEV, generator=g).to(dt)
    w = (torch.randn(s_ * s_ * cout, k * k * cin, device=DEV, generator=g) * (k * k * cin) ** -0.5).to(dt)
    bias = torch.randn(cout, device=DEV, generator=g) * 0.3 if has_bias else None
    ps = (torch.randn(OW, cout // 2, device=DEV, generator=g) * 0.1, torch.randn(OH, cout // 2, device=DEV, generator=g) * 0.1) if pos else None
    slot = Slot.get((n, OH * s_, OW * s_, cout), dt, cout + 8, tag="hc256")
    ops.conv(x, w, bias, dt, cout, ksize=k, stride=stride, upshuffle=up, relu=relu, pos=ps, out=slot.view)
    _sync_check(slot.check)
    used, m, _ = ds.check_conv(tag, mode, x, w, bias, cout, k, stride, up, relu, None, None, ps, False, slot.view, seed=7)
    assert used <= 1.0 and m < M
    print("%s: M = %d (%d tiles + %d), %d GEMM columns, %d k-stages; %d rows referenced, budget used %.3f" % (
        tag, M, M // 256, M % 256, s_ * s_ * cout, k * k * cin // 32, m, used), flush=True)
    _note(mode, {"worst": {"conv 256-pixel": used}, "shares": []})
    Slot.cache.clear()
    torch.cuda.empty_cache()
