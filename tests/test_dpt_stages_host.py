"""CPU: the launch tape and stage checker of tests/dpt_stages.py on the torch emulation of the DPT-head entries (tests/head_ops_emul.py).
HipDPTHead runs unchanged with the emulation in place of the kernels; the tape must equal the schedule written from the reference head's
structure, every launch of the emulated chain must pass the per-element checker in all three modes for both heads at every grid the GPU test
uses, the rounding window of every 16-bit resize must stay under the cap, and each of eight planted defects must fail the checker at its
own launch and at no other (later launches are referenced from their own recorded inputs). For every defect the test prints whether the
whole-head global gate of gpu_selftest.test_heads would have seen it."""
import importlib
import inspect
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import omnivggt_official_amd  # noqa: F401,E402  (root shim: registers the package under an importable name)
import dpt_stages as ds  # noqa: E402
import kernel_guards as kg  # noqa: E402

heads = importlib.import_module("omnivggt_official_amd.heads")
heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")

GRIDS = ds.GRIDS
_CACHE = {}


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _setup(grid, which):
    key = (grid, which)
    if key not in _CACHE:
        if len(_CACHE) > 2:
            _CACHE.clear()
        S, ph, pw = GRIDS[grid]
        head = ds.rand_head(heads, which)
        toks, images = ds.rand_tokens(S, ph, pw)
        _CACHE[key] = (head, toks, images)
    return _CACHE[key]


def _run(grid, which, mode, fused, mutate=None):
    head, toks, images = _setup(grid, which)
    S, ph, pw = GRIDS[grid]
    hip = heads_hip.HipDPTHead(head)
    hip.fused_tail = fused
    tape, val, conf = ds.run_recorded(heads_hip, hip, toks, images, ds.MODES[mode], impl=ds.EMUL, mutate=mutate)
    sched = ds.expected_schedule(ph, pw, ds.HEADS[which][0], fused and mode != "f32")
    return tape, sched, val, conf


def test_recorder_restores_the_entries_and_keeps_production_untouched():
    before = {k: getattr(heads_hip.ops, k) for k in ds.OPS + ("dpt_tail_supported",)}
    with pytest.raises(RuntimeError):
        with ds.recording(heads_hip.ops, impl=ds.EMUL) as tape:
            assert heads_hip.ops.conv is not before["conv"]
            heads_hip.ops.upsample(torch.zeros(1, 2, 2, 8), 3, 3, torch.float32)
            raise RuntimeError("leave through an exception")
    assert len(tape) == 1 and tape[0].op == "upsample" and tape[0].scalars["OH"] == 3 and tape[0].arg("pos") is None
    assert all(getattr(heads_hip.ops, k) is v for k, v in before.items())


def test_schedule_counts_and_a_wrong_schedule_is_noticed():
    for fused, count in ((True, 39), (False, 41)):
        tape, sched, _, _ = _run("4x7", "depth", "bf16", fused)
        assert len(sched) == count
        ds.assert_schedule(tape, sched)
    assert len(_run("4x7", "depth", "f32", True)[0]) == 41          # f32 has no fused output stage
    tape, sched, _, _ = _run("4x7", "depth", "bf16", True)
    for field, value in (("relu", False), ("adds", 1), ("cin", 512)):
        i = [s["name"] for s in sched].index("refinenet3.rcu1.conv2")
        wrong = [dict(s) for s in sched]
        wrong[i][field] = value
        with pytest.raises(AssertionError, match="launch %d " % i):
            ds.assert_schedule(tape, wrong)


def test_sample_conditions_and_the_gathered_reference_equals_conv_ref():
    for n, OH, OW in ((3, 76, 72), (1, 129, 129), (46, 19, 19), (12, 37, 37), (2, 16, 8), (5, 1, 60)):
        rows = ds.sample_rows(n, OH, OW, seed=n)
        ds.assert_sample_conditions(rows, n, OH, OW)
        M = n * OH * OW
        assert rows.numel() <= max(M // 16, 700) or M <= 1024, (n, OH, OW, rows.numel())
        # every condition is load-bearing: drop the rows of one and the assertion fires
        nt = (M + 255) // 256
        for drop in ([0], [M - 1], [OW - 1], [min(255, M - 1)], [((nt - 1) * 256 + M) // 2],[OH * OW] if n > 1 else [OW // 2]):
            keep = rows[~torch.isin(rows, torch.tensor(drop))]
            with pytest.raises(AssertionError):
                ds.assert_sample_conditions(keep, n, OH, OW)
    g = torch.Generator().manual_seed(3)
    for k, stride, up, relu, adds, pos in ((1, 1, 0, False, 0, True), (3, 1, 0, True, 2, False), (3, 2, 0, False, 1, False), (1, 1, 2, False, 0, False), (1, 1, 4, True, 0, True)):
        n, H, W, cin, cout = 3, 19, 23, 32, 16
        s = up if up > 1 else 1
        pd = k // 2
        OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
        x = torch.randn(n, H, W, cin, generator=g).bfloat16()
        w = torch.randn(s * s * cout, k * k * cin, generator=g).bfloat16()
        bias = torch.randn(cout, generator=g)
        a = [torch.randn(n, OH * s, OW * s, cout, generator=g).bfloat16() for _ in range(adds)] + [None, None]
        ps = (torch.randn(OW * s, cout // 2, generator=g), torch.randn(OH * s, cout // 2, generator=g)) if pos else None
        d = lambda t: None if t is None else t.double()
        ref, mag = kg.conv_ref(d(x), d(w), d(bias), cout, k, stride, up, relu, d(a[0]), d(a[1]), None if ps is None else (d(ps[0]), d(ps[1])))
        rows = torch.arange(n * OH * OW)
        r2, m2, got = ds.conv_ref_rows(x, w, bias, cout, k, stride, up, relu, a[0], a[1], ps, rows, out=ref)
        full = lambda t: t.view(n, OH, OW, s, s, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, OH * s, OW * s, cout)
        assert torch.allclose(full(r2), ref, rtol=1e-12, atol=1e-12) and torch.allclose(full(m2), mag, rtol=1e-12, atol=1e-12)
        assert torch.equal(full(got), ref)


def test_bilinear_spec_with_one_pixel_sides_is_source_row_or_column_zero():
    g = torch.Generator().manual_seed(5)
    for H, W, OH, OW in ((1, 3, 1, 5), (3, 1, 5, 1), (2, 3, 1, 1), (3, 4, 1, 7), (4, 3, 6, 1)):
        x = torch.randn(2, H, W, 16, generator=g).double()
        up, mag = kg.bilinear_spec(x, OH, OW)
        ref = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert torch.allclose(up, ref, rtol=0, atol=1e-6), (H, W, OH, OW)
        src = x[:, :1] if OH == 1 else x
        src = src[:, :, :1] if OW == 1 else src
        up0, _ = kg.bilinear_spec(src, OH, OW)
        assert torch.equal(up, up0), "an output side of one pixel reads source row / column 0 alone"
        win = kg.upsample_window(x.bfloat16().double(), OH, OW, None, "bf16")
        kg.check_upsampled_map("spec_%dx%d_to_%dx%d" % (H, W, OH, OW), win["r16"], win)


def _summary(tag, R):
    print("%s: worst used budget %s; window shares %s; sampled launches %d" % (
        tag, ", ".join("%s %.3f" % kv for kv in sorted(R["worst"].items())), ", ".join("#%d %.3f" % (i, s) for i, _, s in R["shares"]), len(R["sampled"])), flush=True)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("which", ["depth", "point"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_emulated_chain_passes_the_stage_checker(grid, which, mode):
    forms = (True,) if (mode == "f32" or grid == "19x18") else (True, False)
    for fused in forms:
        tape, sched, _, _ = _run(grid, which, mode, fused)
        ds.assert_schedule(tape, sched)
        R = ds.check_tape(tape, sched, mode, tag="%s_%s_%s" % (grid, which, mode))
        _summary("emulation %s %s %s fused=%s" % (grid, which, mode, fused), R)
        assert max(R["worst"].values()) <= 1.0
        if mode != "f32":
            assert len(R["shares"]) == 5
            for i, name, share in R["shares"]:
                assert share <= ds.WINDOW_CAP, "%s: the rounding window of launch %d (%s) holds %.1f%% of its map" % (grid, i, name, 100 * share)
        if grid == "19x18":
            assert [s[1] for s in R["sampled"]][:2] == ["layer1_rn", "layer2_rn"] and "output_conv1" in [s[1] for s in R["sampled"]]


# ---- planted defects ------------------------------------------------------------------------------
def _kw(fn, a, kw):
    b = inspect.signature(fn).bind(*a, **kw)
    b.apply_defaults()
    return dict(b.arguments)


def _edit(**changes):
    def f(fn, *a, **kw):
        k = _kw(fn, a, kw)
        k.update(changes)
        return fn(**k)
    return f


def _kstage_zeroed(fn, *a, **kw):
    k = _kw(fn, a, kw)
    k["w"] = k["w"].clone()
    k["w"][:, 32 * 137:32 * 138] = 0             # k-stage 137 of 288: tap 4 (the centre), channels 288..319
    return fn(**k)


def _uv_swapped(fn, *a, **kw):
    k = _kw(fn, a, kw)
    n, ph, pw, _ = k["x"].shape
    k["pos"] = heads_hip.uv_tables(k["cout"], ph, pw, ph * 14, pw * 14, k["x"].device)      # (W, H) are (pw, ph) * 14: passed as (H, W)
    return fn(**k)


def _scatter_transposed(fn, *a, **kw):
    y = fn(*a, **kw)
    n, H2, W2, c = y.shape
    return y.reshape(n, H2 // 2, 2, W2 // 2, 2, c).permute(0, 1, 4, 3, 2, 5).reshape(n, H2, W2, c).contiguous()


def _half_pixel(fn, *a, **kw):
    k = _kw(fn, a, kw)
    y = F.interpolate(k["x"].float().permute(0, 3, 1, 2), size=(k["OH"], k["OW"]), mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous().to(k["dtype"])


def _specials_not_skipped(fn, *a, **kw):
    k = _kw(fn, a, kw)
    tpv, ns = k["tokens_per_view"], k["n_special"]
    x = k["x"].reshape(k["views"], tpv, -1)[:, : tpv - ns].reshape(k["views"] * (tpv - ns), -1)
    return fn(x, k["weight"], k["bias"], k["eps"], k["dtype"], k["views"], tokens_per_view=tpv - ns, n_special=0)


DEFECTS = {
    "bias dropped in refinenet2.out_conv": ("refinenet2.out_conv", _edit(bias=None)),
    "one 32-channel k-stage zeroed in the 3x3 stride 2": ("level3.resize_3x3s2", _kstage_zeroed),
    "UV tables with W and H swapped on level 2": ("level2.project", _uv_swapped),
    "(dy, dx) transposed in the ConvTranspose 2 scatter": ("level1.resize_convT2", _scatter_transposed),
    "ReLU missing on layer4_rn": ("layer4_rn", _edit(relu=False)),
    "add2 ignored in refinenet3.rcu1": ("refinenet3.rcu1.conv2", _edit(add2=None)),
    "align_corners=False in refinenet2.resize": ("refinenet2.resize", _half_pixel),
    "LayerNorm rows taken without skipping the special tokens": ("level1.norm", _specials_not_skipped),
}


def _head_error(val, conf, ref):
    return max(float((val.double() - ref[0].double()).abs().max() / ref[0].abs().max()), float((conf.double() - ref[1].double()).abs().max() / ref[1].abs().max()))


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_fails_at_its_own_launch_and_nowhere_else(defect, mode):
    grid, which = "4x7", "point"
    head, toks, images = _setup(grid, which)
    if "ref" not in _CACHE:
        with torch.no_grad():
            _CACHE["ref"] = head(toks, images=images, patch_start_idx=5)
    ref = _CACHE["ref"]
    name, plant = DEFECTS[defect]
    S, ph, pw = GRIDS[grid]
    sched = ds.expected_schedule(ph, pw, ds.HEADS[which][0], mode != "f32")
    at = [s["name"] for s in sched].index(name)
    clean = _run(grid, which, mode, True)
    tape, sched, val, conf = _run(grid, which, mode, True, mutate={at: plant})
    ds.assert_schedule(tape, sched)
    assert not torch.equal(tape[at].out, clean[0][at].out), "the planted defect changes nothing"
    R = ds.check_tape(tape, sched, mode, collect=True, tag="defect")
    assert [f[0] for f in R["failures"]] == [at], "%s (%s): planted at launch %d (%s), the checker failed at %s" % (
        defect, mode, at, name, [(f[0], f[1]) for f in R["failures"]])
    err, base = _head_error(val, conf, ref), _head_error(clean[2], clean[3], ref)
    print("defect '%s' (%s): caught at launch %d (%s): %s" % (defect, mode, at, name, R["failures"][0][2][:160]), flush=True)
    print("defect '%s' (%s): whole-head error %.3e (clean %.3e) against the global gate %.1e -> the global gate %s it" % (
        defect, mode, err, base, ds.HEAD_GATE[mode], "SEES" if err > ds.HEAD_GATE[mode] else "MISSES"), flush=True)
