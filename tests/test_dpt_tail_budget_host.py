"""CPU-only proof of the per-element budget of the fused DPT output stage (kernel_guards.dpt_tail_budget): on every shape the GPU test
runs, torch's own f32 arithmetic (head_ops_emul: upsample -> conv -> dpt_out) stays inside the budget and every element of its 16-bit map
that differs from the reference's lies inside the rounding window; the window stays a small share of the map; planted defects of that chain
go over budget -- among them defects that gpu_selftest's global gate of the stage does not see. Every figure is printed."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import gpu_selftest as st
import head_ops_emul as emul
import kernel_guards as kg

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _global_ok(got, ref, tol):
    """gpu_selftest.report without touching the module's result list or the log."""
    keep = list(st.results)
    with contextlib.redirect_stdout(io.StringIO()):
        ok = st.report("x", got, ref, tol)
    st.results[:] = keep
    return ok


def _twin(I, mode, up=None, w1=None, b1="same", pad="zeros"):
    """The f32 chain on the case's inputs -> (val, conf, the 16-bit map); the keyword arguments plant a defect."""
    dt = DT[mode]
    up = emul.upsample(I["x"], I["OH"], I["OW"], dt, pos=I["pos"]) if up is None else up
    w1 = I["w1"] if w1 is None else w1
    b1 = I["b1"] if isinstance(b1, str) else b1
    if pad == "zeros":
        h = emul.conv(up, w1, b1, torch.float32, 32, ksize=3, relu=True, out_f32=True)
    else:
        xp = F.pad(up.float().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate")
        h = F.relu(F.conv2d(xp, w1.float().reshape(32, 3, 3, 128).permute(0, 3, 1, 2), None if b1 is None else b1.float())).permute(0, 2, 3, 1).contiguous()
    val, conf = emul.dpt_out(h, I["w2"], I["b2"], I["act"])
    return val, conf, up


def _budget(I, mode):
    return kg.dpt_tail_budget(I["x"].double(), I["OH"], I["OW"], I["pos"], I["w1"].double(), I["b1"], I["w2"], I["b2"], I["act"], mode)


def _verdict(name, val, conf, B, mode):
    """-> (the global gates accept it, the budget accepts it), printed."""
    gate = kg.DPT_TAIL_GATE[mode]
    g_ok = _global_ok(val, B["val"], gate) and _global_ok(conf, B["conf"], gate)
    try:
        used = kg.check_dpt_tail(name, val, conf, B, quiet=True)
        b_ok = True
    except AssertionError as e:
        b_ok, used = False, str(e).split(":", 1)[1].split(";")[0].strip()
    print("%-44s global gate %s, budget %s (%s)" % (name, "accepts" if g_ok else "REJECTS", "accepts" if b_ok else "REJECTS", used if not b_ok else "used %.3f" % used), flush=True)
    return g_ok, b_ok


def test_round16_is_the_formats_own_rounding():
    """round16 against torch's cast on values an f32 holds exactly (no double rounding there), ties and subnormals included, and its
    behaviour where a detour through f32 would go wrong: a float64 value just above a tie must round up."""
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-6, torch.randn(4096, generator=g) * 3e-8,
                   torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 2.0 ** -24, 3 * 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])])
    for mode, dt in DT.items():
        assert torch.equal(kg.round16(v.double(), mode), v.to(dt).double()), mode
    assert float(kg.round16(torch.tensor([1.00390625 + 2.0 ** -40], dtype=torch.float64), "bf16")) == 1.0078125     # f32 would see the tie: 1.0
    assert float(kg.round16(torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64), "f16")) == 1.0 + 2.0 ** -10


def test_bilinear_spec_is_atens_interpolation():
    """The specification's weights are the ones ATen uses: its f32 result is within C_UP u_acc mag of the float64 combination, on
    up- and downscales, degenerate axes and with the tables; the fused form of l differs from the plain one by at most half an ulp of f."""
    g = torch.Generator().manual_seed(2)
    for (H, W, OH, OW) in ((9, 11, 33, 29), (1, 6, 18, 15), (7, 1, 17, 16), (20, 23, 15, 17), (5, 4, 2, 31), (37, 28, 74, 56)):
        x = torch.randn(2, H, W, 16, generator=g)
        pos = (torch.randn(OW, 8, generator=g), torch.randn(OH, 8, generator=g))
        up, mag = kg.bilinear_spec(x.double(), OH, OW, pos)
        got = emul.upsample(x, OH, OW, torch.float32, pos=pos)
        assert kg.elementwise_budget("bilinear_%dx%d_%dx%d" % (H, W, OH, OW), got, up, mag, kg.U_OUT["f32"], kg.C_UP) <= 1.0
        for n_in, n_out in ((H, OH), (W, OW)):
            i0, i1, l = kg._axis_spec(n_in, n_out, False)
            _, _, lf = kg._axis_spec(n_in, n_out, True)
            f = i0.double() + l
            assert bool(((l - lf).abs() <= kg.U_ACC * f + 2.0 ** -149).all()) and bool((l >= 0).all()) and bool((i1 <= n_in - 1).all())


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_the_window_tells_a_contracted_coordinate_from_the_specified_one(mode):
    """l = fl(s o - i0) with the product unrounded (what contracting `fx = sx * oc; lx = fx - x0` into one multiply-subtract would give)
    differs from the specified l by at most half an ulp of f -- and the rounding window is sharp enough to reject the map it produces, while
    ATen's own map (the specified form) stays inside."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 53, 47, 32, generator=g).to(DT[mode])
    win = kg.upsample_window(x.double(), 75, 61, None, mode)
    kg.check_upsampled_map("aten_map_" + mode, emul.upsample(x, 75, 61, DT[mode]), win)
    contracted = kg.round16(kg.bilinear_spec(x.double(), 75, 61, None, fused=(True, True))[0], mode)
    with pytest.raises(AssertionError, match="not an admissible rounding"):
        kg.check_upsampled_map("contracted_l_" + mode, contracted, win)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_f32_twin_meets_the_budget_and_the_window_stays_small(mode):
    worst, worst_share = 0.0, 0.0
    for case in kg.DPT_TAIL_CASES:
        I = kg.dpt_tail_inputs(case, mode)
        B = _budget(I, mode)
        val, conf, up = _twin(I, mode)
        name = "dpt_tail_twin_%s_%s" % (case, mode)
        share, _ = kg.check_upsampled_map(name, up, B["win"])
        used = kg.check_dpt_tail(name, val, conf, B)
        # the condition on the inputs: a generous e_up must not quietly turn the gate into the global one
        assert share <= 0.10, "%s: the rounding window holds %.1f%% of the upsampled map" % (name, 100 * share)
        worst, worst_share = max(worst, used), max(worst_share, share)
        if kg.DPT_TAIL_CASES[case][9]:
            c1 = B["conf"] - 1.0
            print("%s: reference conf - 1 from %.3e to %.3e" % (name, float(c1.min()), float(c1.max())), flush=True)
            assert float(c1.min()) <= 1e-2 and float(B["conf"].max()) >= 10.0, "the confidence case does not span low and high confidences"
    print("dpt_tail f32 twin %s: worst used budget %.3f, largest window share %.2f%%" % (mode, worst, 100 * worst_share), flush=True)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_planted_defects_go_over_budget(mode):
    """Every mutant of the twin must fail the budget. Those that also fail the global gate are printed as such; the two value-level
    mutants below are built to sit under it."""
    I = kg.dpt_tail_inputs("persist_inv_pos", mode)
    B = _budget(I, mode)
    _, _, up = _twin(I, mode)
    tag = "mutant_%s_" % mode
    swapped = I["w1"].clone()
    swapped[:, :128], swapped[:, 128:256] = I["w1"][:, 128:256], I["w1"][:, :128]
    nob1 = I["b1"].clone()
    nob1[0] = 0.0
    hole = up.clone()
    hole[1, 17, 15] = 0
    shifted = emul.upsample(I["x"], I["OH"], I["OW"], DT[mode], pos=(I["pos"][0], torch.roll(I["pos"][1], 1, 0)))
    for name, kw in (("replicate_padding", dict(pad="replicate")), ("two_taps_exchanged", dict(w1=swapped)), ("one_b1_entry_dropped", dict(b1=nob1)),
                     ("one_patch_pixel_zeroed", dict(up=hole)), ("pos_y_shifted_by_one_row", dict(up=shifted))):
        val, conf, _ = _twin(I, mode, **kw)
        g_ok, b_ok = _verdict(tag + name, val, conf, B, mode)
        assert not b_ok, "the budget accepts the mutant %s" % name


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_defects_under_the_global_gate_are_rejected_by_the_budget(mode):
    """(i) inv_log: the sign of every value below a quarter of the global gate (relative to the tensor maximum) flipped: at most half the
    gate off, so the global gate accepts it by construction; the budget must reject it wherever its per-element bound is tighter than twice
    the value: asserted for bf16; in f16 the gate (5e-4) is already at the level of one map ulp carried through the stage, so the verdict
    is printed, not forced. (ii) confidence, both types: exp(o) flushed to zero below half the global gate on the input with low and high confidences."""
    gate = kg.DPT_TAIL_GATE[mode]
    seen = 0
    for case in ("persist_inv_pos", "downscale", "out_dim3"):
        I = kg.dpt_tail_inputs(case, mode)
        B = _budget(I, mode)
        val, conf, _ = _twin(I, mode)
        small = val.abs() < 0.25 * gate * float(B["val"].abs().max())
        bad = torch.where(small, -val, val)
        over = ((bad.double() - B["val"]).abs() > kg.U_OUT["f32"] * B["val"].abs() + B["c"] * kg.U_ACC * B["val_mag"] + B["val_extra"]) & small
        print("mutant_%s_%s sign flip: %d elements flipped, %d of them over budget" % (mode, case, int(small.sum()), int(over.sum())), flush=True)
        g_ok, b_ok = _verdict("mutant_%s_%s_small_values_sign_flipped" % (mode, case), bad, conf, B, mode)
        assert int(small.sum()) > 0 and g_ok, "the mutant was built to pass the global gate"
        if mode == "bf16":
            assert not b_ok, "the budget accepts flipped signs"
        elif b_ok:
            # f16: a quarter of the gate of 5e-4 is 1e-4 of the maximum, and one f16 ulp of a map element inside the window (2^-10 of it),
            # carried through |w1| and |w2|, is of that size: at this level the budget and the global gate are about equally tight
            print("f16 %s: the flipped values (below %.1e) are within the budget the rounding window leaves: not rejected, as derived" % (
                case, 0.25 * gate * float(B["val"].abs().max())), flush=True)
        seen += 0 if b_ok else 1
    I = kg.dpt_tail_inputs("conf_ramp", mode)
    B = _budget(I, mode)
    val, conf, _ = _twin(I, mode)
    e = conf - 1.0
    flushed = torch.where(e < 0.5 * gate * float(B["conf"].max()), torch.zeros_like(e), e) + 1.0
    print("mutant_%s_conf_flush: %d of %d confidences flushed to 1" % (mode, int((flushed != conf).sum()), conf.numel()), flush=True)
    g_ok, b_ok = _verdict("mutant_%s_small_confidences_flushed" % mode, val, flushed, B, mode)
    assert int((flushed != conf).sum()) > 0 and g_ok and not b_ok
    print("%s: %d mutants pass the global gate of %.0e and fail the budget" % (mode, seen + 1, gate), flush=True)
