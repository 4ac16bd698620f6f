"""-m gpu: ovg_flash_attn and ovg_attn_merge under wide logit spreads -- attention sinks, twin sinks, ramps, stairs over segment boundaries,
rows of one workgroup that disagree (tests/attn_spread.py: inputs, windows, the twin that test_attn_spread_host.py holds against the same
gates). Every case is ONE launch into guarded buffers (tests/kernel_guards.py) with poisoned padding and one comparison with the float64
reference of the stored values: outputs against the derived per-element budget of kernel_guards.attn_budget (unchanged), lse against
c u_acc / ln 2 + u_f32 |lse| (test_gpu_edges' own), and the tensor-global gate of test_gpu_edges.GATE -- except, in f32 / f32x only, on
attn_spread.PER_ELEMENT_ONLY, where no f32-accumulating kernel can hold it (shown on the CPU in test_attn_spread_host.py). The fallback
counter is asserted as exactly the (entry, key range, workgroup) units that hold a row outside the documented window. Every test prints
the running totals and the worst used budget fraction per mode."""
import functools
import math

import pytest
import torch

import attn_spread as sp
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops
from test_gpu_edges import DEV, GATE, MODES, SPLIT_FORMS, STORE, Slot, _attn_variants, _global, _need_gpu, _out_slot, _sync_check, _val  # noqa: F401

pytestmark = pytest.mark.gpu
WORST = {}                       # mode -> [outputs, lse]: worst used fraction of the budget so far
SPLIT16 = (L.ATTN_AUTO, L.ATTN_SPEC256, L.ATTN_LAZY256, L.ATTN_SPEC512, L.ATTN_LAZY128)   # kernels of the forced-split cases: every ring, both bodies


@pytest.fixture(autouse=True)
def _totals():
    yield
    for mode, (a, b) in sorted(WORST.items()):
        print("spread: %s worst used budget fraction so far: outputs %.3f, lse %.3f" % (mode, a, b), flush=True)


def _note(mode, f):
    w = WORST.setdefault(mode, [0.0, 0.0])
    w[0], w[1] = max(w[0], f[0]), max(w[1], f[1])


@functools.lru_cache(maxsize=3)
def _case(scn, mode, bg, nq, q_tile, kv_heads=0, nks=None):
    """One reference per (scenario, mode, background): built once at the longest row count its kernels need, shared and never changed."""
    c = sp.build(scn, mode, nq, bg, q_tile=q_tile, kv_heads=kv_heads, nks=nks)
    return c, sp.budget(c), _device_kv(c)


def _planes(t32, mode):
    if mode == "f32x":
        h = ops.to_hilo(t32)
        return [h.hi, h.lo]
    return [t32.to(STORE[mode])]


def _wrap(pl):
    return ops.HiLo((pl[0], pl[1])) if len(pl) == 2 else pl[0]


def _device_q(case, nq):
    """Rows 0..nq-1 of the case's q in a [BH, nq_pad, 64] buffer whose padding rows hold poison (as test_gpu_edges._attn_inputs lays it out)."""
    out = []
    for p_ in _planes(case.q32[:, :nq], case.mode):
        b_ = torch.zeros(sp.BH, ops.pad_to(nq, 64), 64, dtype=p_.dtype, device=DEV)
        b_[:, :nq] = p_.to(DEV)
        out.append(kg.poison_rows(b_, nq))
    return _wrap(out)


def _device_kv(case):
    segs, base = [], 0
    for nk in case.nks:
        nk_pad = ops.pad_to(nk, 64)
        kb, vb = [], []
        for p_ in _planes(case.k32[:, base:base + nk], case.mode):
            b_ = torch.zeros(p_.shape[0], nk_pad, 64, dtype=p_.dtype, device=DEV)
            b_[:, :nk] = p_.to(DEV)
            kb.append(kg.poison_rows(b_, nk))
        for p_ in _planes(case.v32[:, base:base + nk], case.mode):
            b_ = torch.zeros(p_.shape[0], 64, nk_pad, dtype=p_.dtype, device=DEV)
            ops.set_vt(b_, p_.transpose(1, 2))
            vb.append(kg.poison_vt(b_, nk, case.mode != "f32"))
        segs.append((_wrap(kb), _wrap(vb), nk))
        base += nk
    return segs


def _launch(mode, qd, segs, nq, variant=0, kv_heads=0, kv_splits=0, plan=None, cnt=None, cus=0):
    """One guarded launch -> (out [BH, nq, 64] float64, lse [BH, nq] float64). plan: its split workspace is guarded at exactly its bytes."""
    nq_pad = ops.pad_to(nq, 64)
    if kv_heads:
        out, checks = _out_slot(mode, (sp.BH, nq_pad, 64), False, 72, tag="sp_hm")
        out.fill_(-7.25)
    else:
        out, checks = _out_slot(mode, (nq, 1024), False, 1032, tag="sp_tm")
    ls = Slot.get((sp.BH, nq_pad), torch.float32, None, tag="sp_lse")
    ls.view.fill_(-7.25)
    ws = None
    if plan is not None and plan["part_bytes"] > 0:
        a = Slot.get((1, plan["part_bytes"]), torch.uint8, None, spare_rows=0, tag="sp_wsp")
        b = Slot.get((1, plan["lse_bytes"] // 4), torch.float32, None, spare_rows=0, tag="sp_wsl")
        ws, checks = (a.view.view(-1), b.view.view(-1)), checks + [a.check, b.check]
    ops.flash_attn(qd, segs, nq, MODES[mode], out=out, variant=variant, kv_heads=kv_heads, head_major=kv_heads > 0, lse=ls.view,
                   kv_splits=kv_splits, split_ws=ws, fallback_count=cnt, cus=cus)
    _sync_check(ls.check, *checks)
    assert bool((ls.view[:, nq:] == -7.25).all()), "the lse tail nq..nq_pad was written"
    o = _val(out)
    if kv_heads:
        assert bool((o[:, nq:] == -7.25).all()), "head-major rows nq..nq_pad were written"
        o = o[:, :nq]
    else:
        o = o.view(nq, 16, 64).permute(1, 0, 2)
    return o, ls.view[:, :nq].double().cpu()


def _gate(name, mode, scn, o, lse, b, splits=1):
    f = sp.check(name, o, lse, b, mode, splits)
    _note(mode, f)
    if not (mode in ("f32", "f32x") and scn in sp.PER_ELEMENT_ONLY):
        _global(name, o, b.ref, GATE[mode] * (1.5 if splits > 1 else 1.0))          # split launches: test_gpu_edges' own factor
    print("spread %-58s budget used %.3f (outputs) %.3f (lse)" % (name, f[0], f[1]), flush=True)


def _shapes(mode, variants):
    """variant -> (nq, q_tile); nq = 2 q_tile + 17 of the kernel under test (273, 529 or 1041 rows)."""
    return {v: sp.counted_shape(mode, v) for v in variants}


def _numeric(mode, scn, bg, kv_heads=0):
    variants = _attn_variants(mode)
    shapes = _shapes(mode, variants)
    for nq, qt in sorted(set(shapes.values())):
        if sp.SCENARIOS[scn].rows != "all":                  # the gain rows depend on the kernel's q tile: a case per tile
            case, b, segs = _case(scn, mode, bg, nq, qt, kv_heads)
        else:
            case, b, segs = _case(scn, mode, bg, max(n for n, _ in shapes.values()), None, kv_heads)
        qd, bn = _device_q(case, nq), sp.rows_of(b, nq)
        for v in variants:
            if shapes[v] == (nq, qt):
                o, lse = _launch(mode, qd, segs, nq, variant=v, kv_heads=kv_heads)
                _gate("%s_%s_%s_nq%d_v%d%s" % (scn, mode, bg, nq, v, "_kvh8" if kv_heads else ""), mode, scn, o, lse, bn)


@pytest.mark.parametrize("bg", list(sp.BG))
@pytest.mark.parametrize("scn", list(sp.SCENARIOS))
@pytest.mark.parametrize("mode", list(MODES))
def test_every_kernel_on_every_scenario(mode, scn, bg):
    """Every scenario x every kernel the mode has x both backgrounds, three workgroups with a ragged last one. The rising ramp makes the lazy
    rescale fire on every key tile, the falling one lets everything behind tile 0 underflow; twins at +G / +G + 1 carry 1/3 and 2/3 of the
    weight on different v, so a wrong weight shows in the outputs (one sink's would not: lse is what sees it there)."""
    _numeric(mode, scn, bg)
    Slot.cache.clear()


@pytest.mark.parametrize("bg", list(sp.BG))
@pytest.mark.parametrize("scn", [s.name for s in sp.SCENARIOS.values() if s.segs])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_segment_stairs_head_parallel(mode, scn, bg):
    """The multi-segment cases in the head-parallel form: 8 K / V^T heads shared by the 16 entries, head-major output."""
    _numeric(mode, scn, bg, kv_heads=8)
    Slot.cache.clear()


SPLIT_SCENARIOS = ("stairs_up_30", "stairs_down_30", "stairs_up_70", "stairs_down_70", "twins_12", "twins_40", "twins_130",
                   "sink_late_8", "sink_late_40", "sink_late_60", "sink_late_130")


@pytest.mark.parametrize("bg", list(sp.BG))
@pytest.mark.parametrize("scn", SPLIT_SCENARIOS)
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_forced_key_ranges(mode, scn, bg):
    """Whole-launch splits 2, 3, 4 and 8 (8 asks for more ranges than the tiles give: the plan's own count runs): every range's first-tile
    rule, the f32 partials and the merge launch under log-sum-exps that lie up to 210 units apart, in either order. Budget: the unsplit one +
    MARGIN (splits + 2); the two workspaces are guarded at exactly the plan's byte counts."""
    shapes = _shapes(mode, SPLIT16)
    case, b, segs = _case(scn, mode, bg, max(n for n, _ in shapes.values()), None)
    for nq in sorted({n for n, _ in shapes.values()}):
        qd, bn = _device_q(case, nq), sp.rows_of(b, nq)
        for v in SPLIT16:
            if shapes[v][0] != nq:
                continue
            for splits in (2, 3, 4, 8):
                plan = ops.attn_plan(sp.BH, nq, case.nks, MODES[mode], v, splits, nq_pad=ops.pad_to(nq, 64))
                assert plan["splits"] == len(sp.key_ranges(case.nks, splits)) > 1 and plan["tail_q_tile"] == 0, plan
                o, lse = _launch(mode, qd, segs, nq, variant=v, kv_splits=splits, plan=plan)
                _gate("%s_%s_%s_nq%d_v%d_s%d" % (scn, mode, bg, nq, v, splits), mode, scn, o, lse, bn, splits)
    Slot.cache.clear()


# the key layouts of the key-tail cases: a tail rule wants 16 (256-row) / 32 (512-row) key tiles per range, so the scenarios' gain patterns
# sit on longer key sets (the stairs: the four segments, each 16 tiles longer)
KEYTAIL_KEYS = {("key_tail_256", "twins_40"): (2048,), ("key_tail_512", "twins_40"): (4096,),
                ("key_tail_256", "stairs_up_70"): (1124, 1357, 1088, 1224), ("key_tail_512", "stairs_up_70"): (1124, 1357, 1088, 1224)}


@pytest.mark.parametrize("scn", ["twins_40", "stairs_up_70"])
@pytest.mark.parametrize("form", ["key_tail_256", "key_tail_512"])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_key_tail_forms(mode, form, scn):
    """The two key-split-tail forms of test_gpu_edges.SPLIT_FORMS (their nq, cus and plan): the rows beyond the last full round run in two key
    ranges and are merged, the others unsplit, in one call. The reference covers every tail row and 16 rows of the unsplit part."""
    nq, variant, splits, cus, want = SPLIT_FORMS[form]
    nks = KEYTAIL_KEYS[(form, scn)]
    plan = ops.attn_plan(sp.BH, nq, list(nks), MODES[mode], variant, splits, nq_pad=ops.pad_to(nq, 64), cus=cus)
    assert plan == want, (form, plan)
    case = sp.build(scn, mode, nq, "wide", nks=nks)
    o, lse = _launch(mode, _device_q(case, nq), _device_kv(case), nq, variant=variant, kv_splits=splits, plan=plan, cus=cus)
    main = plan["main_rows"]
    rows = torch.cat([torch.arange(0, main, main // 16)[:16], torch.arange(main, nq)])
    b = sp.budget(case._replace(q=case.q[:, rows]))
    _gate("%s_%s_%s" % (scn, mode, form), mode, scn, o[:, rows], lse[:, rows], b, splits)
    Slot.cache.clear()


MERGE_GAPS = (0.0, 1.0, 24.0, 70.0, 126.0, 150.0, 300.0)


@pytest.mark.parametrize("mode", list(MODES))
def test_attn_merge_of_two_real_calls_under_large_lse_gaps(mode):
    """a and b are two ovg_flash_attn results over disjoint key sets (101 keys each) with their lse; the second set's logits are lifted by
    the gap, and both orders are merged. Budget as in test_attn_merge_and_heads_to_tokens_short_rows_strided with the |lse| actually
    present: 16 + 2 ln 2 max |lse| roundings. From a gap of 150 on the smaller weight's exp2 is 0 and the other is 1: the result must be
    the dominant input bit for bit (both planes in f32x).

    Finding recorded here: in f32x the first run of this test gave 47 of 82 944 values (and 72 hi / 119 lo plane entries) that were NOT the
    dominant input at a gap of 150 (the first such case), each off by 2^-24 on a value in [1, 2). An attention output pair holds more bits than an f32 --
    store4_hilo's `a - hi` is fused with the product o * inv that makes a, so lo comes from the unrounded product -- and the merge kernel formed
    hi + lo in f32 before weighting. Inside the mode's 2^-22, but not the identity a weight of 1 against 0 must be: csrc/ovg_elem.hip now
    hands the pair through when a weight is exactly 0. bf16, f16 and f32 were bit-identical from the start."""
    dt, nq = MODES[mode], 81
    g = torch.Generator().manual_seed(7300)
    q32 = torch.randn(sp.BH, nq, 64, generator=g) * sp.BG["narrow"]
    q32[..., 0] = sp.Q_GAIN
    qc = sp.Case("merge", mode, "narrow", nq, [101], q32, None, None, None, None, None, None, None)
    qd = _device_q(qc, nq)
    sides = {}
    for gap in ("base",) + MERGE_GAPS:
        k32, v32 = torch.randn(sp.BH, 101, 64, generator=g), torch.randn(sp.BH, 101, 64, generator=g)
        k32[..., 0] = 0.0 if gap == "base" else gap / sp.Q_GAIN
        c = qc._replace(k32=k32, v32=v32)
        out, checks = _out_slot(mode, (nq, 1024), False, 1040, tag="mg_in%s" % gap)
        ls = Slot.get((sp.BH, ops.pad_to(nq, 64)), torch.float32, None, tag="mg_lse%s" % gap)
        ops.flash_attn(qd, _device_kv(c), nq, dt, out=out, lse=ls.view)
        _sync_check(ls.check, *checks)
        sides[gap] = (out, ls.view, _val(out), ls.view[:, :nq].double().cpu())
    base = sides["base"]
    for gap in MERGE_GAPS:
        lifted = sides[gap]
        for order, (A, B) in (("ab", (base, lifted)), ("ba", (lifted, base))):
            res, checks = _out_slot(mode, (nq, 1024), False, 1040, tag="mg_out")
            ops.attn_merge(A[0], A[1], B[0], B[1], dt, out=res)
            _sync_check(*checks)
            got = _val(res)
            la, lb = A[3].t().repeat_interleave(64, 1), B[3].t().repeat_interleave(64, 1)
            m = torch.maximum(la, lb)
            wa, wb = torch.exp2(la - m), torch.exp2(lb - m)
            ref, mag = (wa * A[2] + wb * B[2]) / (wa + wb), (wa * A[2].abs() + wb * B[2].abs()) / (wa + wb)
            name = "merge_%s_gap%g_%s" % (mode, gap, order)
            true_gap = float((la - lb).abs().median())
            assert abs(true_gap - gap) < 2.0, (name, true_gap)             # the inputs are what the case says (the lifted set is one of 101 keys like the base)
            c = kg.MARGIN * (16 + 2 * math.log(2.0) * float(torch.maximum(la.abs(), lb.abs()).max()))
            f = kg.elementwise_budget(name, got, ref, mag, kg.U_OUT[mode], c, extra=kg.f16_subnormal_floor(mode), quiet=True)
            _global(name, got, ref, GATE[mode])
            if gap >= 150.0:
                dom = A if order == "ba" else B
                same = all(torch.equal(x, y) for x, y in zip(ops.hi_lo(res), ops.hi_lo(dom[0])) if x is not None)
                assert same and torch.equal(got, dom[2]), "%s: the merge of a weight-1 and a weight-0 input is not the weight-1 input" % name
            print("spread %-40s lse gap %.1f, budget used %.3f" % (name, true_gap, f), flush=True)
    Slot.cache.clear()


def _count(mode, variant, kv_splits, scn, poison=7):
    nq, qt = sp.counted_shape(mode, variant)
    case, b, segs = _case(scn, mode, "narrow", nq, qt)
    plan = ops.attn_plan(sp.BH, nq, case.nks, MODES[mode], variant, kv_splits, nq_pad=ops.pad_to(nq, 64)) if mode in ("bf16", "f16") and variant != 1 else None
    cnt = torch.full((1,), poison, dtype=torch.int32, device=DEV)
    _launch(mode, _device_q(case, nq), segs, nq, variant=variant, kv_splits=kv_splits, plan=plan, cnt=cnt)
    return int(cnt.item()) - poison, case, plan


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_fallback_counter_is_exactly_the_units_with_an_offending_row(mode):
    """Narrow background. count == the (entry, key range, workgroup) units that hold at least one row outside the documented window, from the
    float64 logits (never from the kernel's output); 0 where every row is inside; no row is in the guard zone. `nothing is written
    otherwise`: the counter starts at 7 and only ever grows by the count."""
    for variant, kv_splits, scn in sp.counter_cases(mode):
        got, case, plan = _count(mode, variant, kv_splits, scn)
        bad, total, guard = sp.expected_fallbacks(sp.logits(case), case.nks, plan, mode)
        assert guard == 0, "guard zone"
        print("fallbacks %s v%d ranges %d %-20s %d of %d units re-ran, expected %d" % (mode, variant, plan["splits"], scn, got, total, bad), flush=True)
        assert got == bad, "%s v%d kv_splits %d %s: %d units re-ran, %d hold an offending row (of %d)" % (mode, variant, kv_splits, scn, got, bad, total)
        kg.STATS["numeric"] += 1
    Slot.cache.clear()


@pytest.mark.parametrize("mode", list(MODES))
def test_fallback_counter_forced_and_never(mode):
    """FORCED256 counts every unit; the lazy-rescale kernels, the baseline kernel, f32 and f32x never touch the counter (it keeps a non-zero
    value written before the call)."""
    for scn in ("none", "sink_late_130"):
        if mode in ("bf16", "f16"):
            for kv_splits in (1, 3):
                got, case, plan = _count(mode, sp.FORCED256, kv_splits, scn)
                assert got == sp.BH * plan["splits"] * 3, "FORCED256 %s %s: %d of %d units" % (mode, scn, got, sp.BH * plan["splits"] * 3)
                for v in (L.ATTN_LAZY256, L.ATTN_LAZY128):
                    assert _count(mode, v, kv_splits, scn)[0] == 0, "lazy-rescale kernel %d touched the fallback counter" % v
            assert _count(mode, L.ATTN_BASELINE, 0, scn)[0] == 0
            if mode == "f16":
                assert _count(mode, L.ATTN_AUTO, 0, scn)[0] == 0, "the f16 default is a lazy-rescale kernel"
        else:
            assert _count(mode, _attn_variants(mode)[0], 0, scn)[0] == 0, "%s touched the fallback counter" % mode
        kg.STATS["numeric"] += 1
    Slot.cache.clear()
