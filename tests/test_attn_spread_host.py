"""Host checks of tests/attn_spread.py, the method behind test_gpu_attn_spread.py (no GPU): the twin of the documented 16-bit arithmetic
stays inside kernel_guards' unchanged budgets on every scenario, each planted fault is rejected by the gates, the gain values are exact in
every storage type, no row of a counted launch lies in the classifier's guard zone, and the classifier's key ranges and workgroups are
the ones ops.attn_plan reports."""
import functools

import pytest
import torch

import attn_spread as sp
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops

NQ, QT = 81, 32                      # the twin's shape: three "workgroups" of 32 rows, a ragged last one, 16-row groups that end inside them
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}


@functools.lru_cache(maxsize=None)
def _case(scn, mode, bg):
    c = sp.build(scn, mode, NQ, bg, q_tile=QT)
    return c, sp.budget(c)


@pytest.mark.parametrize("bg", list(sp.BG))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("scn", list(sp.SCENARIOS))
def test_twin_of_the_documented_arithmetic_is_inside_the_budget(scn, mode, bg):
    case, b = _case(scn, mode, bg)
    worst = [0.0, 0.0]
    for body in ("lazy", "anchored"):
        for splits in (1, 3):
            out, lse, _ = sp.twin(case, body, splits, wg_rows=QT)
            f = sp.check("twin_%s_%s_%s_%s_s%d" % (scn, mode, bg, body, splits), out, lse, b, mode, splits)
            worst = [max(worst[0], f[0]), max(worst[1], f[1])]
            assert sp.global_err(out, b.ref) <= kg.U_OUT[mode] * 4, "global"
    print("twin %s %s %s: worst used budget fraction %.3f (outputs) %.3f (lse)" % (scn, mode, bg, worst[0], worst[1]))


def _rejected(scn, mode, bg, body, splits, fault):
    case, b = _case(scn, mode, bg)
    out, lse, _ = sp.twin(case, body, splits, fault=fault, wg_rows=QT)
    try:
        sp.check("fault", out, lse, b, mode, splits)
    except AssertionError:
        return True
    return False


def test_every_planted_fault_is_rejected_by_the_gates():
    """The method's self-check: l not rescaled where o is (lazy body), f16 P clamped at 65504 so that the verification accepts an overflowed
    pass (anchored f16), merge weights against range 0's log-sum-exp instead of the maximum (3 ranges)."""
    assert _rejected("ramp_up_200", "bf16", "narrow", "lazy", 1, "l_not_rescaled")
    assert _rejected("sink_late_40", "f16", "wide", "lazy", 1, "l_not_rescaled")
    assert _rejected("twins_40", "f16", "narrow", "anchored", 1, "f16_p_clamped")
    assert _rejected("sink_late_40", "f16", "narrow", "anchored", 1, "f16_p_clamped"), "one clamped sink: lse must see it"
    assert _rejected("stairs_up_70", "bf16", "narrow", "anchored", 3, "merge_against_range0")
    assert _rejected("stairs_up_70", "f16", "wide", "lazy", 3, "merge_against_range0")
    # the same configurations without the fault pass (else the rejections above would prove nothing)
    for scn, mode, bg, body, splits in (("ramp_up_200", "bf16", "narrow", "lazy", 1), ("twins_40", "f16", "narrow", "anchored", 1),
                                        ("stairs_up_70", "bf16", "narrow", "anchored", 3)):
        assert not _rejected(scn, mode, bg, body, splits, None)


def test_one_sink_hides_a_wrong_weight_from_the_outputs_but_not_from_lse():
    """Why lse is asserted everywhere and why there are twins: with ONE +40 sink the clamped-P fault passes the output budget (the output is
    the sink's v whatever its weight) and only lse rejects it."""
    case, b = _case("sink_late_40", "f16", "narrow")
    out, lse, _ = sp.twin(case, "anchored", 1, fault="f16_p_clamped", wg_rows=QT)
    kg.elementwise_budget("one_sink_outputs", out, b.ref, b.mag, kg.U_OUT["f16"], b.c, extra=b.floor, quiet=True)
    assert float((lse - b.lse).abs().max()) > 1.0


def test_gain_values_are_exact_in_every_storage_type():
    for scn in sp.SCENARIOS.values():
        g = sp.key_gains(scn, list(sp.SEGS) if scn.segs else [sp.NK])
        for mode in sp.STORE:
            assert torch.equal(sp.stored(g, mode), g.double()), (scn.name, mode)
            assert torch.equal(sp.stored(torch.tensor([sp.Q_GAIN]), mode), torch.tensor([sp.Q_GAIN], dtype=torch.float64))
        assert float(g.abs().max()) * sp.Q_GAIN <= 210.0
    c = sp.build("twins_40", "bf16", NQ, "wide", q_tile=QT)
    s = sp.logits(c)
    bgd = sp.logits(sp.build("twins_40", "bf16", NQ, "wide", q_tile=QT)._replace(k=c.k * (torch.arange(64) > 0)))
    assert torch.equal((s - bgd)[..., sp.TWIN_KEYS[0]], torch.full((sp.BH, NQ), 40.0, dtype=torch.float64))
    assert torch.equal((s - bgd)[..., sp.TWIN_KEYS[1]], torch.full((sp.BH, NQ), 41.0, dtype=torch.float64))


def test_a_longer_case_extends_the_shorter_one():
    a, b = sp.build("sink_late_60", "f16", 273, "narrow"), sp.build("sink_late_60", "f16", 529, "narrow")
    assert torch.equal(a.q, b.q[:, :273]) and torch.equal(a.k, b.k) and torch.equal(a.v, b.v)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_no_row_of_a_counted_launch_is_in_the_guard_zone(mode):
    """The stated condition of the fallback-counter test, for the committed seeds and the shapes it runs (the plan is a host-only query)."""
    seen = 0
    for variant, splits, scn in sp.counter_cases(mode):
        nq, q_tile = sp.counted_shape(mode, variant)
        case = sp.build(scn, mode, nq, "narrow", q_tile=q_tile)
        plan = ops.attn_plan(sp.BH, nq, case.nks, DT[mode], variant, splits)
        assert plan["q_tile"] == q_tile and plan["splits"] == (splits if splits > 1 else 1), (variant, splits, plan)
        bad, total, guard = sp.expected_fallbacks(sp.logits(case), case.nks, plan, mode)
        assert guard == 0, "%s v%d splits %d %s: %d rows in the guard zone" % (mode, variant, splits, scn, guard)
        assert total == sp.BH * plan["splits"] * 3
        if scn == "none" or scn == "sink_late_8":
            assert bad == 0
        elif scn.startswith("rowmixed"):
            assert bad == sp.BH, "only the middle workgroup of the sink's key range holds an offending row"
        seen += 1
    assert seen >= 20


def test_key_ranges_and_workgroups_are_the_plans():
    for nks in ([sp.NK], list(sp.SEGS)):
        tiles = len(sp.key_tiles(nks))
        assert tiles == sum((n + 63) // 64 for n in nks)
        for splits in (2, 3, 4, 8):
            plan = ops.attn_plan(sp.BH, 529, nks, torch.bfloat16, L.ATTN_SPEC256, splits)
            r = sp.key_ranges(nks, plan["splits"])
            assert len(r) == plan["splits"] and r[0][0] == 0 and r[-1][2] == sum(nks)
            assert all(a[2] == b[0] for a, b in zip(r, r[1:])), "the ranges tile the keys"
            assert plan["part_bytes"] == len(r) * sp.BH * 576 * 64 * 4
    # three ranges of the 10-tile layout start at keys 0 / 256 / 512: key 400 is in the second range and not in its first tile
    assert sp.key_ranges([sp.NK], 3) == [(0, 64, 256), (256, 320, 512), (512, 576, 640)]
    # the two key-tail forms of test_gpu_edges.SPLIT_FORMS: full rounds unsplit, the remaining rows in two key ranges
    for nq, variant, cus, main in ((4140, L.ATTN_PLAN_KEYTAIL256, 24, 3840), (4696, L.ATTN_PLAN_KEYTAIL512, 12, 4608)):
        nks = [nq]
        plan = ops.attn_plan(sp.BH, nq, nks, torch.bfloat16, variant, 2, cus=cus)
        assert sp.launches(plan, nq) == [(1, plan["q_tile"], 0, main), (2, plan["q_tile"], main, nq)]


def test_which_scenarios_the_f32_global_gate_cannot_hold():
    """GATE is max |err| / max |ref| <= 2e-5 (f32) / 1e-5 (f32x). A logit of 130 has an f32 ulp of 2^-16 = 1.5e-5 log2 units, and keys that share
    a row's weight turn an error d of their logit difference into w1 w2 ln 2 |v1 - v2| d on the output. The float64 softmax with its logits
    rounded ONCE to f32 is what any f32-accumulating kernel pays at least; the gain product enters the accumulator with the first step, so all
    S_CHAIN partial sums behind it carry that magnitude and each may round as far. On the scenarios of attn_spread.PER_ELEMENT_ONLY that bound
    exceeds the gate: they are gated per element only (the budget carries the |s| term); every other scenario is also gated globally."""
    for mode, gate in (("f32", 2e-5), ("f32x", 1e-5)):
        for scn in sp.PER_ELEMENT_ONLY:
            once = max(sp.s_rounding_global_error(sp.build(scn, mode, NQ, bg, q_tile=QT)) for bg in sp.BG)
            print("%s %s: one f32 rounding of s = %.2e of max|ref|, x %d = %.2e (gate %.0e)" % (mode, scn, once, sp.S_CHAIN[mode], once * sp.S_CHAIN[mode], gate))
            assert once * sp.S_CHAIN[mode] > gate, (mode, scn, once)
    assert all(float(sp.key_gains(sp.SCENARIOS[n], list(sp.SEGS) if sp.SCENARIOS[n].segs else [sp.NK]).abs().max()) * sp.Q_GAIN >= 130.0 for n in sp.PER_ELEMENT_ONLY)
