"""Attention under wide logit spreads (a plain helper module like kernel_guards; no GPU): synthetic attention sinks, ramps and stairs, a
classifier of the speculative pass's verification windows, and a torch twin of the arithmetic that csrc/ovg_attn16.h documents.

Inputs. Dimension 0 of q / k is a gain channel: q[..., 0] = 4 on the chosen rows (0 elsewhere) and k[..., 0] = boost / 4, so a key's logit
is lifted by `boost` log2 units for exactly those rows. Every gain value is a bf16 number (8 significand bits), hence exact in every
storage type. The other 63 dimensions are randn, q times a background scale (BG: 0.3 "narrow", 1.2 "wide" = the N(0, 9.6) logits of the
other tests); all values are rounded to the storage type before any reference sees them. BH = 16; 640 keys in one segment (10 key tiles)
or the segments 100 + 333 + 64 + 200 (13 key tiles, every kind of segment end: ragged, full, single-tile).

Windows, as the header documents them. A speculative (anchored) pass over one key range anchors every row at a = the maximum over the
range's FIRST key tile (+ 4 in f16) and is accepted when the row sum l = sum 2^(s - a) has an f32 exponent within +-100 and O is finite;
f16 P overflows at 2^16. With L = log2 l from the float64 logits a row is OUTSIDE when L > 101 or L < -100 or (f16) some s - a >= 16, INSIDE
when |L| <= 96 and (f16) every s - a <= 12, and in the GUARD ZONE otherwise; the seeds are chosen so that no row of a counted scenario is in
the guard zone (test_attn_spread_host.py checks it for every counted launch), which makes the expected fallback count exact.
"""
import collections
import math

import torch

import kernel_guards as kg

BH, NK, SEGS, TILE = 16, 640, (100, 333, 64, 200), 64
STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": None}
BG = {"narrow": 0.3, "wide": 1.2}
Q_GAIN = 4.0
ANCHOR_MARGIN = {"bf16": 0.0, "f16": 4.0}                  # csrc/ovg_attn16.h AnchorMargin
RESCALE_THR = 8.0                                          # csrc/ovg_attn16.h RESCALE_THR
WAVE_ROWS = {128: 32, 256: 64, 512: 64}                    # q rows per wave of the 128- / 256- / 512-row kernels (csrc/ovg_attn.hip kKernels16)

Scenario = collections.namedtuple("Scenario", "name kind arg segs rows")


def _scenarios():
    s = [Scenario("none", "none", None, False, "all"), Scenario("sink_first_60", "sink", (5, 60.0), False, "all")]
    s += [Scenario("sink_late_%d" % b, "sink", (400, float(b)), False, "all") for b in (8, 40, 60, 130)]
    s += [Scenario("twins_%d" % g, "twins", float(g), False, "all") for g in (12, 40, 130)]
    s += [Scenario("ramp_up_200", "ramp", 200.0, False, "all"), Scenario("ramp_down_200", "ramp", -200.0, False, "all")]
    s += [Scenario("stairs_%s_%d" % ("up" if b > 0 else "down", abs(b)), "stairs", float(b), True, "all") for b in (30, -30, 70, -70)]
    s += [Scenario("rowmixed_one_130", "sink", (400, 130.0), False, "one"), Scenario("rowmixed_waves_130", "sink", (400, 130.0), False, "waves")]
    return collections.OrderedDict((x.name, x) for x in s)


SCENARIOS = _scenarios()
TWIN_KEYS = (150, 470)


def key_gains(scn, nks):
    """k[..., 0] of every key (flattened over the segments) = boost / 4, as bf16 numbers."""
    nk = sum(nks)
    g = torch.zeros(nk)
    if scn.kind == "sink":
        g[scn.arg[0]] = scn.arg[1] / Q_GAIN
    elif scn.kind == "twins":
        g[TWIN_KEYS[0]], g[TWIN_KEYS[1]] = scn.arg / Q_GAIN, (scn.arg + 1.0) / Q_GAIN
    elif scn.kind == "ramp":
        g = (scn.arg / Q_GAIN) * torch.arange(nk, dtype=torch.float32) / (nk - 1)
    elif scn.kind == "stairs":
        g = torch.cat([torch.full((n,), i * scn.arg / Q_GAIN) for i, n in enumerate(nks)])
    return g.to(torch.bfloat16).float()


def gain_rows(scn, nq, q_tile):
    """The q rows that carry q[..., 0] = 4: all, one row of the middle workgroup, or one row of every wave of the middle workgroup."""
    if scn.rows == "all":
        return torch.arange(nq)
    assert q_tile is not None and nq > 2 * q_tile, "rowmixed wants three workgroups"
    if scn.rows == "one":
        return torch.tensor([q_tile + 37 % q_tile])
    wr = WAVE_ROWS.get(q_tile, max(q_tile // 4, 1))
    return torch.tensor([q_tile + w * wr + 5 % wr for w in range(q_tile // wr)])


def stored(t32, mode):
    """f32 values -> float64 value of what the device holds in `mode` (f32x: hi + lo of the library's split rule)."""
    if mode == "f32x":
        hi = t32.clamp(-65504.0, 65504.0).to(torch.float16)
        return hi.double() + (t32 - hi.float()).clamp(-65504.0, 65504.0).to(torch.float16).double()
    return t32.to(STORE[mode]).double()


Case = collections.namedtuple("Case", "name mode bg nq nks q32 k32 v32 q k v gains rows")


def seed_of(scn_name, bg):
    return 7100 + 2 * list(SCENARIOS).index(scn_name) + (bg == "wide")


def build(scn_name, mode, nq, bg, q_tile=None, kv_heads=0, nks=None):
    """-> Case. q32 / k32 / v32: the f32 values before the storage rounding ([BH, nq, 64], [BHkv, nk, 64]); q / k / v: float64 of the stored
    values. The background does not depend on mode, nq's prefix or q_tile: rows 0..n-1 of a longer case are the shorter case's rows."""
    scn = SCENARIOS[scn_name]
    g = torch.Generator().manual_seed(seed_of(scn_name, bg))
    nks = list(nks) if nks is not None else (list(SEGS) if scn.segs else [NK])      # nks: the same gain pattern on a longer key set
    nk, BHkv = sum(nks), (kv_heads if kv_heads else BH)
    k32, v32 = torch.randn(BHkv, nk, 64, generator=g), torch.randn(BHkv, nk, 64, generator=g)
    q32 = torch.randn(BH, 1041, 64, generator=g)[:, :nq] * BG[bg] if nq <= 1041 else torch.randn(BH, nq, 64, generator=g) * BG[bg]
    gains, rows = key_gains(scn, nks), gain_rows(scn, nq, q_tile)
    q32[..., 0] = 0.0
    k32[..., 0] = 0.0
    if scn.kind != "none":
        q32[:, rows, 0] = Q_GAIN
        k32[..., 0] = gains
    return Case(scn_name, mode, bg, nq, nks, q32, k32, v32, stored(q32, mode), stored(k32, mode), stored(v32, mode), gains, rows)


def expand_heads(t, BHq=BH):
    return t[torch.arange(BHq) % t.shape[0]]


def logits(case):
    return case.q @ expand_heads(case.k).transpose(-1, -2)


# ---------------------------------------------------------------------------------------------
# key ranges, workgroups, windows
# ---------------------------------------------------------------------------------------------
def key_tiles(nks):
    """(first key, end key) of every 64-key tile, flattened over the segments (a segment's last tile is ragged)."""
    out, base = [], 0
    for n in nks:
        out += [(base + t, base + min(t + TILE, n)) for t in range(0, n, TILE)]
        base += n
    return out


def key_ranges(nks, splits):
    """csrc/ovg_attn.hip key_ranges restated: per = ceil(T / splits) tiles per range, ceil(T / per) ranges -> [(first key, end key of the
    range's first tile, end key of the range)]. `splits` is the plan's answer (already clamped to the tiles)."""
    tiles = key_tiles(nks)
    T = len(tiles)
    splits = max(1, min(splits, T))
    per = (T + splits - 1) // splits
    return [(tiles[t][0], tiles[t][1], tiles[min(t + per, T) - 1][1]) for t in range(0, T, per)]


def launches(plan, nq):
    """A plan (ops.attn_plan) -> [(key ranges, q tile, first row, end row)] of its kernel launches."""
    if plan["tail_q_tile"] == 0:
        return [(plan["splits"], plan["q_tile"], 0, nq)]
    key_tail = plan["tail_q_tile"] == plan["q_tile"] and plan["splits"] > 1
    return [(1, plan["q_tile"], 0, plan["main_rows"]), (plan["splits"] if key_tail else 1, plan["tail_q_tile"], plan["main_rows"], nq)]


def classify(s, nks, splits, mode):
    """s [BH, nq, nk] float64 log2 logits -> (outside, inside), bool [ranges, BH, nq], by the documented windows."""
    out, ins = [], []
    f16 = mode == "f16"
    for k0, k1, kend in key_ranges(nks, splits):
        a = s[..., k0:k1].amax(-1, keepdim=True) + ANCHOR_MARGIN[mode]
        d = s[..., k0:kend] - a
        Lg = torch.logsumexp(d * math.log(2.0), -1) / math.log(2.0)
        top = d.amax(-1)
        out.append((Lg > 101.0) | (Lg < -100.0) | ((top >= 16.0) if f16 else torch.zeros_like(top, dtype=torch.bool)))
        ins.append((Lg.abs() <= 96.0) & ((top <= 12.0) if f16 else torch.ones_like(top, dtype=torch.bool)))
    return torch.stack(out), torch.stack(ins)


def expected_fallbacks(s, nks, plan, mode):
    """-> (units that hold at least one outside row, all units, rows in the guard zone) over every (entry, key range, workgroup) of the plan's
    launches. A workgroup's rows beyond nq repeat row nq - 1 (the kernels clamp the row index), so they add nothing."""
    nq = s.shape[1]
    bad = total = guard = 0
    for ranges, q_tile, r0, r1 in launches(plan, nq):
        outside, inside = classify(s[:, r0:r1], nks, ranges, mode)
        guard += int((~outside & ~inside).sum())
        for t in range(0, r1 - r0, q_tile):
            hit = outside[:, :, t:t + q_tile].any(-1)
            bad += int(hit.sum())
            total += hit.numel()
    return bad, total, guard


SPEC128, SPEC256, SPEC512, FORCED256, AUTO = 54, 50, 57, 53, 0         # OVG_ATTN_* of include/omnivggt_hip.h


def counted_shape(mode, variant):
    """-> (nq, q_tile) of a kernel under test: 2 q_tile + 17 rows, three workgroups and a ragged last one (q tiles below 128 rows -- the
    baseline kernel's 64 -- run the 128-row shape)."""
    from omnivggt_official_amd import lib as L, ops
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}[mode]
    qt = max(ops.attn_plan(BH, 273, [NK], dt, variant, 1)["q_tile"], 128)
    return 2 * qt + 17, qt


def counter_cases(mode):
    """(variant, kv_splits, scenario) of the fallback-counter test (narrow background): the speculative kernels unsplit (kv_splits 1 = never)
    and in 3 forced key ranges."""
    if mode == "bf16":
        scns = ("none", "sink_late_60", "sink_late_130", "rowmixed_one_130", "rowmixed_waves_130")
        out = [(v, s, n) for v in (SPEC128, SPEC256, SPEC512, AUTO) for s in (1, 3) for n in scns]
        return out + [(v, 1, "stairs_up_70") for v in (SPEC128, SPEC256, SPEC512, AUTO)]
    scns = ("sink_late_8", "sink_late_60", "rowmixed_one_130", "rowmixed_waves_130")
    return [(v, s, n) for v in (SPEC128, SPEC256, SPEC512) for s in (1, 3) for n in scns]


# f32 / f32x only: scenarios gated per element alone, because the tensor-global gate (2e-5 / 1e-5 of max |ref|) cannot be held by ANY kernel
# that accumulates the logits in f32. Their gain logits reach 130 ... 210 (f32 ulp 2^-16 = 1.5e-5 log2 units) AND several keys share the
# weight, so a logit error moves the output; test_attn_spread_host.py shows it with the float64 softmax of once-rounded logits times the
# number of f32 partial sums of that size the accumulation passes through (S_CHAIN). One sink at +130 is not listed: its output is the
# sink's v whatever its weight was.
PER_ELEMENT_ONLY = ("twins_130", "ramp_up_200", "stairs_up_70")
S_CHAIN = {"f32": 16, "f32x": 6}         # 64 products: 16 steps of the 16x16x4 f32 MFMA; 3 planes x 2 steps of the 16x16x32 f16 MFMA


# ---------------------------------------------------------------------------------------------
# budgets (kernel_guards, unchanged) and the comparison both test files use
# ---------------------------------------------------------------------------------------------
Budget = collections.namedtuple("Budget", "ref mag c lse floor")


def budget(case):
    idx = torch.arange(BH) % case.k.shape[0]
    ref, mag, c, lse = kg.attn_budget(case.q, case.k[idx], case.v[idx], case.mode)
    return Budget(ref, mag, c, lse, kg.attn_p_floor(case.v[idx], case.mode) + kg.f16_subnormal_floor(case.mode))


def rows_of(b, nq):
    return Budget(b.ref[:, :nq], b.mag[:, :nq], b.c[:, :nq], b.lse[:, :nq], b.floor)


def check(name, out, lse, b, mode, splits=1):
    """The per-element budget on the outputs and test_gpu_edges' budget on lse (c u_acc / ln 2 + u_f32 |lse|); a split launch adds
    MARGIN (splits + 2) to c. -> (worst used fraction of the outputs, of lse)."""
    c = b.c + (kg.MARGIN * (splits + 2) if splits > 1 else 0.0)
    f_out = kg.elementwise_budget(name, out, b.ref, b.mag, kg.U_OUT[mode], c, extra=b.floor, quiet=True)
    lse = lse.detach().to("cpu", torch.float64)
    lb = (c.squeeze(-1) * kg.U_ACC) / math.log(2.0) + kg.U_OUT["f32"] * b.lse.abs()
    err = (lse - b.lse).abs()
    err[~torch.isfinite(lse)] = float("inf")
    f_lse = float((err / lb).max())
    assert f_lse <= 1.0, "%s lse: %d rows over their budget, worst %.3g x (err %.3e)" % (name, int((err > lb).sum()), f_lse, float(err.max()))
    kg.STATS["numeric"] += 1
    return f_out, f_lse


def global_err(got, ref):
    got = got.detach().to("cpu", torch.float64)
    err = (got - ref).abs()
    err[~torch.isfinite(got)] = float("inf")
    return float(err.max() / ref.abs().max().clamp_min(1e-30))


def s_rounding_global_error(case):
    """max |err| / max |ref| of the float64 softmax whose logits were rounded ONCE to f32: what any kernel with f32 accumulators pays
    at least (its last partial sum is an f32), before its own order of summation adds to it."""
    s = logits(case)
    v = expand_heads(case.v)
    ref = torch.softmax(s * math.log(2.0), -1) @ v
    got = torch.softmax(s.float().double() * math.log(2.0), -1) @ v
    return global_err(got, ref)


# ---------------------------------------------------------------------------------------------
# the twin of the documented 16-bit arithmetic
# ---------------------------------------------------------------------------------------------
FAULTS = ("l_not_rescaled", "f16_p_clamped", "merge_against_range0")


def _round_p(p, mode, fault):
    if mode == "bf16":
        return p.to(torch.bfloat16).float()
    if fault == "f16_p_clamped":
        p = p.clamp(max=65504.0)
    return p.to(torch.float16).float()                      # overflows to inf from 65520 on, like the hardware convert


def _pass(q, k, v, tiles, mode, body, fault):
    """One pass over the key tiles [(k0, k1)] for all rows: f32 o [BH, nq, 64], l, negm [BH, nq]."""
    nq = q.shape[1]
    o = torch.zeros(q.shape[0], nq, 64)
    l = torch.zeros(q.shape[0], nq)
    negm = torch.zeros(q.shape[0], nq)
    groups = (nq + 15) // 16
    for j, (k0, k1) in enumerate(tiles):
        raw = q @ k[:, k0:k1].transpose(-1, -2)
        if body == "anchored":
            if j == 0:
                negm = -(raw.amax(-1) + ANCHOR_MARGIN[mode])
            s = raw + negm[..., None]
        else:
            s = raw + negm[..., None]
            mx = s.amax(-1)
            if j == 0:
                s = s - mx[..., None]
                negm = -mx
            else:
                over = torch.zeros(q.shape[0], groups * 16, dtype=torch.bool)
                over[:, :nq] = mx > RESCALE_THR
                fire = over.view(-1, groups, 16).any(-1, keepdim=True).expand(-1, -1, 16).reshape(-1, groups * 16)[:, :nq]
                delta = torch.where(fire, mx.clamp(min=0.0), torch.zeros_like(mx))
                alpha = torch.exp2(-delta)
                negm = negm - delta
                if fault != "l_not_rescaled":
                    l = l * alpha
                s = s - delta[..., None]
                o = o * alpha[..., None]
        p = _round_p(torch.exp2(s), mode, fault)
        l = l + p.sum(-1)
        o = o + p @ v[:, k0:k1]
    return o, l, negm


def twin(case, body, splits=1, fault=None, wg_rows=128):
    """The documented arithmetic of the 16-bit kernels in f32 torch: 64-key tiles, P rounded to the operand type, f32 o and l, the lazy
    rescale beyond 8 log2 units per 16-row group, or the anchored pass with its verification (l within 2^+-100, O finite, per workgroup of
    wg_rows rows) and the lazy re-run, f32 partials merged by 2^(lse_s - max). -> (out float64 of the stored type [BH, nq, 64], lse float64
    [BH, nq], re-run units). fault: one of FAULTS planted."""
    mode = case.mode
    assert mode in ("bf16", "f16") and body in ("lazy", "anchored")
    q, k, v = case.q.float(), expand_heads(case.k).float(), expand_heads(case.v).float()
    tiles = key_tiles(case.nks)
    parts, reran = [], 0
    for k0, _, kend in key_ranges(case.nks, splits):
        mine = [t for t in tiles if k0 <= t[0] < kend]
        o, l, negm = _pass(q, k, v, mine, mode, body, fault)
        if body == "anchored":
            e = (l.view(torch.int32) >> 23) & 0xff
            bad = (e > 227) | (e < 27) | ~torch.isfinite(o).all(-1)
            nwg = (case.nq + wg_rows - 1) // wg_rows
            pad = torch.zeros(bad.shape[0], nwg * wg_rows, dtype=torch.bool)
            pad[:, :case.nq] = bad
            wg_bad = pad.view(-1, nwg, wg_rows).any(-1)
            reran += int(wg_bad.sum())
            if bool(wg_bad.any()):
                o2, l2, n2 = _pass(q, k, v, mine, mode, "lazy", fault)
                sel = wg_bad[:, :, None].expand(-1, -1, wg_rows).reshape(-1, nwg * wg_rows)[:, :case.nq]
                o, l, negm = torch.where(sel[..., None], o2, o), torch.where(sel, l2, l), torch.where(sel, n2, negm)
        parts.append((o * (1.0 / l)[..., None], torch.log2(l) - negm))
    if len(parts) == 1:
        out, lse = parts[0]
    else:
        ls = torch.stack([p[1] for p in parts])
        m = ls[0] if fault == "merge_against_range0" else ls.amax(0)
        w = torch.exp2(ls - m)
        wsum = w.sum(0)
        out = sum(w[i][..., None] * parts[i][0] for i in range(len(parts))) * (1.0 / wsum)[..., None]
        lse = m + torch.log2(wsum)
    return out.to(STORE[mode]).double(), lse.double(), reran
