"""-m gpu: the block and head kernels at their tile edges, every output inside guard bands (tests/kernel_guards.py), every padding region
poisoned with large finite values, every result gated twice -- the tensor-global gate of gpu_selftest.TOL and the per-element error budget of
kernel_guards.elementwise_budget -- against float64 CPU references of the dtype-rounded inputs, and every poisoned run compared bit for bit
with the zero-padded run of the same call. A shape the ABI refuses (OVG_E_ARG / OVG_E_UNSUPPORTED) is asserted as a refusal and counted;
no listed shape is skipped. Every test prints the running totals (guarded launches / numeric checks / refusals).

The budgets' constants are derived in kernel_guards.py. bf16 is gated with u_out = 2^-8 (its unit roundoff: 8 significand bits; 2^-9 is not
attainable by a correctly rounded store, test_kernel_guards_host.py pins that)."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_selftest as st
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}
STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": torch.float16}
GATE = dict(st.TOL, f32x=1e-5)           # the existing global gates (f32x: test_f32x's TOLX)
F32_GATE = {"bf16": 2e-5, "f16": 2e-5, "f32": 2e-6, "f32x": 1e-5}      # f32 outputs (out_f32 / RES / PATCH), as gpu_selftest.test_linear gates them


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    st.results.clear()
    yield
    kg.STATS.setdefault("global_only", 0)
    print("guards: %(guarded_launches)d guarded launches, %(numeric)d numeric checks (+ %(global_only)d with the global gate alone), "
          "%(refusals)d refusals" % kg.STATS, flush=True)


def _global(name, got, ref, tol):
    """The existing tensor-global gate, asserted."""
    assert st.report(name, got.detach().double().cpu(), ref, tol), name


def _refused(fn, what):
    with pytest.raises(L.OvgError, match="ARG|UNSUPPORTED"):
        fn()
    kg.STATS["refusals"] += 1
    print("[REFUSED] %s" % what, flush=True)


def _note_refusal(exc, what):
    """A refusal that was caught where it is a valid outcome: counted from the exception, the call is not made again."""
    assert "ARG" in str(exc) or "UNSUPPORTED" in str(exc), (what, exc)
    kg.STATS["refusals"] += 1
    print("[REFUSED] %s (%s)" % (what, exc), flush=True)


def _global_only(n=1):
    kg.STATS["global_only"] = kg.STATS.get("global_only", 0) + n


def _sync_check(*checks):
    torch.cuda.synchronize()
    for i, c in enumerate(checks):
        c("guard %d" % i)


class Slot:
    """One guarded output buffer, re-armed between launches (same shape / dtype / ld)."""
    cache = {}

    def __init__(self, shape, dtype, ld=None, spare_rows=1):
        self.view, self.check = kg.guarded(shape, dtype, DEV, ld=ld, spare_rows=spare_rows)

    @classmethod
    def get(cls, shape, dtype, ld=None, spare_rows=1, tag=""):
        key = (tuple(shape), dtype, ld, spare_rows, tag)
        if key not in cls.cache:
            if len(cls.cache) > 64:
                cls.cache.clear()
            cls.cache[key] = cls(shape, dtype, ld, spare_rows)
        s = cls.cache[key]
        s.check.buffer.fill_(kg.GUARD_BYTE)
        return s


def _strided_input(vals, poison, pad=8):
    """vals [rows, cols] (CPU, storage dtype) -> a device view of the same values whose neighbouring columns and two trailing rows hold the
    poison pattern (or zeros)."""
    rows, cols = vals.shape
    big = kg.poison_values((rows + 2, cols + 2 * pad), vals.dtype, "cpu") if poison else torch.zeros(rows + 2, cols + 2 * pad, dtype=vals.dtype)
    big[:rows, pad:pad + cols] = vals
    return big.to(DEV)[:rows, pad:pad + cols]


def _operand(vals32, mode, poison):
    """f32 CPU values -> (device operand for `mode` as a strided view, float64 value of what the device holds)."""
    if mode == "f32x":
        h = ops.to_hilo(vals32)
        return ops.HiLo((_strided_input(h.hi, poison), _strided_input(h.lo, poison))), h.hi.double() + h.lo.double()
    r = vals32.to(MODES[mode])
    return _strided_input(r, poison), r.double()


def _val(t):
    return (t.hi.double() + t.lo.double()).cpu() if isinstance(t, ops.HiLo) else t.double().cpu()


def _out_slot(mode, shape, f32, ld, tag=""):
    """-> (tensor to pass as out=, [checks]) for a 16-bit / f32 / split output."""
    if f32 or mode == "f32":
        s = Slot.get(shape, torch.float32, ld, tag=tag)
        return s.view, [s.check]
    if mode == "f32x":
        a, b = Slot.get(shape, torch.float16, ld, tag=tag + "hi"), Slot.get(shape, torch.float16, ld, tag=tag + "lo")
        return ops.HiLo((a.view, b.view)), [a.check, b.check]
    s = Slot.get(shape, MODES[mode], ld, tag=tag)
    return s.view, [s.check]


# =============================================================================================
# ovg_linear
# =============================================================================================
LIN_M = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 511, 513)
LIN_N = (128, 256, 384)
LIN_K = (64, 128, 192, 320)


def _linear_all_epilogues(mode, M, N, K, tile, g, tag):
    dt = MODES[mode]
    x32, w32 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g) * 0.3
    bias[:16] *= 0.01                                   # a quiet column group: a dropped bias there hides under the global gate
    res, gamma = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    xd, xv = _operand(x32, mode, True)
    xz, _ = _operand(x32, mode, False)
    wd, wv = _operand(w32, mode, True)
    bd, gd = bias.to(DEV), gamma.to(DEV)
    z = xv @ wv.t() + bias.double()
    mg = kg.gemm_mag(xv, wv, bias)
    u, ld = kg.U_OUT[mode], N + 8
    floor = kg.f16_subnormal_floor(mode)
    legal256 = mode != "f32" and N % 256 == 0
    if tile == L.TILE_256 and not legal256:
        _refused(lambda: ops.linear(xd, wd, bd, dt, tile=tile), "linear %s tile 256" % tag)
        return

    def run(name, ref, mag, c, f32, u_out, gate, prefill=None, check_rows=None, **kw):
        out, checks = _out_slot(mode, ref.shape, f32, ld, tag=name.split("_")[0])
        if prefill is not None:
            out.copy_(prefill.to(DEV))
        ops.linear(xd, wd, bd, dt, out=out, tile=tile, **kw)
        _sync_check(*checks)
        got = _val(out)
        _global("%s_%s" % (name, tag), got, ref, gate)
        kg.elementwise_budget("%s_%s" % (name, tag), got, ref, mag, u_out, c, extra=None if f32 else floor, quiet=True)
        return got

    got = run("store", z, mg, kg.gemm_c(K, mode), False, u, GATE[mode])
    # the same call with zeros instead of poison around x: bit-identical
    out, checks = _out_slot(mode, z.shape, False, ld, tag="zero")
    ops.linear(xz, wd, bd, dt, out=out, tile=tile)
    _sync_check(*checks)
    assert torch.equal(_val(out), got), "linear %s: the result depends on what lies next to x" % tag
    run("storef32", z, mg, kg.gemm_c(K, mode), True, kg.U_OUT["f32"], F32_GATE[mode], out_f32=True)
    run("gelu", F.gelu(z), mg, kg.gelu_c(K, mode), False, u, GATE[mode], epilogue=L.EPI_GELU)
    rd = _strided_input(res, True)
    rref, rmag, rc = res.double() + gamma.double() * z, kg.res_mag(res, gamma, mg), kg.res_c(K, mode)
    got = run("res", rref, rmag, rc, True, kg.U_OUT["f32"], F32_GATE[mode], epilogue=L.EPI_RES, res=rd, gamma=gd)
    # zeros instead of poison beside x, w and res: bit-identical
    wz, _ = _operand(w32, mode, False)
    out, checks = _out_slot(mode, rref.shape, True, ld, tag="zero32")
    ops.linear(xz, wz, bd, dt, out=out, tile=tile, epilogue=L.EPI_RES, res=_strided_input(res, False), gamma=gd)
    _sync_check(*checks)
    assert torch.equal(_val(out), got), "linear RES %s: the result depends on what lies next to x / w / res" % tag
    for per in sorted({1, 7, M, M + 1}):
        inj = torch.randn((M + per - 1) // per, N, generator=g)
        full = torch.zeros(M, N)
        full[::per] = inj[: full[::per].shape[0]]
        run("resinj%d" % per, rref + full.double(), rmag + full.abs().double(), rc + kg.MARGIN, True, kg.U_OUT["f32"], F32_GATE[mode],
            epilogue=L.EPI_RES, res=rd, gamma=gd, inject=inj.to(DEV), inj_period=per)
    # in place: out is res (the guarded buffer holds the residual stream)
    out, checks = _out_slot(mode, rref.shape, True, ld, tag="inplace")
    out.copy_(res.to(DEV))
    ops.linear(xd, wd, bd, dt, out=out, tile=tile, epilogue=L.EPI_RES, res=out, gamma=gd)
    _sync_check(*checks)
    _global("resinplace_" + tag, _val(out), rref, F32_GATE[mode])
    kg.elementwise_budget("resinplace_" + tag, _val(out), rref, rmag, kg.U_OUT["f32"], rc, quiet=True)
    # PATCH: rows (m / p0) * p1 + 5 + m % p0 of an out_rows-row buffer; the special rows and the tail keep their contents
    for p0 in (1, 100):
        p1, views = p0 + 5, (M + p0 - 1) // p0
        out_rows = views * p1 + 3
        table = torch.randn(p0 + 1, N, generator=g)
        m = torch.arange(M)
        dst = (m // p0) * p1 + 5 + m % p0
        keep = torch.full((out_rows, N), 7.25, dtype=torch.float64)
        pref, pmag = keep.clone(), torch.zeros(out_rows, N, dtype=torch.float64)
        pref[dst] = z + table[1:][m % p0].double()
        pmag[dst] = mg + table[1:][m % p0].abs().double()
        got = run("patch%d" % p0, pref, pmag, kg.gemm_c(K, mode) + kg.MARGIN, True, kg.U_OUT["f32"], F32_GATE[mode], prefill=keep.float(),
                  epilogue=L.EPI_PATCH, table=table.to(DEV), p0=p0, p1=p1, row_off=5)
        untouched = torch.ones(out_rows, dtype=torch.bool)
        untouched[dst] = False
        assert bool((got[untouched] == 7.25).all()), "linear PATCH %s p0=%d wrote a row it does not own" % (tag, p0)
        out, checks = _out_slot(mode, pref.shape, True, ld, tag="zero32p")
        out.copy_(keep.float().to(DEV))
        ops.linear(xz, wz, bd, dt, out=out, tile=tile, epilogue=L.EPI_PATCH, table=table.to(DEV), p0=p0, p1=p1, row_off=5)
        _sync_check(*checks)
        assert torch.equal(_val(out), got), "linear PATCH %s p0=%d: the result depends on what lies next to x / w" % (tag, p0)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f32x"])
def test_linear_every_epilogue_at_the_tile_edges(mode):
    g = torch.Generator().manual_seed(101)
    for tile, tname in ((L.TILE_AUTO, "auto"), (L.TILE_128, "t128"), (L.TILE_256, "t256")):
        for N in LIN_N:
            for K in LIN_K:
                for M in LIN_M:
                    _linear_all_epilogues(mode, M, N, K, tile, g, "%s_%s_%dx%dx%d" % (mode, tname, M, N, K))


def _expected_auto_tile(M, N, K, epi):
    """The documented choice of OVG_TILE_AUTO for 16-bit dtypes, N % 256 == 0 (csrc/ovg_gemm.hip choose_256), restated: from M = 20000 the
    256 tile unless the epilogue is RES with K < 2048; below, only fc2 (RES, K >= 2048) from M = 8000 when its 256 tiles fit one round of
    the CUs, and proj (RES, K < 2048) when one round of 256 tiles replaces more than three rounds of 128 tiles."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if M >= 20000:
        return L.TILE_256 if (epi != L.EPI_RES or K >= 2048) else L.TILE_128
    t256, t128 = ((M + 255) // 256) * (N // 256), ((M + 127) // 128) * (N // 128)
    if epi == L.EPI_RES and K >= 2048 and M >= 8000 and t256 <= cus:
        return L.TILE_256
    if epi == L.EPI_RES and K < 2048 and t256 <= cus and t128 > 3 * cus:
        return L.TILE_256
    return L.TILE_128


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_linear_at_the_automatic_tile_switch_points(mode):
    """AUTO is bit-identical to the forced tile that the documented heuristic picks on each side of M = 8000 / 20000, and the two forced
    tiles agree within the dtype gate and each meet the per-element budget on sampled rows. RES at N = K = 1024 (proj) never switches at
    these M (heavy epilogue, short K: 128 throughout) and GELU at N = 4096 (fc1) switches at 20000 only; the M = 8000 switch exists for
    fc2 alone (RES, K >= 2048, one round of 256 tiles), so a RES 1024 x 2048 case carries it. Where the two forced tiles differ in some
    bit, AUTO must also differ from the tile it should not have picked; where they are bit-equal (both kernels add the k steps of an
    element in the same order) the choice cannot be seen in the numbers and only the equality is asserted -- printed as such."""
    g = torch.Generator().manual_seed(103)
    dt = MODES[mode]
    for (N, K, epi) in ((1024, 1024, L.EPI_RES), (4096, 1024, L.EPI_GELU), (1024, 2048, L.EPI_RES)):
        w = (torch.randn(N, K, generator=g) * 0.05).to(dt).to(DEV)
        bias, gamma = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
        for M in (7999, 8000, 19999, 20000):
            x = torch.randn(M, K, generator=g).to(dt).to(DEV)
            res = torch.randn(M, N, generator=g).to(DEV)
            outs = {}
            for tile in (L.TILE_AUTO, L.TILE_128, L.TILE_256):
                s = Slot.get((M, N), torch.float32 if epi == L.EPI_RES else dt, N + 8, tag="sw%d" % tile)
                kw = dict(res=res, gamma=gamma) if epi == L.EPI_RES else {}
                ops.linear(x, w, bias, dt, epilogue=epi, out=s.view, tile=tile, **kw)
                _sync_check(s.check)
                outs[tile] = s.view.clone()
            want = _expected_auto_tile(M, N, K, epi)
            other = L.TILE_128 if want == L.TILE_256 else L.TILE_256
            tag = "%s epi=%d M=%d N=%d K=%d" % (mode, epi, M, N, K)
            assert torch.equal(outs[L.TILE_AUTO], outs[want]), "linear %s: AUTO is not bit-identical to tile %d" % (tag, want)
            visible = not torch.equal(outs[L.TILE_128], outs[L.TILE_256])
            if visible:
                assert not torch.equal(outs[L.TILE_AUTO], outs[other]), "linear %s: AUTO ran tile %d, expected %d" % (tag, other, want)
            print("linear %s: AUTO == tile %d (expected); forced tiles %s" % (tag, want, "differ" if visible else "are bit-equal: choice not visible"), flush=True)
            # (one kernel against the other: there is no reference to budget against here; both are budgeted against float64 below)
            _global("switch_%s_%d_%dx%dx%d_256_vs_128" % (mode, epi, M, N, K), outs[L.TILE_256], outs[L.TILE_128].double().cpu(),
                    F32_GATE[mode] if epi == L.EPI_RES else GATE[mode])
            _global_only()
            rows = torch.tensor(sorted({0, 1, 127, 128, 255, 256, M - 257, M - 129, M - 2, M - 1}), device=DEV)
            z = x[rows].double().cpu() @ w.double().cpu().t() + bias.double().cpu()
            mg = kg.gemm_mag(x[rows].cpu(), w.cpu(), bias.cpu())
            for tile in (L.TILE_128, L.TILE_256):
                got = outs[tile][rows]
                if epi == L.EPI_RES:
                    kg.elementwise_budget("switch_res_%s_%d_t%d" % (mode, M, tile), got, res[rows].double().cpu() + gamma.double().cpu() * z,
                                          kg.res_mag(res[rows].cpu(), gamma.cpu(), mg), kg.U_OUT["f32"], kg.res_c(K, mode), quiet=True)
                else:
                    kg.elementwise_budget("switch_gelu_%s_%d_t%d" % (mode, M, tile), got, F.gelu(z), mg, kg.U_OUT[mode], kg.gelu_c(K, mode), quiet=True)
    Slot.cache.clear()
    torch.cuda.empty_cache()


# =============================================================================================
# LayerNorm family, copy_rows, pack_weights, im2col
# =============================================================================================
LN_ROWS = (1, 3, 4, 5, 257)


def _ln_rows(family, rows, n, g):
    noise = torch.randn(rows, n, generator=g)
    if family == "const":            # short significands: every partial sum of a row is exact, so mean == x and the output is exactly the bias
        return (torch.tensor([3.5, -2.0, 1000.0, 0.0, 0.015625])[torch.arange(rows) % 5]).view(rows, 1).expand(rows, n).contiguous()
    if family == "const_full":       # a full 24-bit significand: zero variance up to the mean's rounding (budget only)
        return (torch.tensor([math.pi, -1e-3 / 3, 12345.678])[torch.arange(rows) % 3]).view(rows, 1).expand(rows, n).contiguous()
    if family == "offset":
        return 1000.0 + 0.01 * noise
    if family == "massive":
        noise[:, 17] = 500.0
        return noise
    if family == "tiny":
        return 1e-20 * noise
    return noise * 2.0 + 0.3


LN_FAMILIES = ("const", "const_full", "offset", "massive", "tiny", "noise")


def _ln_check(name, got, x, w, b, eps, mode, f32, family, add=None):
    ref, mag, c, extra = kg.layernorm_budget(x, w, b, eps)
    if add is not None:
        ref, mag, c = ref + add.double(), mag + add.abs().double(), c + kg.MARGIN
    u = kg.U_OUT["f32"] if f32 else kg.U_OUT[mode]
    assert bool(torch.isfinite(got).all()), name
    # the existing gate of the dtype + the mean's own rounding (kernel_guards.layernorm_budget's `extra`: inherent to any f32 two-pass kernel,
    # it only shows on rows whose mean dwarfs their spread) relative to the tensor maximum
    base = 2e-6 if (f32 or mode in ("f32", "f32x")) else GATE[mode]
    _global(name, got, ref, base + float(extra.max() / ref.abs().max().clamp_min(1e-30)))
    kg.elementwise_budget(name, got, ref, mag, u, c, extra=extra + (0.0 if f32 else kg.f16_subnormal_floor(mode)), quiet=True)
    if family == "const" and add is None:
        exp = b.double() if (f32 or mode == "f32") else (b.to(STORE[mode]).double() if mode != "f32x" else _val(ops.to_hilo(b)))
        assert torch.equal(got, exp.expand_as(got)), "%s: a zero-variance row must come out as exactly the bias" % name


def test_layernorm_row_families_and_row_counts():
    """ovg_layernorm (1024), every dtype + out_f32; rows 1..257; strided poisoned input, guarded strided output. On the `offset` family
    (x = 1000 + 0.01 noise) the mean of 1024 values near 1000 carries a few ulp(1000) = 6e-5 each against a spread of 0.01 in ANY f32
    two-pass kernel: kernel_guards.layernorm_budget's `extra` term bounds that per element, and the global gate is widened by it."""
    g = torch.Generator().manual_seed(105)
    w, b = torch.randn(1024, generator=g) * 0.1 + 1, torch.randn(1024, generator=g) * 0.1
    wd, bd = w.to(DEV), b.to(DEV)
    for family in LN_FAMILIES:
        for rows in LN_ROWS:
            x = _ln_rows(family, rows, 1024, g)
            xd, xz = _strided_input(x, True), _strided_input(x, False)
            for mode, f32 in (("bf16", False), ("f16", False), ("f32", False), ("f32x", False), ("bf16", True)):
                out, checks = _out_slot(mode, (rows, 1024), f32, 1032, tag="ln")
                ops.layernorm(xd, wd, bd, 1e-5, MODES[mode], out=out, out_f32=f32)
                _sync_check(*checks)
                got = _val(out)
                _ln_check("layernorm_%s%s_%s_r%d" % (mode, "_f32out" if f32 else "", family, rows), got, x, w, b, 1e-5, mode, f32, family)
                ops.layernorm(xz, wd, bd, 1e-5, MODES[mode], out=out, out_f32=f32)
                torch.cuda.synchronize()
                assert torch.equal(_val(out), got)


def test_head_layernorm_and_assemble_tokens_layernorm():
    g = torch.Generator().manual_seed(107)
    w, b = torch.randn(2048, generator=g) * 0.2 + 1, torch.randn(2048, generator=g) * 0.1
    for family in LN_FAMILIES:
        for rows in LN_ROWS:
            tpv = rows + 5
            x = _ln_rows(family, 2 * tpv, 2048, g)
            xd = _strided_input(x, True)
            keep = torch.cat([torch.arange(5, tpv), torch.arange(tpv + 5, 2 * tpv)])
            for mode in ("bf16", "f16", "f32"):
                s = Slot.get((2 * rows, 2048), MODES[mode], 2056, tag="hln")
                ops.head_layernorm(xd, w.to(DEV), b.to(DEV), 1e-5, MODES[mode], 2, tokens_per_view=tpv, out=s.view)
                _sync_check(s.check)
                _ln_check("head_layernorm_%s_%s_r%d" % (mode, family, rows), _val(s.view), x[keep], w, b, 1e-5, mode, False, family)
    # the LayerNorm inside ovg_assemble_tokens (f32 in, f32 out), view 0 + placeholder, view 1 + depth tokens
    w, b = torch.randn(1024, generator=g) * 0.1 + 1, torch.randn(1024, generator=g) * 0.1
    cam, regt, cam_add, ph = torch.randn(2, 1024, generator=g), torch.randn(2, 4, 1024, generator=g), torch.randn(2, 1024, generator=g), torch.randn(1024, generator=g)
    for family in LN_FAMILIES:
        for rows in LN_ROWS:
            P = rows + 5
            x = _ln_rows(family, 2 * P, 1024, g)
            dtok = torch.randn(rows, 1024, generator=g)
            s = Slot.get((2 * P, 1024), torch.float32, 1032, tag="asm")
            ops.assemble_tokens(_strided_input(x, True), w.to(DEV), b.to(DEV), 1e-6, cam.to(DEV), regt.to(DEV), cam_add.to(DEV), dtok.to(DEV),
                                torch.tensor([-1, 0], dtype=torch.int32, device=DEV), ph.to(DEV), s.view, 2, 2, tokens_per_view=P)
            _sync_check(s.check)
            got = _val(s.view).view(2, P, 1024)
            assert torch.equal(got[:, 0], (cam + cam_add).double()) and torch.equal(got[:, 1:5], regt.double())
            add = torch.cat([ph.expand(rows, 1024), dtok])
            patch = torch.cat([x[5:P], x[P + 5:]])
            _ln_check("assemble_ln_%s_r%d" % (family, rows), torch.cat([got[0, 5:], got[1, 5:]]), patch, w, b, 1e-6, "f32", True, family, add=add)


def test_copy_rows_is_bit_exact_and_stays_inside_its_rows():
    g = torch.Generator().manual_seed(109)
    for n in (4, 1020, 1024):
        for rows in (1, 1375):
            x = torch.randn(rows, n, generator=g)
            s = Slot.get((rows, n), torch.float32, n + 12, tag="copy")
            ops.copy_rows(_strided_input(x, True), s.view)
            _sync_check(s.check)
            assert torch.equal(s.view.cpu(), x), "copy_rows n=%d rows=%d" % (n, rows)
            kg.STATS["numeric"] += 1


def test_pack_weights_and_im2col_zero_their_poisoned_k_padding():
    g = torch.Generator().manual_seed(111)
    for mode in MODES:
        dt, sdt = MODES[mode], STORE[mode]
        for rows in (1, 1024):
            w = torch.randn(rows, 588, generator=g)
            planes = [Slot.get((rows, 640), sdt, 648, tag="pack%d" % i) for i in range(2 if mode == "f32x" else 1)]
            for s in planes:
                s.view.copy_(kg.poison_values((rows, 640), sdt, DEV))
                kg.poison_cols(s.view, 588)
            out = ops.HiLo((planes[0].view, planes[1].view)) if mode == "f32x" else planes[0].view
            ops.pack_weights(w.to(DEV), dt, k_pad=640, out=out)
            _sync_check(*[s.check for s in planes])
            exp = ops.to_hilo(w) if mode == "f32x" else w.to(sdt)
            for s, e in zip(planes, (exp.hi, exp.lo) if mode == "f32x" else (exp,)):
                assert torch.equal(s.view[:, :588].cpu(), e) and float(s.view[:, 588:].float().abs().max()) == 0.0, "pack_weights %s rows=%d" % (mode, rows)
            kg.STATS["numeric"] += 1
        # im2col: rgb (588 -> 640) and depth (392 -> 448); dense [patches, k_pad] output pre-filled with poison, one spare row behind it
        img = torch.rand(2, 3, 28, 42, generator=g)
        depth, mask = 0.5 + 5 * torch.rand(2, 28, 42, generator=g), (torch.rand(2, 28, 42, generator=g) > 0.2).float()
        stats = ops.depth_stats(depth.reshape(1, -1).to(DEV), mask.reshape(1, -1).to(DEV))
        mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        cols_rgb = F.unfold((img.double() - mean.double()) / std.double(), 14, stride=14).transpose(1, 2).reshape(12, 588)
        den = (depth.double() * (mask > 0)).sum() / (mask > 0).sum() + 1e-8
        cols_d = F.unfold(torch.stack([depth.double() / den * mask.double(), mask.double()], 1), 14, stride=14).transpose(1, 2).reshape(12, 392)
        for kind, kv, kp, ref in (("rgb", 588, 640, cols_rgb), ("depth", 392, 448, cols_d)):
            planes = [Slot.get((12, kp), sdt, None, tag="i2c%d" % i) for i in range(2 if mode == "f32x" else 1)]
            for s in planes:
                s.view.copy_(kg.poison_values((12, kp), sdt, DEV))
            out = ops.HiLo((planes[0].view, planes[1].view)) if mode == "f32x" else planes[0].view
            if kind == "rgb":
                ops.im2col_rgb(img.to(DEV), dt, out=out)
            else:
                ops.im2col_depth(depth.to(DEV), mask.to(DEV), stats, 2, dt, out=out)
            _sync_check(*[s.check for s in planes])
            got = _val(out)
            assert float(got[:, kv:].abs().max()) == 0.0, "im2col %s %s: K padding must come back exactly zero" % (kind, mode)
            # (x - mean) / std resp. depth / (f32(sum / count) + 1e-8) * mask in f32: at most four roundings, each on the value itself
            kg.elementwise_budget("im2col_%s_%s" % (kind, mode), got[:, :kv], ref, ref.abs(), kg.U_OUT[mode], 4 * kg.MARGIN,
                                  extra=kg.f16_subnormal_floor(mode), quiet=True)


# =============================================================================================
# ovg_qkv
# =============================================================================================
def _qkv_case(mode, seq, gw, M, global_mode, norm_rope, tile, g, tag):
    dt, sdt = MODES[mode], STORE[mode]
    tpv = seq
    aseq = M if global_mode else seq
    BH = (M // aseq) * 16
    cos, sin = st.orc.rope_tables(38)
    x32, w32, bias = torch.randn(M, 1024, generator=g), torch.randn(3072, 1024, generator=g) * 0.03, torch.randn(3072, generator=g) * 0.1
    qn = [torch.randn(64, generator=g) * 0.1 + 1.5, torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1 + 1.5, torch.randn(64, generator=g) * 0.1]
    xd, xv = _operand(x32, mode, True)
    if mode == "f32x":                                   # the weight matrix is dense [3072, 1024] (the entry takes no row stride for it)
        wh = ops.to_hilo(w32)
        wd, wv = ops.HiLo(wh.planes.to(DEV)), wh.hi.double() + wh.lo.double()
    else:
        wd, wv = w32.to(dt).to(DEV), w32.to(dt).double()
    qr, kr, vr = st.qkv_reference(xv, wv, bias.double(), aseq, [t.double() for t in qn] if norm_rope else None,
                                  (cos.double(), sin.double()) if norm_rope else None, tpv, gw)
    npad = ops.pad_to(aseq, 64)
    nplanes = 2 if mode == "f32x" else 1

    def buffers(poison, which):
        out = []
        for nm, shape in (("q", (BH, npad, 64)), ("k", (BH, npad, 64)), ("vt", (BH, 64, npad))):
            pl = [Slot.get(shape, sdt, None, spare_rows=0, tag="%s%s%d" % (which, nm, i)) for i in range(nplanes)]
            for s in pl:
                s.view.zero_()
                if poison:
                    (kg.poison_vt(s.view, aseq, mode != "f32") if nm == "vt" else kg.poison_rows(s.view, aseq))
            out.append(pl)
        return out

    def launch(bufs, part):
        t = [ops.HiLo((pl[0].view, pl[1].view)) if nplanes == 2 else pl[0].view for pl in bufs]
        ops.qkv(xd, wd, bias.to(DEV), aseq, dt, t[0], t[1], t[2], qk_norm=[v.to(DEV) for v in qn] if norm_rope else None,
                rope=(cos[:, :16].contiguous().to(DEV), sin[:, :16].contiguous().to(DEV)) if norm_rope else None,
                tokens_per_view=tpv, grid_w=gw, part=part, tile=tile)
        return t

    pb = buffers(True, "p")
    before = [[s.view.clone() for s in pl] for pl in pb]
    t = launch(pb, 0)
    _sync_check(*[s.check for pl in pb for s in pl])
    # the padding IS the guard: rows seq.. of q / k and the dead V^T columns keep their poison bit for bit
    key = (kg.vt_pos16(npad) if mode != "f32" else torch.arange(npad)).to(DEV)
    for (nm, pl), bf in zip(zip("qkv", pb), before):
        for s, b0 in zip(pl, bf):
            if nm == "v":
                assert torch.equal(s.view[:, :, key >= aseq], b0[:, :, key >= aseq]), "qkv %s: V^T padding columns were written" % tag
            else:
                assert torch.equal(s.view[:, aseq:], b0[:, aseq:]), "qkv %s: %s padding rows were written" % (tag, nm)
    q, k = _val(t[0])[:, :aseq], _val(t[1])[:, :aseq]
    vt_nat = torch.empty(BH, 64, npad, dtype=torch.float64)
    vt_nat[:, :, key.cpu()] = _val(t[2])
    v = vt_nat[:, :, :aseq]
    tol = GATE[mode] * (2 if mode in ("bf16", "f16") else (5 if mode == "f32" else 1))
    _global("qkv_%s.q" % tag, q, qr.reshape(BH, aseq, 64), tol)
    _global("qkv_%s.k" % tag, k, kr.reshape(BH, aseq, 64), tol)
    _global("qkv_%s.vt" % tag, v, vr.reshape(BH, aseq, 64).transpose(1, 2), tol)
    # per element: V is the plain GEMM; without q/k-norm and RoPE so are k and q (q: one more product by q_scale)
    mg = kg.gemm_mag(xv, wv, bias).reshape(M // aseq, aseq, 3, 16, 64).permute(2, 0, 3, 1, 4).reshape(3, BH, aseq, 64)
    u, c, fl = kg.U_OUT[mode], kg.gemm_c(1024, mode), kg.f16_subnormal_floor(mode)
    kg.elementwise_budget("qkv_%s.vt" % tag, v, vr.reshape(BH, aseq, 64).transpose(1, 2), mg[2].transpose(1, 2), u, c, extra=fl, quiet=True)
    qs = 0.125 * 1.4426950408889634
    if not norm_rope:
        kg.elementwise_budget("qkv_%s.k" % tag, k, kr.reshape(BH, aseq, 64), mg[1], u, c, extra=fl, quiet=True)
        kg.elementwise_budget("qkv_%s.q" % tag, q, qr.reshape(BH, aseq, 64), mg[0] * qs, u, c + kg.MARGIN, extra=fl, quiet=True)
    else:
        # q/k-norm + RoPE (the form the model runs): the GEMM's budget carried through the 64-wide LayerNorm and the rotation
        # (kernel_guards.qk_norm_rope_error), + the store's u_out |ref| and one product (q_scale)
        B_ = M // aseq
        zz = (xv @ wv.t() + bias.double()).reshape(B_, aseq, 3, 16, 64).permute(2, 0, 3, 1, 4)
        ez = (c * kg.U_ACC * mg).reshape(3, B_, 16, aseq, 64)
        tt = torch.arange(M) % tpv
        pp = (tt - 5).clamp(min=0)
        pos = torch.stack([torch.where(tt >= 5, pp // gw + 1, torch.zeros_like(tt)), torch.where(tt >= 5, pp % gw + 1, torch.zeros_like(tt))], -1).reshape(B_, aseq, 2)
        for nm, i, got_, ref_, sc in (("q", 0, q, qr, qs), ("k", 1, k, kr, 1.0)):
            err = kg.qk_norm_rope_error(zz[i], ez[i], qn[2 * i], qn[2 * i + 1], 1e-5, pos, cos, sin, sc).reshape(BH, aseq, 64)
            kg.elementwise_budget("qkv_%s.%s" % (tag, nm), got_, ref_.reshape(BH, aseq, 64), ref_.reshape(BH, aseq, 64).abs(), u, kg.MARGIN, extra=err + fl, quiet=True)
    # zero padding: the same valid bits; part 1 then part 2 == part 0
    got = [[s.view.clone() for s in pl] for pl in pb]
    for part in ((0,), (1, 2)):
        zb = buffers(False, "z")
        for p_ in part:
            launch(zb, p_)
            if p_ == 1:
                torch.cuda.synchronize()
                assert all(float(s.view.float().abs().max()) == 0.0 for s in zb[0]), "qkv %s: part 1 wrote q" % tag
        _sync_check(*[s.check for pl in zb for s in pl])
        for (nm, pl), gp in zip(zip("qkv", zb), got):
            for s, gt in zip(pl, gp):
                if nm == "v":
                    assert torch.equal(s.view[:, :, key < aseq], gt[:, :, key < aseq]), "qkv %s part %s: V^T differs from the poisoned run" % (tag, part)
                else:
                    assert torch.equal(s.view[:, :aseq], gt[:, :aseq]), "qkv %s part %s: %s differs from the poisoned run" % (tag, part, nm)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f32x"])
def test_qkv_short_sequences_poisoned_padding(mode):
    g = torch.Generator().manual_seed(113)
    for seq, gw in ((6, 1), (64, 10), (65, 10), (127, 11), (129, 31), (5 + 28 * 37, 37)):
        for global_mode in (False, True):
            for norm_rope in (True, False):
                for tile in ((L.TILE_AUTO,) if mode == "f32" else (L.TILE_AUTO, L.TILE_256)):
                    _qkv_case(mode, seq, gw, 3 * seq, global_mode, norm_rope, tile, g,
                              "%s_seq%d_%s_%s_t%d" % (mode, seq, "global" if global_mode else "frame", "norm_rope" if norm_rope else "plain", tile))
        Slot.cache.clear()


# =============================================================================================
# ovg_flash_attn, ovg_attn_merge, ovg_heads_to_tokens
# =============================================================================================
ATT_NQ = (1, 15, 16, 17, 63, 64, 65, 255, 257)
ATT_KEYS = ([1], [63], [64], [65], [1, 1, 1], [64, 1], [7, 129])


def _attn_inputs(mode, BHq, BHkv, nq, nks, g, poison):
    """-> q device buffer, segments, and the float64 values (q [BHq,nq,64], k / v [BHkv, sum nk, 64])."""
    sdt = STORE[mode]
    nplanes = 2 if mode == "f32x" else 1

    def split(v32):
        if mode == "f32x":
            h = ops.to_hilo(v32)
            return [h.hi, h.lo], h.hi.double() + h.lo.double()
        r = v32.to(sdt)
        return [r], r.double()

    def mk(shape):
        return [torch.zeros(shape, dtype=sdt, device=DEV) for _ in range(nplanes)]

    def wrap(pl):
        return ops.HiLo((pl[0], pl[1])) if nplanes == 2 else pl[0]

    nq_pad = ops.pad_to(nq, 64)
    qp, qv = split(torch.randn(BHq, nq, 64, generator=g) * 1.2)
    qb = mk((BHq, nq_pad, 64))
    for b_, p_ in zip(qb, qp):
        b_[:, :nq] = p_.to(DEV)
        if poison:
            kg.poison_rows(b_, nq)
    segs, kvs, vvs = [], [], []
    for nk in nks:
        nk_pad = ops.pad_to(nk, 64)
        kp, kv = split(torch.randn(BHkv, nk, 64, generator=g))
        vp, vv = split(torch.randn(BHkv, nk, 64, generator=g))
        kb, vb = mk((BHkv, nk_pad, 64)), mk((BHkv, 64, nk_pad))
        for b_, p_ in zip(kb, kp):
            b_[:, :nk] = p_.to(DEV)
            if poison:
                kg.poison_rows(b_, nk)
        for b_, p_ in zip(vb, vp):
            ops.set_vt(b_, p_.transpose(1, 2))
            if poison:
                kg.poison_vt(b_, nk, mode != "f32")
        segs.append((wrap(kb), wrap(vb), nk))
        kvs.append(kv)
        vvs.append(vv)
    return wrap(qb), segs, qv, torch.cat(kvs, 1), torch.cat(vvs, 1)


def _attn_variants(mode):
    return {"bf16": st.ATTN16_VARIANTS, "f16": st.ATTN16_VARIANTS, "f32": (1,), "f32x": (0,)}[mode]


def _attn_shape(mode, BH, kv_heads, nq, nks, seed):
    head_major = kv_heads > 0
    BHkv = kv_heads if kv_heads else BH
    tag = "%s_bh%d_kvh%d_nq%d_k%s" % (mode, BH, kv_heads, nq, "+".join(map(str, nks)))
    ins = [_attn_inputs(mode, BH, BHkv, nq, nks, torch.Generator().manual_seed(seed), poison) for poison in (True, False)]
    qd, segs, qv, kv, vv = ins[0]
    idx = torch.arange(BH) % BHkv
    ref, mag, c, lse_ref = kg.attn_budget(qv, kv[idx], vv[idx], mode)
    floor = kg.attn_p_floor(vv[idx], mode) + kg.f16_subnormal_floor(mode)
    nq_pad = ops.pad_to(nq, 64)
    dt = MODES[mode]
    for variant in _attn_variants(mode):
        outs = []
        for (qd, segs, _, _, _) in ins:
            if head_major:
                out, checks = _out_slot(mode, (BH, nq_pad, 64), False, 72, tag="attn_hm")
                out.fill_(-7.25)
            else:
                out, checks = _out_slot(mode, ((BH // 16) * nq, 1024), False, 1032, tag="attn_tm")
            ls = Slot.get((BH, nq_pad), torch.float32, None, tag="lse")
            ls.view.fill_(-7.25)
            ops.flash_attn(qd, segs, nq, dt, out=out, variant=variant, kv_heads=kv_heads, head_major=head_major, lse=ls.view)
            _sync_check(ls.check, *checks)
            assert bool((ls.view[:, nq:] == -7.25).all()), "attn %s v%d: the lse tail nq..nq_pad was written" % (tag, variant)
            o = _val(out)
            if head_major:
                assert bool((o[:, nq:] == -7.25).all()), "attn %s v%d: head-major rows nq..nq_pad were written" % (tag, variant)
            o = o[:, :nq] if head_major else o.view(BH // 16, nq, 16, 64).permute(0, 2, 1, 3).reshape(BH, nq, 64)
            outs.append((o, ls.view[:, :nq].double().cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), \
            "attn %s v%d: the result depends on the contents of the q / K / V^T padding" % (tag, variant)
        o, ls = outs[0]
        _global("attn_%s_v%d" % (tag, variant), o, ref, GATE[mode])
        kg.elementwise_budget("attn_%s_v%d" % (tag, variant), o, ref, mag, kg.U_OUT[mode], c, extra=floor, quiet=True)
        # log2-sum-exp2: absolute error = the relative error of the row sum / ln 2 (same constant as the output's, without the P rounding
        # when the sum is taken before it; gated with it: an upper bound) + the f32 store
        lse_budget = (c.squeeze(-1) * kg.U_ACC) / math.log(2.0) + kg.U_OUT["f32"] * lse_ref.abs()
        err = (ls - lse_ref).abs()
        assert bool((err <= lse_budget).all()), "attn %s v%d lse: max err %.3e budget %.3e" % (tag, variant, float(err.max()), float(lse_budget.min()))
        _global("attn_%s_v%d.lse" % (tag, variant), ls, lse_ref, 2e-5 if mode in ("f32", "f32x") else 2e-3)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f32x"])
def test_flash_attention_small_shapes_poisoned_padding_and_lse(mode):
    """Finding recorded here: the first derivation of the budget had no absolute term for P. In the f16 formats P also has an absolute quantum
    (2^-25 below 2^-14), and the f16 speculative kernels anchor 4 log2 units above the first tile's maximum, so the row sum can be as small as
    2^-4: on keys [1, 1, 1] variant 50 was 6.8e-7 off on an output of 8.9e-5 against a budget of 3.2e-7 without that term. The kernel is
    right (its documented head-room); the derivation was incomplete: kernel_guards.attn_p_floor now carries the term, from the format and
    the documented anchor, not from the measured error."""
    seed = 200
    for nq in ATT_NQ:
        for nks in ATT_KEYS:
            for BH, kvh in ((16, 0), (48, 0), (16, 8)):
                seed += 1
                if kvh and mode == "f32x":        # the header: split-f16 has no kv_heads / head-major form
                    qd, segs, _, _, _ = _attn_inputs(mode, BH, kvh, nq, nks, torch.Generator().manual_seed(seed), False)
                    _refused(lambda: ops.flash_attn(qd, segs, nq, MODES[mode], kv_heads=kvh, head_major=True), "attn f32x kv_heads nq=%d keys=%s" % (nq, nks))
                    continue
                _attn_shape(mode, BH, kvh, nq, nks, seed)
    Slot.cache.clear()


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_split_kv_forced_on_short_queries_stays_inside_its_workspace(mode):
    dt = MODES[mode]
    seed = 300
    for nq, nks in ((65, [7, 129]), (17, [65]), (1, [64, 1]), (63, [64, 64, 64, 64, 64, 64, 64, 63])):
        seed += 1
        qd, segs, qv, kv, vv = _attn_inputs(mode, 16, 16, nq, nks, torch.Generator().manual_seed(seed), True)
        ref, mag, c, lse_ref = kg.attn_budget(qv, kv, vv, mode)
        tiles = sum((n + 63) // 64 for n in nks)
        for splits in range(2, 9):
            tag = "%s_nq%d_k%s_s%d" % (mode, nq, "+".join(map(str, nks)), splits)
            try:
                plan = ops.attn_plan(16, nq, nks, dt, 0, splits, nq_pad=qd.shape[1])
            except L.OvgError as e:
                assert splits > tiles, "attn_plan %s refused %d splits of %d key tiles: %s" % (tag, splits, tiles, e)
                _note_refusal(e, "attn_plan " + tag)
                continue
            assert 1 <= plan["splits"] <= splits, "plan %s: %d splits" % (tag, plan["splits"])
            print("split-KV %s: %d key tiles, plan runs %d splits" % (tag, tiles, plan["splits"]), flush=True)
            ws = None
            checks = []
            if plan["splits"] > 1:
                a = Slot.get((1, plan["part_bytes"]), torch.uint8, None, spare_rows=0, tag="wsp")
                b = Slot.get((1, plan["lse_bytes"] // 4), torch.float32, None, spare_rows=0, tag="wsl")
                ws, checks = (a.view.view(-1), b.view.view(-1)), [a.check, b.check]
            out, oc = _out_slot(mode, (nq, 1024), False, 1032, tag="attn_sp")
            try:
                ops.flash_attn(qd, segs, nq, dt, out=out, kv_splits=splits, split_ws=ws)
            except L.OvgError as e:
                assert splits > tiles, "flash_attn %s refused %d splits of %d key tiles: %s" % (tag, splits, tiles, e)
                _note_refusal(e, "flash_attn " + tag)
                _sync_check(*(checks + oc))
                continue
            _sync_check(*(checks + oc))
            o = _val(out).view(nq, 16, 64).permute(1, 0, 2)
            _global("attn_split_" + tag, o, ref, GATE[mode] * 1.5)
            # f32 partials merged exactly: the unsplit budget + one more weighted sum per split (splits + 2 roundings)
            kg.elementwise_budget("attn_split_" + tag, o, ref, mag, kg.U_OUT[mode], c + kg.MARGIN * (splits + 2),
                                  extra=kg.attn_p_floor(vv, mode) + kg.f16_subnormal_floor(mode), quiet=True)


# The three forms of a plan that writes partials, each at the smallest shape that reaches it (16 entries; confirmed with ops.attn_plan on the
# CPU): a tail rule needs nq >= 4096 and 16 (256-row) / 32 (512-row) key tiles per range, so the chip is shrunk with `cus` and the tail forced
# with the plan knobs (kv_splits = key ranges).  name: (nq, variant, kv_splits, cus, the plan)
SPLIT_FORMS = {
    # 6 key tiles in 3 ranges, partials for all 384 padded rows of every entry
    "whole_launch": (321, L.ATTN_SPEC256, 3, 0,
                     {"splits": 3, "q_tile": 256, "main_rows": 321, "tail_q_tile": 0, "part_bytes": 3 * 16 * 384 * 64 * 4, "lse_bytes": 3 * 16 * 384 * 4}),
    # 272 units of 256 rows on 48 slots: 5 full rounds = 240 units = 3840 rows unsplit, the other 300 rows (padded to 512) in 2 key ranges
    "key_tail_256": (4140, L.ATTN_PLAN_KEYTAIL256, 2, 24,
                     {"splits": 2, "q_tile": 256, "main_rows": 3840, "tail_q_tile": 256, "part_bytes": 2 * 16 * 512 * 64 * 4, "lse_bytes": 2 * 16 * 512 * 4}),
    # 160 units of 512 rows on 12 slots: 13 full rounds = 156 units -> 9 tiles = 4608 rows per entry unsplit, the other 88 rows (padded to 512) in 2 ranges
    "key_tail_512": (4696, L.ATTN_PLAN_KEYTAIL512, 2, 12,
                     {"splits": 2, "q_tile": 512, "main_rows": 4608, "tail_q_tile": 512, "part_bytes": 2 * 16 * 512 * 64 * 4, "lse_bytes": 2 * 16 * 512 * 4}),
}


@pytest.mark.parametrize("form", list(SPLIT_FORMS))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_split_workspace_of_every_plan_form_is_exactly_what_the_plan_reports(mode, form):
    """One sizing function serves ovg_attn_plan's answer, ovg_flash_attn's refusal and the kernels' partial layout: a launch with workspaces of
    exactly the reported byte counts stays inside them and equals the baseline kernel (output and log-sum-exp, gpu_selftest.TOL); four bytes
    less of either buffer is OVG_E_ARG before anything is written."""
    nq, variant, splits, cus, want = SPLIT_FORMS[form]
    dt = MODES[mode]
    qd, segs, _, _, _ = _attn_inputs(mode, 16, 16, nq, [nq], torch.Generator().manual_seed(400 + len(form)), True)
    nq_pad = qd.shape[1]
    plan = ops.attn_plan(16, nq, [nq], dt, variant, splits, nq_pad=nq_pad, cus=cus)
    assert plan == want, (form, plan)

    def run(variant, splits, ws, cus):
        out, oc = _out_slot(mode, (nq, 1024), False, 1032, tag="attn_form")
        ls = Slot.get((16, nq_pad), torch.float32, None, tag="lse_form")
        out.fill_(-7.25)
        ls.view.fill_(-7.25)
        return out, ls, oc + [ls.check], lambda: ops.flash_attn(qd, segs, nq, dt, out=out, variant=variant, lse=ls.view, kv_splits=splits, split_ws=ws, cus=cus)

    out, ls, checks, call = run(L.ATTN_BASELINE, 1, None, 0)
    call()
    _sync_check(*checks)
    ref_o, ref_l = _val(out).clone(), ls.view[:, :nq].double().cpu()

    a = Slot.get((1, plan["part_bytes"]), torch.uint8, None, spare_rows=0, tag="wsp")
    b = Slot.get((1, plan["lse_bytes"] // 4), torch.float32, None, spare_rows=0, tag="wsl")
    part, lse = a.view.view(-1), b.view.view(-1)
    out, ls, checks, call = run(variant, splits, (part, lse), cus)
    call()
    _sync_check(a.check, b.check, *checks)
    assert bool((ls.view[:, nq:] == -7.25).all()), "%s %s: the lse tail nq..nq_pad was written" % (form, mode)
    _global("attn_form_%s_%s" % (form, mode), _val(out), ref_o, st.TOL[mode])
    _global("attn_form_%s_%s.lse" % (form, mode), ls.view[:, :nq].double().cpu(), ref_l, st.TOL[mode])
    _global_only(2)

    for what, ws in (("part", (part[:-4], lse)), ("lse", (part, lse[:-1]))):        # 4 bytes short of either buffer
        out, ls, checks, call = run(variant, splits, ws, cus)
        with pytest.raises(L.OvgError, match="OVG_E_ARG"):
            call()
        kg.STATS["refusals"] += 1
        print("[REFUSED] attn %s %s: %s workspace 4 bytes short" % (form, mode, what), flush=True)
        _sync_check(a.check, b.check, *checks)
        assert bool((_val(out) == -7.25).all()) and bool((ls.view == -7.25).all()), "%s %s: a refused launch wrote its output" % (form, mode)
    Slot.cache.clear()


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f32x"])
def test_attn_merge_and_heads_to_tokens_short_rows_strided(mode):
    g = torch.Generator().manual_seed(115)
    dt, sdt = MODES[mode], STORE[mode]
    for rows in (1, 63, 65):
        n_pad = ops.pad_to(rows, 64)
        a32, b32 = torch.randn(rows, 1024, generator=g), torch.randn(rows, 1024, generator=g)
        la, lb = torch.randn(16, n_pad, generator=g) * 3, torch.randn(16, n_pad, generator=g) * 3
        ad, av = _operand(a32, mode, True)
        bd, bv = _operand(b32, mode, True)
        out, checks = _out_slot(mode, (rows, 1024), False, 1040, tag="merge")
        ops.attn_merge(ad, la.to(DEV), bd, lb.to(DEV), dt, out=out)
        _sync_check(*checks)
        wa = torch.exp2(la.double()[:, :rows].t()).repeat_interleave(64, 1)
        wb = torch.exp2(lb.double()[:, :rows].t()).repeat_interleave(64, 1)
        ref = (wa * av + wb * bv) / (wa + wb)
        mag = (wa * av.abs() + wb * bv.abs()) / (wa + wb)
        _global("attn_merge_%s_r%d" % (mode, rows), _val(out), ref, GATE[mode])
        # two exp2 (2 ulp each on an argument with one rounding of |lse| <= 16: ln2 * 16 u), two products, two sums, a reciprocal, a product: 16
        kg.elementwise_budget("attn_merge_%s_r%d" % (mode, rows), _val(out), ref, mag, kg.U_OUT[mode], kg.MARGIN * (16 + 2 * math.log(2.0) * 16),
                              extra=kg.f16_subnormal_floor(mode), quiet=True)
        if mode in ("bf16", "f16"):
            x = torch.randn(16, n_pad, 64, generator=g).to(sdt)
            kg.poison_rows(x, rows)
            s = Slot.get((rows, 1024), sdt, 1040, tag="h2t")
            ops.heads_to_tokens(x.to(DEV), rows, dt, out=s.view)
            _sync_check(s.check)
            assert torch.equal(s.view.cpu(), x[:, :rows].permute(1, 0, 2).reshape(rows, 1024)), "heads_to_tokens %s rows=%d" % (mode, rows)
            kg.STATS["numeric"] += 1


# =============================================================================================
# head kernels
# =============================================================================================
_conv_ref = kg.conv_ref          # the float64 reference and magnitude of ovg_conv (shared with dpt_stages.py)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_conv_small_maps_guarded(mode):
    """ovg_conv below and above the 256-kernel's 16384-output-pixel line; tiny maps whose 128-pixel tile is almost empty."""
    g = torch.Generator().manual_seed(117)
    dt = MODES[mode]
    d64 = lambda t: None if t is None else t.double()
    forms = (("1x1_pos", dict(k=1, pos=True)), ("3x3_add2_relu", dict(k=3, adds=2, relu=True)), ("3x3s2_add1", dict(k=3, stride=2, adds=1)),
             ("convT2", dict(up=2)), ("convT4", dict(up=4)))
    for (H, W), imgs in (((1, 1), (1, 3)), ((1, 17), (1, 3)), ((3, 2), (1, 3)), ((127, 129), (1,)), ((128, 128), (1,))):
        for n in imgs:
            for fname, f in forms:
                k, stride, up, relu, adds, pos = f.get("k", 1), f.get("stride", 1), f.get("up", 0), f.get("relu", False), f.get("adds", 0), f.get("pos", False)
                cin = 64 if H * W > 1000 else 128
                cout = 128 if up != 4 else 32
                rows = up * up * cout if up > 1 else cout
                x = torch.randn(n, H, W, cin, generator=g).to(dt)
                w = (torch.randn(rows, k * k * cin, generator=g) * (k * k * cin) ** -0.5).to(dt)
                bias = torch.randn(cout, generator=g) * 0.3
                pd = k // 2
                OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
                s_ = up if up > 1 else 1
                adds_t = [torch.randn(n, OH, OW, cout, generator=g).to(dt) for _ in range(adds)]
                ps = (torch.randn(OW, cout // 2, generator=g) * 0.1, torch.randn(OH, cout // 2, generator=g) * 0.1) if pos else None
                tag = "conv_%s_%s_n%d_%dx%d" % (fname, mode, n, H, W)

                def strided(t):          # an NHWC view with a pixel stride of cout + 8, poison in the gaps
                    big = kg.poison_values(tuple(t.shape[:-1]) + (t.shape[-1] + 8,), t.dtype, "cpu")
                    big[..., : t.shape[-1]] = t
                    return big.to(DEV)[..., : t.shape[-1]]
                slot = Slot.get((n, OH * s_, OW * s_, cout), dt, cout + 8, tag="conv")
                ops.conv(x.to(DEV), w.to(DEV), bias.to(DEV), dt, cout, ksize=k, stride=stride, upshuffle=up, relu=relu,
                         add1=strided(adds_t[0]) if adds >= 1 else None, add2=strided(adds_t[1]) if adds >= 2 else None,
                         pos=None if ps is None else (ps[0].to(DEV), ps[1].to(DEV)), out=slot.view)
                _sync_check(slot.check)
                ref, mag = _conv_ref(x.double(), w.double(), bias.double(), cout, k, stride, up, relu, d64(adds_t[0]) if adds >= 1 else None,
                                     d64(adds_t[1]) if adds >= 2 else None, None if ps is None else (ps[0].double(), ps[1].double()))
                got = _val(slot.view)
                _global(tag, got, ref, GATE[mode])
                # an implicit GEMM over k*k*cin products + bias / tables / adds (up to 4 more sums)
                kg.elementwise_budget(tag, got, ref, mag, kg.U_OUT[mode], kg.gemm_c(k * k * cin, mode) + 4 * kg.MARGIN, extra=kg.f16_subnormal_floor(mode), quiet=True)
    Slot.cache.clear()


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_upsample_edges_guarded(mode):
    g = torch.Generator().manual_seed(119)
    dt = MODES[mode]
    for (H, W, OH, OW) in ((1, 1, 5, 7), (2, 3, 2, 3), (37, 28, 74, 56), (8, 8, 5, 5), (1, 3, 1, 5), (3, 1, 5, 1), (2, 3, 1, 1)):
        x = torch.randn(2, H, W, 64, generator=g).to(dt)
        slot = Slot.get((2, OH, OW, 64), dt, 72, tag="up")
        try:
            ops.upsample(x.to(DEV), OH, OW, dt, out=slot.view)
        except L.OvgError as e:
            assert OH < H or OW < W, "upsample %dx%d -> %dx%d refused: %s" % (H, W, OH, OW, e)      # only the downscale may be refused
            _note_refusal(e, "upsample %dx%d -> %dx%d" % (H, W, OH, OW))
            continue
        _sync_check(slot.check)
        xd = x.double().permute(0, 3, 1, 2)
        ref = F.interpolate(xd, size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        mag = x.double().abs().amax((1, 2), keepdim=True).expand(2, OH, OW, 64)
        got = _val(slot.view)
        tag = "upsample_%s_%dx%d_to_%dx%d" % (mode, H, W, OH, OW)
        if (H, W) == (OH, OW):
            assert torch.equal(got, x.double()), tag + ": the identity resize must copy"
        _global(tag, got, ref, GATE[mode])
        # source coordinate o * (H - 1) / (OH - 1) in f32: 2 roundings on a value < max(H, W), so each axis' weight pair moves by 2 max(H, W) u
        # and the result by that times the difference of two neighbours (<= 2 max|x| of the channel); four products and three sums on top:
        # (8 max(H, W) + 8) u on mag = max|x| of the image's channel
        kg.elementwise_budget(tag, got, ref, mag, kg.U_OUT[mode], kg.MARGIN * (8 * max(H, W) + 8), extra=kg.f16_subnormal_floor(mode), quiet=True)
        if mode != "f32":
            # stricter, with the documented f32 coordinate arithmetic as the specification: bit-equal to its rounding outside the rounding
            # window, one of the admissible roundings inside (kernel_guards.upsample_window)
            kg.check_upsampled_map(tag, got, kg.upsample_window(x.double(), OH, OW, None, mode))


def test_dpt_out_and_dpt_tail_small_maps_guarded():
    g = torch.Generator().manual_seed(121)
    for OH, OW in ((1, 1), (15, 17), (70, 1)):
        for act, od in (("exp", 2), ("inv_log", 4)):
            h = F.relu(torch.randn(2, OH, OW, 32, generator=g))
            w2, b2 = torch.randn(od, 32, generator=g) * 0.2, torch.randn(od, generator=g) * 0.1
            sv, sc = Slot.get((2, OH, OW, od - 1), torch.float32, None, tag="dov"), Slot.get((2 * OH, OW), torch.float32, None, tag="doc")
            ops.dpt_out(h.to(DEV), w2.to(DEV), b2.to(DEV), act, out=(sv.view, sc.view.view(2, OH, OW)))
            _sync_check(sv.check, sc.check)
            o = h.double() @ w2.double().t() + b2.double()
            m = h.double() @ w2.abs().double().t() + b2.abs().double()
            val = torch.exp(o[..., :-1]) if act == "exp" else torch.sign(o[..., :-1]) * torch.expm1(o[..., :-1].abs())
            conf = 1 + torch.exp(o[..., -1])
            tag = "dpt_out_%s_%dx%d" % (act, OH, OW)
            _global(tag + ".val", _val(sv.view), val, 2e-5)
            _global(tag + ".conf", _val(sc.view).view(2, OH, OW), conf, 2e-5)
            # exp(o): o carries (32 + 1) u mag_o, which exp turns into a relative error; the f32 exp itself within 4 ulp: budget on
            # mag = (|val| + 1) (1 + mag_o) with c = 2 (33 + 8)
            kg.elementwise_budget(tag + ".val", _val(sv.view), val, (val.abs() + 1) * (1 + m[..., :-1]), kg.U_OUT["f32"], kg.MARGIN * 41, quiet=True)
            kg.elementwise_budget(tag + ".conf", _val(sc.view).view(2, OH, OW), conf, conf.abs() * (1 + m[..., -1]), kg.U_OUT["f32"], kg.MARGIN * 41, quiet=True)
            for mode in ("bf16", "f16"):
                dt = MODES[mode]
                x = torch.randn(2, 5, 4, 128, generator=g).to(dt)
                w1 = torch.zeros(128, 9 * 128, dtype=dt)
                w1[:32] = (torch.randn(32, 9 * 128, generator=g) * (9 * 128) ** -0.5).to(dt)
                b1 = torch.randn(32, generator=g) * 0.3
                tv, tc = Slot.get((2, OH, OW, od - 1), torch.float32, None, tag="dtv"), Slot.get((2 * OH, OW), torch.float32, None, tag="dtc")
                call = lambda: ops.dpt_tail(x.to(DEV), OH, OW, dt, None, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), act, out=(tv.view, tc.view.view(2, OH, OW)))
                if OH <= 1 or OW <= 1:
                    _refused(call, "dpt_tail %s -> %dx%d" % (mode, OH, OW))
                    continue
                call()
                _sync_check(tv.check, tc.check)
                up = F.interpolate(x.double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).to(dt).double()
                hmap, _ = _conv_ref(up, w1.double(), b1.double(), 32, 3, 1, 0, True, None, None, None)
                o = hmap @ w2.double().t() + b2.double()
                val = torch.exp(o[..., :-1]) if act == "exp" else torch.sign(o[..., :-1]) * torch.expm1(o[..., :-1].abs())
                gate = 4e-3 if mode == "bf16" else 5e-4           # gpu_selftest's dpt_tail gates (the 16-bit rounding of the upsampled map is inside)
                _global("dpt_tail_%s_%s_%dx%d.val" % (act, mode, OH, OW), _val(tv.view), val, gate)
                _global("dpt_tail_%s_%s_%dx%d.conf" % (act, mode, OH, OW), _val(tc.view).view(2, OH, OW), 1 + torch.exp(o[..., -1]), gate)
                # per element too: against a float64 bilinear reference a map value on a rounding boundary may go the other way (one 16-bit
                # ulp of a conv INPUT) and no bound in u_acc holds, but with the coordinate arithmetic the kernels document the boundary cases
                # are a known small set (kernel_guards.upsample_window) whose ulp dpt_tail_budget carries through the stage
                B = kg.dpt_tail_budget(x.double(), OH, OW, None, w1.double(), b1, w2, b2, act, mode)
                kg.check_dpt_tail("dpt_tail_%s_%s_%dx%d" % (act, mode, OH, OW), _val(tv.view), _val(tc.view).view(2, OH, OW), B, quiet=True)


def test_camera_head_every_row_block_edge_guarded():
    import head_ops_emul as emul
    heads = importlib.import_module("omnivggt_official_amd.heads")
    heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")
    torch.manual_seed(21)
    head = heads.CameraHead(dim_in=2048).eval()
    with torch.no_grad():
        for name, p in head.named_parameters():
            if name.endswith("gamma"):
                p.fill_(0.7)
            elif name == "empty_pose_tokens":
                p.normal_(0, 0.5)
            elif p.dim() > 1:
                p.mul_(1.5)
            elif "bias" in name:
                p.uniform_(-0.1, 0.1)
    hip = heads_hip.HipCameraHead(head.to(DEV))
    g = torch.Generator().manual_seed(123)
    tol_twin = {"bf16": 1.5e-2, "f16": 2e-3, "f32": 1e-5}          # gpu_selftest.test_camera_head's gates against the rounding twin
    for mode in ("bf16", "f16", "f32"):
        dt = MODES[mode]
        with torch.no_grad():
            W = hip._weights(dt, torch.device(DEV))
        Wc = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in W.items() if k != "blocks"}
        Wc["blocks"] = [{k: v.cpu() for k, v in blk.items()} for blk in W["blocks"]]
        for S in (1, 2, 15, 16, 17, 63, 64, 65):
            toks = torch.randn(S, 2048, generator=g) * 1.3
            slot = Slot.get((4 * S, 9), torch.float32, None, tag="cam")
            # the workspace: exactly the queried byte count, inside a guard band of its own
            wsb = Slot.get((1, ops.camera_head_workspace_bytes(S, dt)), torch.uint8, None, spare_rows=0, tag="camws")
            ops.camera_head(_strided_input(toks, True), W, dt, ws=wsb.view.view(-1), out=slot.view.view(4, S, 9))
            _sync_check(slot.check, wsb.check)
            with torch.no_grad():
                twin = emul.camera_head(toks, Wc, dt)
            # global gate only: the reference is the rounding twin (float32, 16-bit activation buffers rounded where the kernel stores them)
            # through 4 refinement rounds of a 4-block trunk; a boundary case of any of those roundings moves an element by a 16-bit ulp
            # of an intermediate, so there is no per-element budget in u_acc to derive
            _global("camera_head_%s_S%d_vs_twin" % (mode, S), _val(slot.view).view(4, S, 9), twin.double(), tol_twin[mode])
            # the same gate per component group (translation, quaternion, field of view each against its own maximum); the stages of the
            # head have per-element budgets in test_gpu_camera_head_stages.py
            assert kg.camera_group_gate("camera_head_%s_S%d_vs_twin" % (mode, S), _val(slot.view).view(4, S, 9), twin.double(), tol_twin[mode])
            _global_only()
