"""-m gpu: the block and head kernels on operands whose byte offsets pass 2 GiB and 4 GiB and whose element indices pass 2^31
(tests/address_range.py holds the shapes; tests/test_address_range_host.py proves them by arithmetic and plants a 32-bit wrap on the CPU).

stride form   every entry with a row or pixel stride in its parameter struct, ONE operand at a time 16 MiB + 64 B per row apart (257 rows of
              a 16-bit operand, 513 of an f32 one), the others at ld = row length + 8. The far call must equal its near twin -- the same
              call with every operand near -- bit for bit; the near twin is gated per element against float64 (kernel_guards).
count form    dense layouts, inputs periodic with period 1031 (rows, pixels, heads, frames): output row m must equal row m mod 1031, compared
              on the device in 256 MiB chunks; the first 1031 rows are the near twin and are gated per element against float64. Where a
              kernel's result legitimately depends on the position (ovg_upsample, ovg_unproject: the pixel coordinate enters the value) the
              far result itself is gated against a float64 reference computed on the device in chunks.
Tiles and attention variants are forced, so that a far call and its twin run the same kernel. Every far output sits in a guard band
(kernel_guards.guarded_chunked: a wrapped store lands at a low address of that buffer or in its gaps). No test holds more than 24 GiB
(asserted from torch.cuda.max_memory_allocated), caches are emptied between cases, too little free memory is a failure, nothing is skipped.

Dense operands that cannot cross a line within 12 GiB for one tensor or a second of compute are not run: address_range.NOT_RUN lists them
with the size that rules them out (printed by test_operands_that_are_not_run_are_listed).

Findings (by reading, before the first GPU run; DESIGN.md "Address ranges of the model-path kernels"):
 * the 256 x 256 GEMM main loop forms a tile row's byte offset in 32 bits: from ld = 8 421 505 elements on (16.06 MiB per row) row 255 wraps.
   OVG_TILE_AUTO now takes the 128 tile there and a forced OVG_TILE_256 is OVG_E_UNSUPPORTED (test_linear_256_tile_leading_dimension_limit:
   at the largest legal ld the 256 tile still equals its twin). The stride of this module, 16 MiB + 64 B, is below that line by design of the
   issue's figure: 255 rows of it are 4 278 206 400 bytes.
 * FastDiv (row index / period in the PATCH, injection and QKV epilogues) is exact for quotients below 2^22 only: refused beyond (host test).
 * ovg_conv's 256-pixel form assumed a tile touches two images; maps of fewer than 256 pixels put more into one tile: the host condition
   now counts them. The block entries refuse every row-count limit of the entries they sequence before their first launch."""
import importlib
import math
import time
import zlib

import pytest
import torch
import torch.nn.functional as F

import address_range as ar
import block_reference as br
import gpu_selftest as st
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}
STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": torch.float16}
EPI = {"store": L.EPI_STORE, "gelu": L.EPI_GELU, "res": L.EPI_RES, "patch": L.EPI_PATCH}
TILE = {128: L.TILE_128, 256: L.TILE_256}
ATTN_VARIANT = {"bf16": L.ATTN_SPEC256, "f16": L.ATTN_LAZY256, "f32": L.ATTN_BASELINE, "f32x": L.ATTN_AUTO}      # one kernel each, whatever the shape
P = ar.PERIOD
REPORT = []


@pytest.fixture(autouse=True)
def _memory_and_time():
    L.require_gpu()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                            # a device fault is sticky: nothing more of this module is started on that device
        pytest.exit("the device reported %s: the remaining address-range tests are not started" % str(e).splitlines()[0], returncode=3)
    peak, dt = torch.cuda.max_memory_allocated(), time.perf_counter() - t0
    torch.cuda.empty_cache()
    REPORT.append((peak, dt))
    print("address range: this test held at most %.2f GiB and took %.2f s; the module so far: %d tests, %.1f s, largest %.2f GiB; "
          "%d guarded launches, %d numeric checks, %d refusals" % (peak / ar.GIB, dt, len(REPORT), sum(r[1] for r in REPORT),
                                                                   max(r[0] for r in REPORT) / ar.GIB, kg.STATS["guarded_launches"],
                                                                   kg.STATS["numeric"], kg.STATS["refusals"]), flush=True)
    assert peak <= ar.MEM_CAP, "the test held %.2f GiB of device memory, the limit is %d GiB" % (peak / ar.GIB, ar.MEM_CAP // ar.GIB)


def _estimate(case):
    return sum(o.bytes for o in case.operands.values()) + case.scratch


def _need(*cases):
    """Too little free device memory for a listed case is a failure that says so, never a skip."""
    need = max(_estimate(c) for c in cases)
    free = torch.cuda.mem_get_info()[0]
    assert free >= need, "%s needs %.2f GiB of device memory, %.2f GiB are free" % (cases[0].name, need / ar.GIB, free / ar.GIB)


def _cases(prefix):
    got = [c for n, c in ar.CASES.items() if n.startswith(prefix)]
    assert got, prefix
    return got


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _store(v32, mode):
    """f32 CPU values -> (what the device holds: a tensor of the storage dtype, or a HiLo pair; its float64 value)."""
    if mode == "f32x":
        h = ops.to_hilo(v32)
        return h, h.hi.double() + h.lo.double()
    r = v32.to(STORE[mode])
    return r, r.double()


def _val(t):
    return (t.hi.double() + t.lo.double()).cpu() if isinstance(t, ops.HiLo) else t.double().cpu()


def _planes(t):
    return [t.hi, t.lo] if isinstance(t, ops.HiLo) else [t]


def _strides(shape, ld):
    s = [1, ld]
    for d in reversed(shape[1:-1]):
        s.append(s[-1] * d)
    return tuple(reversed(s[: len(shape)]))


class Placer:
    """Puts the strided operands of one stride-form case where the table says (the far run) or all of them near (the twin run)."""

    def __init__(self, case, far_run):
        self.case, self.far_run, self.checks = case, far_run, []

    def op(self, name):
        o = self.case.operands[name]
        return o if self.far_run else ar.twin_of(o)

    def _inp(self, name, vals):
        o = self.op(name)
        assert vals.numel() == o.rows * o.cols and vals.element_size() == o.esz and vals.shape[-1] == o.cols, (self.case.name, name, vals.shape, o)
        buf = torch.empty(o.last_elem + 1, dtype=vals.dtype, device=DEV)       # not initialised: no kernel may read between the rows
        v = buf.as_strided(tuple(vals.shape), _strides(vals.shape, o.ld))
        v.copy_(vals.to(DEV))
        return v

    def inp(self, name, vals):
        if isinstance(vals, ops.HiLo):
            return ops.HiLo((self._inp(name, vals.hi), self._inp(name, vals.lo)))
        return self._inp(name, vals)

    def out(self, name, shape, dtype, planes=1, fill=None):
        o = self.op(name)
        rows = 1
        for d in shape[:-1]:
            rows *= d
        assert rows == o.rows and shape[-1] == o.cols and torch.empty((), dtype=dtype).element_size() == o.esz, (self.case.name, name, shape, o)
        views = []
        for _ in range(planes):
            v, c = (kg.guarded_chunked if o.bytes > ar.CHUNK_BYTES else kg.guarded)(shape, dtype, DEV, ld=o.ld)
            if fill is not None:
                v.fill_(fill)
            views.append(v)
            self.checks.append(c)
        return ops.HiLo(tuple(views)) if planes == 2 else views[0]

    def check(self):
        torch.cuda.synchronize()
        for i, c in enumerate(self.checks):
            c("%s %s guard %d" % (self.case.name, "far" if self.far_run else "twin", i))


def _stride(case, build):
    """build(placer) -> {name: output tensor or HiLo}: run it with every operand near (the twin), then as the table says (one operand far);
    both inside guard bands, the far outputs bit-equal to the twin's. -> the twin's outputs as dense copies."""
    _need(case)
    assert case.form == "stride" and list(case.far) == [case.arg["far"]]
    res = []
    for far_run in (False, True):
        pl = Placer(case, far_run)
        outs = build(pl)
        pl.check()
        res.append({k: [p.contiguous().clone() for p in _planes(v)] for k, v in outs.items()})
        del pl, outs
        torch.cuda.empty_cache()
    for k in res[0]:
        for i, (a, b) in enumerate(zip(res[0][k], res[1][k])):
            if not torch.equal(a, b):
                bad = torch.nonzero((a != b).reshape(a.shape[0] if a.dim() > 1 else 1, -1).any(1)).flatten()
                raise AssertionError("%s: output %s%s differs from its near twin in %d rows, first %d, last %d (operand %s is %d bytes per row apart)" % (
                    case.name, k, "_lo" if i else "", bad.numel(), int(bad[0]), int(bad[-1]), case.arg["far"], case.operands[case.arg["far"]].ld * case.operands[case.arg["far"]].esz))
    kg.STATS["numeric"] += 1
    return {k: (ops.HiLo(tuple(v)) if len(v) == 2 else v[0]) for k, v in res[0].items()}


def _periodic(name, t, period=P):
    """Count form: row m of t (dense, on the device) must equal row m mod period bit for bit."""
    bad = ar.first_aperiodic_row(t, period)
    assert bad is None, "%s: row %d differs from row %d (= %d mod %d), byte offset %d of the output" % (
        name, bad, bad % period, bad, period, bad * t[0].numel() * t.element_size())
    kg.STATS["numeric"] += 1


def _refused(fn, what):
    with pytest.raises(L.OvgError, match="ARG|UNSUPPORTED"):
        fn()
    kg.STATS["refusals"] += 1
    print("[REFUSED] %s" % what, flush=True)


# =============================================================================================
# ovg_linear
# =============================================================================================
def _linear_values(mode, epi, M, N, K, out_rows, g):
    """-> (x, w storage + values, bias, extra keyword tensors (CPU), ref, mag, c, u) of one ovg_linear call."""
    x32, w32, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g) * 0.3
    xs, xv = _store(x32, mode)
    ws, wv = _store(w32, mode)
    z, mg = xv @ wv.t() + bias.double(), kg.gemm_mag(xv, wv, bias)
    kw = {}
    if epi == "store":
        ref, mag, c, u = z, mg, kg.gemm_c(K, mode), kg.U_OUT[mode]
    elif epi == "gelu":
        ref, mag, c, u = F.gelu(z), mg, kg.gelu_c(K, mode), kg.U_OUT[mode]
    elif epi == "res":
        kw["res"], kw["gamma"] = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
        ref, mag, c, u = kw["res"].double() + kw["gamma"].double() * z, kg.res_mag(kw["res"], kw["gamma"], mg), kg.res_c(K, mode), kg.U_OUT["f32"]
    else:
        p0, p1, off = ar.PATCH_P0, ar.PATCH_P1, ar.PATCH_OFF
        kw["table"] = torch.randn(p0 + 1, N, generator=g)
        m = torch.arange(M)
        dst = (m // p0) * p1 + off + m % p0
        assert int(dst.max()) + 1 == out_rows
        ref, mag = torch.full((out_rows, N), 7.25, dtype=torch.float64), torch.zeros(out_rows, N, dtype=torch.float64)      # rows the call does not own keep 7.25 exactly
        ref[dst], mag[dst] = z + kw["table"][1:][m % p0].double(), mg + kw["table"][1:][m % p0].abs().double()
        c, u = kg.gemm_c(K, mode) + kg.MARGIN, kg.U_OUT["f32"]
    return xs, ws, bias, kw, ref, mag, c, u


def _linear_stride(case):
    a, o = case.arg, case.operands
    mode, epi, tile = a["mode"], a["epi"], a["tile"]
    M, K, N, out_rows = o["x"].rows, o["x"].cols, o["w"].rows, o["y"].rows
    xs, ws, bias, kw, ref, mag, c, u = _linear_values(mode, epi, M, N, K, out_rows, _gen(case.name))
    f32 = o["y"].esz == 4
    bd = bias.to(DEV)

    def build(pl):
        out = pl.out("y", (out_rows, N), torch.float32 if f32 else STORE[mode], planes=1 if f32 else o["y"].planes, fill=7.25 if epi == "patch" else None)
        k2 = {k: v.to(DEV) for k, v in kw.items() if k != "res"}
        if epi == "res":
            k2["res"] = pl.inp("res", kw["res"])
        if epi == "patch":
            k2.update(p0=ar.PATCH_P0, p1=ar.PATCH_P1, row_off=ar.PATCH_OFF)
        ops.linear(pl.inp("x", xs), pl.inp("w", ws), bd, MODES[mode], epilogue=EPI[epi], out=out, tile=TILE[tile], **k2)
        return {"y": out}

    got = _val(_stride(case, build)["y"])
    kg.elementwise_budget(case.name, got, ref, mag, u, c, extra=None if f32 else kg.f16_subnormal_floor(mode), quiet=True)


@pytest.mark.parametrize("combo", ["%s.%s.t%d" % (e, m, t) for m, e, t in ar.LINEAR_COMBOS])
def test_linear_one_operand_16_mib_per_row_apart(combo):
    """x, w, y (and res) of ovg_linear in turn, both forced tiles: STORE in bf16 / f32 / split-f16, GELU / RES / PATCH in bf16."""
    for case in _cases("linear.%s." % combo):
        _linear_stride(case)


def test_linear_256_tile_leading_dimension_limit():
    """The 256 x 256 main loop holds a tile row's byte offset in 32 bits: the largest leading dimension it can address is 8 421 504 elements
    (255 ld 2 + 64 <= 2^32). At that ld -- x, then w -- the forced 256 tile equals its near twin and OVG_TILE_AUTO equals it too; one 16-byte
    step further the forced tile is refused (OVG_E_UNSUPPORTED, the guarded output untouched) while the 128 tile still equals its twin.
    OVG_TILE_AUTO is checked at M = 20 000 rows, where its documented rule picks the 256 tile: with w at the largest legal ld it must give
    the 256 tile's bits, one step further the 128 tile's (w is the far operand there: 512 rows of 16 MiB, not 20 000)."""
    ld_max = (((1 << 32) - 64) // 255) // 2
    assert 255 * ld_max * 2 + 64 <= (1 << 32) < 255 * (ld_max + 8) * 2 + 64
    g = _gen("ld256")
    M, N, K = 257, 512, 64
    x, w, bias = torch.randn(M, K, generator=g).to(torch.bfloat16), (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16), torch.randn(N, generator=g).to(DEV)
    ref = x.double() @ w.double().t() + bias.double().cpu()
    mag = kg.gemm_mag(x.double(), w.double(), bias.cpu())

    def strided(vals, ld):
        buf = torch.empty((vals.shape[0] - 1) * ld + vals.shape[1], dtype=vals.dtype, device=DEV)
        v = buf.as_strided(tuple(vals.shape), (ld, 1))
        v.copy_(vals.to(DEV))
        return v

    def run(xd, wd, tile):
        out, chk = kg.guarded((M, N), torch.bfloat16, DEV, ld=N + 8)
        ops.linear(xd, wd, bias, torch.bfloat16, out=out, tile=tile)
        torch.cuda.synchronize()
        chk("ld256 tile %d" % tile)
        return out.clone()

    twin = {t: run(strided(x, K + 8), strided(w, K + 8), t) for t in (L.TILE_128, L.TILE_256)}
    kg.elementwise_budget("ld256.twin256", _val(twin[L.TILE_256]), ref, mag, kg.U_OUT["bf16"], kg.gemm_c(K, "bf16"), quiet=True)
    kg.elementwise_budget("ld256.twin128", _val(twin[L.TILE_128]), ref, mag, kg.U_OUT["bf16"], kg.gemm_c(K, "bf16"), quiet=True)
    for which in ("x", "w"):
        for ld, fits in ((ld_max, True), (ld_max + 8, False)):
            xd = strided(x, ld if which == "x" else K + 8)
            wd = strided(w, ld if which == "w" else K + 8)
            tag = "ld256 %s at ld = %d" % (which, ld)
            if fits:
                assert torch.equal(run(xd, wd, L.TILE_256), twin[L.TILE_256]), tag + ": the forced 256 tile differs from its near twin"
            else:
                out, chk = kg.guarded((M, N), torch.bfloat16, DEV, ld=N + 8)
                with pytest.raises(L.OvgError, match="UNSUPPORTED"):
                    ops.linear(xd, wd, bias, torch.bfloat16, out=out, tile=L.TILE_256)
                torch.cuda.synchronize()
                chk(tag)
                assert bool((chk.buffer == kg.GUARD_BYTE).all()), tag + ": a refused call wrote its output"
                kg.STATS["refusals"] += 1
            assert torch.equal(run(xd, wd, L.TILE_128), twin[L.TILE_128]), tag + ": the 128 tile differs from its near twin"
            del xd, wd
            torch.cuda.empty_cache()
    # AUTO at a row count whose documented choice is the 256 tile (M >= 20000, STORE): beyond the limit it must run the 128 tile instead.
    # The operand that is far is w (512 rows): x stays dense, so the case costs 512 x 16 MiB, not 20000 x 16 MiB
    Mb = 20000
    xb = torch.randn(Mb, K, generator=g).to(torch.bfloat16).to(DEV)
    outs = {}
    for ld in (K + 8, ld_max, ld_max + 8):
        wd = strided(w, ld)
        for tile in (L.TILE_AUTO, L.TILE_128) + ((L.TILE_256,) if ld <= ld_max else ()):
            out, chk = kg.guarded((Mb, N), torch.bfloat16, DEV, ld=N + 8)
            ops.linear(xb, wd, bias, torch.bfloat16, out=out, tile=tile)
            torch.cuda.synchronize()
            chk("ld256 auto")
            outs[(ld, tile)] = out.clone()
        del wd
        torch.cuda.empty_cache()
    for ld in (ld_max, ld_max + 8):
        for tile in (L.TILE_128, L.TILE_256):
            if (ld, tile) in outs:
                assert torch.equal(outs[(ld, tile)], outs[(K + 8, tile)]), "ld256: tile %d at ldw = %d differs from its near twin" % (tile, ld)
    assert torch.equal(outs[(ld_max, L.TILE_AUTO)], outs[(K + 8, L.TILE_256)]), "ld256: AUTO at the largest legal ldw is not the 256 tile's result"
    assert torch.equal(outs[(ld_max + 8, L.TILE_AUTO)], outs[(K + 8, L.TILE_128)]), "ld256: AUTO beyond the limit is not the 128 tile's result"
    same = torch.equal(outs[(K + 8, L.TILE_128)], outs[(K + 8, L.TILE_256)])
    print("ld256: at this shape the two tiles' results %s" % ("are bit-equal: which tile AUTO ran cannot be told from the numbers, only that its result is right"
                                                              if same else "differ bit for bit: AUTO's choice on either side of the limit is visible"), flush=True)


@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("linear.count.")])
def test_linear_2_pow_24_rows(name):
    """M = 2^24 + 257 rows (2^23 + 257 for the f32 output of the 256 tile: 8 GiB instead of 16), K = 64, rows periodic with period 1031."""
    case = ar.CASES[name]
    _need(case)
    a = case.arg
    M, N, K, res = a["M"], a["N"], ar.LINEAR_K, a["out"] == "res"
    f32 = a["out"] != "16"
    xs, ws, bias, kw, ref, mag, c, u = _linear_values("bf16", "res" if res else "store", P, N, K, P, _gen(name))
    x = ar.tile_periodic(xs.to(DEV), M)
    k2 = {}
    if res:
        k2 = dict(res=ar.tile_periodic(kw["res"].to(DEV), M), gamma=kw["gamma"].to(DEV))
    out, chk = kg.guarded_chunked((M, N), torch.float32 if f32 else torch.bfloat16, DEV)
    ops.linear(x, ws.to(DEV), bias.to(DEV), torch.bfloat16, epilogue=L.EPI_RES if res else L.EPI_STORE, out=out, out_f32=f32, tile=TILE[a["tile"]], **k2)
    torch.cuda.synchronize()
    chk(name)
    kg.elementwise_budget(name + ".twin", _val(out[:P]), ref, mag, kg.U_OUT["f32"] if f32 else u, c, quiet=True)
    _periodic(name, out)


# =============================================================================================
# ovg_qkv, ovg_flash_attn, ovg_attn_merge, ovg_heads_to_tokens
# =============================================================================================
@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("qkv.")])
def test_qkv_x_16_mib_per_row_apart(name):
    """x of ovg_qkv (the one strided operand of its struct), one sequence of 257 / 513 tokens, plain projection (no q/k-norm, no RoPE: the
    epilogue is the GEMM's, so the plain GEMM budget holds for q, k and V^T)."""
    case = ar.CASES[name]
    mode, M, dt, sdt = case.arg["mode"], case.arg["M"], MODES[case.arg["mode"]], STORE[case.arg["mode"]]
    g = _gen(name)
    x32, w32, bias = torch.randn(M, 1024, generator=g), torch.randn(3072, 1024, generator=g) * 0.03, torch.randn(3072, generator=g) * 0.1
    xs, xv = _store(x32, mode)
    ws, wv = _store(w32, mode)
    wd = ops.HiLo(ws.planes.to(DEV)) if mode == "f32x" else ws.to(DEV)
    npad = ops.pad_to(M, 64)

    def build(pl):
        q, k, vt = ops.alloc_qkv(16, M, M, dt, DEV)
        ops.qkv(pl.inp("x", xs), wd, bias.to(DEV), M, dt, q, k, vt, tile=TILE[case.arg["tile"]])
        return {"q": q, "k": k, "vt": vt}

    t = _stride(case, build)
    qr, kr, vr = st.qkv_reference(xv, wv, bias.double(), M, None, None, M, 1)
    key = kg.vt_pos16(npad) if mode != "f32" else torch.arange(npad)
    vt_nat = torch.empty(16, 64, npad, dtype=torch.float64)
    vt_nat[:, :, key] = _val(t["vt"])
    mg = kg.gemm_mag(xv, wv, bias).reshape(1, M, 3, 16, 64).permute(2, 0, 3, 1, 4).reshape(3, 16, M, 64)
    u, c, fl = kg.U_OUT[mode], kg.gemm_c(1024, mode), kg.f16_subnormal_floor(mode)
    qs = 0.125 * 1.4426950408889634
    kg.elementwise_budget(name + ".vt", vt_nat[:, :, :M], vr.reshape(16, M, 64).transpose(1, 2), mg[2].transpose(1, 2), u, c, extra=fl, quiet=True)
    kg.elementwise_budget(name + ".k", _val(t["k"])[:, :M], kr.reshape(16, M, 64), mg[1], u, c, extra=fl, quiet=True)
    kg.elementwise_budget(name + ".q", _val(t["q"])[:, :M], qr.reshape(16, M, 64), mg[0] * qs, u, c + kg.MARGIN, extra=fl, quiet=True)


def _attn_operands(mode, BH, nq, nk, g):
    """q [BH, nq_pad, 64], k [BH, nk_pad, 64], V^T [BH, 64, nk_pad] on the device (zero padding) + their float64 values [BH, n, 64]."""
    sdt = STORE[mode]
    nq_pad, nk_pad = ops.pad_to(nq, 64), ops.pad_to(nk, 64)
    vals, dev = [], []
    for n, n_pad, scale, is_v in ((nq, nq_pad, 1.2, False), (nk, nk_pad, 1.0, False), (nk, nk_pad, 1.0, True)):
        s, v = _store(torch.randn(BH, n, 64, generator=g) * scale, mode)
        planes = []
        for p_ in _planes(s):
            if is_v:
                b = ops.set_vt(torch.zeros(BH, 64, n_pad, dtype=sdt, device=DEV), p_.transpose(1, 2))
            else:
                b = torch.zeros(BH, n_pad, 64, dtype=sdt, device=DEV)
                b[:, :n] = p_.to(DEV)
            planes.append(b)
        dev.append(ops.HiLo(tuple(planes)) if mode == "f32x" else planes[0])
        vals.append(v)
    return dev, vals


@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("flash_attn.") and ar.CASES[n].form == "stride"])
def test_flash_attn_output_rows_16_mib_apart(name):
    case = ar.CASES[name]
    mode, nq, nk = case.arg["mode"], case.arg["nq"], case.arg["nk"]
    (qd, kd, vd), (qv, kv, vv) = _attn_operands(mode, 16, nq, nk, _gen(name))

    def build(pl):
        out = pl.out("out", (nq, 1024), STORE[mode], planes=2 if mode == "f32x" else 1)
        ops.flash_attn(qd, [(kd, vd, nk)], nq, MODES[mode], out=out, variant=ATTN_VARIANT[mode])
        return {"out": out}

    got = _val(_stride(case, build)["out"]).view(nq, 16, 64).permute(1, 0, 2)
    ref, mag, c, _ = kg.attn_budget(qv, kv, vv, mode)
    kg.elementwise_budget(name, got, ref, mag, kg.U_OUT[mode], c, extra=kg.attn_p_floor(vv, mode) + kg.f16_subnormal_floor(mode), quiet=True)


def test_flash_attn_half_a_million_short_sequences():
    """BH = 2^19 + 16 heads of 64 queries and 50 keys: q, k, V^T and the token-major output all pass 4 GiB and 2^31 elements; heads periodic
    with period 1031, so head bh of the output must equal head bh mod 1031."""
    case = ar.CASES["flash_attn.count"]
    _need(case)
    BH, nq, nk = case.arg["BH"], case.arg["nq"], case.arg["nk"]
    (q0, k0, v0), (qv, kv, vv) = _attn_operands("bf16", P, nq, nk, _gen(case.name))
    q, k, vt = ar.tile_periodic(q0, BH), ar.tile_periodic(k0, BH), ar.tile_periodic(v0, BH)
    del q0, k0, v0
    out, chk = kg.guarded_chunked(((BH // 16) * nq, 1024), torch.bfloat16, DEV)
    ops.flash_attn(q, [(k, vt, nk)], nq, torch.bfloat16, out=out, variant=ATTN_VARIANT["bf16"])
    torch.cuda.synchronize()
    chk(case.name)
    del q, k, vt
    # token-major [B nq, 16 x 64] -> one row per head: [B, nq, 16, 64] -> [B, 16, nq, 64], in chunks of whole batches of 16 heads
    o4 = out.view(BH // 16, nq, 16, 64)
    ref, mag, c, _ = kg.attn_budget(qv, kv, vv, "bf16")
    nb = (P + 15) // 16
    twin = o4[:nb].permute(0, 2, 1, 3).reshape(nb * 16, nq * 64)[:P].clone()
    kg.elementwise_budget(case.name + ".twin", _val(twin).view(P, nq, 64), ref, mag, kg.U_OUT["bf16"], c, quiet=True)
    step = max(1, ar.CHUNK_BYTES // (16 * nq * 64 * 2))
    for b0 in range(0, BH // 16, step):
        b1 = min(b0 + step, BH // 16)
        heads = o4[b0:b1].permute(0, 2, 1, 3).reshape((b1 - b0) * 16, nq * 64)
        idx = torch.arange(b0 * 16, b1 * 16, device=DEV) % P
        diff = (heads.view(torch.int16) != twin.view(torch.int16)[idx]).any(1)
        assert not bool(diff.any()), "%s: head %d differs from head %d" % (case.name, b0 * 16 + int(torch.nonzero(diff)[0]), (b0 * 16 + int(torch.nonzero(diff)[0])) % P)
    kg.STATS["numeric"] += 1


@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("attn_merge.")])
def test_attn_merge_one_operand_16_mib_per_row_apart(name):
    case = ar.CASES[name]
    mode, rows = case.arg["mode"], case.arg["rows"]
    g = _gen(name.rsplit(".", 1)[0])
    n_pad = ops.pad_to(rows, 64)
    (as_, av), (bs, bv) = _store(torch.randn(rows, 1024, generator=g), mode), _store(torch.randn(rows, 1024, generator=g), mode)
    la, lb = torch.randn(16, n_pad, generator=g) * 3, torch.randn(16, n_pad, generator=g) * 3

    def build(pl):
        out = pl.out("out", (rows, 1024), STORE[mode], planes=2 if mode == "f32x" else 1)
        ops.attn_merge(pl.inp("a", as_), la.to(DEV), pl.inp("b", bs), lb.to(DEV), MODES[mode], out=out)
        return {"out": out}

    got = _val(_stride(case, build)["out"])
    wa = torch.exp2(la.double()[:, :rows].t()).repeat_interleave(64, 1)
    wb = torch.exp2(lb.double()[:, :rows].t()).repeat_interleave(64, 1)
    # the constant of test_gpu_edges.test_attn_merge_and_heads_to_tokens_short_rows_strided
    kg.elementwise_budget(name, got, (wa * av + wb * bv) / (wa + wb), (wa * av.abs() + wb * bv.abs()) / (wa + wb), kg.U_OUT[mode],
                          kg.MARGIN * (16 + 2 * math.log(2.0) * 16), extra=kg.f16_subnormal_floor(mode), quiet=True)


def test_heads_to_tokens_output_rows_16_mib_apart():
    case = ar.CASES["heads_to_tokens.bf16.y"]
    n, n_pad = case.arg["n"], case.arg["n_pad"]
    x = torch.randn(16, n_pad, 64, generator=_gen(case.name)).to(torch.bfloat16)

    def build(pl):
        out = pl.out("y", (n, 1024), torch.bfloat16)
        ops.heads_to_tokens(x.to(DEV), n, torch.bfloat16, out=out)
        return {"y": out}

    assert torch.equal(_stride(case, build)["y"].cpu(), x[:, :n].permute(1, 0, 2).reshape(n, 1024)), case.name


# =============================================================================================
# the row kernels: LayerNorm family, copy_rows, pack_weights, dino_specials, assemble_tokens
# =============================================================================================
def _ln_gate(name, got, x, w, b, eps, u, floor=0.0, add=None):
    ref, mag, c, extra = kg.layernorm_budget(x, w, b, eps)
    if add is not None:
        ref, mag, c = ref + add.double(), mag + add.abs().double(), c + kg.MARGIN
    kg.elementwise_budget(name, got, ref, mag, u, c, extra=extra + floor, quiet=True)


@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("layernorm.") and ar.CASES[n].form == "stride"])
def test_layernorm_one_operand_16_mib_per_row_apart(name):
    case = ar.CASES[name]
    mode, f32, rows = case.arg["mode"], case.arg["f32"], case.arg["rows"]
    g = _gen(name.rsplit(".", 1)[0])
    x, w, b = torch.randn(rows, 1024, generator=g) * 2 + 0.3, torch.randn(1024, generator=g) * 0.1 + 1, torch.randn(1024, generator=g) * 0.1

    def build(pl):
        out = pl.out("y", (rows, 1024), torch.float32 if f32 else STORE[mode], planes=case.operands["y"].planes)
        ops.layernorm(pl.inp("x", x), w.to(DEV), b.to(DEV), 1e-5, MODES[mode], out=out, out_f32=f32)
        return {"y": out}

    _ln_gate(name, _val(_stride(case, build)["y"]), x, w, b, 1e-5, kg.U_OUT["f32" if f32 else mode], 0.0 if f32 else kg.f16_subnormal_floor(mode))


def test_layernorm_2_pow_20_rows():
    case = ar.CASES["layernorm.count"]
    _need(case)
    rows = case.arg["rows"]
    g = _gen(case.name)
    x, w, b = torch.randn(P, 1024, generator=g) * 2 + 0.3, torch.randn(1024, generator=g) * 0.1 + 1, torch.randn(1024, generator=g) * 0.1
    out, chk = kg.guarded_chunked((rows, 1024), torch.bfloat16, DEV)
    ops.layernorm(ar.tile_periodic(x.to(DEV), rows), w.to(DEV), b.to(DEV), 1e-5, torch.bfloat16, out=out)
    torch.cuda.synchronize()
    chk(case.name)
    _ln_gate(case.name + ".twin", _val(out[:P]), x, w, b, 1e-5, kg.U_OUT["bf16"])
    _periodic(case.name, out)


@pytest.mark.parametrize("name", [n for n in ar.CASES if n.startswith("head_layernorm.") and ar.CASES[n].form == "stride"])
def test_head_layernorm_one_operand_16_mib_per_row_apart(name):
    case = ar.CASES[name]
    mode, views, tpv = case.arg["mode"], case.arg["views"], case.arg["tpv"]
    g = _gen(name.rsplit(".", 1)[0])
    x, w, b = torch.randn(views * tpv, 2048, generator=g) * 2 + 0.3, torch.randn(2048, generator=g) * 0.2 + 1, torch.randn(2048, generator=g) * 0.1
    keep = torch.cat([torch.arange(v * tpv + 5, (v + 1) * tpv) for v in range(views)])

    def build(pl):
        out = pl.out("y", (views * (tpv - 5), 2048), STORE[mode])
        ops.head_layernorm(pl.inp("x", x), w.to(DEV), b.to(DEV), 1e-5, MODES[mode], views, tokens_per_view=tpv, out=out)
        return {"y": out}

    _ln_gate(name, _val(_stride(case, build)["y"]), x[keep], w, b, 1e-5, kg.U_OUT[mode])


def test_head_layernorm_second_trip_of_its_grid():
    """262144 + 7 rows: the grid is capped at 2^16 blocks of four rows, so the last seven rows are the second trip of the grid-stride loop;
    x passes 2 GiB."""
    case = ar.CASES["head_layernorm.count"]
    _need(case)
    rows = case.arg["rows"]
    g = _gen(case.name)
    x, w, b = torch.randn(P, 2048, generator=g) * 2 + 0.3, torch.randn(2048, generator=g) * 0.2 + 1, torch.randn(2048, generator=g) * 0.1
    xd = torch.empty(rows + 5, 2048, device=DEV)
    xd[:5] = 1e4                                          # the five special rows of the one view: never read
    xd[5:] = ar.tile_periodic(x.to(DEV), rows)
    out, chk = kg.guarded_chunked((rows, 2048), torch.bfloat16, DEV)
    ops.head_layernorm(xd, w.to(DEV), b.to(DEV), 1e-5, torch.bfloat16, 1, tokens_per_view=rows + 5, out=out)
    torch.cuda.synchronize()
    chk(case.name)
    _ln_gate(case.name + ".twin", _val(out[:P]), x, w, b, 1e-5, kg.U_OUT["bf16"])
    _periodic(case.name, out)


def test_copy_rows_far_operands_and_2_pow_20_rows():
    for case in _cases("copy_rows.") :
        if case.form != "stride":
            continue
        x = torch.randn(case.arg["rows"], case.arg["n"], generator=_gen("copy_rows"))

        def build(pl):
            out = pl.out("y", tuple(x.shape), torch.float32)
            ops.copy_rows(pl.inp("x", x), out)
            return {"y": out}

        assert torch.equal(_stride(case, build)["y"].cpu(), x), case.name
    case = ar.CASES["copy_rows.count"]
    _need(case)
    rows = case.arg["rows"]
    x = ar.tile_periodic(torch.randn(P, 1024, generator=_gen(case.name)).to(DEV), rows)
    out, chk = kg.guarded_chunked((rows, 1024), torch.float32, DEV)
    ops.copy_rows(x, out)
    torch.cuda.synchronize()
    chk(case.name)
    assert torch.equal(out[:P], x[:P]), case.name
    _periodic(case.name, out)


@pytest.mark.parametrize("mode", ["bf16", "f32", "f32x"])
def test_pack_weights_one_operand_16_mib_per_row_apart(mode):
    for case in _cases("pack_weights.%s." % mode):
        rows = case.arg["rows"]
        w = torch.randn(rows, 588, generator=_gen("pack_weights"))
        far_src = case.arg["far"] == "src"

        def build(pl):
            out = pl.out("dst", (rows, 640), STORE[mode], planes=2 if mode == "f32x" else 1, fill=3.0)
            # ops.pack_weights makes its source dense: the entry is called directly, with the source's own row stride
            src = pl.inp("src", w)
            o_hi, o_lo = ops.hi_lo(out)
            L.call("ovg_pack_weights", L.PackWeightsParams(L.ptr(src), src.stride(0), L.ptr(o_hi), o_hi.stride(0), rows, 588, 640, L.dtype_code(MODES[mode]), L.ptr(o_lo)),
                   torch.cuda.current_stream().cuda_stream)
            return {"dst": out}

        got = _stride(case, build)["dst"]
        exp = ops.to_hilo(w) if mode == "f32x" else w.to(STORE[mode])
        for gp, e in zip(_planes(got), _planes(exp)):
            assert torch.equal(gp[:, :588].cpu(), e) and float(gp[:, 588:].float().abs().max()) == 0.0, "%s (%s far)" % (case.name, "src" if far_src else "dst")


def test_dino_specials_and_assemble_tokens_one_operand_16_mib_per_row_apart():
    case = ar.CASES["dino_specials.x"]
    V, tpv = case.arg["V"], case.arg["tpv"]
    g = _gen(case.name)
    cls, pos0, reg = torch.randn(1024, generator=g), torch.randn(1024, generator=g), torch.randn(4, 1024, generator=g)

    def build(pl):
        x = pl.out("x", (V * tpv, 1024), torch.float32)
        ops.dino_specials(x, V, tpv, cls.to(DEV), pos0.to(DEV), reg.to(DEV))
        return {"x": x}

    got = _stride(case, build)["x"].cpu().view(V, tpv, 1024)
    assert torch.equal(got[:, 0], (cls + pos0).expand(V, 1024)) and torch.equal(got[:, 1:5], reg.expand(V, 4, 1024)), case.name
    w, b = torch.randn(1024, generator=g) * 0.1 + 1, torch.randn(1024, generator=g) * 0.1
    cam, regt, ph = torch.randn(2, 1024, generator=g), torch.randn(2, 4, 1024, generator=g), torch.randn(1024, generator=g)
    for case in _cases("assemble_tokens."):
        V, tpv = case.arg["V"], case.arg["tpv"]
        x, cam_add, dtok = torch.randn(V * tpv, 1024, generator=g) * 2 + 0.3, torch.randn(V, 1024, generator=g), torch.randn(V // 2, 1024, generator=g)
        drow = torch.tensor([(v // 2 if v % 2 else -1) for v in range(V)], dtype=torch.int32)      # odd views carry one depth token each

        def build(pl):
            out = pl.out("out", (V * tpv, 1024), torch.float32)
            ops.assemble_tokens(pl.inp("xd", x), w.to(DEV), b.to(DEV), 1e-6, cam.to(DEV), regt.to(DEV), cam_add.to(DEV), dtok.to(DEV), drow.to(DEV),
                                ph.to(DEV), out, V, 2, tokens_per_view=tpv)
            return {"out": out}

        got = _val(_stride(case, build)["out"]).view(V, tpv, 1024)
        slot = torch.tensor([0 if v % 2 == 0 else 1 for v in range(V)])
        assert torch.equal(got[:, 0], (cam[slot] + cam_add).double()) and torch.equal(got[:, 1:5], regt[slot].double()), case.name
        add = torch.stack([dtok[v // 2] if v % 2 else ph for v in range(V)])
        _ln_gate(case.name, got[:, 5], x.view(V, tpv, 1024)[:, 5], w, b, 1e-6, kg.U_OUT["f32"], add=add)


# =============================================================================================
# head kernels
# =============================================================================================
def _conv_values(mode, n, H, W, cin, cout, g):
    dt = STORE[mode]
    x, w = torch.randn(n, H, W, cin, generator=g).to(dt), (torch.randn(cout, 9 * cin, generator=g) * (9 * cin) ** -0.5).to(dt)
    bias = torch.randn(cout, generator=g) * 0.3
    adds = [torch.randn(n, H, W, cout, generator=g).to(dt) for _ in range(2)]
    return x, w, bias, adds


def _conv_reference(x, w, bias, adds, cout):
    """-> (ref, mag) of the 3 x 3 ReLU convolution with its adds: computed once, shared by the cases of one shape."""
    return kg.conv_ref(x.double(), w.double(), bias.double(), cout, 3, 1, 0, True, adds[0].double() if adds else None, adds[1].double() if adds else None, None)


def _conv_gate(name, got, mode, cin, refmag):
    # the constant of test_gpu_edges.test_conv_small_maps_guarded
    kg.elementwise_budget(name, got, refmag[0], refmag[1], kg.U_OUT[mode], kg.gemm_c(9 * cin, mode) + 4 * kg.MARGIN, extra=kg.f16_subnormal_floor(mode), quiet=True)


@pytest.mark.parametrize("prefix", ["conv128.bf16.", "conv128.f32.", "conv256.bf16."])
def test_conv_one_operand_far(prefix):
    """x, y, add1, add2 of ovg_conv in turn (3 x 3, 64 -> 128 channels, two adds, ReLU): the 128-pixel form on a 23 x 23 map at 16 MiB + 64 B per
    pixel; the 256-pixel form on 129 x 128 pixels at 512 KiB + 64 B per pixel (x of that form is bounded by its own dispatch condition:
    test_conv256_on_both_sides_of_its_32_bit_line)."""
    from test_gpu_head_edges import _expected_conv256
    refmag = None
    for case in _cases(prefix):
        a = case.arg
        mode, n, H, W, cin, cout = a["mode"], a["n"], a["H"], a["W"], a["cin"], a["cout"]
        x, w, bias, adds = _conv_values(mode, n, H, W, cin, cout, _gen(prefix))
        refmag = refmag or _conv_reference(x, w, bias, adds, cout)
        for far_run in (False, True):
            ldx = (case.operands["x"] if far_run else ar.twin_of(case.operands["x"])).ld
            assert _expected_conv256(mode, n, H, W, cin, cout, 3, 1, 0, ldx) == (128 if prefix.startswith("conv256") else None), (case.name, ldx)

        def build(pl):
            out = pl.out("y", (n, H, W, cout), STORE[mode])
            ops.conv(pl.inp("x", x), w.to(DEV), bias.to(DEV), MODES[mode], cout, ksize=3, relu=True, add1=pl.inp("add1", adds[0]), add2=pl.inp("add2", adds[1]), out=out)
            return {"y": out}

        _conv_gate(case.name, _val(_stride(case, build)["y"]), mode, cin, refmag)


def test_conv256_on_both_sides_of_its_32_bit_line():
    """Two images of 129 x 128 pixels, 3 x 3, 64 -> 128 channels. The 256-pixel form addresses the images of a tile through one 32-bit buffer
    descriptor: it runs while 2 H W ldx 2 < 2^32 - 65536, i.e. up to a pixel stride of 65024 elements (x: 4.29 GB, its last byte just below
    4 GiB), and from 65032 on the 128-pixel form runs (64-bit pointers; x passes 4 GiB and 2^31 elements). Both must equal the reference
    everywhere -- in particular in the tile that spans the two images (pixels 16384 .. 16639; image 1 starts at pixel 16512) -- and the
    256-pixel result must equal its near twin bit for bit."""
    from test_gpu_head_edges import _expected_conv256
    cases = [ar.CASES["conv256.count.ldx%d" % l] for l in ar.CONV256_LDX]
    _need(*cases)
    a = cases[0].arg
    n, H, W, cin, cout = a["n"], a["H"], a["W"], a["cin"], a["cout"]
    x, w, bias, _ = _conv_values("bf16", n, H, W, cin, cout, _gen("conv256.count"))
    assert [_expected_conv256("bf16", n, H, W, cin, cout, 3, 1, 0, l) for l in (cin + 8,) + ar.CONV256_LDX] == [128, 128, None]
    outs = {}
    for ldx in (cin + 8,) + ar.CONV256_LDX:
        buf = torch.empty((n * H * W - 1) * ldx + cin, dtype=torch.bfloat16, device=DEV)
        xd = buf.as_strided((n, H, W, cin), _strides((n, H, W, cin), ldx))
        xd.copy_(x.to(DEV))
        out, chk = kg.guarded((n, H, W, cout), torch.bfloat16, DEV, ld=cout + 8)
        ops.conv(xd, w.to(DEV), bias.to(DEV), torch.bfloat16, cout, ksize=3, relu=True, out=out)
        torch.cuda.synchronize()
        chk("conv256 ldx %d" % ldx)
        outs[ldx] = out.contiguous().clone()
        del buf, xd, out, chk
        torch.cuda.empty_cache()
    refmag = _conv_reference(x, w, bias, None, cout)
    for ldx, o in outs.items():
        _conv_gate("conv256.count.ldx%d" % ldx, _val(o), "bf16", cin, refmag)
    assert torch.equal(outs[ar.CONV256_LDX[0]], outs[cin + 8]), "the 256-pixel form at the largest pixel stride it accepts differs from its near twin"
    same = torch.equal(outs[ar.CONV256_LDX[1]], outs[cin + 8])
    print("conv256: the 128-pixel form one step beyond the line is %s to the 256-pixel form (both within the budget)" % ("bit-equal" if same else "not bit-equal"), flush=True)


def _up_values(mode, n, H, W, C, g):
    return torch.randn(n, H, W, C, generator=g).to(STORE[mode])


def _up_gate(name, got, x, OH, OW, mode):
    """The gates of test_gpu_edges.test_upsample_edges_guarded."""
    H, W = x.shape[1:3]
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    mag = x.double().abs().amax((1, 2), keepdim=True).expand_as(ref)
    kg.elementwise_budget(name, got, ref, mag, kg.U_OUT[mode], kg.MARGIN * (8 * max(H, W) + 8), extra=kg.f16_subnormal_floor(mode), quiet=True)
    if mode != "f32":
        kg.check_upsampled_map(name, got, kg.upsample_window(x.double(), OH, OW, None, mode))


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_upsample_one_operand_16_mib_per_pixel_apart(mode):
    for case in _cases("upsample.%s." % mode):
        a = case.arg
        x = _up_values(mode, 1, a["H"], a["W"], a["C"], _gen("upsample." + mode))

        def build(pl):
            out = pl.out("y", (1, a["OH"], a["OW"], a["C"]), STORE[mode])
            ops.upsample(pl.inp("x", x), a["OH"], a["OW"], MODES[mode], out=out)
            return {"y": out}

        _up_gate(case.name, _val(_stride(case, build)["y"]), x, a["OH"], a["OW"], mode)


def test_upsample_2_pow_28_pixels():
    """A 5 x 4 source of 8 channels resized to 16385 x 16385 pixels: 2^28 + 32769 work items (the second trip of the 2^20-block grid), an
    output past 4 GiB and 2^31 elements. The value depends on the pixel's position, so the far result itself is gated: against the float64
    bilinear reference, computed on the device in row blocks, with the budget of test_gpu_edges.test_upsample_edges_guarded. (The scales
    4 / 16384 and 3 / 16384 and every product with an output index are exact in f32: the coordinate arithmetic adds nothing here.)"""
    case = ar.CASES["upsample.count"]
    _need(case)
    a = case.arg
    H, W, OH, OW, C = a["H"], a["W"], a["OH"], a["OW"], a["C"]
    x = _up_values("bf16", 1, H, W, C, _gen(case.name))
    out, chk = kg.guarded_chunked((1, OH, OW, C), torch.bfloat16, DEV)
    ops.upsample(x.to(DEV), OH, OW, torch.bfloat16, out=out)
    torch.cuda.synchronize()
    chk(case.name)
    xd = x.to(DEV).double()[0]
    mag = xd.abs().amax((0, 1))
    c = kg.MARGIN * (8 * max(H, W) + 8)
    fx = torch.arange(OW, device=DEV, dtype=torch.float64) * ((W - 1) / (OW - 1))
    x0 = fx.floor().long().clamp_max(W - 1)
    x1 = (x0 + 1).clamp_max(W - 1)
    lx = (fx - x0).view(1, OW, 1)
    worst, step = 0.0, max(1, (ar.CHUNK_BYTES // 8) // (OW * C * 8))          # float64 temporaries of 32 MiB: a handful live at once
    for r0 in range(0, OH, step):
        r1 = min(r0 + step, OH)
        fy = torch.arange(r0, r1, device=DEV, dtype=torch.float64) * ((H - 1) / (OH - 1))
        y0 = fy.floor().long().clamp_max(H - 1)
        y1 = (y0 + 1).clamp_max(H - 1)
        ly = (fy - y0).view(-1, 1, 1)
        top = xd[y0][:, x0] * (1 - lx) + xd[y0][:, x1] * lx
        bot = xd[y1][:, x0] * (1 - lx) + xd[y1][:, x1] * lx
        ref = top * (1 - ly) + bot * ly
        worst = max(worst, kg.elementwise_budget("%s rows %d..%d" % (case.name, r0, r1), out[0, r0:r1], ref, mag.expand_as(ref), kg.U_OUT["bf16"], c, quiet=True))
    print("%s: budget used %.3f over %d pixels" % (case.name, worst, OH * OW), flush=True)
    kg.STATS["numeric"] += 1


def test_unproject_2_pow_28_pixels():
    """One frame of 16385 x 16385 pixels: the second trip of unproject's 2^20-block grid, an output past 2 GiB. The result depends on (u, v):
    gated against the header's expression evaluated in float64 on the device, in row blocks, with kernel_guards.unproject_budget /
    C_UNPROJECT (derived there from the kernel's two rounding points; tighter than the 1e-6 global gate of test_gpu_pointcloud)."""
    case = ar.CASES["unproject.count"]
    _need(case)
    H, W = case.arg["H"], case.arg["W"]
    g = _gen(case.name)
    row = (1.0 + torch.rand(P, generator=g)).to(DEV)
    depth = ar.tile_periodic(row, H * W).view(1, H, W)
    cam = torch.tensor([[0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6, 0.5, -1.0, 2.0, 9000.0, 9100.0, 8192.0, 8100.0]], device=DEV)
    out, chk = kg.guarded_chunked((H * W, 3), torch.float32, DEV)
    L.call("ovg_unproject", L.UnprojectParams(L.ptr(depth), L.ptr(cam), L.ptr(out), 1, H, W), torch.cuda.current_stream().cuda_stream)      # (ops.unproject allocates its own output)
    torch.cuda.synchronize()
    chk(case.name)
    c = cam[0].double()
    u = torch.arange(W, device=DEV, dtype=torch.float64).view(1, W)
    o3 = out.view(H, W, 3)
    worst, step = 0.0, max(1, (ar.CHUNK_BYTES // 8) // (W * 3 * 8))
    for r0 in range(0, H, step):
        r1 = min(r0 + step, H)
        d = depth[0, r0:r1].double()
        v = torch.arange(r0, r1, device=DEV, dtype=torch.float64).view(-1, 1)
        ref, mag = kg.unproject_budget(d, u, v, c)
        worst = max(worst, kg.elementwise_budget("%s rows %d..%d" % (case.name, r0, r1), o3[r0:r1], ref, mag, kg.U_OUT["f32"], kg.C_UNPROJECT, quiet=True))
    print("%s: budget used %.3f over %d pixels" % (case.name, worst, H * W), flush=True)
    kg.STATS["numeric"] += 1


def _tail_values(n, H, W, OH, OW, g):
    x = torch.randn(n, H, W, 128, generator=g).to(torch.bfloat16)
    w1 = torch.zeros(128, 9 * 128, dtype=torch.bfloat16)
    w1[:32] = (torch.randn(32, 9 * 128, generator=g) * (9 * 128) ** -0.5).to(torch.bfloat16)
    b1, w2, b2 = torch.randn(32, generator=g) * 0.3, torch.randn(4, 32, generator=g) * 0.2, torch.randn(4, generator=g) * 0.1
    pos = (torch.randn(OW, 64, generator=g) * 0.1, torch.randn(OH, 64, generator=g) * 0.1)
    return x, w1, b1, w2, b2, pos


def _tail_run(xd, v, OH, OW, tag):
    x, w1, b1, w2, b2, pos = v
    n = x.shape[0]
    val, cv = kg.guarded((n, OH, OW, 3), torch.float32, DEV)
    conf, cc = kg.guarded((n * OH, OW), torch.float32, DEV)
    ops.dpt_tail(xd, OH, OW, torch.bfloat16, (pos[0].to(DEV), pos[1].to(DEV)), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), "inv_log",
                 out=(val, conf.view(n, OH, OW)))
    torch.cuda.synchronize()
    cv(tag + " val")
    cc(tag + " conf")
    return val.clone(), conf.view(n, OH, OW).clone()


def test_dpt_tail_source_pixels_far_apart_and_at_its_element_limit():
    """ovg_dpt_tail indexes one source image with 32-bit element offsets and refuses H W ldx >= 2^31 (header). Stride form: two images of
    16 x 15 pixels 16 MiB + 64 B per pixel apart (the second image lies past 3.75 GiB, its pixels past 4 GiB). Count form: a 5 x 4 source at
    the largest pixel stride below the refusal, 107 374 176 elements (x: 8.6 GB); one step further the call is refused and writes nothing."""
    for case, tag in ((ar.CASES["dpt_tail.bf16.x"], "stride"), (ar.CASES["dpt_tail.count"], "count")):
        _need(case)
        a = case.arg
        n, H, W, OH, OW = a["n"], a["H"], a["W"], a["OH"], a["OW"]
        v = _tail_values(n, H, W, OH, OW, _gen(case.name))
        x = v[0]
        got = {}
        for ldx in (128 + ar.NEAR_PAD, case.operands["x"].ld):
            buf = torch.empty((n * H * W - 1) * ldx + 128, dtype=torch.bfloat16, device=DEV)
            xd = buf.as_strided((n, H, W, 128), _strides((n, H, W, 128), ldx))
            xd.copy_(x.to(DEV))
            assert ops.dpt_tail_supported(xd, torch.bfloat16, OH, OW)
            got[ldx] = _tail_run(xd, v, OH, OW, "%s ldx %d" % (case.name, ldx))
            del buf, xd
            torch.cuda.empty_cache()
        near, farr = got[128 + ar.NEAR_PAD], got[case.operands["x"].ld]
        assert torch.equal(near[0], farr[0]) and torch.equal(near[1], farr[1]), "%s: the far call differs from its near twin" % case.name
        B = kg.dpt_tail_budget(x.double(), OH, OW, (v[5][0], v[5][1]), v[1].double(), v[2], v[3], v[4], "inv_log", "bf16")
        kg.check_dpt_tail(case.name, _val(near[0]), _val(near[1]), B, quiet=True)
        if tag == "count":
            ldx = case.operands["x"].ld + 8
            assert H * W * (ldx - 8) < (1 << 31) <= H * W * ldx
            # the refusal reads no memory: a small buffer stands in for the 8.6 GB one
            xd = torch.empty(n * H * W * 136, dtype=torch.bfloat16, device=DEV).as_strided((n, H, W, 128), _strides((n, H, W, 128), 136))
            val, cv = kg.guarded((n, OH, OW, 3), torch.float32, DEV)
            conf, cc = kg.guarded((n * OH, OW), torch.float32, DEV)
            p = L.DptTailParams()
            p.x, p.ldx, p.w1, p.ldw1, p.w2, p.b2, p.val, p.conf = L.ptr(xd), ldx, L.ptr(v[1].to(DEV)), 1152, L.ptr(v[3].to(DEV)), L.ptr(v[4].to(DEV)), L.ptr(val), L.ptr(conf)
            p.n_img, p.H, p.W, p.OH, p.OW, p.C, p.out_dim, p.activation, p.dtype = n, H, W, OH, OW, 128, 4, 1, L.OVG_BF16
            _refused(lambda: L.call("ovg_dpt_tail", p, torch.cuda.current_stream().cuda_stream), "dpt_tail at H W ldx = %d >= 2^31" % (H * W * ldx))
            torch.cuda.synchronize()
            cv("refused val")
            cc("refused conf")
            assert bool((cv.buffer == kg.GUARD_BYTE).all()) and bool((cc.buffer == kg.GUARD_BYTE).all()), "a refused ovg_dpt_tail wrote its outputs"


_CAM = {}


def _camera_weights(mode):
    if not _CAM:
        heads = importlib.import_module("omnivggt_official_amd.heads")
        heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")
        torch.manual_seed(21)
        _CAM["hip"] = heads_hip.HipCameraHead(heads.CameraHead(dim_in=2048).eval().to(DEV))
    if mode not in _CAM:
        with torch.no_grad():
            W = dict(_CAM["hip"]._pack(MODES[mode], torch.device(DEV)))
        W["blocks"] = W["blocks"][:1]                      # one trunk block, one round: the tokens are read by the first stage alone
        _CAM[mode] = W
    return _CAM[mode]


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_camera_head_tokens_16_mib_per_row_apart(mode):
    """ld_tokens of ovg_camera_head: 513 camera tokens 16 MiB + 64 B apart. The tokens are read by the first stage only (token LayerNorm ->
    the workspace's `tok`): that stage is gated per element on the twin (kernel_guards.check_camera_stages' gate of it), and the pose of
    the far call must equal the twin's bit for bit."""
    case = ar.CASES["camera_head.%s.tokens" % mode]
    S, dt = case.arg["S"], MODES[mode]
    W = _camera_weights(mode)
    toks = kg.camera_tokens(S, 1000 + S)

    def build(pl):
        out, chk = kg.guarded((S, 9), torch.float32, DEV)
        ws, cw = kg.guarded((1, ops.camera_head_workspace_bytes(S, dt)), torch.uint8, DEV)
        pl.checks += [chk, cw]
        ops.camera_head(pl.inp("tokens", toks), W, dt, iters=1, ws=ws.view(-1), out=out.view(1, S, 9))
        torch.cuda.synchronize()
        return {"out": out, "tok": kg.camera_ws_views(ws.view(-1), S, dt)["tok"]}

    t = _stride(case, build)
    assert bool(torch.isfinite(t["out"]).all())
    _ln_gate(case.name + ".tok", _val(t["tok"]), toks, W["token_norm_w"].cpu(), W["token_norm_b"].cpu(), 1e-5, kg.U_OUT["f32"])


# =============================================================================================
# ovg_block_forward
# =============================================================================================
class _Knobs:
    def __init__(self, mode, tile):
        self.gemm_tile, self.attn_variant, self.attn_kv_splits, self.attn_cus = tile, ATTN_VARIANT[mode], 1, 0


_BLOCK = {}


def _block_runner(mode, tile):
    """-> (aggregator.BlockRunner with forced tile / attention kernel, float64 values of its weights, rope tables)."""
    if mode not in _BLOCK:
        from omnivggt_official_amd import aggregator as agg
        cos, sin = br.rope_tables()
        r = agg.BlockRunner({"blk." + k: v for k, v in br.draw_weights().items()}, "blk", MODES[mode], DEV, qk_norm=True, rope=True, ln_eps=1e-5,
                            rope_tables=(cos[:, :16].contiguous().to(DEV), sin[:, :16].contiguous().to(DEV)))
        _BLOCK.clear()                                     # one mode's weights at a time
        _BLOCK[mode] = (r, {k: _val(t) for k, t in r.tensors.items()}, (cos, sin))
    r, wv, rope = _BLOCK[mode]
    r.knobs = _Knobs(mode, tile)
    return r, wv, rope


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_block_forward_residual_stream_16_mib_per_row_apart(mode):
    """ld_in, then ld_out, of ovg_block_forward: one sequence of 513 tokens; forced 128 tile and attention kernel. The twin is gated against
    the float64 block (block_reference) at block_reference.GATE, the gate of test_gpu_block_entries."""
    from omnivggt_official_amd import aggregator as agg
    ref = None
    for case in _cases("block_forward.%s." % mode):
        a = case.arg
        M, seq, tpv, gw = a["M"], a["seq"], a["tpv"], a["gw"]
        r, wv, rope = _block_runner(mode, L.TILE_128)
        x = torch.randn(M, 1024, generator=_gen("block_forward." + mode))

        def build(pl):
            ws = agg.Workspace(M, seq, MODES[mode], DEV)
            out = pl.out("x_out", (M, 1024), torch.float32)
            L.call("ovg_block_forward", r.params(ws, pl.inp("x_in", x), out, tokens_per_view=tpv, grid_w=gw), torch.cuda.current_stream().cuda_stream)
            return {"x_out": out}

        got = _val(_stride(case, build)["x_out"])
        ref = br.block_reference(x, wv, seq, tpv, gw, rope) if ref is None else ref
        assert st.report(case.name, got, ref, br.GATE[mode]), case.name


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_block_forward_hidden_activation_past_2_gib(mode):
    """The product-reachable case: Workspace.hid [M, 4096] passes 2 GiB at M = 262144 + 128 tokens in the 16-bit modes and 131072 + 128 in
    f32 (frame layout, 64 tokens per frame). Frames are periodic with period 1031: every output frame must equal frame f mod 1031 bit for
    bit (forced 256 / 128 tile and attention kernel: the same kernels at any row count), and the first eight frames are gated against the
    float64 block -- attention is per frame, so their reference needs no other frame."""
    from omnivggt_official_amd import aggregator as agg
    case = ar.CASES["block_forward.count.%s" % mode]
    _need(case)
    a = case.arg
    M, seq, gw = a["M"], a["seq"], a["gw"]
    r, wv, rope = _block_runner(mode, L.TILE_128 if mode == "f32" else L.TILE_256)
    base = torch.randn(P * seq, 1024, generator=_gen(case.name))
    x = ar.tile_periodic(base.to(DEV).view(P, seq * 1024), M // seq).view(M, 1024)
    # the far tensor is ws_hid: it sits in a guard band of its own (the Workspace takes its LN / attention / hidden scratch from `share`)
    class _Scratch:
        pass
    share = _Scratch()
    share.xn, share.attn = (torch.empty(M, 1024, dtype=STORE[mode], device=DEV) for _ in range(2))
    share.hid, chk_hid = kg.guarded_chunked((M, 4096), STORE[mode], DEV)
    ws = agg.Workspace(M, seq, MODES[mode], DEV, share=share)
    assert ws.hid is share.hid and ws.hid.numel() * ws.hid.element_size() == case.operands["hid"].bytes >= (1 << 31)
    out, chk = kg.guarded_chunked((M, 1024), torch.float32, DEV)
    L.call("ovg_block_forward", r.params(ws, x, out, tokens_per_view=seq, grid_w=gw), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    chk(case.name)
    chk_hid(case.name + " ws_hid")
    _periodic(case.name, out.view(M // seq, seq * 1024))
    _periodic(case.name + ".hid", ws.hid.view(M // seq, seq * 4096))
    ref = br.block_reference(base[:8 * seq], wv, seq, seq, gw, rope)
    assert st.report(case.name + ".twin", _val(out[:8 * seq]), ref, br.GATE[mode]), case.name


def test_operands_that_are_not_run_are_listed():
    for what, why, nbytes in ar.NOT_RUN:
        assert nbytes > ar.TENSOR_CAP or "the issue" in why, what
        print("not run: %s -- %s (%.1f GiB)" % (what, why, nbytes / ar.GIB), flush=True)
