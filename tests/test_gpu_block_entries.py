"""-m gpu: the three block entries the model calls -- ovg_block_forward, ovg_block_attn_prologue, ovg_block_attn_epilogue -- as compositions.
test_gpu_edges.py budgets every kernel under them per element against float64; here the entries are tied to those kernels bit for bit and
run inside the buffers their contract promises:

 1. ovg_block_forward == the seven entries it sequences, called one by one through ops (x_out and all six workspace tensors torch.equal)
 2. prologue(0) + epilogue == forward; prologue(1) then prologue(2) == prologue(0), and part 1 leaves q alone; skip_attention on a copied
    ws_attn == forward
 3. x_in / x_out as the two halves of a [M, 2048] buffer (both directions) and x_out aliasing x_in (strided and dense) == the dense
    out-of-place run; the half that is not written and a spare row keep their poison
 4. every workspace tensor (each plane in the split-f16 mode) and the split-KV buffers sit in guard bands at EXACTLY the byte counts of
    ops.block_workspace_bytes / ops.attn_plan -- in every test of this module; aggregator.Workspace allocates those sizes; poison in the
    q / k rows beyond seq and the dead V^T columns changes no bit of x_out and is not overwritten
 5. extra K / V^T segments (nseg_extra 1, 2, 7; 1 / 63 / 64 / 65 keys; the block's own keys first, in the middle, last) == the chain of
    (1) with ops.flash_attn over the same segment order, and in the f32 / split-f16 modes the float64 reference over the concatenated
    keys; bad arguments are refused by all three entries before anything is launched (the buffers keep their pattern)
 6. the whole block against a float64 reference (tests/block_reference.py, pinned to the oracle by test_block_reference_host.py) at
    gpu_selftest.test_block's gates; LayerScale gammas of order 1, inject every seq rows (frame) / every row and every M + 1 rows (global).
    Measured maxima of max|got - ref| / max|ref|: f32 1.2e-6, f32x 4.1e-7 (gate 5e-5), bf16 1.3e-3 (3e-2), f16 1.4e-4 (6e-3)

Shapes (tokens_per_view, grid_w): (6, 1), (25, 5), (64, 10), (65, 10), (129, 31); frame mode with 1 and 3 views, global mode with the 3 views
as one sequence (18, 75, 192, 195, 387 keys). Trimmed for time: f16 and f32x run the three largest shapes only (bf16 and f32 run all five);
the extra-segment test runs the global sequences of 75 and 195 rows. (1) carries the per-element claim for the 16-bit modes: (6) has no
per-element budget there, intermediates are rounded to 16 bits at every store (as test_gpu_edges says of the camera head).

Finding (read from csrc/ovg_block.hip): ovg_block_forward / ovg_block_attn_prologue launched LN1 before ovg_qkv refused nq_pad < seq or
nk_pad % 64, and forward ran LN1 + QKV before ovg_flash_attn refused an unusable extra[] segment: check_block looked at neither. It now
refuses what ovg_block_workspace_bytes refuses, and such a segment, up front."""
import pytest
import torch

import block_reference as br
import gpu_selftest as st
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}
STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": torch.float16}
ALL = ["bf16", "f16", "f32", "f32x"]
ENTRIES = ("ovg_block_forward", "ovg_block_attn_prologue", "ovg_block_attn_epilogue")
WS_NAMES = ("xn", "attn", "hid", "q", "k", "vt")


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    st.results.clear()
    yield
    kg.STATS.setdefault("global_only", 0)
    print("guards: %(guarded_launches)d guarded launches, %(numeric)d numeric checks (+ %(global_only)d with the global gate alone), "
          "%(refusals)d refusals" % kg.STATS, flush=True)
    torch.cuda.empty_cache()


def _global(name, got, ref, tol):
    assert st.report(name, got.detach().double().cpu(), ref, tol), name
    kg.STATS["global_only"] = kg.STATS.get("global_only", 0) + 1


def _refused(fn, what):
    with pytest.raises(L.OvgError, match="ARG|UNSUPPORTED"):
        fn()
    kg.STATS["refusals"] += 1
    print("[REFUSED] %s" % what, flush=True)


def _val(t):
    return (t.hi.double() + t.lo.double()).cpu() if isinstance(t, ops.HiLo) else t.double().cpu()


def _planes(t):
    return [t.hi, t.lo] if isinstance(t, ops.HiLo) else [t]


class Knobs:
    def __init__(self, gemm_tile=L.TILE_AUTO, attn_variant=0, attn_kv_splits=0, attn_cus=0):
        self.gemm_tile, self.attn_variant, self.attn_kv_splits, self.attn_cus = gemm_tile, attn_variant, attn_kv_splits, attn_cus

    def __repr__(self):
        return "tile%d_v%d_s%d" % (self.gemm_tile, self.attn_variant, self.attn_kv_splits)


def _knob_sets(mode, seq):
    ks = [Knobs()]
    if mode != "f32":
        ks.append(Knobs(gemm_tile=L.TILE_256))
    if mode in ("bf16", "f16"):
        ks.append(Knobs(attn_variant=1))
        if seq > 64:                                   # two key tiles: a forced split has something to cut
            ks.append(Knobs(attn_kv_splits=2))
    return ks


_W = {}


def _runner(mode):
    """-> (aggregator.BlockRunner holding the device weights of `mode`, {name: float64 CPU value of what the device holds}, rope (cos, sin))."""
    if mode not in _W:
        from omnivggt_official_amd import aggregator as agg
        keys = {"blk." + k: v for k, v in br.draw_weights().items()}
        cos, sin = br.rope_tables()
        tables = (cos[:, :16].contiguous().to(DEV), sin[:, :16].contiguous().to(DEV))
        r = agg.BlockRunner(keys, "blk", MODES[mode], DEV, qk_norm=True, rope=True, ln_eps=1e-5, rope_tables=tables, knobs=Knobs())
        _W[mode] = (r, {k: _val(t) for k, t in r.tensors.items()}, (cos, sin))
    return _W[mode]


def _cases(mode, layouts=("frame", "global")):
    """(layout, tokens_per_view, grid_w, M, seq)"""
    for tpv, gw in (br.SHAPES if mode in ("bf16", "f32") else br.SHAPES[-3:]):
        if "frame" in layouts:
            for views in (1, 3):
                yield "frame", tpv, gw, views * tpv, tpv
        if "global" in layouts:
            yield "global", tpv, gw, 3 * tpv, 3 * tpv


class WS:
    """The six scratch tensors of one block call (each plane in the split-f16 mode) and its split-KV buffers, every one inside its own
    guard band at exactly the byte count the library's queries report. xn / attn / hid start as poison; q / k / V^T as zeros with (poison=True)
    poison in the rows beyond seq and the dead V^T columns. Quacks like aggregator.Workspace for BlockRunner.params."""

    def __init__(self, mode, M, seq, poison=True):
        self.mode, self.M, self.seq, self.dtype = mode, M, seq, MODES[mode]
        self.BH, self.npad = (M // seq) * 16, ops.pad_to(seq, ops.KV_TILE)
        self.bytes = ops.block_workspace_bytes(M, seq, self.dtype)
        self.nks = [seq]                                  # the key counts the attention launch will see (extra segments: set by the test)
        shapes = {"xn": (M, 1024), "attn": (M, 1024), "hid": (M, 4096), "q": (self.BH, self.npad, 64), "k": (self.BH, self.npad, 64),
                  "vt": (self.BH, 64, self.npad)}
        self.checks, self._split = [], {}
        sdt = STORE[mode]
        for name in WS_NAMES:
            planes = []
            for _ in range(2 if mode == "f32x" else 1):
                v, c = kg.guarded(shapes[name], sdt, DEV)
                assert v.numel() * v.element_size() == self.bytes[name], (name, v.shape, self.bytes)
                if name in ("xn", "attn", "hid"):
                    v.copy_(kg.poison_values(v.shape, sdt, DEV))
                else:
                    v.zero_()
                    if poison:
                        kg.poison_vt(v, seq, mode != "f32") if name == "vt" else kg.poison_rows(v, seq)
                planes.append(v)
                self.checks.append(c)
            setattr(self, name, ops.HiLo(tuple(planes)) if mode == "f32x" else planes[0])

    def split_ws(self, variant=0, kv_splits=0, cus=0):
        key = (variant, kv_splits, cus, tuple(self.nks))
        if key not in self._split:
            self._split[key] = ops.attn_split_ws(self.BH, self.seq, self.nks, self.dtype, ops.AttnKnobs(variant, kv_splits, cus, None), self.npad, DEV,
                                                 alloc=self._guarded_split)
        return self._split[key]

    def _guarded_split(self, plan, device):
        if plan["splits"] <= 1:
            return None, None
        a, ca = kg.guarded((1, plan["part_bytes"]), torch.uint8, device)
        b, cb = kg.guarded((1, plan["lse_bytes"] // 4), torch.float32, device)
        self.checks += [ca, cb]
        print("split-KV %s BH=%d nq=%d keys=%s: plan runs %d splits in %d + %d bytes" % (
            self.mode, self.BH, self.seq, self.nks, plan["splits"], plan["part_bytes"], plan["lse_bytes"]), flush=True)
        return a.view(-1), b.view(-1)

    def check(self, what):
        for i, c in enumerate(self.checks):
            c("%s workspace guard %d" % (what, i))

    def snapshot(self):
        return {n: [p.clone() for p in _planes(getattr(self, n))] for n in WS_NAMES}


def _same(a, b, what, names=WS_NAMES):
    for n in names:
        for i, (x, y) in enumerate(zip(a[n], b[n])):
            assert torch.equal(x, y), "%s: ws_%s%s differs" % (what, n, "_lo" if i else "")


def _xbuf(M, ld=1024):
    """A guarded f32 [M, 1024] view with row stride ld and one spare row."""
    return kg.guarded((M, 1024), torch.float32, DEV, ld=ld, spare_rows=1)


def _params(mode, ws, x_in, x_out, tpv, gw, knobs, inject=None, per=0):
    r = _runner(mode)[0]
    r.knobs = knobs
    return r.params(ws, x_in, x_out, inject, per, tokens_per_view=tpv, grid_w=gw)


def _call(entry, p):
    L.call(entry, p, torch.cuda.current_stream().cuda_stream)


def _parts(mode, ws, x_in, x_out, tpv, gw, knobs, inject=None, per=0, segments=None, local=0):
    """The seven entries ovg_block_forward sequences, one ops call each, nothing aliased: LN1 goes to a buffer of its own, the proj
    result to x_mid. -> (LN1 output, x_mid)."""
    r = _runner(mode)[0]
    t, dt, seq = r.tensors, MODES[mode], ws.seq
    xn1 = ops.layernorm(x_in, t["norm1.weight"], t["norm1.bias"], 1e-5, dt)
    ops.qkv(xn1, t["attn.qkv.weight"], t["attn.qkv.bias"], seq, dt, ws.q, ws.k, ws.vt,
            qk_norm=[t["attn.q_norm.weight"], t["attn.q_norm.bias"], t["attn.k_norm.weight"], t["attn.k_norm.bias"]], rope=r.rope_tables,
            tokens_per_view=tpv, grid_w=gw, tile=knobs.gemm_tile)
    segs = list(segments or [])
    segs.insert(local, (ws.k, ws.vt, seq))
    ak = ops.attn_knobs(knobs, dt)
    ops.flash_attn(ws.q, segs, seq, dt, out=ws.attn, variant=ak.variant, kv_splits=ak.kv_splits, split_ws=ws.split_ws(ak.variant, ak.kv_splits, ak.cus), cus=ak.cus)
    x_mid = torch.empty(ws.M, 1024, device=DEV)
    ops.linear(ws.attn, t["attn.proj.weight"], t["attn.proj.bias"], dt, epilogue=L.EPI_RES, out=x_mid, res=x_in, gamma=t["ls1.gamma"],
               tile=knobs.gemm_tile)
    ops.layernorm(x_mid, t["norm2.weight"], t["norm2.bias"], 1e-5, dt, out=ws.xn)
    ops.linear(ws.xn, t["mlp.fc1.weight"], t["mlp.fc1.bias"], dt, epilogue=L.EPI_GELU, out=ws.hid, tile=knobs.gemm_tile)
    ops.linear(ws.hid, t["mlp.fc2.weight"], t["mlp.fc2.bias"], dt, epilogue=L.EPI_RES, out=x_out, res=x_mid, gamma=t["ls2.gamma"],
               inject=inject, inj_period=per, tile=knobs.gemm_tile)
    return xn1, x_mid


def _inputs(M, seed, periods):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 1024, generator=g)
    inj = {per: torch.randn((M + per - 1) // per, 1024, generator=g) for per in periods}
    return x, inj


def _periods(layout, M, seq):
    return (seq,) if layout == "frame" else (1, M + 1)


def _forward(mode, M, seq, tpv, gw, x_dev, knobs=None, inject=None, per=0, poison=True, ws=None):
    """One guarded ovg_block_forward, dense and out of place -> (x_out clone, ws)."""
    ws = ws or WS(mode, M, seq, poison)
    out, chk = _xbuf(M)
    _call("ovg_block_forward", _params(mode, ws, x_dev, out, tpv, gw, knobs or Knobs(), inject, per))
    torch.cuda.synchronize()
    chk("x_out")
    ws.check("forward")
    return out.clone(), ws


# =============================================================================================
# 1. the composite equals its parts
# =============================================================================================
@pytest.mark.parametrize("mode", ALL)
def test_block_entries_forward_equals_its_seven_parts_bit_for_bit(mode):
    for layout, tpv, gw, M, seq in _cases(mode):
        x, injs = _inputs(M, 400 + M, _periods(layout, M, seq))
        xd = x.to(DEV)
        runs = [(k, _periods(layout, M, seq)[0]) for k in _knob_sets(mode, seq)]
        if layout == "global":
            runs.append((Knobs(), M + 1))
        for knobs, per in runs:
            tag = "%s %s M=%d seq=%d %r inj%d" % (mode, layout, M, seq, knobs, per)
            inj = injs[per].to(DEV)
            got, wa = _forward(mode, M, seq, tpv, gw, xd, knobs, inj, per)
            wb = WS(mode, M, seq)
            out, chk = _xbuf(M)
            _parts(mode, wb, xd, out, tpv, gw, knobs, inj, per)
            torch.cuda.synchronize()
            chk("x_out of the parts")
            wb.check("parts")
            assert torch.equal(got, out), "block %s: x_out differs from the chain of its parts" % tag
            _same(wa.snapshot(), wb.snapshot(), "block " + tag)
            kg.STATS["numeric"] += 1


# =============================================================================================
# 2. the split forms equal the whole
# =============================================================================================
@pytest.mark.parametrize("mode", ALL)
def test_block_entries_split_forms_equal_the_whole_bit_for_bit(mode):
    for layout, tpv, gw, M, seq in _cases(mode):
        per = _periods(layout, M, seq)[0]
        x, injs = _inputs(M, 500 + M, (per,))
        xd, inj = x.to(DEV), injs[per].to(DEV)
        tag = "%s %s M=%d seq=%d" % (mode, layout, M, seq)
        whole, ww = _forward(mode, M, seq, tpv, gw, xd, None, inj, per)
        whole_ws = ww.snapshot()

        # prologue(0), then the epilogue
        w0 = WS(mode, M, seq)
        out, chk = _xbuf(M)
        p = _params(mode, w0, xd, out, tpv, gw, Knobs(), inj, per)
        p.qkv_part = 0
        _call("ovg_block_attn_prologue", p)
        torch.cuda.synchronize()
        w0.check("prologue 0")
        after_pro = w0.snapshot()
        t = _runner(mode)[0].tensors
        xn1 = ops.layernorm(xd, t["norm1.weight"], t["norm1.bias"], 1e-5, MODES[mode])
        assert all(torch.equal(a, b) for a, b in zip(after_pro["xn"], _planes(xn1))), "prologue %s: ws_xn is not LN1(x_in)" % tag
        _same(after_pro, whole_ws, "prologue(0) vs forward " + tag, ("q", "k", "vt"))
        _call("ovg_block_attn_epilogue", p)
        torch.cuda.synchronize()
        chk("x_out")
        w0.check("epilogue")
        assert torch.equal(out, whole), "block %s: prologue(0) + epilogue differs from forward" % tag
        _same(w0.snapshot(), whole_ws, "prologue(0) + epilogue vs forward " + tag)

        # part 1 (LN1 + k, v), q untouched; then part 2 (q only, reads the ws_xn part 1 left)
        w12 = WS(mode, M, seq)
        q_before = [t.clone() for t in _planes(w12.q)]
        p = _params(mode, w12, xd, out, tpv, gw, Knobs(), inj, per)
        p.qkv_part = 1
        _call("ovg_block_attn_prologue", p)
        torch.cuda.synchronize()
        w12.check("prologue 1")
        assert all(torch.equal(a, b) for a, b in zip(_planes(w12.q), q_before)), "prologue(1) %s wrote q" % tag
        _same(w12.snapshot(), after_pro, "prologue(1) " + tag, ("xn", "k", "vt"))
        p.qkv_part = 2
        _call("ovg_block_attn_prologue", p)
        torch.cuda.synchronize()
        w12.check("prologue 2")
        _same(w12.snapshot(), after_pro, "prologue(1) then (2) vs prologue(0) " + tag, ("xn", "q", "k", "vt"))

        # the epilogue without attention, on a copy of the whole run's ws_attn; q / k / V^T are left as allocated (poisoned padding, zeros)
        ws_ = WS(mode, M, seq)
        for dst, src in zip(_planes(ws_.attn), whole_ws["attn"]):
            dst.copy_(src)
        out2, chk2 = _xbuf(M)
        p = _params(mode, ws_, xd, out2, tpv, gw, Knobs(), inj, per)
        p.skip_attention = 1
        _call("ovg_block_attn_epilogue", p)
        torch.cuda.synchronize()
        chk2("x_out")
        ws_.check("epilogue, skip_attention")
        assert torch.equal(out2, whole), "block %s: the epilogue with skip_attention differs from forward" % tag
        _same(ws_.snapshot(), whole_ws, "skip_attention vs forward " + tag, ("xn", "attn", "hid"))
        kg.STATS["numeric"] += 4


# =============================================================================================
# 3. aliasing and strides
# =============================================================================================
@pytest.mark.parametrize("mode", ALL)
def test_block_entries_concat_halves_and_in_place_equal_the_dense_run(mode):
    for layout, tpv, gw, M, seq in _cases(mode):
        per = _periods(layout, M, seq)[0]
        x, injs = _inputs(M, 600 + M, (per,))
        xd, inj = x.to(DEV), injs[per].to(DEV)
        dense, wd = _forward(mode, M, seq, tpv, gw, xd, None, inj, per)
        dense_ws = wd.snapshot()
        for form in ("left to right", "right to left", "in place, ld 2048", "in place, dense"):
            tag = "%s %s M=%d seq=%d %s" % (mode, layout, M, seq, form)
            width = 1024 if form == "in place, dense" else 2048
            big, chk = kg.guarded((M + 1, width), torch.float32, DEV)
            big.copy_(kg.poison_values((M + 1, width), torch.float32, DEV))
            src = 1024 if form == "right to left" else 0
            dst = src if form.startswith("in place") else 1024 - src
            big[:M, src:src + 1024] = xd
            before = big.clone()
            ws = WS(mode, M, seq)
            _call("ovg_block_forward", _params(mode, ws, big[:M, src:src + 1024], big[:M, dst:dst + 1024], tpv, gw, Knobs(), inj, per))
            torch.cuda.synchronize()
            chk("concat buffer")
            ws.check(form)
            assert torch.equal(big[:M, dst:dst + 1024], dense), "block %s: differs from the dense out-of-place run" % tag
            _same(ws.snapshot(), dense_ws, "block " + tag)
            assert torch.equal(big[M], before[M]), "block %s: the spare row was written" % tag
            if width == 2048:
                other = 1024 - dst
                assert torch.equal(big[:M, other:other + 1024], before[:M, other:other + 1024]), "block %s: the other half was written" % tag
            kg.STATS["numeric"] += 1


# =============================================================================================
# 4. exact-size workspaces, poisoned padding
# =============================================================================================
@pytest.mark.parametrize("mode", ALL)
def test_block_entries_exact_size_workspaces_and_poisoned_padding(mode):
    from omnivggt_official_amd import aggregator as agg
    for layout, tpv, gw, M, seq in _cases(mode):
        tag = "%s %s M=%d seq=%d" % (mode, layout, M, seq)
        by = ops.block_workspace_bytes(M, seq, MODES[mode])
        # what the model allocates: every tensor (plane) of aggregator.Workspace has the queried size, and they add up to `total`
        aw = agg.Workspace(M, seq, MODES[mode], DEV)
        sizes = {n: [ops.nbytes(pl) for pl in _planes(getattr(aw, n))] for n in WS_NAMES}
        for n in WS_NAMES:
            assert len(sizes[n]) == (2 if mode == "f32x" else 1) and all(s == by[n] for s in sizes[n]), "Workspace %s: %s is %s bytes, the query says %d" % (tag, n, sizes[n], by[n])
        assert sum(sizes[n][0] for n in WS_NAMES) == by["total"], "Workspace %s: total" % tag
        del aw
        per = _periods(layout, M, seq)[0]
        x, injs = _inputs(M, 700 + M, (per,))
        xd, inj = x.to(DEV), injs[per].to(DEV)
        for knobs in _knob_sets(mode, seq):
            wp = WS(mode, M, seq, poison=True)                  # (WS asserts each view is exactly the queried size)
            before = wp.snapshot()
            got_p, _ = _forward(mode, M, seq, tpv, gw, xd, knobs, inj, per, ws=wp)
            got_z, wz = _forward(mode, M, seq, tpv, gw, xd, knobs, inj, per, poison=False)
            assert torch.equal(got_p, got_z), "block %s %r: x_out depends on the contents of the q / k / V^T padding" % (tag, knobs)
            after = wp.snapshot()
            key = (kg.vt_pos16(wp.npad) if mode != "f32" else torch.arange(wp.npad)).to(DEV)
            for n in ("q", "k"):
                for a, b in zip(after[n], before[n]):
                    assert torch.equal(a[:, seq:], b[:, seq:]), "block %s: the %s rows beyond seq were written" % (tag, n)
            for a, b in zip(after["vt"], before["vt"]):
                assert torch.equal(a[:, :, key >= seq], b[:, :, key >= seq]), "block %s: dead V^T columns were written" % tag
            zs = wz.snapshot()
            _same(after, zs, "block %s poisoned vs zero padding" % tag, ("xn", "attn", "hid"))
            for n in ("q", "k"):
                assert all(torch.equal(a[:, :seq], b[:, :seq]) for a, b in zip(after[n], zs[n])), "block %s: %s differs between paddings" % (tag, n)
            assert all(torch.equal(a[:, :, key < seq], b[:, :, key < seq]) for a, b in zip(after["vt"], zs["vt"])), "block %s: V^T differs between paddings" % tag
            kg.STATS["numeric"] += 1


# =============================================================================================
# 5. extra K / V^T segments
# =============================================================================================
def _extra_segments(mode, lens, g):
    """-> ([(k [16, nk_pad, 64], vt [16, 64, nk_pad], nk)] on the device, every other one with poisoned padding, [(k, v) float64 [16, nk, 64]])."""
    sdt, nplanes = STORE[mode], 2 if mode == "f32x" else 1
    dev, vals = [], []
    for i, nk in enumerate(lens):
        pad = ops.pad_to(nk, 64)
        pair = []
        for kind in ("k", "v"):
            v32 = torch.randn(16, nk, 64, generator=g)
            if mode == "f32x":
                h = ops.to_hilo(v32)
                planes, v64 = [h.hi, h.lo], h.hi.double() + h.lo.double()
            else:
                planes, v64 = [v32.to(sdt)], v32.to(sdt).double()
            bufs = []
            for pl in planes:
                if kind == "k":
                    b = torch.zeros(16, pad, 64, dtype=sdt, device=DEV)
                    b[:, :nk] = pl.to(DEV)
                    if i % 2 == 0:
                        kg.poison_rows(b, nk)
                else:
                    b = ops.set_vt(torch.zeros(16, 64, pad, dtype=sdt, device=DEV), pl.transpose(1, 2))
                    if i % 2 == 0:
                        kg.poison_vt(b, nk, mode != "f32")
                bufs.append(b)
            pair.append((ops.HiLo(tuple(bufs)) if nplanes == 2 else bufs[0], v64))
        dev.append((pair[0][0], pair[1][0], nk))
        vals.append((pair[0][1], pair[1][1]))
    return dev, vals


@pytest.mark.parametrize("mode", ALL)
def test_block_entries_extra_kv_segments(mode):
    _, wvals, rope = _runner(mode)
    lens_all = (1, 63, 64, 65, 1, 63, 64)
    for tpv, gw in ((25, 5), (65, 10)):
        M = seq = 3 * tpv
        x, _ = _inputs(M, 800 + M, ())
        xd = x.to(DEV)
        for nseg in (1, 2, 7):
            segs, svals = _extra_segments(mode, lens_all[:nseg], torch.Generator().manual_seed(900 + nseg))
            outs = {}
            for local in sorted({0, (nseg + 1) // 2, nseg}):
                tag = "%s M=%d extra=%s local=%d" % (mode, M, list(lens_all[:nseg]), local)
                nks = [s[2] for s in segs]
                nks.insert(local, seq)
                wa, wb = WS(mode, M, seq), WS(mode, M, seq)
                wa.nks = wb.nks = nks
                out, chk = _xbuf(M)
                p = ops.block_extra_segments(_params(mode, wa, xd, out, tpv, gw, Knobs()), segs, local)
                _call("ovg_block_forward", p)
                out_b, chk_b = _xbuf(M)
                _parts(mode, wb, xd, out_b, tpv, gw, Knobs(), segments=segs, local=local)
                torch.cuda.synchronize()
                chk("x_out")
                chk_b("x_out of the parts")
                wa.check("forward with extra segments")
                wb.check("parts with extra segments")
                assert torch.equal(out, out_b), "block %s: x_out differs from the chain of its parts over the same segments" % tag
                _same(wa.snapshot(), wb.snapshot(), "block " + tag)
                kg.STATS["numeric"] += 1
                outs[local] = out.clone()
                if mode in ("f32", "f32x"):
                    ref = br.block_reference(x, wvals, seq, tpv, gw, rope, segments=svals, local_seg_index=local)
                    _global("block_extra_%s_M%d_n%d_local%d" % (mode, M, nseg, local), out, ref, br.GATE[mode])
            if mode == "f32":       # attention is order-free in exact arithmetic: own keys first and last agree to the f32 gate (not bit for bit)
                _global("block_extra_f32_M%d_n%d_last_vs_first" % (M, nseg), outs[nseg], outs[0].double().cpu(), br.GATE["f32"])


class _Loose:
    """Plain (unguarded) buffers for calls that must be refused: sized for twice the heads and one more key tile than the valid call,
    so that not even an unrefused call would leave them; filled with a pattern that must survive."""

    def __init__(self, mode, M, seq):
        self.M, self.seq, self.BH, self.dtype = M, seq, (M // seq) * 16, MODES[mode]
        rows = ops.pad_to(seq, 64) + 64
        sdt, n = STORE[mode], 2 if mode == "f32x" else 1
        self.tensors = []

        def mk(*shape):
            pl = [kg.poison_values(shape, sdt, DEV) for _ in range(n)]
            self.tensors += pl
            return ops.HiLo(tuple(pl)) if n == 2 else pl[0]
        self.xn, self.attn, self.hid = mk(M, 1024), mk(M, 1024), mk(M, 4096)
        self.full = {"q": mk(2 * self.BH, rows, 64), "k": mk(2 * self.BH, rows, 64), "vt": mk(2 * self.BH, 64, rows)}
        npad = ops.pad_to(seq, 64)                      # BlockRunner.params reads nq_pad / nk_pad from the shapes: views shaped like the valid call's

        def head(t, vt):
            pl = [u[: self.BH, :, :npad] if vt else u[: self.BH, :npad] for u in _planes(t)]
            return ops.HiLo(tuple(pl)) if n == 2 else pl[0]
        self.q, self.k, self.vt = head(self.full["q"], False), head(self.full["k"], False), head(self.full["vt"], True)
        self.x_out = kg.poison_values((M, 1024), torch.float32, DEV)
        self.tensors.append(self.x_out)
        self.before = [t.clone() for t in self.tensors]

    def untouched(self):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(self.tensors, self.before))


@pytest.mark.parametrize("mode", ALL)
def test_block_entries_refuse_bad_arguments_before_any_launch(mode):
    """Every entry answers OVG_E_ARG to each bad argument, and nothing was launched on the way to the refusal: xn, attn, hid, q, k, V^T and
    x_out keep their pattern. (The _Loose views pass pointers only: the q / k / V^T rows the entries assume come from nq_pad / nk_pad.)"""
    tpv, gw = 25, 5
    M = seq = 75
    ws = _Loose(mode, M, seq)
    xd = torch.randn(M, 1024, generator=torch.Generator().manual_seed(5)).to(DEV)
    segs, _ = _extra_segments(mode, (64,) * L.OVG_MAX_SEG, torch.Generator().manual_seed(6))

    def fresh():
        p = _params(mode, ws, xd, ws.x_out, tpv, gw, Knobs())
        assert (p.nq_pad, p.nk_pad, p.BH) == (128, 128, 16)
        return p

    def bad(what, change, entries=ENTRIES):
        for entry in entries:
            p = fresh()
            change(p)
            _refused(lambda: _call(entry, p), "%s %s: %s" % (entry, mode, what))
        assert ws.untouched(), "%s: something was launched before the refusal" % what

    bad("nseg_extra = OVG_MAX_SEG", lambda p: ops.block_extra_segments(p, segs, 0))
    bad("local_seg_index > nseg_extra", lambda p: ops.block_extra_segments(p, segs[:1], 2))
    bad("M % seq != 0", lambda p: setattr(p, "seq", 74))
    bad("BH off by 16", lambda p: setattr(p, "BH", 32))
    bad("nq_pad < seq", lambda p: setattr(p, "nq_pad", 64))
    bad("nk_pad % 64 != 0", lambda p: setattr(p, "nk_pad", 160))
    bad("nk_pad < seq", lambda p: setattr(p, "nk_pad", 64))
    bad("an extra segment without keys", lambda p: setattr(ops.block_extra_segments(p, segs[:2], 1).extra[1], "k", None), ENTRIES[::2])
    bad("an extra segment with nk_pad % 64 != 0", lambda p: setattr(ops.block_extra_segments(p, segs[:1], 0).extra[0], "nk_pad", 96), ENTRIES[::2])
    if mode == "f32x":
        bad("ws_q_lo missing", lambda p: setattr(p, "ws_q_lo", None))
        bad("ws_hid_lo missing", lambda p: setattr(p, "ws_hid_lo", None))
        bad("extra[0].k_lo missing", lambda p: setattr(ops.block_extra_segments(p, segs[:1], 1).extra[0], "k_lo", None), ENTRIES[::2])
    else:
        print("(%s has no _lo planes: the missing-plane refusals run in the f32x case)" % mode, flush=True)
    # the same parameters unchanged are a valid call (so the refusals above are about the one changed field)
    _call("ovg_block_forward", ops.block_extra_segments(fresh(), segs[:7], 3))
    assert not ws.untouched()


# =============================================================================================
# 6. the whole block against float64
# =============================================================================================
@pytest.mark.parametrize("layout", ["frame", "global"])
@pytest.mark.parametrize("mode", ALL)
def test_block_entries_whole_block_against_float64(mode, layout):
    _, wvals, rope = _runner(mode)
    worst = 0.0
    for _, tpv, gw, M, seq in _cases(mode, (layout,)):
        periods = _periods(layout, M, seq)
        x, injs = _inputs(M, 1000 + M, periods)
        xd = x.to(DEV)
        base = br.block_reference(x, wvals, seq, tpv, gw, rope)
        for per in periods:
            got, _ = _forward(mode, M, seq, tpv, gw, xd, None, injs[per].to(DEV), per)
            _global("block_%s_%s_M%d_seq%d_inj%d" % (mode, layout, M, seq, per), got, base + br.inject_rows(M, injs[per], per), br.GATE[mode])
            worst = max(worst, st.results[-1]["rel"])
    print("block entries %s %s: largest max|got - ref| / max|ref| over the shapes %.3e (gate %.1e)" % (mode, layout, worst, br.GATE[mode]), flush=True)
