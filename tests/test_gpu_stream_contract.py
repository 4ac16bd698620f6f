"""-m gpu: every entry of include/omnivggt_hip.h held to the header's stream and no-sync contract by the gated run of stream_contract.py:
behind a blocker on a side stream S the entry is called with S as its stream on buffers that until then held decoy inputs and stale
outputs; it must return while the blocker still runs (no synchronise, no blocking copy), allocate and free nothing, and leave exactly the
bytes of its default-stream run on the real inputs -- which a stage queued on any other stream cannot, it runs early, on the decoys or on
workspace that is refilled afterwards.

The four self-checks plant a fault each (torch operations only) and require the protocol to report it; the concurrency control picks a side
stream that really runs next to the null stream. test_every_entry_of_the_header_is_gated parses the header and asserts that the set of
entries the families below reached equals the declared set minus the commented exclusions, so a new entry cannot go untested.

Every entry below is gated on BYTES: each is deterministic by its own family's tests ("two runs: identical bytes", fixed reduction orders,
integer atomics). No entry is documented to synchronise, so none is exempt from `early`.

Cases are the smallest of the family's own GPU test that still take every launch path of the entry; decoys are the other seed, or the same
cloud reversed and shifted: always valid data of the same kind.
"""
import contextlib
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aggregator_oracle as orc
import block_reference as br
import kernel_guards as kg
import stream_contract as sc
import tsdf_twin
from omnivggt_official_amd import lib as L, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnivggt_hip.h")

# entries that take a stream but are not gated here, each with its reason
EXCLUDED = {
    "ovg_probe_mfma": "a one-wave hardware probe of the MFMA lane layout (tools, gpu_selftest): no parameter struct, not part of the model path",
}
# nothing in the header needs more than one GPU: the sharded path reaches the same single-GPU entries from sharding.py

COVERED = {}          # entry name -> [case names], filled by the family tests, read by the coverage test (which runs last in this file)


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device fault is sticky: start nothing more on this GPU
        pytest.exit("the device reported %s; stopping the session" % e, returncode=3)
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def raw(name, p):
    L.call(name, p, _stream())


def capture(fn):
    """Run an ops wrapper once (default stream) and hand back the parameter struct it built, for entries whose wrapper allocates its
    outputs: the test then points the struct's outputs / workspace at guarded buffers and calls the raw entry. -> (entry name, struct)."""
    got = []
    orig = L.call

    def call(name, params, stream):
        got.append((name, params))
        return orig(name, params, stream)
    L.call = call
    try:
        fn()
    finally:
        L.call = orig
    torch.cuda.synchronize()
    assert len(got) == 1, [n for n, _ in got]
    return got[0]


def family(builders, tag):
    cases = sc.run_family(builders)
    for c in cases:
        for e in c.entries:
            COVERED.setdefault(e, []).append(c.name)
    print("%s: %d gated cases, entries %s" % (tag, len(cases), sorted({e for c in cases for e in c.entries})), flush=True)
    return cases


def cloud(n, seed, scale=1.0):
    return (torch.rand(n, 3, generator=_gen(seed)) - 0.5) * scale


def shifted(t, by=0.03):
    """The same cloud reversed and translated."""
    return t.flip(-2) + by


# =============================================================================================
# the method must not pass silently
# =============================================================================================
def _toy(name="toy"):
    """A stand-in entry made of torch operations: y = 2 x + 1 on the current stream."""
    c = sc.Case(name)
    x = c.inp(torch.randn(257, 64, generator=_gen(1)))
    y = c.out((257, 64), F32)

    def good():
        torch.mul(x, 2.0, out=y)
        y.add_(1.0)
    c.call = good
    return c, x, y


def test_self_check_blocker_is_calibrated_and_a_side_stream_runs_concurrently():
    g = sc.Gate.get()
    print("calibrated blocker: %d cycles = %.1f ms; concurrency control settled on fresh stream %d" % (g.cycles, g.block_ms, g.stream_index), flush=True)
    for line in g.concurrency_log:
        print("  " + line, flush=True)
    assert g.block_ms >= sc.MIN_BLOCK_MS
    g.require_stream()
    ok, msg = g.concurrent(g.stream)               # once more, on the stream the tests will use
    assert ok, msg


def test_self_check_a_correct_stand_in_passes():
    c, _, _ = _toy()
    sc.setup_case(c)
    r = sc.gated_group([c], check_stream_handle=False)[0]
    assert r.faults() == [], r.faults()


def test_self_check_wrong_stream_is_reported_as_a_byte_mismatch():
    c, x, y = _toy("toy on the default stream")

    def wrong():
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.mul(x, 2.0, out=y)
            y.add_(1.0)
    c.call = wrong
    sc.setup_case(c)
    r = sc.gated_group([c], check_stream_handle=False)[0]
    print("planted: work on the default stream -> %s" % r.faults(), flush=True)
    assert not r.bytes_equal and "bytes differ" in r.mismatch, r.faults()
    assert r.early and not (r.allocated or r.freed)
    with pytest.raises(sc.ContractError, match="bytes"):
        r.ok()


def test_self_check_host_block_is_reported_as_not_early():
    c, x, y = _toy("toy that synchronises")
    S = sc.Gate.get().require_stream()

    def blocking():
        torch.mul(x, 2.0, out=y)
        y.add_(1.0)
        if torch.cuda.current_stream() == S:
            S.synchronize()
    c.call = blocking
    sc.setup_case(c)
    r = sc.gated_group([c], check_stream_handle=False)[0]
    print("planted: a synchronise -> %s" % r.faults(), flush=True)
    assert r.early is False and r.bytes_equal, r.faults()
    with pytest.raises(sc.ContractError, match="early"):
        r.ok()


def test_self_check_allocation_is_reported():
    c, x, y = _toy("toy that allocates")
    keep = []

    def allocating():
        keep.append(torch.empty(1 << 20, device=DEV))
        torch.mul(x, 2.0, out=y)
        y.add_(1.0)
    c.call = allocating
    sc.setup_case(c)
    r = sc.gated_group([c], check_stream_handle=False)[0]
    print("planted: torch.empty inside the call -> %s" % r.faults(), flush=True)
    assert r.allocated >= 1 and r.bytes_equal and r.early, r.faults()
    with pytest.raises(sc.ContractError, match="allocation"):
        r.ok()


def test_self_check_a_decoy_that_changes_nothing_is_refused():
    c, x, y = _toy("toy with a dead decoy")
    c.decoy[0].copy_(c.real[0])
    with pytest.raises(sc.ContractError, match="cannot tell"):
        sc.setup_case(c)


# =============================================================================================
# element-wise
# =============================================================================================
def test_elementwise_entries_257_rows():
    rows = 257

    def layernorm():
        c = sc.Case("layernorm bf16 257 rows")
        x = c.inp(torch.randn(rows, 1024, generator=_gen(2)))
        w, b = c.const(torch.randn(1024, generator=_gen(3)) * 0.2 + 1), c.const(torch.randn(1024, generator=_gen(4)) * 0.1)
        y = c.out((rows, 1024), BF16, ld=1032)
        c.call = lambda: ops.layernorm(x, w, b, 1e-5, BF16, out=y)
        return c

    def head_layernorm():
        c = sc.Case("head_layernorm f16 257 rows")
        x = c.inp(torch.randn(rows + 5, 2048, generator=_gen(5)))
        w, b = c.const(torch.randn(2048, generator=_gen(6)) * 0.2 + 1), c.const(torch.randn(2048, generator=_gen(7)) * 0.1)
        y = c.out((rows, 2048), F16)
        c.call = lambda: ops.head_layernorm(x, w, b, 1e-5, F16, 1, tokens_per_view=rows + 5, out=y)
        return c

    def copy_rows():
        c = sc.Case("copy_rows 257 x 1020")
        x = c.inp(torch.randn(rows, 1020, generator=_gen(8)))
        y = c.out((rows, 1020), F32, ld=1032)
        c.call = lambda: ops.copy_rows(x, y)
        return c

    def im2col_rgb():
        c = sc.Case("im2col rgb bf16")
        img = c.inp(torch.rand(2, 3, 28, 42, generator=_gen(9)))
        out = c.out((12, 640), BF16)
        c.call = lambda: ops.im2col_rgb(img, BF16, out=out)
        return c

    def depth_stats_then_im2col_depth():
        c = sc.Case("depth_stats -> im2col depth f32")
        depth = c.inp(0.5 + 5 * torch.rand(2, 28, 42, generator=_gen(10)))
        mask = c.inp((torch.rand(2, 28, 42, generator=_gen(11)) > 0.2).float())
        stats = c.out((1, 2), torch.float64)
        partial = c.ws(1 * 256 * 2 * 8)
        out = c.out((12, 448), F32)
        p = L.DepthStatsParams(L.ptr(depth), L.ptr(mask), 1, 2 * 28 * 42, L.ptr(stats), L.ptr(partial), 256)

        def call():
            raw("ovg_depth_stats", p)
            ops.im2col_depth(depth, mask, stats, 2, F32, out=out)
        c.call = call
        return c

    def pack_weights():
        c = sc.Case("pack_weights f16 257 x 588 -> 640")
        w = c.inp(torch.randn(rows, 588, generator=_gen(12)))
        out = c.out((rows, 640), F16, ld=648)
        c.call = lambda: ops.pack_weights(w, F16, k_pad=640, out=out)
        return c

    def dino_specials():
        c = sc.Case("dino_specials 2 views of 130 tokens")
        x = c.inout(torch.randn(260, 1024, generator=_gen(13)))
        cls, pos0, reg = (c.inp(torch.randn(*s, generator=_gen(14 + i))) for i, s in enumerate(((1024,), (1024,), (4, 1024))))
        c.call = lambda: ops.dino_specials(x, 2, 130, cls, pos0, reg)
        return c

    def assemble_tokens():
        c = sc.Case("assemble_tokens 2 views of 133 tokens")
        P = 133
        xd = c.inp(torch.randn(2 * P, 1024, generator=_gen(20)))
        w, b = c.const(torch.randn(1024, generator=_gen(21)) * 0.1 + 1), c.const(torch.randn(1024, generator=_gen(22)) * 0.1)
        cam, regt, cam_add = c.inp(torch.randn(2, 1024, generator=_gen(23))), c.inp(torch.randn(2, 4, 1024, generator=_gen(24))), c.inp(torch.randn(2, 1024, generator=_gen(25)))
        dtok, ph = c.inp(torch.randn(P - 5, 1024, generator=_gen(26))), c.inp(torch.randn(1024, generator=_gen(27)))
        row = c.const(torch.tensor([-1, 0], dtype=torch.int32))
        out = c.out((2 * P, 1024), F32, ld=1032)
        c.call = lambda: ops.assemble_tokens(xd, w, b, 1e-6, cam, regt, cam_add, dtok, row, ph, out, 2, 2, tokens_per_view=P)
        return c

    def heads_to_tokens():
        c = sc.Case("heads_to_tokens bf16 257 rows")
        x = c.inp(torch.randn(16, 320, 64, generator=_gen(28)).to(BF16))
        out = c.out((rows, 1024), BF16, ld=1040)
        c.call = lambda: ops.heads_to_tokens(x, rows, BF16, out=out)
        return c

    family([layernorm, head_layernorm, copy_rows, im2col_rgb, depth_stats_then_im2col_depth, pack_weights, dino_specials, assemble_tokens,
            heads_to_tokens], "element-wise")


# =============================================================================================
# GEMM
# =============================================================================================
def _linear_case(tile, epi, N=256, dt=BF16):
    M, K = 300, 128
    name = {L.EPI_STORE: "STORE", L.EPI_GELU: "GELU", L.EPI_RES: "RES", L.EPI_PATCH: "PATCH"}[epi]

    def build():
        c = sc.Case("linear %s tile %d M=%d N=%d K=%d" % (name, tile, M, N, K))
        g = _gen(100 + 10 * tile + epi)
        x = c.inp(torch.randn(M, K, generator=g).to(dt))
        w = c.inp((torch.randn(N, K, generator=g) * K ** -0.5).to(dt))
        bias = c.const(torch.randn(N, generator=g) * 0.1)
        kw = {}
        if epi == L.EPI_RES:
            kw = dict(res=c.inp(torch.randn(M, N, generator=g)), gamma=c.const(torch.randn(N, generator=g)),
                      inject=c.inp(torch.randn(2, N, generator=g)), inj_period=150)
            y = c.out((M, N), F32, ld=N + 8)
        elif epi == L.EPI_PATCH:
            kw = dict(table=c.inp(torch.randn(151, N, generator=g)), p0=150, p1=155, row_off=5)
            y = c.out((310, N), F32)
        else:
            y = c.out((M, N), dt, ld=N + 8)
        c.call = lambda: ops.linear(x, w, bias, dt, epilogue=epi, out=y, tile=tile, **kw)
        return c
    return build


def test_gemm_linear_both_tiles_every_epilogue():
    builders = [_linear_case(tile, epi) for tile in (L.TILE_128, L.TILE_256) for epi in (L.EPI_STORE, L.EPI_GELU, L.EPI_RES, L.EPI_PATCH)]
    builders.append(_linear_case(L.TILE_256, L.EPI_STORE, N=1024, dt=F16))       # four column tiles of the 256 x 256 kernel
    family(builders, "ovg_linear")


def test_gemm_qkv_both_tiles_seq_129():
    seq, M = 129, 258
    cos, sin = br.rope_tables()

    def case(tile):
        def build():
            c = sc.Case("qkv bf16 tile %d seq %d" % (tile, seq))
            g = _gen(140 + tile)
            x = c.inp(torch.randn(M, 1024, generator=g).to(BF16))
            w = c.const((torch.randn(3072, 1024, generator=g) * 0.03).to(BF16))
            bias = c.const(torch.randn(3072, generator=g) * 0.1)
            norm = [c.const(torch.randn(64, generator=g) * 0.2 + 1) if i % 2 == 0 else c.const(torch.randn(64, generator=g) * 0.1) for i in range(4)]
            rope = (c.const(cos[:, :16]), c.const(sin[:, :16]))
            q, k, vt = c.out((32, 192, 64), BF16), c.out((32, 192, 64), BF16), c.out((32, 64, 192), BF16)
            c.call = lambda: ops.qkv(x, w, bias, seq, BF16, q, k, vt, qk_norm=norm, rope=rope, tokens_per_view=seq, grid_w=31, tile=tile)
            return c
        return build
    family([case(L.TILE_128), case(L.TILE_256)], "ovg_qkv")


# =============================================================================================
# attention
# =============================================================================================
def _attn_tensors(dt, BH, nq, nks, seed):
    g = _gen(seed)
    nq_pad = ops.pad_to(nq, 64)
    q = torch.zeros(BH, nq_pad, 64, dtype=dt)
    q[:, :nq] = (torch.randn(BH, nq, 64, generator=g) * 1.2).to(dt)
    segs = []
    for nk in nks:
        nk_pad = ops.pad_to(nk, 64)
        k = torch.zeros(BH, nk_pad, 64, dtype=dt)
        k[:, :nk] = torch.randn(BH, nk, 64, generator=g).to(dt)
        vt = ops.set_vt(torch.zeros(BH, 64, nk_pad, dtype=dt), torch.randn(BH, 64, nk, generator=g).to(dt))
        segs.append((k, vt, nk))
    return q, segs


def _attn_case(name, dt, nq, nks, variant=0, kv_splits=0, cus=0, split=False):
    def build():
        c = sc.Case("flash_attn %s nq=%d keys=%s" % (name, nq, nks))
        (qa, sa), (qb, sb) = _attn_tensors(dt, 16, nq, nks, 201), _attn_tensors(dt, 16, nq, nks, 202)
        q = c.inp(qa, qb)
        segs = [(c.inp(ka, kb), c.inp(va, vb), nk) for (ka, va, nk), (kb, vb, _) in zip(sa, sb)]
        out = c.out((nq, 1024), dt, ld=1032)
        lse = c.out((16, q.shape[1]), F32)
        ws = None
        if split:
            plan = ops.attn_plan(16, nq, nks, dt, variant, kv_splits, nq_pad=q.shape[1], cus=cus)
            assert plan["splits"] > 1, plan
            ws = (c.ws(plan["part_bytes"]), c.ws(plan["lse_bytes"]).view(F32))
        c.call = lambda: ops.flash_attn(q, segs, nq, dt, out=out, variant=variant, lse=lse, kv_splits=kv_splits, split_ws=ws, cus=cus)
        return c
    return build


def test_attention_kernels_split_and_merge():
    import test_gpu_edges as tge
    nq, var, splits, cus, _ = tge.SPLIT_FORMS["whole_launch"]

    def merge():
        c = sc.Case("attn_merge bf16 65 rows")
        g = _gen(210)
        a, b = c.inp(torch.randn(65, 1024, generator=g).to(BF16)), c.inp(torch.randn(65, 1024, generator=g).to(BF16))
        la, lb = c.inp(torch.randn(16, 128, generator=g) * 3), c.inp(torch.randn(16, 128, generator=g) * 3)
        out = c.out((65, 1024), BF16, ld=1040)
        c.call = lambda: ops.attn_merge(a, la, b, lb, BF16, out=out)
        return c

    family([_attn_case("baseline bf16", BF16, 65, [7, 129], variant=L.ATTN_BASELINE),
            _attn_case("default plan bf16", BF16, 65, [7, 129]),
            _attn_case("default plan f16", F16, 65, [7, 129]),
            _attn_case("LDS-DMA speculative 128 bf16", BF16, 65, [7, 129], variant=L.ATTN_SPEC128),
            _attn_case("baseline f32", F32, 65, [7, 129], variant=L.ATTN_BASELINE),
            _attn_case("forced split-KV x2 + merge launch bf16", BF16, 65, [7, 129], kv_splits=2, split=True),
            _attn_case("split form whole_launch bf16", BF16, nq, [nq], variant=var, kv_splits=splits, cus=cus, split=True),
            merge], "attention")


# =============================================================================================
# block entries
# =============================================================================================
def _block_case(mode, pair):
    import test_gpu_block_entries as tbe
    tpv, gw, M, seq = 1374, 37, 2748, 1374

    def build():
        c = sc.Case("block %s %s 2 views of 1374 tokens" % ("prologue + epilogue" if pair else "forward", mode))
        x = c.inp(torch.randn(M, 1024, generator=_gen(300)))
        inj = c.inp(torch.randn(2, 1024, generator=_gen(301)))
        ws = tbe.WS(mode, M, seq)
        out = c.out((M, 1024), F32)
        p = tbe._params(mode, ws, x, out, tpv, gw, tbe.Knobs(), inj, seq)
        p.qkv_part = 0
        for chk in ws.checks:                           # the six scratch tensors and the default plan's split-KV buffers, if it wants any
            c.checks.append(chk)
            c.bufs.append(chk.buffer)
        c.keep = (ws, p)

        def call():
            if pair:
                raw("ovg_block_attn_prologue", p)
                raw("ovg_block_attn_epilogue", p)
            else:
                raw("ovg_block_forward", p)
        c.call = call
        return c
    return build


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_block_forward_and_split_form(mode):
    family([_block_case(mode, False), _block_case(mode, True)], "block " + mode)


# =============================================================================================
# heads
# =============================================================================================
def _conv_case(H, W, cin):
    def build():
        c = sc.Case("conv 3x3 relu bf16 %dx%d (%d output pixels)" % (H, W, H * W))
        g = _gen(400 + H)
        x = c.inp(torch.randn(1, H, W, cin, generator=g).to(BF16))
        w = c.const((torch.randn(128, 9 * cin, generator=g) * (9 * cin) ** -0.5).to(BF16))
        bias = c.const(torch.randn(128, generator=g) * 0.3)
        y = c.out((1, H, W, 128), BF16, ld=136)
        c.call = lambda: ops.conv(x, w, bias, BF16, 128, ksize=3, relu=True, out=y)
        return c
    return build


def _dpt_tail_case(dt):
    def build():
        c = sc.Case("dpt_tail %s 5x4 -> 15x17" % dt)
        g = _gen(412)
        x = c.inp(torch.randn(2, 5, 4, 128, generator=g).to(dt))
        w1 = torch.zeros(128, 9 * 128, dtype=dt)
        w1[:32] = (torch.randn(32, 9 * 128, generator=g) * (9 * 128) ** -0.5).to(dt)
        w1, b1 = c.const(w1), c.const(torch.randn(32, generator=g) * 0.3)
        w2, b2 = c.const(torch.randn(2, 32, generator=g) * 0.2), c.const(torch.randn(2, generator=g) * 0.1)
        pos = (c.const(torch.randn(17, 64, generator=g) * 0.1), c.const(torch.randn(15, 64, generator=g) * 0.1))
        val, conf = c.out((2, 15, 17, 1), F32), c.out((2, 15, 17), F32)
        c.call = lambda: ops.dpt_tail(x, 15, 17, dt, pos, w1, b1, w2, b2, "exp", out=(val, conf))
        return c
    return build


def test_head_entries():
    def upsample():
        c = sc.Case("upsample bf16 5x4 -> 15x17 with position tables")
        g = _gen(410)
        x = c.inp(torch.randn(2, 5, 4, 64, generator=g).to(BF16))
        pos = (c.const(torch.randn(17, 32, generator=g) * 0.1), c.const(torch.randn(15, 32, generator=g) * 0.1))
        y = c.out((2, 15, 17, 64), BF16, ld=72)
        c.call = lambda: ops.upsample(x, 15, 17, BF16, pos=pos, out=y)
        return c

    def dpt_out():
        c = sc.Case("dpt_out inv_log 15x17")
        g = _gen(411)
        h = c.inp(F.relu(torch.randn(2, 15, 17, 32, generator=g)))
        w2, b2 = c.const(torch.randn(4, 32, generator=g) * 0.2), c.const(torch.randn(4, generator=g) * 0.1)
        val, conf = c.out((2, 15, 17, 3), F32), c.out((2, 15, 17), F32)
        c.call = lambda: ops.dpt_out(h, w2, b2, "inv_log", out=(val, conf))
        return c

    def unproject():
        c = sc.Case("unproject 2 frames of 15x17")
        g = _gen(413)
        depth = c.inp(0.5 + torch.rand(2, 15, 17, generator=g))
        cam = c.inp(torch.cat([torch.eye(3).reshape(1, 9).repeat(2, 1), torch.randn(2, 3, generator=g), torch.tensor([[20.0, 21.0, 8.0, 7.0], [18.0, 19.0, 8.5, 7.5]])], 1))
        out = c.out((2, 15, 17, 3), F32)
        p = L.UnprojectParams(L.ptr(depth), L.ptr(cam), L.ptr(out), 2, 15, 17)
        c.call = lambda: raw("ovg_unproject", p)
        return c

    def camera_tables():
        c = sc.Case("camera_tables B=1 S=3 cameras [0, 2]")
        g = _gen(414)
        G, S, hw = 2, 3, (392, 518)
        pw, pb = c.const(torch.randn(G * 1024, 9, generator=g) * 0.3), c.const(torch.randn(G * 1024, generator=g) * 0.1)
        aw, ab = c.const(torch.randn(G, 1024, 1024, generator=g) * 0.03), c.const(torch.randn(G, 1024, generator=g) * 0.1)
        a, b = orc.synthetic_inputs(S, seed=100, hw=hw), orc.synthetic_inputs(S, seed=101, hw=hw)
        ext, intr = c.inp(a["extrinsics"].float(), b["extrinsics"].float()), c.inp(a["intrinsics"].float(), b["intrinsics"].float())
        idx = c.const(torch.tensor([0, 2], dtype=torch.int32))
        _, p = capture(lambda: ops.camera_tables(ext, intr, idx, S, hw, pw, pb, aw, ab))
        assert p.extrinsics == ext.data_ptr() and p.intrinsics == intr.data_ptr()
        enc, emb, out = c.ws(2 * 9 * 4), c.ws(G * 2 * 1024 * 4), c.out((G, S, 1024), F32)
        p.enc, p.emb, p.tables = L.ptr(enc), L.ptr(emb), L.ptr(out)
        c.call = lambda: raw("ovg_camera_tables", p)
        return c

    family([_conv_case(3, 2, 128), _conv_case(128, 128, 64), upsample, dpt_out, _dpt_tail_case(BF16), _dpt_tail_case(F16), unproject, camera_tables], "heads")


def test_camera_head_two_views():
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
            elif "bias" in name:
                p.uniform_(-0.1, 0.1)
    hip = heads_hip.HipCameraHead(head.to(DEV))

    def case(dt):
        def build():
            c = sc.Case("camera_head %s S=2" % dt)
            with torch.no_grad():
                W = hip._weights(dt, torch.device(DEV))
            toks = c.inp(torch.randn(2, 2048, generator=_gen(420)) * 1.3)
            ws = c.ws(ops.camera_head_workspace_bytes(2, dt))
            out = c.out((4, 2, 9), F32)
            c.call = lambda: ops.camera_head(toks, W, dt, ws=ws, out=out)
            return c
        return build
    family([case(BF16), case(F32)], "camera head")


# =============================================================================================
# pre-processing
# =============================================================================================
def test_preprocess_two_frames_of_different_sizes():
    from omnivggt_official_amd import preprocess as P
    dev = torch.device("cuda", torch.cuda.current_device())
    kept = []

    class Keep(P._Staging):                              # the parameter struct points into the staging buffers: keep them alive
        def __init__(self, sizes):
            super().__init__(sizes)
            kept.append(self)

    @contextlib.contextmanager
    def keeping():
        orig = P._Staging
        P._Staging = Keep
        try:
            yield
        finally:
            P._Staging = orig

    rng = np.random.default_rng(5)

    def resample():
        c = sc.Case("resample_frames 60x40 -> 30x20 and 47x33 -> 25x31 (u8 HWC)")
        frames = [rng.integers(0, 256, (40, 60, 3)).astype(np.uint8), rng.integers(0, 256, (33, 47, 3)).astype(np.uint8)]
        geoms, total = [], 0
        for w, h in ((30, 20), (25, 31)):
            geoms.append(dict(res_w=w, res_h=h, crop_y=0, out_h=h, canvas_w=w, canvas_h=h, pad_top=0, pad_left=0, canvas_off=total))
            total += 3 * w * h
        scratch = torch.empty(total, dtype=torch.uint8, device=dev)
        with keeping():
            _, p = capture(lambda: P._resample_chunk(list(zip(geoms, frames)), scratch, L.RS_U8_HWC, dev))
        st = kept[-1]
        real = st.dev.clone()
        decoy = real.clone()
        a, n = st.offsets[3], p.src_bytes
        decoy[a:a + n] = 255 - decoy[a:a + n]                                   # the other pictures: the negatives
        c.live.append(st.dev), c.real.append(real), c.decoy.append(decoy)       # the struct points into st.dev: that IS the live tensor
        out, ws = c.out((total,), torch.uint8), c.ws(max(p.ws_bytes, 16))
        p.out, p.ws = L.ptr(out), L.ptr(ws)
        c.keep = st
        c.call = lambda: raw("ovg_resample_frames", p)
        return c

    def depth():
        c = sc.Case("depth_frames 60x40 -> 30x20 and 47x33 -> 25x31")
        maps = [(0.3 + 90 * rng.random((40, 60))).astype(np.float32), (0.3 + 150 * rng.random((33, 47))).astype(np.float32)]
        geoms = [dict(res_w=30, res_h=20, crop_y=0, out_h=20, out_off=0), dict(res_w=25, res_h=31, crop_y=0, out_h=31, out_off=600)]
        total = 600 + 775
        d0, m0 = torch.empty(total, device=dev), torch.empty(total, device=dev)
        with keeping():
            _, p = capture(lambda: P._depth_chunk(list(zip(geoms, maps)), d0, m0, 100, dev))
        st = kept[-1]
        real = st.dev.clone()
        decoy = real.clone()
        a, n = st.offsets[2], 4 * p.src_elems
        decoy[a:a + n] = real[a:a + n].view(F32).flip(0).view(torch.uint8)      # the same depths, in reverse order
        c.live.append(st.dev), c.real.append(real), c.decoy.append(decoy)
        dout, mout = c.out((total,), F32), c.out((total,), F32)
        p.depth, p.mask = L.ptr(dout), L.ptr(mout)
        c.keep = st
        c.call = lambda: raw("ovg_depth_frames", p)
        return c

    family([resample, depth], "pre-processing")


# =============================================================================================
# point cloud
# =============================================================================================
def _cams(V, H, W, seed=0):
    """[V, 16] world-to-camera rows looking at the unit box around the origin from V places."""
    rng = np.random.default_rng(seed)
    eyes = [(1.6 * np.cos(a), 0.4 * rng.standard_normal(), 1.6 * np.sin(a)) for a in np.linspace(0.3 + seed, 2.0 + seed, V)]
    ext = np.stack([tsdf_twin.look_at(e, (0.0, 0.0, 0.0)) for e in eyes])
    intr = np.stack([tsdf_twin.pinhole(H, W, 70.0) for _ in range(V)])
    return torch.from_numpy(tsdf_twin.pack_cams(ext, intr))


def _percentile_case(n):
    def build():
        c = sc.Case("percentile 3 columns {5, 95} + norm, n = %d" % n)
        pts = c.inp(torch.randn(n, 3, generator=_gen(500)), torch.randn(n, 3, generator=_gen(501)) * 1.5)
        mask = c.inp((torch.rand(n, generator=_gen(502)) > 0.3).float())
        _, p = capture(lambda: ops.percentile(pts, n, 3, 1, 3, (5.0, 95.0), mask=mask, norm=True))
        out, nrm, ws = c.out((3, 2), F32), c.out((1,), F32), c.ws(ops.percentile_workspace_bytes(n, 3))
        p.out, p.norm_out, p.ws, p.ws_bytes = L.ptr(out), L.ptr(nrm), L.ptr(ws), ws.numel()
        c.call = lambda: raw("ovg_percentile", p)
        return c
    return build


def test_point_cloud_extraction_entries():
    def point_filter():
        c = sc.Case("point_filter COUNT then SCATTER, 3 frames of 37 x 53")
        hw, n = 37 * 53, 3 * 37 * 53
        conf = c.inp(1 + 4 * torch.rand(n, generator=_gen(510)))
        images = c.inp(torch.rand(3, 3, hw, generator=_gen(511)))
        points = c.inp(torch.randn(n, 3, generator=_gen(512)))
        thr = c.inp(torch.tensor([2.5]), torch.tensor([3.5]))
        ws = c.ws(ops.point_filter_workspace_bytes(n))
        count = c.out((1,), torch.int64)
        ops.point_filter(L.PF_COUNT, conf, images, points, hw, ws, threshold=thr, flags=L.PF_BLACK_BG, out_count=count)
        cap = int(count.item())
        assert 0 < cap < n
        op, oc, oi = c.out((cap, 3), F32), c.out((cap, 3), torch.uint8), c.out((cap,), torch.int64)

        def call():
            ops.point_filter(L.PF_COUNT, conf, images, points, hw, ws, threshold=thr, flags=L.PF_BLACK_BG, out_count=count)
            ops.point_filter(L.PF_SCATTER, conf, images, points, hw, ws, threshold=thr, flags=L.PF_BLACK_BG, index_base=7, out_count=count,
                             capacity=cap, out_points=op, out_colors=oc, out_index=oi)
        c.call = call
        return c

    def voxel_downsample():
        c = sc.Case("voxel_downsample COUNT then SCATTER, 5000 points")
        n = 5000
        pts = c.inp(cloud(n, 520), shifted(cloud(n, 520)) * 0.9)
        conf = c.inp(torch.rand(n, generator=_gen(521)))
        col = c.inp(torch.randint(0, 256, (n, 3), generator=_gen(522), dtype=torch.uint8))
        voxel = c.const(torch.tensor([0.08]))
        ws = c.ws(ops.voxel_downsample_workspace_bytes(n))
        count = c.out((2,), torch.int64)
        ops.voxel_downsample(L.VG_COUNT, pts, voxel, ws, conf=conf, colors=col, out_count=count)
        cap = int(count[0].item())
        assert 0 < cap < n
        op, oc, oi = c.out((cap, 3), F32), c.out((cap, 3), torch.uint8), c.out((cap,), torch.int64)

        def call():
            ops.voxel_downsample(L.VG_COUNT, pts, voxel, ws, conf=conf, colors=col, out_count=count)
            ops.voxel_downsample(L.VG_SCATTER, pts, voxel, ws, conf=conf, colors=col, out_count=count, capacity=cap, out_points=op, out_colors=oc, out_index=oi)
        c.call = call
        return c

    def render_points():
        c = sc.Case("render_points 3 views of 37 x 53, radius 2")
        n, V, H, W = 4000, 3, 37, 53
        pts = c.inp(cloud(n, 530), shifted(cloud(n, 530)))
        col = c.inp(torch.randint(0, 256, (n, 3), generator=_gen(531), dtype=torch.uint8))
        cams = c.inp(_cams(V, H, W, 0), _cams(V, H, W, 1))
        _, p = capture(lambda: ops.render_points(pts, col, cams, H, W, radius=2, index=True))
        ws = c.ws(ops.render_workspace_bytes(V, H, W))
        rgb, dep, idx = c.out((V, H, W, 3), torch.uint8), c.out((V, H, W), F32), c.out((V, H, W), torch.int64)
        p.ws, p.ws_bytes, p.out_rgb, p.out_depth, p.out_index = L.ptr(ws), ws.numel(), L.ptr(rgb), L.ptr(dep), L.ptr(idx)
        c.call = lambda: raw("ovg_render_points", p)
        return c

    def consistency():
        c = sc.Case("multiview_consistency 3 views of 37 x 53")
        S, H, W = 3, 37, 53
        pts = c.inp(cloud(S * H * W, 540).reshape(S, H, W, 3), shifted(cloud(S * H * W, 540)).reshape(S, H, W, 3))
        cams = c.inp(_cams(S, H, W, 0), _cams(S, H, W, 1))
        valid = c.inp((torch.rand(S, H, W, generator=_gen(541)) > 0.1).to(torch.uint8))
        _, p = capture(lambda: ops.multiview_consistency(pts, cams, 0.05, valid=valid, occluded=True))
        ws = c.ws(ops.consistency_workspace_bytes(S, H, W))
        sup, vio, occ = (c.out((S, H, W), torch.int16) for _ in range(3))
        p.ws, p.ws_bytes, p.support, p.violations, p.occluded = L.ptr(ws), ws.numel(), L.ptr(sup), L.ptr(vio), L.ptr(occ)
        c.call = lambda: raw("ovg_multiview_consistency", p)
        return c

    family([_percentile_case(257), _percentile_case((1 << 20) + 1), point_filter, voxel_downsample, render_points, consistency], "point cloud")


# =============================================================================================
# search and clustering
# =============================================================================================
R2, CELL = 0.0064, 0.09        # radius 0.08 in a unit box of a few thousand points: a handful of neighbours each


def _grid_bytes(q, r, ws_bytes):
    """The grid radius_search(BUILD) leaves in a workspace, as a plain byte tensor (an INPUT of the search-only case)."""
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    ops.radius_search(L.RS_BUILD, q.to(DEV), r.to(DEV), R2, CELL, ws)
    torch.cuda.synchronize()
    return ws


def _fps_case(path, n, npoint):
    def build():
        c = sc.Case("farthest_point_sample %s n=%d npoint=%d" % ({1: "one workgroup", 2: "per step"}[path], n, npoint))
        pts = c.inp(cloud(n, 610).reshape(1, n, 3), shifted(cloud(n, 610)).reshape(1, n, 3))
        ws = c.ws(ops.fps_workspace_bytes(1, n, npoint))
        idx, d, dist = c.out((1, npoint), torch.int32), c.out((1, npoint), F32), c.out((1, n), F32)
        c.call = lambda: ops.farthest_point_sample(pts, npoint, path=path, ws=ws, index=idx, sqdist=d, distance=dist)
        return c
    return build


def _radius_case(search_only):
    def build():
        c = sc.Case("radius_search %s 900 queries, 3000 references" % ("search only on a built grid" if search_only else "build + search"))
        qa, ra = cloud(900, 620), cloud(3000, 621)
        qb, rb = shifted(qa), shifted(ra)
        q, r = c.inp(qa, qb), c.inp(ra, rb)
        need = ops.radius_workspace_bytes(900, 3000)
        stats, cnt, idx, d = c.out((4,), torch.int64), c.out((900,), torch.int32), c.out((900,), torch.int32), c.out((900,), F32)
        if search_only:
            ws = c.inp(_grid_bytes(qa, ra, need), _grid_bytes(qb, rb, need))
            stage = L.RS_SEARCH
        else:
            ws, stage = c.ws(need), L.RS_BUILD | L.RS_SEARCH
        c.call = lambda: ops.radius_search(stage, q, r, R2, CELL, ws, max_pairs=1 << 40, out_stats=stats, count=cnt, index=idx, sqdist=d)
        return c
    return build


def test_search_entries():
    def nn():
        c = sc.Case("nearest_neighbours 700 queries, 1300 references")
        q, r = c.inp(cloud(700, 600), shifted(cloud(700, 600))), c.inp(cloud(1300, 601), shifted(cloud(1300, 601)))
        ws = c.ws(ops.nn_workspace_bytes(700, 1300))
        idx, d = c.out((700,), torch.int32), c.out((700,), F32)
        c.call = lambda: ops.nearest_neighbours(q, r, splits=3, ws=ws, index=idx, sqdist=d)
        return c

    def knn(k):
        def build():
            c = sc.Case("radius build -> knn_search k=%d" % k)
            q, r = c.inp(cloud(900, 630), shifted(cloud(900, 630))), c.inp(cloud(3000, 631), shifted(cloud(3000, 631)))
            ws = c.ws(ops.radius_workspace_bytes(900, 3000))
            bstats = c.out((4,), torch.int64)
            stats, cnt, idx, d = c.out((4,), torch.int64), c.out((900,), torch.int32), c.out((900, k), torch.int32), c.out((900, k), F32)

            def call():
                ops.radius_search(L.RS_BUILD, q, r, R2, CELL, ws, out_stats=bstats)
                ops.knn_search(q, r, R2, CELL, ws, k, max_pairs=1 << 40, out_stats=stats, count=cnt, index=idx, sqdist=d)
            c.call = call
            return c
        return build

    family([nn, _fps_case(1, 500, 33), _fps_case(2, 2500, 17), _radius_case(False), _radius_case(True), knn(3), knn(8), knn(13), knn(32)], "search")


def test_cluster_and_normals_entries():
    def cluster(mn):
        def build():
            c = sc.Case("radius build -> cluster %s, 3000 points" % ("components" if mn == 0 else "DBSCAN min_neighbours %d" % mn))
            pts = c.inp(cloud(3000, 640), shifted(cloud(3000, 640)) * 0.95)
            valid = c.inp((torch.rand(3000, generator=_gen(641)) > 0.05).to(torch.uint8))
            ws = c.ws(ops.radius_workspace_bytes(3000, 3000))
            bstats, stats = c.out((4,), torch.int64), c.out((4,), torch.int64)
            root, kind, deg = c.out((3000,), torch.int32), c.out((3000,), torch.uint8), c.out((3000,), torch.int32)

            def call():
                ops.radius_search(L.RS_BUILD, pts, pts, R2, CELL, ws, query_valid=valid, reference_valid=valid, exclude_self=True, out_stats=bstats)
                ops.cluster(pts, R2, CELL, ws, mn, valid=valid, max_pairs=1 << 40, out_stats=stats, root=root, kind=kind, degree=deg)
            c.call = call
            return c
        return build

    def normals():
        c = sc.Case("knn_normals 900 rows of 8 neighbours")
        pa, pb = cloud(900, 650), shifted(cloud(900, 650)) * 0.9
        tables = []
        for pts in (pa, pb):
            ws = torch.zeros(ops.radius_workspace_bytes(900, 900), dtype=torch.uint8, device=DEV)
            ops.radius_search(L.RS_BUILD, pts.to(DEV), pts.to(DEV), 0.04, 0.21, ws)
            tables.append(ops.knn_search(pts.to(DEV), pts.to(DEV), 0.04, 0.21, ws, 8, max_pairs=1 << 40)[2].cpu())
        pts = c.inp(pa, pb)
        index = c.inp(tables[0], tables[1])
        view = c.inp(torch.tensor([0.0, 0.0, 3.0]), torch.tensor([3.0, 0.0, 0.0]))
        nrm, cur, cov, used = c.out((900, 3), F32), c.out((900,), F32), c.out((900, 6), torch.float64), c.out((900,), torch.int32)
        c.call = lambda: ops.knn_normals(pts, pts, index, viewpoint=view, normal=nrm, curvature=cur, covariance=cov, used=used)
        return c

    family([cluster(0), cluster(3), normals], "clustering and normals")


# =============================================================================================
# alignment and plane fitting
# =============================================================================================
def _moments_of(src, tgt, index=None, valid=None):
    cnt, sums = ops.align_moments(src.to(DEV), tgt.to(DEV), index=None if index is None else index.to(DEV), source_valid=None if valid is None else valid.to(DEV))
    torch.cuda.synchronize()
    return cnt.cpu(), sums.cpu()


def _rigid(seed):
    g = _gen(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = q * 1.1, torch.randn(3, generator=g, dtype=torch.float64)
    return T


def test_alignment_entries():
    n, m = 1500, 1700
    src, tgt = (cloud(n, 700), shifted(cloud(n, 700))), (cloud(m, 701), shifted(cloud(m, 701)))
    index = (torch.randint(0, m, (n,), generator=_gen(702), dtype=torch.int32), torch.randint(0, m, (n,), generator=_gen(703), dtype=torch.int32))

    def moments():
        c = sc.Case("align_moments 1500 pairs into 1700 targets, gated")
        s, t, i = c.inp(*src), c.inp(*tgt), c.inp(*index)
        d = c.inp(torch.rand(n, generator=_gen(704)))
        ws = c.ws(ops.align_workspace_bytes(n))
        cnt, sums = c.out((1,), torch.int64), c.out((18,), torch.float64)
        c.call = lambda: ops.align_moments(s, t, index=i, sqdist=d, max_sqdist=0.8, ws=ws, count=cnt, sums=sums)
        return c

    def solve():
        c = sc.Case("align_solve with scale")
        ma, mb = _moments_of(src[0], tgt[0], index[0]), _moments_of(src[1], tgt[1], index[1])
        cnt, sums = c.inp(ma[0], mb[0]), c.inp(ma[1], mb[1])
        T, scale, rms, oc, status = c.out((4, 4), torch.float64), c.out((1,), torch.float64), c.out((1,), torch.float64), c.out((1,), torch.int64), c.out((1,), torch.int32)
        c.call = lambda: ops.align_solve(cnt, sums, T, scale=scale, rms=rms, out_count=oc, status=status)
        return c

    def apply():
        c = sc.Case("align_apply 1500 points")
        p = c.inp(*src)
        T = c.inp(_rigid(705), _rigid(706))
        out = c.out((n, 3), F32)
        c.call = lambda: ops.align_apply(p, T, out=out)
        return c

    family([moments, solve, apply], "alignment")


def test_plane_entries():
    n, H = 2000, 600

    def scene(seed):
        g = _gen(seed)
        p = cloud(n, seed)
        p[: n // 2, 1] = 0.1 * seed / 710 + 0.01 * torch.randn(n // 2, generator=g)          # half the points near a horizontal plane
        return p[torch.randperm(n, generator=g)]
    pa, pb = scene(710), scene(711)

    def planes_of(p, seed):
        pl, _ = ops.plane_hypotheses(p.to(DEV), H, seed=seed)
        torch.cuda.synchronize()
        return pl.cpu()
    ha, hb = planes_of(pa, 5), planes_of(pb, 6)
    plane_a, plane_b = torch.tensor([0.0, 1.0, 0.0, -0.1]), torch.tensor([0.0, 0.6, 0.8, 0.05])

    def hypotheses():
        c = sc.Case("plane_hypotheses 600 draws from 2000 points, with an axis")
        p = c.inp(pa, pb)
        valid = c.inp((torch.rand(n, generator=_gen(712)) > 0.05).to(torch.uint8))
        axis = c.const(torch.tensor([0.0, 1.0, 0.0]))
        planes, index = c.out((H, 4), F32), c.out((H, 3), torch.int32)
        c.call = lambda: ops.plane_hypotheses(p, H, seed=5, valid=valid, axis=axis, min_abs_cos=0.5, planes=planes, index=index)
        return c

    def score():
        c = sc.Case("plane_score 600 planes x 2000 points, 3 splits")
        p, pl = c.inp(pa, pb), c.inp(ha, hb)
        count = c.out((H,), torch.int32)
        c.call = lambda: ops.plane_score(p, pl, 0.03, splits=3, count=count)
        return c

    def select():
        c = sc.Case("plane_select of 600")
        counts = []
        for p, h in ((pa, ha), (pb, hb)):
            counts.append(ops.plane_score(p.to(DEV), h.to(DEV), 0.03).cpu())
        cnt, pl = c.inp(*counts), c.inp(ha, hb)
        best, plane, bc, status = c.out((1,), torch.int32), c.out((4,), F32), c.out((1,), torch.int32), c.out((1,), torch.int32)
        c.call = lambda: ops.plane_select(cnt, pl, min_inliers=10, best=best, plane=plane, best_count=bc, status=status)
        return c

    def mask():
        c = sc.Case("plane_mask 2000 points with distances")
        p, pl = c.inp(pa, pb), c.inp(plane_a, plane_b)
        inl, dist, cnt = c.out((n,), torch.uint8), c.out((n,), F32), c.out((1,), torch.int64)
        c.call = lambda: ops.plane_mask(p, pl, 0.03, inlier=inl, distance=dist, out_count=cnt)
        return c

    def fit():
        c = sc.Case("plane_fit from the inliers' moments")
        ms = []
        for p, pl in ((pa, plane_a), (pb, plane_b)):
            inl = ops.plane_mask(p.to(DEV), pl.to(DEV), 0.03)[0]
            ms.append(_moments_of(p, p, valid=inl.cpu()))
        cnt, sums = c.inp(ms[0][0], ms[1][0]), c.inp(ms[0][1], ms[1][1])
        plane = c.inout(plane_a, plane_b)
        rms, eig, status = c.out((1,), torch.float64), c.out((3,), torch.float64), c.out((1,), torch.int32)
        c.call = lambda: ops.plane_fit(cnt, sums, plane, rms=rms, eigen=eig, status=status)
        return c

    family([hypotheses, score, select, mask, fit], "plane fitting")


# =============================================================================================
# fusion and meshing
# =============================================================================================
def test_fusion_entries():
    import test_gpu_tsdf as tt

    def integrate():
        c = sc.Case("tsdf_integrate dims (9, 5, 3), S = 2, valid + obs_weight + colors")
        dims = (9, 5, 3)
        a, b = tt._scene(dims, 2, seed=2), tt._scene(dims, 2, seed=7)
        t = lambda s, k: torch.from_numpy(np.ascontiguousarray(s[k]))
        fresh = tsdf_twin.fresh(dims)
        T, Wt, C = (c.inout(torch.from_numpy(v)) for v in fresh)
        depth, cams, valid, obs, colors = (c.inp(t(a, k), t(b, k)) for k in ("depth", "cams", "valid", "obs_weight", "colors"))
        origin = [float(v) for v in a["origin"]]
        c.call = lambda: ops.tsdf_integrate(T, Wt, depth, cams, origin, float(a["voxel"]), float(a["trunc"]), color=C, valid=valid, obs_weight=obs, colors=colors)
        return c

    def extract():
        c = sc.Case("tsdf_extract COUNT then SCATTER, the 9^3 sphere")
        tsdf, weight, origin, voxel, _ = tsdf_twin.sdf_volume("sphere", 9)
        small = tsdf_twin.sdf_volume("sphere", 9, radius=0.45)[0]                 # the decoy: a smaller sphere, fewer vertices than the capacities
        T = c.inp(torch.from_numpy(tsdf), torch.from_numpy(small))
        Wt = c.const(torch.from_numpy(weight))
        col = c.inp(torch.rand(9, 9, 9, 4, generator=_gen(800)) * torch.tensor([255.0, 255.0, 255.0, 1.0]))
        origin, voxel = [float(v) for v in origin], float(voxel)
        ws = c.ws(ops.tsdf_extract_workspace_bytes(9, 9, 9))
        count = c.out((2,), torch.int64)
        ops.tsdf_extract(L.TSDF_COUNT, T, Wt, origin, voxel, ws, color=col, out_count=count)
        M, Q = (int(v) for v in count.cpu())
        assert M > 0 and Q > 0
        vert, nrm, vc, faces = c.out((M, 3), F32), c.out((M, 3), F32), c.out((M, 3), torch.uint8), c.out((2 * Q, 3), torch.int32)

        def call():
            ops.tsdf_extract(L.TSDF_COUNT, T, Wt, origin, voxel, ws, color=col, out_count=count)
            ops.tsdf_extract(L.TSDF_SCATTER, T, Wt, origin, voxel, ws, color=col, out_count=count, vertex_capacity=M, quad_capacity=Q,
                             vertices=vert, normals=nrm, colors=vc, faces=faces)
        c.call = call
        return c

    family([integrate, extract], "fusion")


def test_render_mesh_lane_and_cooperative_paths():
    import test_gpu_raster as tr
    vert, nrm, faces, col = tr._mesh("sphere", 9)
    V, H, W = 3, 37, 53

    def case(coop, what):
        def build():
            c = sc.Case("render_mesh %s path, 3 views of 37 x 53" % what)
            v = c.inp(torch.from_numpy(vert), torch.from_numpy(vert) * 0.9 + 0.05)
            f = c.const(torch.from_numpy(faces))
            nr = c.inp(torch.from_numpy(nrm))
            cl = c.inp(torch.from_numpy(col))
            cams = c.inp(_cams(V, H, W, 0), _cams(V, H, W, 1))
            ws = c.ws(ops.render_mesh_workspace_bytes(V, H, W))
            rgb, dep, idx = c.out((V, H, W, 3), torch.uint8), c.out((V, H, W), F32), c.out((V, H, W), torch.int64)
            c.call = lambda: ops.render_mesh(v, f, cams, H, W, normals=nr, colors=cl, shading=L.MESH_SHADE_HEADLIGHT, coop_threshold=coop,
                                             ws=ws, out=(rgb, dep, idx), background=tr.BG)
            return c
        return build
    family([case(tr.HUGE, "lane"), case(1, "cooperative")], "meshing")


# =============================================================================================
# coverage: the header's entries == what the families above reached (keep this test last in the file)
# =============================================================================================
def declared_entries(text):
    """Names of every `int ovg_*(const <params>*..., void* stream)` declaration (comments removed first)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\bint\s+(ovg_\w+)\s*\(\s*const\b[^;{]*?\bvoid\s*\*\s*(?:hip_)?stream\s*\)\s*;", text))


def test_every_entry_of_the_header_is_gated():
    with open(HEADER) as fh:
        declared = declared_entries(fh.read())
    bound = {n for n, (_, args) in L.SYMBOLS.items() if len(args) >= 2 and args[-1] is L.vp}      # the ctypes binding's view: (..., void* stream)
    assert len(declared) >= 48, sorted(declared)
    assert declared == bound, "the header parse and the ctypes binding disagree: %s" % sorted(declared ^ bound)
    assert declared_entries("int ovg_x(const ovg_x_params*, void* stream);\n/* int ovg_y(const p*, void* stream); */\nint ovg_z(const p*, ovg_o* out);") == {"ovg_x"}
    want = declared - set(EXCLUDED)
    got = set(COVERED)
    print("gated entries: %d of %d declared (%d excluded)" % (len(got & want), len(declared), len(EXCLUDED)), flush=True)
    for e in sorted(got):
        print("  %-32s %s" % (e, "; ".join(COVERED[e])), flush=True)
    assert got - want == set(), "gated but not declared with a stream: %s" % sorted(got - want)
    assert want - got == set(), "entries of the header that no gated case reached (did a family above fail or get deselected?): %s" % sorted(want - got)
