"""CPU-only: what test_gpu_block_entries.py leans on is checked here first. The float64 block reference (tests/block_reference.py) against
oracle.aggregator_oracle.block in f32, frame and global, with and without inject, at gpu_selftest.test_block's f32 gate (5e-5); the
byte sizes ovg_block_workspace_bytes reports (a host-only entry: the library loads without a device) against the header's formula; and
the shapes that query refuses."""
import contextlib
import io

import pytest
import torch

import block_reference as br
import gpu_selftest as st
from omnivggt_official_amd import lib as L, ops


def _report(name, got, ref, tol):
    keep = list(st.results)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ok = st.report(name, got, ref, tol)
    st.results[:] = keep
    print(buf.getvalue().strip())
    return ok


@pytest.mark.parametrize("tpv,gw", [(25, 5), (65, 10)])
def test_float64_block_reference_agrees_with_the_oracle_block(tpv, gw):
    views = 3
    M = views * tpv
    W = br.draw_weights()
    sd = {"blk." + k: v for k, v in W.items()}
    g = torch.Generator().manual_seed(31)
    x = torch.randn(M, 1024, generator=g)
    rope = br.rope_tables()
    pos = br.positions(M, tpv, gw)
    for mode, seq in (("frame", tpv), ("global", M)):
        B = M // seq
        with torch.no_grad():
            orc = st.orc.block(x.view(B, seq, 1024), sd, "blk", pos.view(B, seq, 2), rope, True).reshape(M, 1024)
        for per in (0, seq, 1, M + 1):
            inj = None if per == 0 else torch.randn((M + per - 1) // per, 1024, generator=g)
            ref = br.block_reference(x, W, seq, tpv, gw, rope, inject=inj, inj_period=per)
            want = orc.double() if inj is None else orc.double() + br.inject_rows(M, inj, per)
            assert _report("block_reference_%s_tpv%d_inj%d" % (mode, tpv, per), want, ref, br.GATE["f32"])
    # with gammas of order 1 a missing branch cannot hide under a gate
    ref = br.block_reference(x, W, tpv, tpv, gw, rope)
    for drop in ("ls1.gamma", "ls2.gamma"):
        W0 = dict(W)
        W0[drop] = torch.zeros(1024)
        moved = float((br.block_reference(x, W0, tpv, tpv, gw, rope) - ref).abs().max() / ref.abs().max())
        print("without %s the output moves by %.3f of its maximum" % (drop, moved))
        assert moved > max(br.GATE.values()), (drop, moved)                # each branch is visible under the loosest dtype gate


def test_reference_positions_and_extra_segments():
    pos = br.positions(2 * 25, 25, 5)
    assert pos[:5].abs().sum() == 0 and pos[5].tolist() == [1, 1] and pos[9].tolist() == [1, 5] and pos[10].tolist() == [2, 1]
    assert torch.equal(pos[:25], pos[25:])
    # attention over concatenated keys does not depend on where the block's own keys sit, and an extra segment changes the result
    W = br.draw_weights()
    g = torch.Generator().manual_seed(33)
    x = torch.randn(18, 1024, generator=g)
    segs = [(torch.randn(16, n, 64, generator=g), torch.randn(16, n, 64, generator=g)) for n in (1, 7)]
    rope = br.rope_tables()
    a = br.block_reference(x, W, 18, 6, 1, rope, segments=segs, local_seg_index=0)
    b = br.block_reference(x, W, 18, 6, 1, rope, segments=segs, local_seg_index=2)
    plain = br.block_reference(x, W, 18, 6, 1, rope)
    assert float((a - b).abs().max()) < 1e-12 and float((a - plain).abs().max()) > 1e-3


MODES = {"bf16": (torch.bfloat16, 2), "f16": (torch.float16, 2), "f32": (torch.float32, 4), "f32x": (L.F32X, 2)}


@pytest.mark.parametrize("mode", list(MODES))
def test_workspace_query_reports_the_documented_sizes(mode):
    dt, esz = MODES[mode]
    for tpv, _ in br.SHAPES:
        for views in (1, 3):
            M = views * tpv
            for seq in sorted({tpv, M}):
                assert ops.block_workspace_bytes(M, seq, dt) == br.expected_workspace_bytes(M, seq, esz), (mode, M, seq)
    # paddings other than the default (the sharded path pads q / k / V^T to the largest shard)
    assert ops.block_workspace_bytes(195, 65, dt, nq_pad=65, nk_pad=256) == br.expected_workspace_bytes(195, 65, esz, 65, 256)


def test_workspace_query_refuses_what_the_block_cannot_run():
    for what, kw in (("nq_pad < seq", dict(nq_pad=64)), ("nk_pad < seq", dict(nk_pad=64)), ("nk_pad % 64", dict(nk_pad=96)),
                     ("BH off by 16", dict(BH=64))):
        with pytest.raises(L.OvgError, match="OVG_E_ARG"):
            ops.block_workspace_bytes(195, 65, torch.bfloat16, **kw)
    with pytest.raises(L.OvgError, match="OVG_E_ARG"):
        ops.block_workspace_bytes(195, 64, torch.bfloat16)                  # M % seq
    with pytest.raises(L.OvgError, match="OVG_E_DTYPE"):
        ops.block_workspace_bytes(195, 65, 7)                               # no such dtype code
    assert ops.block_workspace_bytes(195, 65, torch.bfloat16, nq_pad=65, nk_pad=128)["q"] == 48 * 65 * 64 * 2


def test_block_entries_refuse_bad_paddings_on_the_host():
    """check_block refuses what ovg_block_workspace_bytes refuses before anything is launched: with fake (never dereferenced) pointers
    the three entries answer on a host without a device."""
    lib = L.load()
    fake = 1 << 20

    def params(**kw):
        p = L.BlockParams()
        for f in ("x_in", "x_out", "ws_xn", "ws_q", "ws_k", "ws_vt", "ws_attn", "ws_hid"):
            setattr(p, f, fake)
        p.M, p.seq, p.BH, p.nq_pad, p.nk_pad, p.dtype = 195, 65, 48, 128, 128, L.OVG_BF16
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = (("nq_pad < seq", dict(nq_pad=64), -1), ("nk_pad < seq", dict(nk_pad=64), -1), ("nk_pad % 64", dict(nk_pad=160), -1),
             ("dtype", dict(dtype=7), -2), ("M % seq", dict(seq=64), -1), ("BH", dict(BH=64), -1), ("nseg_extra", dict(nseg_extra=L.OVG_MAX_SEG), -1),
             ("local_seg_index", dict(nseg_extra=1, local_seg_index=2), -1), ("lo planes", dict(dtype=L.OVG_F16X2), -1),
             ("empty extra segment", dict(nseg_extra=1), -1))
    for name in ("ovg_block_forward", "ovg_block_attn_prologue", "ovg_block_attn_epilogue"):
        for what, kw, rc in cases:
            if what == "empty extra segment" and name == "ovg_block_attn_prologue":
                continue                                  # the prologue runs before the caller has the remote segments
            assert getattr(lib, name)(L.C.byref(params(**kw)), None) == rc, (name, what)
