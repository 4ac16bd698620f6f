"""CPU-only proof that tests/kernel_guards.py catches what it is for: plain float32 evaluations of linear / attention / LayerNorm (rounded
to the stored dtype) pass the per-element budget against float64, every planted defect is flagged, and -- the reason the comparator
exists -- gpu_selftest.report() at the existing TOL does NOT flag the dropped bias or the quiet attention row."""
import contextlib
import io
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_selftest as st
import kernel_guards as kg

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _report(name, got, ref, tol):
    """gpu_selftest.report without touching the module's result list or the log."""
    keep = list(st.results)
    with contextlib.redirect_stdout(io.StringIO()):
        ok = st.report(name, got, ref, tol)
    st.results[:] = keep
    return ok


def _linear_case(mode, M=130, N=256, K=192, seed=3):
    g = torch.Generator().manual_seed(seed)
    dt = DT[mode]
    x = torch.randn(M, K, generator=g).to(dt)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dt)
    w[:4] *= 12                                    # a few loud output columns: the tensor maximum the global gate divides by
    bias = torch.randn(N, generator=g) * 0.02
    ref = x.double() @ w.double().t() + bias.double()
    got = (x.float() @ w.float().t() + bias).to(dt)
    return x, w, bias, ref, got


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_reference_linear_passes_and_planted_defects_are_flagged(mode):
    x, w, bias, ref, got = _linear_case(mode)
    K = x.shape[1]
    mag, c, u = kg.gemm_mag(x, w, bias), kg.gemm_c(K, mode), kg.U_OUT[mode]
    assert kg.elementwise_budget("linear_" + mode, got, ref, mag, u, c) <= 1.0
    # GELU and RES on the same GEMM
    assert kg.elementwise_budget("gelu_" + mode, F.gelu(x.float() @ w.float().t() + bias).to(DT[mode]), F.gelu(ref), mag, u, kg.gelu_c(K, mode)) <= 1.0
    g = torch.Generator().manual_seed(5)
    res, gamma = torch.randn(ref.shape, generator=g), torch.randn(ref.shape[1], generator=g)
    z32 = x.float() @ w.float().t() + bias
    rref = res.double() + gamma.double() * ref
    rmag, rc = kg.res_mag(res, gamma, mag), kg.res_c(K, mode)
    assert kg.elementwise_budget("res_" + mode, res + gamma * z32, rref, rmag, kg.U_OUT["f32"], rc) <= 1.0
    # defect 1: the bias dropped on one 16-column group
    bad = (x.float() @ w.float().t() + bias)
    bad[:, 64:80] -= bias[64:80]
    bad = bad.to(DT[mode])
    with pytest.raises(AssertionError, match="over their budget"):
        kg.elementwise_budget("linear_nobias16_" + mode, bad, ref, mag, u, c, quiet=True)
    if mode != "f32":      # (the f32 gate, 2e-5, does see it)
        assert _report("linear_nobias16_" + mode, bad, ref, st.TOL[mode]), "the global gate should not see a dropped small bias"
    # defect 2: one element replaced by its neighbour
    bad = got.clone()
    bad[77, 101] = bad[77, 100]
    with pytest.raises(AssertionError, match=r"worst @\[77, 101\]"):
        kg.elementwise_budget("linear_neighbour_" + mode, bad, ref, mag, u, c, quiet=True)
    # defect 4: gamma dropped (taken as 1) on four columns of the RES epilogue
    gbad = gamma.clone()
    gbad[40:44] = 1.0
    with pytest.raises(AssertionError, match="over their budget"):
        kg.elementwise_budget("res_nogamma4_" + mode, res + gbad * z32, rref, rmag, kg.U_OUT["f32"], rc, quiet=True)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_reference_attention_passes_and_a_dropped_key_tile_in_a_quiet_row_is_flagged(mode):
    g = torch.Generator().manual_seed(9)
    dt, BH, nq, nk = DT[mode], 4, 70, 256
    q = (torch.randn(BH, nq, 64, generator=g) * 1.2).to(dt)
    k = torch.randn(BH, nk, 64, generator=g).to(dt)
    v = torch.randn(BH, nk, 64, generator=g).to(dt)
    v[0] *= 60                                     # a loud head sets the tensor maximum
    q[1, 33] *= 0.05                               # a quiet row: flat softmax, small output
    ref, mag, c, lse = kg.attn_budget(q, k, v, mode)
    # the plain evaluation with P rounded where the kernels round it
    s = (q.float() @ k.float().transpose(1, 2))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    got = ((p.to(dt).float() @ v.float()) / p.sum(-1, keepdim=True)).to(dt)
    assert kg.elementwise_budget("attn_" + mode, got, ref, mag, kg.U_OUT[mode], c) <= 1.0
    # defect 3: keys 64..127 left out of the quiet row
    p2 = p[1, 33].clone()
    p2[64:128] = 0
    bad = got.clone()
    bad[1, 33] = ((p2.to(dt).float() @ v[1].float()) / p2.sum()).to(dt)
    with pytest.raises(AssertionError, match=r"worst @\[1, 33, "):
        kg.elementwise_budget("attn_quiet_row_" + mode, bad, ref, mag, kg.U_OUT[mode], c, quiet=True)
    assert _report("attn_quiet_row_" + mode, bad, ref, st.TOL[mode]), "the global gate should not see one quiet row"


def test_reference_layernorm_passes_on_every_row_family_and_a_one_pass_variance_does_not():
    g = torch.Generator().manual_seed(11)
    n = 1024
    x = torch.randn(6, n, generator=g)
    x[1] = 1000.0 + 0.01 * torch.randn(n, generator=g)
    x[2, 17] = 500.0
    x[3] = 1e-20 * torch.randn(n, generator=g)
    x[4] = 3.5
    w, b = torch.randn(n, generator=g) * 0.1 + 1, torch.randn(n, generator=g) * 0.1
    ref, mag, c, extra = kg.layernorm_budget(x, w, b, 1e-5)
    got = F.layer_norm(x, (n,), w, b, 1e-5)
    assert kg.elementwise_budget("layernorm_f32", got, ref, mag, kg.U_OUT["f32"], c, extra=extra) <= 1.0
    assert kg.elementwise_budget("layernorm_bf16", got.to(torch.bfloat16), ref, mag, kg.U_OUT["bf16"], c, extra=extra) <= 1.0
    assert torch.equal(got[4], b)                  # zero variance: exactly the bias
    # a one-pass E[x^2] - mean^2 in f32 on the row whose mean dwarfs its spread
    mean = x.mean(-1, keepdim=True)
    var1 = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    bad = (x - mean) / torch.sqrt(var1 + 1e-5) * w + b
    with pytest.raises(AssertionError, match=r"worst @\[1, "):
        kg.elementwise_budget("layernorm_one_pass", bad, ref, mag, kg.U_OUT["f32"], c, extra=extra, quiet=True)
    # a dropped weight lane (4 columns) in a quiet row next to the massive activation
    bad = got.clone()
    bad[0, 100:104] = ((x[0] - x[0].mean()) / torch.sqrt(x[0].var(unbiased=False) + 1e-5) + b)[100:104]
    with pytest.raises(AssertionError, match="over their budget"):
        kg.elementwise_budget("layernorm_now4", bad, ref, mag, kg.U_OUT["f32"], c, extra=extra, quiet=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_guard_finds_a_flipped_guard_byte_and_a_flipped_row_gap_byte(dtype):
    view, check = kg.guarded((5, 128), dtype, "cpu", ld=136, guard_bytes=256, spare_rows=2)
    esz = view.element_size()
    assert view.shape == (5, 128) and view.stride() == (136, 1) and view.data_ptr() % 16 == 0
    assert bool(torch.isfinite(view.float()).all()) and bool((view.float() != 0).all())     # the fill reads as finite non-zero values
    view.copy_(torch.randn(5, 128).to(dtype))       # writes inside the view are free
    check("clean")
    buf, gb = check.buffer, check.guard_bytes
    for off, what in ((gb - 1, r"byte -1 "), (gb + 5 * 136 * esz + 3, r"row 5, col"), (buf.numel() - 1, "first byte"),
                      (gb + 2 * 136 * esz + 128 * esz, r"row 2, col 128"), (gb + 136 * esz * 4 + 135 * esz + esz - 1, r"row 4, col 135")):
        old = int(buf[off])
        buf[off] = old ^ 0x01
        with pytest.raises(kg.GuardError, match=what):
            check("flipped")
        buf[off] = old
    check("restored")
    # 3-D / 4-D views (q buffers, NHWC maps): the gap after every row of the second-to-last dimension is guarded
    v4, chk4 = kg.guarded((2, 3, 5, 8), dtype, "cpu", ld=16, guard_bytes=64)
    assert v4.stride() == (3 * 5 * 16, 5 * 16, 16, 1)
    v4.fill_(1.0)
    chk4("nhwc")
    chk4.buffer[64 + (7 * 16 + 8) * esz] ^= 0xFF
    with pytest.raises(kg.GuardError, match="row 7, col 8"):
        chk4("nhwc gap")


def test_poison_helpers_fill_exactly_the_padding_with_finite_alternating_values():
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        q = torch.zeros(3, 128, 64, dtype=dt)
        kg.poison_rows(q, 70)
        assert float(q[:, :70].abs().max()) == 0 and bool((q[:, 70:].abs() == kg.POISON).all())
        assert bool((q[:, 70:] > 0).any()) and bool((q[:, 70:] < 0).any()) and bool(torch.isfinite(q.float() * q.float()).all())
        w = torch.zeros(16, 640, dtype=dt)
        kg.poison_cols(w, 588)
        assert float(w[:, :588].abs().max()) == 0 and bool((w[:, 588:].abs() == kg.POISON).all())
        vt = torch.zeros(2, 64, 128, dtype=dt)
        kg.poison_vt(vt, 70, sixteen_bit=dt is not torch.float32)
        key = kg.vt_pos16(128) if dt is not torch.float32 else torch.arange(128)
        assert float(vt[:, :, key < 70].abs().max()) == 0 and bool((vt[:, :, key >= 70].abs() == kg.POISON).all())
    # the V^T column order against a table written out from the header's rule: inside every block of 32 keys column 8 g + 4 h + i holds
    # key 16 h + 4 g + i (g < 4, h < 2, i < 4)
    table = [0] * 96
    for blk in range(3):
        for g_ in range(4):
            for h in range(2):
                for i in range(4):
                    table[32 * blk + 8 * g_ + 4 * h + i] = 32 * blk + 16 * h + 4 * g_ + i
    assert kg.vt_pos16(96).tolist() == table
    assert table[:12] == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7]


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """A correctly rounded bf16 store is up to 2^-8 |ref| away (8 significand bits), not 2^-9: the comparator's u_out for bf16."""
    ref = torch.tensor([1.00394157], dtype=torch.float64)
    got = ref.float().to(torch.bfloat16)
    err = float((got.double() - ref).abs())
    assert 2.0 ** -9 * float(ref) < err <= 2.0 ** -8 * float(ref)
    assert kg.U_OUT["bf16"] == 2.0 ** -8 and kg.U_OUT["f16"] == 2.0 ** -11 and kg.U_OUT["f32"] == 2.0 ** -24


def test_qk_norm_rope_error_bound_holds_for_a_float32_evaluation_and_flags_a_wrong_rotated_pair():
    import aggregator_oracle as orc
    g = torch.Generator().manual_seed(21)
    B, H, n = 2, 3, 9
    z = torch.randn(B, H, n, 64, generator=g) * 0.8
    z[0, 1] *= 0.01                                                    # a quiet head
    w, b = torch.randn(64, generator=g) * 0.1 + 1.5, torch.randn(64, generator=g) * 0.1
    cos, sin = orc.rope_tables(38)
    pos = torch.randint(0, 38, (B, n, 2), generator=g)
    ez = 1e-6 * z.abs().double()                                       # what the GEMM in front would carry
    zin = z.double() + ez * torch.sign(torch.randn(z.shape, generator=g)).double()
    ref = orc.rope_2d(F.layer_norm(z.double(), (64,), w.double(), b.double(), 1e-5), pos, cos.double(), sin.double()) * 0.18
    got = orc.rope_2d(F.layer_norm(zin.float(), (64,), w, b, 1e-5), pos, cos, sin) * 0.18
    err = kg.qk_norm_rope_error(z.double(), ez, w, b, 1e-5, pos, cos, sin, 0.18)
    assert kg.elementwise_budget("qk_norm_rope", got, ref, ref.abs(), kg.U_OUT["f32"], kg.MARGIN, extra=err) <= 1.0
    bad = got.clone()
    bad[0, 1, 4, 3], bad[0, 1, 4, 19] = got[0, 1, 4, 19], got[0, 1, 4, 3]      # one rotated pair swapped in the quiet head
    with pytest.raises(AssertionError, match=r"worst @\[0, 1, 4, "):
        kg.elementwise_budget("qk_norm_rope_swapped", bad, ref, ref.abs(), kg.U_OUT["f32"], kg.MARGIN, extra=err, quiet=True)
