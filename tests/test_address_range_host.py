"""Host side of the address-range tests (no GPU): the case table of tests/address_range.py proved by arithmetic, every size refusal of the
model-path entries from the raw C entry without a device, the chunked guard checker held to kernel_guards.guarded, and planted defects --
a numpy model of a kernel that forms its row offset in 32 bits -- that the guard checker and the periodic comparison must report."""
import ctypes

import numpy as np
import pytest
import torch

import address_range as ar
import kernel_guards as kg
from omnivggt_official_amd import lib as L

BIG = 1 << 40                       # a fake, 16-byte aligned device pointer: every call below fails its checks before anything dereferences it


# =============================================================================================
# the case table
# =============================================================================================
def test_every_case_passes_exactly_the_lines_it_claims_and_fits_its_memory_budget():
    assert ar.FAR_STRIDE_BYTES == (16 << 20) + 64 and ar.PERIOD == 1031 and all(ar.PERIOD % d for d in range(2, 33))
    assert 128 * ar.FAR_STRIDE_BYTES > (1 << 31) > 127 * ar.FAR_STRIDE_BYTES + 8192             # row 128 starts past 2 GiB
    assert 256 * ar.FAR_STRIDE_BYTES > (1 << 32) > 255 * ar.FAR_STRIDE_BYTES + 8192             # row 256 past 4 GiB = 2^31 16-bit elements
    assert 512 * ar.FAR_STRIDE_BYTES // 4 > (1 << 31) > 511 * ar.FAR_STRIDE_BYTES // 4 + 2048   # row 512 past 2^31 f32 elements
    seen = set()
    for case in ar.CASES.values():
        assert case.form in ("stride", "count") and case.far, case.name
        for name, op in case.operands.items():
            claimed = case.far.get(name, ())
            # the last addressed element and byte, from the shape and the stride alone
            last_elem = (op.rows - 1) * op.ld + op.cols - 1
            last_byte = (last_elem + 1) * op.esz - 1
            passed = tuple(n for n in ar.ALL3 if (last_elem if n == "2^31el" else last_byte) >= ar.LINES[n])
            assert passed == tuple(claimed), "%s: operand %s passes %s, the table claims %s" % (case.name, name, passed, claimed)
            if name not in case.far:
                assert last_byte < (1 << 31), "%s: operand %s is not the far one and ends at byte %d" % (case.name, name, last_byte)
            assert op.ld >= op.cols and (op.ld * op.esz) % 16 == 0 or op.ld == op.cols, (case.name, name)
            assert (last_byte + 1) <= ar.TENSOR_CAP, "%s: operand %s needs %.1f GiB" % (case.name, name, (last_byte + 1) / ar.GIB)
        estimate = sum(o.bytes for o in case.operands.values()) + case.scratch
        assert estimate <= ar.MEM_CAP, "%s: %.1f GiB" % (case.name, estimate / ar.GIB)
        if case.form == "stride":
            (which, lines), = case.far.items()
            assert lines == ar.ALL3 and which == case.arg["far"], case.name           # one operand far, past all three lines
            far_op = case.operands[which]
            assert far_op.ld * far_op.esz in (ar.FAR_STRIDE_BYTES, ar.CONV256_STRIDE_BYTES)
            assert all(o.ld <= o.cols + ar.NEAR_PAD for n, o in case.operands.items() if n != which), case.name
            assert far_op.rows >= (ar.ROWS16 if far_op.esz == 2 else ar.ROWS32), case.name
        seen.add(case.entry)
    # every entry with a row or pixel stride in its parameter struct has a stride-form case
    strided = {"ovg_layernorm", "ovg_linear", "ovg_qkv", "ovg_flash_attn", "ovg_attn_merge", "ovg_copy_rows", "ovg_pack_weights", "ovg_dino_specials",
               "ovg_assemble_tokens", "ovg_head_layernorm", "ovg_heads_to_tokens", "ovg_conv", "ovg_upsample", "ovg_dpt_tail", "ovg_camera_head",
               "ovg_block_forward"}
    assert strided <= {c.entry for c in ar.CASES.values() if c.form == "stride"}
    assert seen == strided | {"ovg_unproject"}
    # ovg_linear: x, w, y (and res) x both forced tiles x the listed dtypes / epilogues
    names = set(ar.CASES)
    for mode, epi, tile in ar.LINEAR_COMBOS:
        for which in ("x", "w", "y") + (("res",) if epi == "res" else ()):
            assert "linear.%s.%s.t%d.%s" % (epi, mode, tile, which) in names
    assert {(m, e) for m, e, _ in ar.LINEAR_COMBOS} == {("bf16", "store"), ("f32", "store"), ("f32x", "store"), ("bf16", "gelu"), ("bf16", "res"), ("bf16", "patch")}
    assert all((("bf16", e, t) in ar.LINEAR_COMBOS) for e in ("store", "gelu", "res", "patch") for t in (128, 256))
    # the count form's shapes
    c = ar.CASES
    assert c["linear.count.N128.16"].arg["M"] == (1 << 24) + 257 == c["linear.count.N256.16"].arg["M"] == c["linear.count.N128.res"].arg["M"]
    assert c["layernorm.count"].arg["rows"] == c["copy_rows.count"].arg["rows"] == (1 << 20) + 5
    assert c["head_layernorm.count"].arg["rows"] == 262144 + 7 > 4 * (1 << 16)                      # grid_1d's cap: 2^16 blocks of four rows
    for n in ("upsample.count", "unproject.count"):
        a = c[n].arg
        assert (a.get("OH", a["H"]) * a.get("OW", a["W"])) > (1 << 28) == 256 * (1 << 20)            # grid_1d's cap of 2^20 blocks of 256 items
    assert c["block_forward.count.bf16"].arg["M"] == 262144 + 128 and c["block_forward.count.f32"].arg["M"] == 131072 + 128
    # ovg_conv's 256-pixel form: 2 H W ldx 2 < 2^32 - 65536 holds at the first pixel stride and fails at the next legal one
    lo, hi = ar.CONV256_LDX
    assert hi == lo + 8 and 2 * 129 * 128 * lo * 2 < (1 << 32) - 65536 <= 2 * 129 * 128 * hi * 2
    assert 5 * 4 * ar.DPT_TAIL_LDX < (1 << 31) <= 5 * 4 * (ar.DPT_TAIL_LDX + 8) and ar.DPT_TAIL_LDX % 8 == 0
    for what, why, nbytes in ar.NOT_RUN:
        assert nbytes > ar.TENSOR_CAP or "the issue" in why, what      # a real tensor size above the cap, or an operand the issue itself rules out


# =============================================================================================
# refusals, from the raw entries, without a device
# =============================================================================================
def _linear(**kw):
    p = L.LinearParams(x=BIG, ldx=64, w=BIG, ldw=64, bias=BIG, y=BIG, ldy=128, M=257, N=128, K=64, dtype=L.OVG_BF16, epilogue=L.EPI_STORE, tile=L.TILE_128)
    for k, v in kw.items():
        setattr(p, k, v)
    return L.load().ovg_linear(ctypes.byref(p), None)


def _qkv(**kw):
    p = L.QkvParams(x=BIG, ldx=1024, w=BIG, bias=BIG, q=BIG, k=BIG, vt=BIG, M=64, seq=64, nq_pad=64, nk_pad=64, dtype=L.OVG_BF16, tile=L.TILE_128)
    for k, v in kw.items():
        setattr(p, k, v)
    return L.load().ovg_qkv(ctypes.byref(p), None)


LD256_MAX = (((1 << 32) - 64) // 255) // 2        # 255 ld 2 + 64 <= 2^32


def test_row_count_and_leading_dimension_refusals_of_the_gemm_entries():
    assert LD256_MAX == 8421504 and 255 * LD256_MAX * 2 + 64 <= (1 << 32) < 255 * (LD256_MAX + 8) * 2 + 64
    assert ar.FAR_STRIDE_BYTES // 2 <= LD256_MAX               # the stride of the GPU cases is one the 256 tile can address
    # M > 2^30
    assert _linear(M=(1 << 30) + 1) == -1 and _qkv(M=(1 << 30) + 1, seq=(1 << 30) + 1, nq_pad=1 << 31, nk_pad=1 << 31) == -1
    # a forced 256 tile whose 32-bit lane offsets cannot span 256 rows of x or w: OVG_E_UNSUPPORTED (the automatic choice falls back to 128)
    for kw in (dict(ldx=LD256_MAX + 8), dict(ldw=LD256_MAX + 8), dict(ldx=1 << 31), dict(ldw=1 << 40), dict(ldx=-64), dict(ldw=-64)):
        assert _linear(tile=L.TILE_256, N=256, ldy=256, **kw) == -4, kw
        assert _linear(tile=L.TILE_256, N=256, ldy=256, dtype=L.OVG_F16X2, x_lo=BIG, w_lo=BIG, y_lo=BIG, **kw) == -4, kw
    assert _qkv(tile=L.TILE_256, ldx=LD256_MAX + 8) == -4 and _qkv(tile=L.TILE_256, ldx=1 << 33) == -4
    assert _linear(tile=L.TILE_256, N=128) == -1                # (still OVG_E_ARG: a tile this shape cannot run at all)
    # FastDiv's range: row index / period below 2^22, the period an int
    q = 1 << 22
    assert _linear(epilogue=L.EPI_PATCH, table=BIG, p0=1, p1=2, M=q + 1) == -1
    assert _linear(epilogue=L.EPI_PATCH, table=BIG, p0=3, p1=5, M=3 * q + 1) == -1
    assert _linear(epilogue=L.EPI_PATCH, table=BIG, p0=1 << 31, p1=1 << 32, M=257) == -1
    assert _linear(epilogue=L.EPI_RES, res=BIG, ldres=128, gamma=BIG, inject=BIG, inj_period=1, M=q + 1) == -1
    assert _linear(epilogue=L.EPI_RES, res=BIG, ldres=128, gamma=BIG, inject=BIG, inj_period=1 << 31, M=257) == -1
    assert _qkv(M=q + 1, seq=1, nq_pad=64, nk_pad=64) == -1
    assert _qkv(M=6 * q + 6, seq=6 * q + 6, nq_pad=6 * q + 64, nk_pad=6 * q + 64 - (6 * q + 64) % 64 + 64, rope=1, rope_cos=BIG, rope_sin=BIG, max_pos=38,
                tokens_per_view=6, grid_w=1, n_special=5) == -1


def test_pixel_count_and_element_refusals_of_the_head_entries():
    lib = L.load()
    # ovg_conv: more than 2^30 output pixels
    p = L.ConvParams(x=BIG, ldx=64, w=BIG, bias=None, y=BIG, ldy=128, n_img=(1 << 30) + 1, H=1, W=1, Cin=64, Cout=128, w_rows=128, ksize=1, stride=1,
                     dtype=L.OVG_BF16)
    assert lib.ovg_conv(ctypes.byref(p), None) == -1
    p.n_img, p.H, p.W = 1 << 11, 1 << 10, (1 << 10) + 1         # the same through the image size
    assert lib.ovg_conv(ctypes.byref(p), None) == -1
    # ovg_dpt_tail: one source image of 2^31 elements (OVG_E_UNSUPPORTED: the three-launch form serves it)
    for H, W, ldx in ((4, 4, 1 << 27), (5, 4, ar.DPT_TAIL_LDX + 8), (1 << 10, 1 << 10, 2048)):
        t = L.DptTailParams(x=BIG, ldx=ldx, w1=BIG, ldw1=1152, w2=BIG, b2=BIG, val=BIG, conf=BIG, n_img=2, H=H, W=W, OH=20, OW=19, C=128, out_dim=4,
                            activation=1, dtype=L.OVG_BF16)
        assert H * W * ldx >= (1 << 31) and lib.ovg_dpt_tail(ctypes.byref(t), None) == -4, (H, W, ldx)


def test_int_narrowing_refusals_of_the_row_kernels():
    """ovg_pack_weights / ovg_im2col (k_pad / 8 is an int), ovg_dino_specials (one block per special row, an int block index),
    ovg_assemble_tokens (an int token index): the last accepted value goes on to the entry's NEXT check (an unknown dtype -> OVG_E_DTYPE;
    a NULL pointer -> OVG_E_ARG behind an OVG_E_UNSUPPORTED size check), the first refused one answers the limit's own code."""
    lib = L.load()
    top = 1 << 34

    def pack(k_pad, dtype=99):
        p = L.PackWeightsParams(src=BIG, lds=8, dst=BIG, ldd=k_pad, rows=1, k=8, k_pad=k_pad, dtype=dtype)
        return lib.ovg_pack_weights(ctypes.byref(p), None)

    assert pack(top - 8) == -2 and pack(top) == -1 and pack(top + 8) == -1 and pack(1 << 40) == -1

    def im2col(k_pad, dtype=99):
        p = L.Im2colParams(img=BIG, out=BIG, k_pad=k_pad, V=1, C=3, Hpx=14, Wpx=14, dtype=dtype, mode=0)
        return lib.ovg_im2col(ctypes.byref(p), None)

    assert im2col(top - 64) == -2 and im2col(top) == -1 and im2col(1 << 40) == -1

    def dino(V, n_reg, ldx=1024):
        p = L.DinoSpecialsParams(x=None, ldx=ldx, V=V, tokens_per_view=1374, cls=BIG, pos0=BIG, reg=BIG, n_reg=n_reg)
        return lib.ovg_dino_specials(ctypes.byref(p), None)

    for n_reg in (0, 1, 4, 6):
        last = ((1 << 31) - 1) // (1 + n_reg)                # V (1 + n_reg) <= 2^31 - 1, exactly
        assert last * (1 + n_reg) < (1 << 31) <= (last + 1) * (1 + n_reg)
        assert dino(last, n_reg) == -1 and dino(last + 1, n_reg) == -4 and dino(1 << 40, n_reg) == -4, n_reg      # -1: the NULL x behind the size check
    assert dino(5, -1) == -1 and dino(0, 4) == -1 and dino(5, 4, ldx=1022) == -1

    def assemble(tpv):
        p = L.AssembleParams(xd=None, ldxd=1024, norm_w=BIG, norm_b=BIG, eps=1e-6, camera_token=BIG, register_token=BIG, cam_add=BIG, placeholder=BIG,
                             out=BIG, ldo=1024, V=1, S=1, tokens_per_view=tpv, n_special=5, view0=0)
        return lib.ovg_assemble_tokens(ctypes.byref(p), None)

    assert assemble((1 << 31) - 1) == -1 and assemble(1 << 31) == -4 and assemble(1 << 40) == -4 and assemble(5) == -1


def test_count_refusals_of_attention_and_the_block_entries():
    lib = L.load()

    def attn(**kw):
        p = L.AttnParams(q=BIG, nq=64, nq_pad=64, nseg=1, out=BIG, ldo=1024, BH=16, dtype=L.OVG_BF16)
        p.seg[0].k, p.seg[0].vt, p.seg[0].nk, p.seg[0].nk_pad = BIG, BIG, 64, 64
        for k, v in kw.items():
            if k in ("nk", "nk_pad"):
                setattr(p.seg[0], k, v)
            else:
                setattr(p, k, v)
        return lib.ovg_flash_attn(ctypes.byref(p), None)

    # the last accepted value of each limit goes on to the next check (a misaligned q: OVG_E_ARG too, so the limit's own line is shown by
    # OVG_E_DTYPE behind every argument check: dtype 99 is looked at last)
    ok = dict(dtype=99)
    assert attn(**ok) == -2
    assert attn(nq=(1 << 27) - 1, nq_pad=1 << 27, BH=1, **ok) == -2 and attn(nq=1 << 27, nq_pad=1 << 27, BH=1, **ok) == -1
    assert attn(nk=(1 << 27) - 1, nk_pad=1 << 27, **ok) == -2 and attn(nk=1 << 27, nk_pad=1 << 27, **ok) == -1
    assert attn(BH=1 << 27, **ok) == -2 and attn(BH=(1 << 27) + 16, **ok) == -1
    assert attn(BH=1 << 26, nq=128, nq_pad=128, **ok) == -2 and attn(BH=1 << 26, nq=129, nq_pad=192, **ok) == -1      # 2^27 / more (entry, 64-row tile) units

    def block(entry, **kw):
        p = L.BlockParams(x_in=BIG, ld_in=1024, x_out=BIG, ld_out=1024, M=64, seq=64, BH=16, nq_pad=64, nk_pad=64, dtype=L.OVG_BF16,
                          ws_xn=BIG, ws_q=BIG, ws_k=BIG, ws_vt=BIG, ws_attn=BIG, ws_hid=BIG)
        for k, v in kw.items():
            setattr(p, k, v)
        return getattr(lib, entry)(ctypes.byref(p), None)

    for entry in ("ovg_block_forward", "ovg_block_attn_prologue", "ovg_block_attn_epilogue"):
        M = (1 << 30) + 64
        assert block(entry, M=M, BH=(M // 64) * 16) == -1, entry                 # more rows than ovg_qkv / ovg_linear take
        M = ((1 << 22) + 1) * 64
        assert block(entry, M=M, BH=(M // 64) * 16) == -1, entry                 # more sequences than the QKV epilogue's row / seq division holds
        M = 1 << 27
        assert block(entry, M=M, seq=M, BH=16, nq_pad=M, nk_pad=M) == -1, entry  # a sequence ovg_flash_attn's int indices cannot hold
        M = 255 * (1 << 22) + 255
        assert block(entry, M=M, seq=M, BH=16, nq_pad=M + 1, nk_pad=M + 1, rope=1, rope_cos=BIG, rope_sin=BIG, max_pos=38, tokens_per_view=255, grid_w=37) == -1, entry
        assert block(entry, M=64, rope=1, rope_cos=BIG, rope_sin=BIG, max_pos=38, tokens_per_view=1 << 31, grid_w=37) == -1, entry


# =============================================================================================
# the chunked guard checker reports what guarded() reports
# =============================================================================================
GUARD_SHAPES = (((5, 7), torch.float32, 11, 1), ((3, 4, 6), torch.bfloat16, 8, 0), ((9, 16), torch.float16, None, 2), ((2, 3), torch.uint8, 16, 1))


@pytest.mark.parametrize("chunk", [16, 48, 1000, 1 << 28])
def test_chunked_guard_checker_reports_the_same_first_and_last_byte_as_guarded(chunk):
    for shape, dtype, ld, spare in GUARD_SHAPES:
        va, ca = kg.guarded(shape, dtype, "cpu", ld=ld, guard_bytes=64, spare_rows=spare)
        vb, cb = kg.guarded_chunked(shape, dtype, "cpu", ld=ld, guard_bytes=64, spare_rows=spare, chunk_bytes=chunk)
        assert va.shape == vb.shape and va.stride() == vb.stride() and ca.buffer.numel() == cb.buffer.numel()
        assert va.data_ptr() - ca.buffer.data_ptr() == vb.data_ptr() - cb.buffer.data_ptr() == 64
        for v in (va, vb):                              # writes inside the view: no report
            v.fill_(1)
        ca("clean")
        cb("clean")
        inside = torch.zeros(ca.buffer.numel(), dtype=torch.bool)
        esz = va.element_size()
        inside[64:64 + (inside.numel() - 128) // esz * esz].view(torch.uint8).view(-1, esz).as_strided(
            tuple(shape) + (esz,), tuple(s * esz for s in va.stride()) + (1,)).fill_(1)
        outside = torch.nonzero(~inside.view(torch.bool)).flatten().tolist()
        rng = np.random.default_rng(chunk + len(outside))
        picks = [[outside[0]], [outside[-1]], [63], [64 + (inside.numel() - 128)], list(rng.choice(outside, 5, replace=False)), outside]
        if ld is not None and ld > shape[-1]:
            picks.append([64 + shape[-1] * esz])        # the first byte behind row 0
        for pick in picks:
            msgs = []
            for c in (ca, cb):
                c.buffer.fill_(kg.GUARD_BYTE)
                c.buffer[torch.tensor(pick)] = 0
                with pytest.raises(kg.GuardError) as e:
                    c("planted")
                msgs.append(str(e.value))
            assert msgs[0] == msgs[1] and "first byte %d " % (min(pick) - 64) in msgs[0] and "last byte %d " % (max(pick) - 64) in msgs[0], msgs


# =============================================================================================
# planted defects: a kernel that forms r * ld in 32 bits
# =============================================================================================
def test_a_32_bit_row_offset_is_reported_by_the_guard_checker_and_by_the_periodic_comparison():
    """The stride form at its real size on the CPU: 257 rows of 128 bytes, 16 MiB + 64 B apart, in a guarded_chunked buffer (4.3 GB). A store
    whose row offset is taken mod 2^32 puts row 256 at byte 16384 of the buffer -- in the gap behind row 0 -- and leaves the true row 256
    untouched: the guard checker names that byte, the comparison with the twin names row 256 = address_range.first_wrapped_row. A gather
    with the same defect returns for row 256 what lies at byte 16384: the periodic comparison names row 256."""
    rows, rowb, ldb = ar.ROWS16, 128, ar.FAR_STRIDE_BYTES
    first_bad = ar.first_wrapped_row(ldb)
    assert first_bad == 256 and (first_bad * ldb) % (1 << 32) == 16384 and ((first_bad - 1) * ldb) < (1 << 32)
    view, check = kg.guarded_chunked((rows, rowb), torch.uint8, "cpu", ld=ldb)
    buf = check.buffer.numpy()
    period = 7
    value = (np.arange(rows)[:, None] % period * 16 + np.arange(rowb)[None, :] % 16 + 1).astype(np.uint8)      # row m = pattern(m mod 7), never the guard byte
    assert not (value == kg.GUARD_BYTE).any()
    # the store with 32-bit offsets
    ar.strided_store(buf, check.guard_bytes, rows, ldb, rowb, value, wrap32=True)
    with pytest.raises(kg.GuardError) as e:
        check("32-bit offsets")
    assert "%d bytes outside" % rowb in str(e.value) and "first byte 16384 (row 0, col 16384)" in str(e.value) and "last byte %d " % (16384 + rowb - 1) in str(e.value)
    differs = np.nonzero((view.numpy() != value).any(1))[0]
    assert differs.tolist() == [first_bad], differs                        # what the comparison with the near twin names
    assert ar.first_aperiodic_row(view, period) == first_bad
    # the correct kernel (the same buffer, repaired: the stray row back to the guard pattern, the correct store over everything): nothing to report
    buf[check.guard_bytes + 16384:check.guard_bytes + 16384 + rowb] = kg.GUARD_BYTE
    ar.strided_store(buf, check.guard_bytes, rows, ldb, rowb, value)
    check("64-bit offsets")
    assert np.array_equal(view.numpy(), value) and ar.first_aperiodic_row(view, period) is None
    got = ar.strided_gather(buf[check.guard_bytes:], rows, ldb, rowb)
    assert ar.first_aperiodic_row(torch.from_numpy(got), period) is None
    # the gather with 32-bit offsets, on the correctly filled buffer
    got = ar.strided_gather(buf[check.guard_bytes:], rows, ldb, rowb, wrap32=True)
    assert ar.first_aperiodic_row(torch.from_numpy(got), period) == first_bad


def test_periodic_comparison_and_tiling_in_chunks():
    base = torch.arange(5 * 3, dtype=torch.float32).view(5, 3)
    t = ar.tile_periodic(base, 23)
    assert torch.equal(t, base[torch.arange(23) % 5]) and ar.first_aperiodic_row(t, 5, chunk_rows=4) is None
    for bad in (5, 11, 22):
        u = t.clone()
        u[bad, 2] += 1
        u[22, 0] = -u[22, 0]
        assert ar.first_aperiodic_row(u, 5, chunk_rows=4) == bad == ar.first_aperiodic_row(u, 5)
    z = torch.zeros(12, 2, dtype=torch.bfloat16)
    z[7, 1] = -0.0                                           # bit for bit: -0.0 is not 0.0
    assert ar.first_aperiodic_row(z, 3) == 7
    assert torch.equal(ar.tile_periodic(torch.arange(4.0), 10), torch.arange(10.0) % 4)
