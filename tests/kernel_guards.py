"""Guard bands, poisoned padding and a per-element error budget for the kernel tests (a plain helper module like gpu_selftest;
the host test test_kernel_guards_host.py proves on the CPU that each helper catches what it is for).

guarded()            an output view inside a larger byte buffer pre-filled with a finite non-zero pattern + a checker that every byte
                     outside the view is bit-unchanged afterwards (front / back guard, row gaps, spare rows)
poison_*()           large finite values of alternating sign in the padding a kernel must not depend on
elementwise_budget() |got - ref| <= u_out |ref| + c u_acc mag for EVERY element (gpu_selftest.report gates the tensor-global maximum only)
*_budget()           the constants c, each derived from the rounding points of its kernel (never fitted to a kernel's output)
conv_ref()           ovg_conv's float64 reference and magnitude (test_gpu_edges.py, test_gpu_head_edges.py, dpt_stages.py)
upsample_window()    the 16-bit roundings a bilinear kernel may hold per element; dpt_tail_budget() carries them through the fused output stage
                     (test_dpt_tail_budget_host.py); camera_tables_budget() for ovg_camera_tables (test_camera_tables_budget_host.py)
camera_*()           ovg_camera_head stage by stage from the buffers it leaves in its workspace: camera_ws_views() (the layout), camera_ksplit()
                     (the split-K plan), one budget per stage, rounding_window() for the overwritten 16-bit xn buffers, check_camera_stages() /
                     check_camera_round2() (test_camera_head_budget_host.py, test_gpu_camera_head_stages.py)
"""
import math

import torch

# 0xA5 in every byte: bf16 / f16 0xA5A5 (-2.9e-16 / -2.2e-2) and f32 0xA5A5A5A5 (-2.9e-16) are finite, so a read of a guard cannot make NaNs
GUARD_BYTE = 0xA5
POISON = 16384.0              # +-2^14: exact in bf16, f16 and f32, its square (2^28) still finite in f32
U_ACC = 2.0 ** -24            # f32 unit roundoff: every accumulator of the library
# unit roundoff of the stored dtype = half the spacing of its significand: f16 11 bits, f32 24 bits, and bf16 EIGHT bits (1 implicit + 7
# stored) -> 2^-8. (2^-9 is not attainable: round-to-nearest of 1.00394 to bf16 is 1.0078125, 3.9e-3 = 0.99 x 2^-8 away;
# test_kernel_guards_host.py pins this with torch's own cast.) f32x: the split-f16 mode's documented pair precision.
U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24, "f32x": 2.0 ** -22}
STATS = {"guarded_launches": 0, "numeric": 0, "refusals": 0}


class GuardError(AssertionError):
    pass


def guarded(shape, dtype, device, ld=None, guard_bytes=1 << 16, fill=GUARD_BYTE, spare_rows=0):
    """-> (view, check). `view` has `shape` and `dtype`; its second-to-last dimension has stride `ld` elements (default shape[-1]: dense),
    the leading dimensions are dense over that, and it sits `guard_bytes` behind the start of a byte buffer that also holds `spare_rows`
    rows and `guard_bytes` after the last one. Every byte of the buffer starts as `fill`. check(name) -- call it after a synchronize -- raises
    GuardError naming the first and last changed byte outside the view (offset relative to the view's first byte, row, column in elements)."""
    shape = tuple(int(s) for s in shape)
    esz = torch.empty((), dtype=dtype).element_size()
    cols = shape[-1]
    ld = cols if ld is None else int(ld)
    assert ld >= cols and guard_bytes % 16 == 0 and len(shape) >= 2
    rows = 1
    for s in shape[:-1]:
        rows *= s
    total = 2 * guard_bytes + (rows + spare_rows) * ld * esz
    total = (total + 15) // 16 * 16
    buf = torch.full((total,), fill, dtype=torch.uint8, device=device)
    strides = [1, ld]
    for s in reversed(shape[1:-1]):
        strides.append(strides[-1] * s)
    strides = tuple(reversed(strides[: len(shape)]))
    typed = buf[guard_bytes:guard_bytes + (total - 2 * guard_bytes) // esz * esz].view(dtype)
    view = typed.as_strided(shape, strides)
    assert view.data_ptr() % 16 == 0, "the ABI wants 16-byte aligned tensors"
    inside = torch.zeros(total, dtype=torch.bool, device=device)
    inside[guard_bytes:guard_bytes + (total - 2 * guard_bytes) // esz * esz].view(torch.uint8).view(-1, esz).as_strided(
        shape + (esz,), tuple(s * esz for s in strides) + (1,)).fill_(1)
    inside = inside.view(torch.bool)

    def check(name="guard"):
        bad = (buf != fill) & ~inside
        if bool(bad.any()):
            where = torch.nonzero(bad).flatten()
            first, last = int(where[0]) - guard_bytes, int(where[-1]) - guard_bytes

            def rc(off):
                return "byte %d (row %d, col %d)" % (off, off // (ld * esz) if off >= 0 else -1, (off % (ld * esz)) // esz if off >= 0 else -1)
            raise GuardError("%s: %d bytes outside the %s view were written; first %s, last %s" % (name, int(where.numel()), shape, rc(first), rc(last)))
        STATS["guarded_launches"] += 1

    check.buffer = buf
    check.guard_bytes = guard_bytes
    return view, check


def guarded_chunked(shape, dtype, device, ld=None, guard_bytes=1 << 16, fill=GUARD_BYTE, spare_rows=0, chunk_bytes=1 << 28):
    """guarded() for views that span several GiB (tests/test_gpu_address_range.py: a row stride of 16 MiB, 2^24 rows): the same layout, the
    same view and the same report, but check() keeps no mask of the buffer and makes no full-size temporary -- it walks the front guard,
    the gap behind each row (whole rows at a time, as a [rows, ld - cols] byte view) and the spare rows + back guard in steps of at most
    `chunk_bytes` bytes each. tests/test_address_range_host.py holds it to guarded()'s report on small shapes. (The layout lines repeat
    guarded()'s on purpose: guarded() itself is left as the existing tests pinned it.)"""
    shape = tuple(int(s) for s in shape)
    esz = torch.empty((), dtype=dtype).element_size()
    cols = shape[-1]
    ld = cols if ld is None else int(ld)
    assert ld >= cols and guard_bytes % 16 == 0 and len(shape) >= 2 and chunk_bytes > 0
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ldb, rowb = ld * esz, cols * esz
    total = 2 * guard_bytes + (rows + spare_rows) * ldb
    total = (total + 15) // 16 * 16
    buf = torch.full((total,), fill, dtype=torch.uint8, device=device)
    strides = [1, ld]
    for s in reversed(shape[1:-1]):
        strides.append(strides[-1] * s)
    strides = tuple(reversed(strides[: len(shape)]))
    typed = buf[guard_bytes:guard_bytes + (total - 2 * guard_bytes) // esz * esz].view(dtype)
    view = typed.as_strided(shape, strides)
    assert view.data_ptr() % 16 == 0, "the ABI wants 16-byte aligned tensors"

    def pieces():
        """(2-D byte view outside the tensor, buffer offset of its [0, 0], buffer bytes between its rows), each at most chunk_bytes."""
        for a, b in ((0, guard_bytes), (guard_bytes + rows * ldb, total)):        # front guard; spare rows + back guard
            for o in range(a, b, chunk_bytes):
                yield buf[o:min(o + chunk_bytes, b)].view(1, -1), o, 0
        gap = ldb - rowb
        if gap > 0:
            body = buf[guard_bytes:guard_bytes + rows * ldb].view(rows, ldb)
            for c0 in range(rowb, ldb, chunk_bytes):                               # (one column block unless a single gap exceeds a step)
                c1 = min(c0 + chunk_bytes, ldb)
                step = max(1, chunk_bytes // (c1 - c0))
                for r0 in range(0, rows, step):
                    yield body[r0:r0 + step, c0:c1], guard_bytes + r0 * ldb + c0, ldb

    fill64 = int.from_bytes(bytes([fill]) * 8, "little", signed=True)

    def check(name="guard"):
        count, first, last = 0, None, None
        for piece, origin, pitch in pieces():
            if piece.shape[1] % 8 == 0 and pitch % 8 == 0 and (piece.data_ptr() % 8) == 0:
                if not bool((piece.view(torch.int64) != fill64).any()):      # eight bytes per comparison; the bytes are looked at only where a word differs
                    continue
            bad = piece != fill
            n = int(bad.sum())
            if n:
                where = torch.nonzero(bad)
                off = origin + where[:, 0] * pitch + where[:, 1]
                lo, hi = int(off.min()), int(off.max())
                count, first, last = count + n, lo if first is None else min(first, lo), hi if last is None else max(last, hi)
        if count:
            first, last = first - guard_bytes, last - guard_bytes

            def rc(off):
                return "byte %d (row %d, col %d)" % (off, off // (ld * esz) if off >= 0 else -1, (off % (ld * esz)) // esz if off >= 0 else -1)
            raise GuardError("%s: %d bytes outside the %s view were written; first %s, last %s" % (name, count, shape, rc(first), rc(last)))
        STATS["guarded_launches"] += 1

    check.buffer = buf
    check.guard_bytes = guard_bytes
    return view, check


# ---------------------------------------------------------------------------------------------
# poisoned padding
# ---------------------------------------------------------------------------------------------
def poison_values(shape, dtype, device, scale=POISON):
    """+-scale, the sign alternating along the flattened index (so that sums of poison do not cancel pairwise per row: odd row lengths
    shift the phase), as `dtype`."""
    n = 1
    for s in shape:
        n *= int(s)
    i = torch.arange(n, device=device)
    v = torch.where((i + i // 7) % 2 == 0, scale, -scale).to(torch.float32)
    return v.reshape(tuple(shape)).to(dtype)


def poison_rows(t, first):
    """t [..., rows_pad, cols]: rows first.. of every leading entry <- poison (q rows nq..nq_pad, K rows nk..nk_pad)."""
    if t.shape[-2] > first:
        t[..., first:, :] = poison_values(t[..., first:, :].shape, t.dtype, t.device)
    return t


def poison_cols(t, first):
    """t [..., rows, cols_pad]: columns first.. <- poison (packed-weight / im2col K padding; f32 V^T columns nk..nk_pad)."""
    if t.shape[-1] > first:
        t[..., first:] = poison_values(t[..., first:].shape, t.dtype, t.device)
    return t


def vt_pos16(n_pad, device="cpu"):
    """idx[pos] = key stored at column pos of a 16-bit V^T row (header: inside every block of 32 keys column 8 g + 4 h + i holds
    key 16 h + 4 g + i); restated here so that the helper does not lean on the code under test."""
    pos = torch.arange(n_pad, device=device)
    k = pos & 31
    return (pos & ~31) | (((k >> 2) & 1) << 4) | (((k >> 3) & 3) << 2) | (k & 3)


def poison_vt(vt, nk, sixteen_bit):
    """vt [BH, 64, nk_pad]: the columns that hold keys nk..nk_pad (in the vt_pos16 order for the 16-bit dtypes) <- poison."""
    n_pad = vt.shape[-1]
    key = vt_pos16(n_pad, vt.device) if sixteen_bit else torch.arange(n_pad, device=vt.device)
    dead = torch.nonzero(key >= nk).flatten()
    if dead.numel():
        vt[..., dead] = poison_values(vt[..., dead].shape, vt.dtype, vt.device)
    return vt


# ---------------------------------------------------------------------------------------------
# the per-element comparator
# ---------------------------------------------------------------------------------------------
def elementwise_budget(name, got, ref, mag, u_out, c, extra=None, u_acc=U_ACC, quiet=False):
    """Asserts |got - ref| <= u_out |ref| + c u_acc mag (+ extra) for every element; got: the kernel's result, ref / mag (/ extra): float64,
    c: a number or a float64 tensor broadcastable to ref (a per-row constant). Returns the worst used fraction of the budget."""
    dev = ref.device if (ref.is_cuda and torch.is_tensor(mag) and mag.device == ref.device) else "cpu"    # the camera head's large references stay on their device
    got = got.detach().to(dev, torch.float64)
    ref = ref.detach().to(dev, torch.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    budget = u_out * ref.abs() + c * u_acc * mag.to(torch.float64)
    if extra is not None:
        budget = budget + extra
    budget = budget.expand_as(ref)
    err = (got - ref).abs()
    err[~torch.isfinite(got)] = float("inf")
    frac = err / budget.clamp_min(1e-300)
    frac[(err == 0)] = 0.0
    worst = float(frac.max()) if frac.numel() else 0.0
    if not quiet:
        print("[%s] %-52s budget used %.3f" % ("PASS" if worst <= 1.0 else "FAIL", name + ".elementwise", worst), flush=True)
    if worst > 1.0:
        idx = int(frac.flatten().argmax())
        pos = []
        for s in reversed(ref.shape):
            pos.append(idx % s)
            idx //= s
        flat = int(frac.flatten().argmax())
        raise AssertionError("%s: %d of %d elements over their budget; worst @%s got=%.9g ref=%.9g |err|=%.3e budget=%.3e" % (
            name, int((frac > 1.0).sum()), frac.numel(), list(reversed(pos)), float(got.flatten()[flat]), float(ref.flatten()[flat]),
            float(err.flatten()[flat]), float(budget.flatten()[flat])))
    STATS["numeric"] += 1
    return worst


MARGIN = 2.0     # over every derived constant: summation order, and the hardware exp2 / rcp / rsq approximations (about 1 ulp each, not pinned)


# ---- ovg_unproject (csrc/ovg_head.hip unproject_kernel) ---------------------------------------------------------------------------
# x_cam = (u - cu) d / fu and y_cam likewise are evaluated in double and rounded to f32 (one rounding each, as the numpy reference does);
# world = R (x_cam, y_cam, d) + t is evaluated in double and rounded to f32 on store (elementwise_budget's u_out |ref|). The double
# arithmetic contributes nothing at f32 scale, so an output is within u_out |ref| + 1 u_acc (|R| |cam|): C_UNPROJECT = MARGIN x 1 on
# mag = |R| |cam| + |t|.
C_UNPROJECT = 2.0 * 1


def unproject_budget(depth, u, v, cam):
    """depth [rows, W] float64, u [1, W] / v [rows, 1] pixel coordinates (float64), cam [16] float64 (R row-major, t, fu, fv, cu, cv), all
    on one device -> (ref, mag) [rows, W, 3] float64 for elementwise_budget(..., U_OUT["f32"], C_UNPROJECT)."""
    R, t = cam[:9].view(3, 3), cam[9:12]
    pts = torch.stack([(u - cam[14]) * depth / cam[12], (v - cam[15]) * depth / cam[13], depth], -1)
    return pts @ R.t() + t, pts.abs() @ R.abs().t() + t.abs()


# ---- GEMM ----------------------------------------------------------------------------------
# acc = sum_k x_k w_k in f32 on the matrix pipe. 16-bit operands: every product is exact in f32, so the error is the accumulation's alone:
# K - 1 additions, each within u_acc of a partial sum that never exceeds sum |x||w|  ->  (K - 1) u_acc (|x| |w|^T)  (the standard
# gamma_(K-1) bound, whatever the order). f32 operands: one more rounding per product (K). + bias: one addition (1) on |acc| + |bias|.
# Split-f16 (reference = the float64 product of the hi + lo VALUES): three MFMA chains (3 K roundings at most), and the dropped lo x lo
# term: |lo| <= 2^-11 |hi| on both sides -> 2^-22 |x||w| = 4 u_acc per product (4).
def gemm_mag(x, w, bias):
    m = x.abs().double() @ w.abs().double().t()
    return m if bias is None else m + bias.abs().double()


def gemm_c(K, mode):
    return MARGIN * ({"bf16": K, "f16": K, "f32": 2 * K, "f32x": 3 * K + 4}[mode] + 1)


# GELU(z) = z/2 (1 + erf(z / sqrt 2)) evaluated in f32 on z = acc + bias: |d gelu / dz| <= 1.13 carries z's error (1.13 x the GEMM constant);
# the evaluation: z / sqrt 2 (1 rounding), an f32 erf within 4 ulp of 1 (8 u_acc, times |z| / 2 -> 4 |z|), the sum and two products
# (3 on |ref| <= |z|). |z| <= mag, so everything is charged to mag: 1.13 c_gemm + 8.
def gelu_c(K, mode):
    return 1.13 * gemm_c(K, mode) + MARGIN * 8


# RES: y = res + gamma (acc + bias) [+ inject] in f32: mag = |res| + |gamma| mag_gemm [+ |inject|]; the product and the one or two sums add 3
# roundings to the GEMM's. PATCH: y = acc + bias + table: mag = mag_gemm + |table|, one more sum.
def res_c(K, mode):
    return gemm_c(K, mode) + MARGIN * 3


def res_mag(res, gamma, mg, inject=None):
    m = res.abs().double() + gamma.abs().double() * mg
    return m if inject is None else m + inject.abs().double()


# ---- LayerNorm (rows of n values, two-pass in f32) -----------------------------------------
# y = (x - mean) rstd w + b, one wave per row (csrc/ovg_elem.hip row_stats, csrc/ovg_head.hip): a lane adds its n / 256 float4 groups, each
# group summed in at most 3 additions and the groups one after the other (n / 256), then a 6-level butterfly: a sum of n terms is within
# d u_acc sum|terms| with d = 3 + n / 256 + 6 (13 for n = 1024, 17 for 2048; a fully sequential lane would be n / 64 + 6 = 22 / 38).
# mag = |w| |x - mean| rstd + |b| carries: the subtraction, two products, one sum (4), and rstd's relative error: the squares (1 rounding
# each) and their sum (d), halved by the square root, then the scale by 1 / n, + eps, sqrt, reciprocal (4): (d + 1) / 2 + 4.
# The MEAN's error does not scale with |x - mean|: mean is within d u_acc mean|x|, and y moves by |w| rstd times that: the `extra` term
# (x 2 margin like the rest). A one-pass E[x^2] - mean^2 kernel breaks this by orders of magnitude on rows whose mean dwarfs their spread.
def layernorm_budget(x, w, b, eps):
    """-> (ref, mag, c, extra), all float64, for x [rows, n] f32 values."""
    x, w, b = x.double(), w.double(), b.double()
    n = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = (x - mean) * rstd * w + b
    mag = w.abs() * (x - mean).abs() * rstd + b.abs()
    depth = 3 + max(n // 256, 1) + 6
    c = MARGIN * (4 + (depth + 1) / 2.0 + 4)
    extra = MARGIN * depth * U_ACC * x.abs().mean(-1, keepdim=True) * rstd * w.abs()
    return ref, mag, c, extra


# ---- attention -----------------------------------------------------------------------------
# out = sum_k p_k v_k / sum_k p_k, p_k = 2^(s_k - m), s = q . k (q pre-scaled, 64 products accumulated in f32). mag = sum_k p_k |v_k| / sum_k p_k.
#  * P is rounded to the operand format before the PV product (u_p = 2^-8 bf16, 2^-11 f16, 2^-22 for the split pair, 0 for f32): numerator
#    within u_p mag; the denominator (summed from rounded or unrounded p) within u_p, i.e. |out| u_p <= u_p mag           -> 2 u_p / u_acc
#  * s: 64 (f32 operands 128, split 3 x 64 + 4) u_acc sum_d |q_d||k_d| = e_s log2 units; s - m: one rounding on |s - m| <= 2 max|s|;
#    exp2: 2 ulp. p moves by ln2 (e_s + 2 u_acc max|s|) + 2 u_acc relative, numerator and denominator both       -> 2 (ln2 (64 A + 2 S) + 2)
#    with A = max_k sum_d |q_d||k_d| and S = max_k |s_k| of the row
#  * the PV and row-sum accumulations over nk keys in f32, the running rescales (one product per 64-key tile), the final division
#                                                                                                               -> nk + nk / 64 + 2
# c is per query row (A, S depend on the row).
def attn_budget(q, k, v, mode, p_bits=None):
    """q [BH, nq, 64], k / v [BH, nk, 64] float64 (the dtype-rounded values) -> (ref [BH, nq, 64], mag, c [BH, nq, 1], lse [BH, nq])."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2)
    p = torch.softmax(s * math.log(2.0), -1)
    ref, mag = p @ v, p @ v.abs()
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    S = s.abs().amax(-1, keepdim=True)
    nk = k.shape[-2]
    u_p = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32x": 2.0 ** -22, "f32": 0.0}[mode] if p_bits is None else 2.0 ** -p_bits
    kd = {"bf16": 64, "f16": 64, "f32": 128, "f32x": 196}[mode]
    c = MARGIN * (2 * u_p / U_ACC + 2 * (math.log(2.0) * (kd * A + 2 * S) + 2) + nk + nk / 64.0 + 2)
    lse = torch.logsumexp(s * math.log(2.0), -1) / math.log(2.0)
    return ref, mag, c, lse


def attn_p_floor(v, mode):
    """P in an f16 format (f16 mode; both planes of the split pair) has an ABSOLUTE quantum as well: below 2^-14 the spacing is 2^-24, so
    every key's weight is within 2^-25 whatever its size. Relative to the row sum l that is 2^-25 / l per key: numerator within
    2^-25 sum_k |v_k| / l, the denominator's share |out| nk 2^-25 / l <= the same -> 2 x 2^-25 sum_k |v_k| / l (x margin).
    l >= the weight of the row's largest key: 1 in the lazy-rescale kernels (the reference maximum never exceeds the running maximum:
    split-f16 mode, the f16 default), but 2^-4 in the f16 SPECULATIVE kernels, which anchor 4 log2 units above the first key tile's maximum
    to leave head-room below f16's 2^16 (csrc/ovg_attn16.h, AnchorMargin<f16_t>): every f16 variant is gated with l >= 2^-4.
    bf16 has f32's exponent range: no floor. v [BH, nk, 64] float64 -> [BH, 1, 64]."""
    if mode not in ("f16", "f32x"):
        return 0.0
    inv_l = 2.0 ** 4 if mode == "f16" else 1.0
    return MARGIN * 2 * 2.0 ** -25 * inv_l * v.double().abs().sum(-2, keepdim=True)


def f16_subnormal_floor(mode):
    """Half the f16 subnormal spacing: the absolute floor of an f16 store (and of the lo plane of a split-f16 pair), added as `extra`."""
    return {"f16": 2.0 ** -25, "f32x": 2.0 ** -25}.get(mode, 0.0)


# ---- q / k of ovg_qkv with q/k-norm and RoPE ------------------------------------------------
# z = the GEMM's 64 values of one (token, head), each within ez = c_gemm u_acc mag_gemm. y = LayerNorm_64(z) w + b, then the rotation
# out = y cos + rot(y) sin (rot pairs j with j +- 16 inside each half of the head), then q only: x q_scale.
#  * ez through the LayerNorm (first order; y_i = zh_i w_i + b_i, zh = (z - mean) rstd):
#      |dy_i| <= |w_i| rstd (ez_i + mean(ez) + |zh_i| mean(|zh| ez))
#  * the LayerNorm's own f32 rounding as in layernorm_budget with n = 64 in ANY order (d = 64): (4 + (d + 1) / 2 + 4) u_acc (|w||zh| + |b|)
#    + d u_acc mean|z| rstd |w|, x margin
#  * the rotation carries both errors through |cos|, |sin| and adds two products and a sum: 3 u_acc (|y cos| + |rot(y) sin|), x margin
#  * q_scale: the error scales with it; the product's own rounding is left to the caller (one more u_acc |ref|).
def qk_norm_rope_error(z, ez, w, b, eps, pos, cos, sin, scale=1.0):
    """z, ez [B, H, n, 64] float64; w, b [64]; pos [B, n, 2] (y, x) indices into cos / sin [max_pos, 32] -> absolute error bound like z."""
    w, b = w.double(), b.double()
    mean = z.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + eps)
    zh = (z - mean) * rstd
    d = 64
    ey = w.abs() * rstd * (ez + ez.mean(-1, keepdim=True) + zh.abs() * (zh.abs() * ez).mean(-1, keepdim=True))
    ey = ey + MARGIN * U_ACC * ((4 + (d + 1) / 2.0 + 4) * (w.abs() * zh.abs() + b.abs()) + d * z.abs().mean(-1, keepdim=True) * rstd * w.abs())
    y = zh * w + b

    def rope_abs(t):
        def one_axis(x, p):
            c = torch.nn.functional.embedding(p, cos.double().abs())[:, None, :, :]
            s_ = torch.nn.functional.embedding(p, sin.double().abs())[:, None, :, :]
            h = x.shape[-1] // 2
            return x * c + torch.cat((x[..., h:], x[..., :h]), dim=-1) * s_
        a, b_ = t.chunk(2, dim=-1)
        return torch.cat((one_axis(a, pos[..., 0]), one_axis(b_, pos[..., 1])), dim=-1)
    return scale * (rope_abs(ey) + MARGIN * 3 * U_ACC * rope_abs(y.abs()))


# ---- ovg_conv (NHWC implicit GEMM) ---------------------------------------------------------------
def conv_ref(x, w, bias, cout, k, stride, up, relu, a1, a2, pos):
    """x [n, H, W, cin], w [rows, k k cin] taps-major, bias [cout] / a1 / a2 [n, OH, OW, cout] / pos = (pos_x [OW, cout/2], pos_y [OH, cout/2])
    or None, all float64 (the values of the stored operands) -> (ref, mag): the convolution (up > 1: ConvTranspose with kernel = stride = up,
    rows ordered (dy, dx, co)) + bias + adds + tables, ReLU'd if asked, and the magnitude sum |x||w| + |bias| + |adds| + |table| that the
    accumulation's budget scales with."""
    n, H, W, cin = x.shape
    if up > 1:
        y = (x.reshape(-1, cin) @ w.t()).reshape(n, H, W, up, up, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, H * up, W * up, cout)
        m = (x.abs().reshape(-1, cin) @ w.abs().t()).reshape(n, H, W, up, up, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, H * up, W * up, cout)
    else:
        wt = w[:cout].reshape(cout, k, k, cin).permute(0, 3, 1, 2)
        y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt, None, stride=stride, padding=k // 2).permute(0, 2, 3, 1)
        m = torch.nn.functional.conv2d(x.abs().permute(0, 3, 1, 2), wt.abs(), None, stride=stride, padding=k // 2).permute(0, 2, 3, 1)
    y, m = y.contiguous(), m.contiguous()
    for t in (bias, a1, a2):
        if t is not None:
            y, m = y + t, m + t.abs()
    if pos is not None:
        half = cout // 2
        for arr, f in ((y, lambda t: t), (m, torch.abs)):
            arr[..., :half] += f(pos[0])[None, None]
            arr[..., half:] += f(pos[1])[None, :, None]
    return (torch.relu(y) if relu else y), m


# ---- bilinear resize (align_corners = True) ---------------------------------------------------
# The specification both kernels document (csrc/ovg_head.hip upsample_kernel, csrc/ovg_dpt_tail.h xgeo / ygeo) and ATen implements:
#   s = (in - 1) / (out - 1) an f32 quotient, f = s o an f32 product, i0 = min(int(f), in - 1), i1 = i0 + (i0 < in - 1), l = f - i0 (exact:
#   f < 2^24 and i0 = floor(f) unless clamped, where l stays tiny), value = (1-ly)(1-lx) a + (1-ly) lx b + ly (1-lx) c + ly lx d + table.
# The coordinate arithmetic is part of the specification: a float64 s o differs from the f32 product by up to u f, which moves the weights by
# (in - 1) u -- orders of magnitude more than the interpolation's own rounding.
# `fused` evaluates a DEVIATION from it, exactly: `fx = sx * oc; lx = fx - x0` contracted into one multiply-subtract, l' = fl(s o - i0) with
# the product unrounded (the default -ffp-contract=fast would permit it; a product of two f32 values and its difference with an integer
# < 2^24 are exact in float64). It moves l by up to half an ulp of f, and the window below is sharp enough to tell the two apart: the host
# test uses it as a mutant, and on the MI355X ovg_upsample held the plain form on every one of 1.1e7 elements of a 148 -> 296 map while the
# fused form left 0.3 % (bf16) / 1.8 % (f16) of them outside the window.
# An output side of ONE pixel has no (out - 1) to divide by: the header of ovg_upsample documents s = 0 for it (source row / column 0 with
# weight 1, what ATen's area_pixel_compute_scale gives for align_corners with an output size <= 1), whatever the input side.
def _axis_spec(n_in, n_out, fused):
    if n_out > 1:
        s = torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32)
    else:
        s = torch.zeros((), dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    f = s * o
    i0 = f.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l = ((s.double() * o.double() - i0.double()).float() if fused else f - i0.float()).double()
    return i0, i1, l


def bilinear_spec(x, OH, OW, pos=None, fused=(False, False)):
    """x [n, H, W, C] float64 (the values of the stored inputs), pos = (pos_x [OW, C/2], pos_y [OH, C/2]) or None ->
    (up, mag) [n, OH, OW, C] float64: the interpolated value + table entry with the weights of the specification above, the four taps and the
    table combined in float64, and its magnitude sum w |tap| + |table|. fused = (y, x): the contracted form of l per axis (a mutant, see above)."""
    x = x.double()
    n, H, W, C = x.shape
    y0, y1, ly = _axis_spec(H, OH, fused[0])
    x0, x1, lx = _axis_spec(W, OW, fused[1])
    ly, lx = ly.view(1, OH, 1, 1), lx.view(1, 1, OW, 1)
    up, mag = torch.zeros(n, OH, OW, C, dtype=torch.float64), torch.zeros(n, OH, OW, C, dtype=torch.float64)
    for yi, wy in ((y0, 1.0 - ly), (y1, ly)):
        for xi, wx in ((x0, 1.0 - lx), (x1, lx)):
            tap = x[:, yi][:, :, xi]
            up += wy * wx * tap
            mag += wy * wx * tap.abs()
    if pos is not None:
        half = C // 2
        px, py = pos[0].double()[None, None, :, :], pos[1].double()[None, :, None, :]
        up[..., :half] += px
        up[..., half:] += py
        mag[..., :half] += px.abs()
        mag[..., half:] += py.abs()
    return up, mag


# The f32 value a kernel holds before its 16-bit store is within C_UP u_acc mag of `up`:
#   both kernels: hx = fl(1 - lx), hy = fl(1 - ly): one rounding each (lx, ly themselves are exact, see above)
#   ovg_dpt_tail.h phase 1: w00 = fl(hy hx) carries 3 roundings, w01 = fl(hy lx) and w10 = fl(ly hx) 2, w11 = fl(ly lx) 1 -> at most 3 on
#     sum w |tap|; then four FMAs o = fma(w, tap, o) starting from the table entry, one rounding each on a partial sum <= mag -> 4.  Total 7.
#   upsample_kernel: hy (hx a + lx b) + ly (hx c + lx d) + table: hx a: hx's rounding + the product's (2), lx b: 1, their sum 1 -> 3 on the
#     inner sum; times hy: its rounding + the product's -> 5; the outer sum 1 -> 6; + table 1 -> 7 (a contraction to FMAs only removes roundings).
C_UP = MARGIN * 7


def round16(v, mode):
    """float64 -> the nearest value of the 16-bit format, ties to even, as float64, WITHOUT a detour through f32 (a double rounding could
    cross a tie): the quantum is 2^(e - bits) for |v| in [2^(e-1), 2^e), not below the format's subnormal spacing. Monotone."""
    bits, qmin = {"bf16": (8, -133), "f16": (11, -24)}[mode]
    v = v.double()
    _, e = torch.frexp(v)
    q = torch.ldexp(torch.ones_like(v), (e - bits).clamp_min(qmin))
    return torch.round(v / q) * q


def upsample_window(x, OH, OW, pos, mode):
    """The 16-bit map a correct kernel may hold. -> dict: up / mag (the specification, float64), r16 = round16(up) (what the reference
    chain continues with), lo16 <= hi16 (the roundings of the two ends of [up - e_up, up + e_up],
    e_up = C_UP u_acc mag: rounding is monotone, so the kernel's value lies between them), delta = max(hi16 - r16, r16 - lo16) (zero
    wherever both ends round to r16: there the kernel must hold exactly r16), window = lo16 != hi16."""
    up, mag = bilinear_spec(x, OH, OW, pos)
    e_up = C_UP * U_ACC * mag
    r16, lo16, hi16 = round16(up, mode), round16(up - e_up, mode), round16(up + e_up, mode)
    return {"up": up, "mag": mag, "r16": r16, "lo16": lo16, "hi16": hi16, "delta": torch.maximum(hi16 - r16, r16 - lo16), "window": lo16 != hi16}


def check_upsampled_map(name, got, win):
    """The strict gate of a 16-bit upsampled map: lo16 <= got <= hi16 for every element, i.e. bit-equal to the reference outside the
    rounding window and one of the admissible roundings inside it. -> (share of elements inside the window, share that differs from r16)."""
    got = got.detach().double().cpu()
    bad = ~((got >= win["lo16"]) & (got <= win["hi16"]))
    differs = got != win["r16"]
    share, dshare = float(win["window"].double().mean()), float(differs.double().mean())
    print("[%s] %-52s window holds %.3f%% of the map, %d elements differ from the reference's rounding, %d outside the window" % (
        "FAIL" if bool(bad.any()) else "PASS", name + ".window", 100 * share, int(differs.sum()), int(bad.sum())), flush=True)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError("%s: %d of %d map elements are not an admissible rounding; first @flat %d got=%.9g lo=%.9g hi=%.9g up=%.12g" % (
            name, int(bad.sum()), bad.numel(), i, float(got.flatten()[i]), float(win["lo16"].flatten()[i]), float(win["hi16"].flatten()[i]),
            float(win["up"].flatten()[i])))
    STATS["numeric"] += 1
    return share, dshare


# ---- the fused DPT output stage (csrc/ovg_dpt_tail.h; the same arithmetic as ovg_upsample -> ovg_conv -> ovg_dpt_out) -----------
# up16 (above) -> h = relu(conv3x3(up16, w1) + b1) -> o = w2 h + b2 -> val = exp(o) | sign(o) expm1(|o|), conf = 1 + exp(o).
#  * hidden layer: the kernel's map differs from r16 by at most delta per element (zero outside the window), which the convolution carries
#    as conv(|w1|, delta); its own f32 accumulation over K = 9 x 128 exact products + the bias is the GEMM bound on
#    mag_h = conv(|w1|, |r16|) + |b1|:  e_h = conv(|w1|, delta) + gemm_c(1152) u_acc mag_h.  (|r16| <= the kernel's |map| + delta: second order.)
#  * ReLU is 1-Lipschitz: e_h passes unchanged.
#  * output layer, plain f32: 32 products (one rounding each unless fused) and the bias, summed as 8 FMAs per lane, a 4-lane exchange and the
#    bias (kernel), or sequentially (dpt_out_kernel): a term passes through at most 32 additions in any order -> 33 on mag_o = |w2| h + |b2|:
#    e_o = |w2| e_h + C_OUT u_acc mag_o.
#  * activations: exp(o + d) - exp(o) = exp(o) expm1(d); sign(o) expm1(|o|) has the derivative exp(|o|) and is odd, and expm1 is
#    superadditive, so across zero too |f(o + d) - f(o)| <= exp(|o|) expm1(|d|). The confidence 1 + exp(o) carries the factor on exp(o) ALONE:
#    a low-confidence pixel (exp(o) << 1) gets a budget of expm1(e_o) exp(o) + one rounding of 1 + exp(o), not a share of the 1.
#  * expf / expm1f: the device library documents <= 3 ulp = 6 u_acc relative for both (OpenCL full-profile bounds, which it meets); the final
#    f32 rounding (val: inside those 3 ulp; conf: the addition) is elementwise_budget's u_out |ref|.
C_OUT = MARGIN * 33
C_EXP = MARGIN * 6


def conv3x3_nhwc(x, w):
    """x [n, H, W, C] float64, w [co, 9 C] taps-major (tap = 3 ky + kx, as ovg_conv orders them) -> the zero-padded 3 x 3 convolution
    [n, H, W, co], as nine matrix products."""
    n, H, W, C = x.shape
    xp = torch.zeros(n, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x
    y = torch.zeros(n, H, W, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + H, kx:kx + W] @ w[:, (3 * ky + kx) * C:(3 * ky + kx + 1) * C].double().t()
    return y


def dpt_tail_budget(x, OH, OW, pos, w1, b1, w2, b2, activation, mode):
    """x [n, H, W, 128] / w1 [>= 32, 1152] (the 16-bit values), b1 [32] or None, w2 [od, 32], b2 [od] -> dict with the float64 chain
    (val [n, OH, OW, od - 1], conf [n, OH, OW]) and, per output, what elementwise_budget takes: *_mag, *_c, *_extra; + the window dict."""
    win = upsample_window(x, OH, OW, pos, mode)
    w1 = w1[:32].double()
    b1 = torch.zeros(32, dtype=torch.float64) if b1 is None else b1.double()
    w2, b2 = w2.double(), b2.double()
    h = conv3x3_nhwc(win["r16"], w1) + b1
    mag_h = conv3x3_nhwc(win["r16"].abs(), w1.abs()) + b1.abs()
    e_h = conv3x3_nhwc(win["delta"], w1.abs()) + gemm_c(9 * 128, mode) * U_ACC * mag_h
    hr = torch.relu(h)
    o = hr @ w2.t() + b2
    mag_o = hr @ w2.abs().t() + b2.abs()
    e_o = e_h @ w2.abs().t() + C_OUT * U_ACC * mag_o
    ov, oc = o[..., :-1], o[..., -1]
    out = {"win": win, "o": o, "e_o": e_o, "c": C_EXP}
    if activation == "exp":
        out["val"], out["val_mag"] = torch.exp(ov), torch.exp(ov)
    else:
        out["val"], out["val_mag"] = torch.sign(ov) * torch.expm1(ov.abs()), torch.exp(ov.abs())
    out["val_extra"] = out["val_mag"] * torch.expm1(e_o[..., :-1])
    out["conf"], out["conf_mag"] = 1.0 + torch.exp(oc), torch.exp(oc)
    out["conf_extra"] = out["conf_mag"] * torch.expm1(e_o[..., -1])
    return out


def check_dpt_tail(name, val, conf, B, quiet=False):
    """Both outputs of the stage against dpt_tail_budget's result, every element. -> the worst used fraction of the two."""
    a = elementwise_budget(name + ".val", val, B["val"], B["val_mag"], U_OUT["f32"], B["c"], extra=B["val_extra"], quiet=quiet)
    b = elementwise_budget(name + ".conf", conf, B["conf"], B["conf_mag"], U_OUT["f32"], B["c"], extra=B["conf_extra"], quiet=quiet)
    return max(a, b)


DPT_TAIL_GATE = {"bf16": 4e-3, "f16": 5e-4}      # gpu_selftest.test_heads' global gates of the stage (max error / tensor maximum)

# The shapes of the stage that the host test (the f32 twin and its mutants against the budget) and the GPU test (the kernels) share.
# n = 0: as many images as give every workgroup two or three tiles with a partial last round (the GPU test takes it from the device; the
# budget does not depend on it, the host test runs 3). Tiles are 16 rows x 14 columns of output. Ratios (in - 1) / (out - 1) are non-dyadic
# where the shape is free: a dyadic ratio puts exact ties ((a + b) / 2 of two 16-bit values) into the window.
#               n  H   W   OH  OW  od  activation  tables  b1     conf_ramp
DPT_TAIL_CASES = {
    "persist_exp_pos":  (0, 9, 11, 33, 29, 2, "exp", True, True, False),       # 3 x 3 tiles per image, the last row / column of tiles one pixel wide
    "persist_exp":      (0, 9, 11, 33, 29, 2, "exp", False, True, False),
    "persist_inv_pos":  (0, 9, 11, 33, 29, 4, "inv_log", True, True, False),
    "persist_inv":      (0, 9, 11, 33, 29, 4, "inv_log", False, True, False),
    "out_dim3":         (2, 7, 6, 20, 19, 3, "inv_log", True, True, False),
    "no_b1":            (2, 7, 6, 20, 19, 2, "exp", True, False, False),
    "oh2":              (2, 5, 4, 2, 31, 4, "inv_log", True, True, False),
    "ow2":              (2, 4, 5, 35, 2, 2, "exp", True, True, False),
    "whole_tiles":      (1, 8, 7, 32, 28, 4, "inv_log", True, True, False),    # OH = 16 k, OW = 14 k (k + 1: the persist shapes)
    "src_1xW":          (2, 1, 6, 18, 15, 4, "inv_log", False, True, False),   # sy = 0: dy = 0 for every row
    "src_Hx1":          (2, 7, 1, 17, 16, 2, "exp", True, True, False),        # sx = 0: x1 = x0 for every column
    "downscale":        (2, 20, 23, 15, 17, 4, "inv_log", True, True, False),  # an output smaller than the source: accepted, must equal the reference
    "conf_ramp":        (1, 7, 6, 20, 19, 2, "exp", False, True, True),        # confidences from below 1 + 1e-2 to above 10 (asserted on the reference)
}


def dpt_tail_inputs(case, mode, n=None):
    """-> dict of CPU tensors for a DPT_TAIL_CASES entry: x [n, H, W, 128] and w1 [32, 1152] in the 16-bit dtype, b1 / w2 / b2 f32,
    pos (pos_x [OW, 64], pos_y [OH, 64]) f32 or None. conf_ramp: a spatial ramp in x and a scaled confidence row of w2 / b2 spread exp(o)
    over three decades (plain randn weights leave every confidence near 2, where a flush of small exp(o) to zero goes unseen)."""
    n0, H, W, OH, OW, od, act, pos, has_b1, ramp = DPT_TAIL_CASES[case]
    n = n if n is not None else (n0 if n0 else 3)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[mode]
    g = torch.Generator().manual_seed(1000 + sorted(DPT_TAIL_CASES).index(case))
    x = torch.randn(n, H, W, 128, generator=g)
    w1 = torch.randn(32, 9 * 128, generator=g) * (9 * 128) ** -0.5
    b1 = torch.randn(32, generator=g) * 0.3
    w2, b2 = torch.randn(od, 32, generator=g) * 0.2, torch.randn(od, generator=g) * 0.1
    ps = (torch.randn(OW, 64, generator=g) * 0.1, torch.randn(OH, 64, generator=g) * 0.1) if pos else None
    if ramp:
        x = 0.5 * x + torch.linspace(-2.0, 2.0, W).view(1, 1, W, 1) * torch.sign(torch.randn(128, generator=g))
        w2[-1] *= 3.0
        b2[-1] = 0.3
    return {"x": x.to(dt), "w1": w1.to(dt), "b1": b1 if has_b1 else None, "w2": w2, "b2": b2, "pos": ps, "OH": OH, "OW": OW, "act": act, "od": od, "n": n}


# ---- ovg_camera_tables (csrc/ovg_camtab.hip) -------------------------------------------------
# enc [B, Sc, 9] = (t / scale, quaternion xyzw, fov_h, fov_w) of the selected cameras relative to the first, a fixed short chain of f32
# operations on exact inputs E_r = [R_r | t_r], E_0; u = u_acc, x MARGIN throughout:
#  * c = -R_0^T t_0: 3 products, 2 sums -> within 3 u m0, m0_j = sum_k |R_0[k][j]| |t_0[k]| (and |c_j| <= m0_j)
#  * t_i = sum_j E[i][j] c_j + E[i][3]: 4 terms (4) + the inherited 3 -> e_t = 7 u mag_t, mag_t_i = sum_j |R[i][j]| m0_j + |t_r[i]|
#  * scale = max(mean_r |t(r) - t(0)|, 1e-6): the norm and the clamp are 1-Lipschitz, so it moves by at most mean_r sum_i (e_t_i(r) + e_t_i(0))
#    + the norm's own roundings (difference, squares, their sum halved by the root, the root: 4 u dist) + the sum over the cameras (a lane adds
#    ceil(Sc / 256) values, then an 8-level tree) + the division: e_s. t / scale then carries (e_t + |t / scale| e_s) / (scale - e_s) + the division.
#    With all cameras at one position scale is the clamp, 1e-6, and e_t / 1e-6 is the honest conditioning of that output.
#  * R = R_r R_0^T: 3 exact-input products -> e_R = 3 u mR, mR = |R_r| |R_0|^T. raw_b = 1 +- R00 +- R11 +- R22: three additions on a
#    magnitude <= 1 + |R00| + |R11| + |R22| + the three e_R: e_raw; q_best = sqrt(raw_best) >= 1 (the four raw values sum to 4):
#    relative rho = e_raw / (2 raw_best) + u. The picked candidate row: q_best^2 (2 rho + u) or R[a][b] +- R[b][a] (2 max e_R + u (|Rab| + |Rba|)),
#    divided by den = 2 max(q_best, 0.1) >= 2 (relative rho + u): every component within (2 max e_R + 2 u max|R|) / den + |q| (3 rho + 2 u).
#    (The branch choice and the sign normalisation are discontinuous: the test keeps its cameras away from ties and from w = 0 and asserts so.)
#  * fov = 2 atanf((size / 2) / f): the quotient's rounding moves atan(a) by a / (1 + a^2) u <= atan(a) u; atanf within 5 ulp (the OpenCL bound
#    the device library meets) -> 11 u |fov|.
# tables: emb = pose_w enc + pose_b, 9 FMAs and a sum (10 u on its magnitude) + |pose_w| e_enc; row = adapt_w emb + adapt_b on the exact-f32
# matrix pipe: gemm_c(1024, "f32") u on its magnitude + |adapt_w| e_emb. Views without a camera hold adapt_b exactly.
def camera_tables_budget(ext, intr, idx, hw, pose_w, pose_b, adapt_w, adapt_b):
    """ext [B, S, 3, 4], intr [B, S, 3, 3] f32, idx: list of views, pose_w [G * 1024, 9], pose_b [G * 1024], adapt_w [G, 1024, 1024], adapt_b [G, 1024]
    -> dict: enc [B, Sc, 9], e_enc (absolute), tables [G, B * S, 1024], e_tab (absolute), rows (the table rows that carry a camera), and the
    conditions on the inputs (gap: raw_best - the runner-up, w: the quaternion's real part, es_rel: e_s / scale)."""
    u = U_ACC
    sel = torch.tensor(idx)
    E, K = ext.double()[:, sel], intr.double()[:, sel]
    B, Sc = E.shape[:2]
    G = adapt_b.shape[0]
    R, t = E[..., :3], E[..., 3]
    R0, t0 = R[:, :1], t[:, :1]
    c = -(R0.transpose(-1, -2) @ t0.unsqueeze(-1)).squeeze(-1)                       # [B, 1, 3]
    m0 = (R0.abs().transpose(-1, -2) @ t0.abs().unsqueeze(-1)).squeeze(-1)
    tr = (R @ c.unsqueeze(-1)).squeeze(-1) + t
    e_t = MARGIN * 7 * u * ((R.abs() @ m0.unsqueeze(-1)).squeeze(-1) + t.abs())      # [B, Sc, 3]
    if Sc > 1:
        dist = (tr - tr[:, :1]).norm(dim=-1)[:, 1:]
        scale = dist.mean(1, keepdim=True).clamp_min(1e-6)                           # [B, 1]
        depth = (Sc + 255) // 256 + 8
        e_s = (e_t.sum(-1)[:, 1:] + e_t.sum(-1)[:, :1]).mean(1, keepdim=True) + MARGIN * (4 + depth + 1) * u * dist.mean(1, keepdim=True)
        tout = tr / scale.unsqueeze(-1)
        e_tout = (e_t + tout.abs() * e_s.unsqueeze(-1)) / (scale - e_s).clamp_min(1e-300).unsqueeze(-1) + MARGIN * u * tout.abs()
        es_rel = float((e_s / scale).max())
    else:
        tout, e_tout, es_rel = tr, e_t, 0.0
    Rr = R @ R0.transpose(-1, -2)
    e_R = MARGIN * 3 * u * (R.abs() @ R0.abs().transpose(-1, -2))
    d0, d1, d2 = Rr[..., 0, 0], Rr[..., 1, 1], Rr[..., 2, 2]
    raw = torch.stack([1 + d0 + d1 + d2, 1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2], -1)
    top = raw.topk(2, dim=-1).values
    e_raw = MARGIN * 3 * u * (1 + d0.abs() + d1.abs() + d2.abs()) + e_R[..., 0, 0] + e_R[..., 1, 1] + e_R[..., 2, 2]
    rho = e_raw / (2 * top[..., 0]) + MARGIN * u
    from omnivggt_official_amd import camera_math
    q = camera_math.rotation_to_quaternion(Rr)
    den = 2 * torch.sqrt(top[..., 0]).clamp_min(0.1)
    e_q = ((2 * e_R.amax((-1, -2)) + MARGIN * 2 * u * Rr.abs().amax((-1, -2))) / den).unsqueeze(-1) + q.abs() * (3 * rho + MARGIN * 2 * u).unsqueeze(-1)
    fov = torch.stack([2 * torch.atan((hw[0] / 2.0) / K[..., 1, 1]), 2 * torch.atan((hw[1] / 2.0) / K[..., 0, 0])], -1)
    enc = torch.cat([tout, q, fov], -1)
    e_enc = torch.cat([e_tout, e_q, MARGIN * 11 * u * fov.abs()], -1)
    S = ext.shape[1]
    tables = adapt_b.double().unsqueeze(1).repeat(1, B * S, 1)
    e_tab = torch.zeros_like(tables)
    rows = (torch.arange(B).unsqueeze(1) * S + sel.unsqueeze(0)).reshape(-1)
    ef, ee = enc.reshape(-1, 9), e_enc.reshape(-1, 9)
    for g_ in range(G):
        pw, pb = pose_w[g_ * 1024:(g_ + 1) * 1024].double(), pose_b[g_ * 1024:(g_ + 1) * 1024].double()
        aw, ab = adapt_w[g_].double(), adapt_b[g_].double()
        emb = ef @ pw.t() + pb
        e_emb = ee @ pw.abs().t() + MARGIN * 10 * u * (ef.abs() @ pw.abs().t() + pb.abs())
        tables[g_, rows] = emb @ aw.t() + ab
        e_tab[g_, rows] = e_emb @ aw.abs().t() + gemm_c(1024, "f32") * u * (emb.abs() @ aw.abs().t() + ab.abs())
    return {"enc": enc, "e_enc": e_enc, "tables": tables, "e_tab": e_tab, "rows": rows, "gap": float((top[..., 0] - top[..., 1]).min()),
            "w": float(q[..., 3].min()), "es_rel": es_rel}


def camera_case(B, S, seed, position=None, spread=2.0, max_angle=0.7, flips=False):
    """-> (ext [B, S, 3, 4], intr [B, S, 3, 3]) f32: cameras with rotations of at most max_angle rad about random axes (so that the rotation
    relative to any of them stays below 2 max_angle: the quaternion's real part away from zero, its branch away from a tie) at random
    positions (or all at `position`), fx != fy."""
    g = torch.Generator().manual_seed(seed)
    axis = torch.nn.functional.normalize(torch.randn(B, S, 3, generator=g, dtype=torch.float64), dim=-1)
    ang = (torch.rand(B, S, 1, generator=g, dtype=torch.float64) * 2 - 1) * max_angle
    if flips:                # views 1..3: 170 degrees about x, y, z seen from an almost unrotated view 0 -> the three other quaternion branches
        ang[:, 0] = 0.05
        ang[:, 1:4] = math.radians(170.0)
        axis[:, 1:4] = torch.eye(3, dtype=torch.float64)
    qv, qw = axis * torch.sin(ang / 2), torch.cos(ang / 2)
    x, y, z = qv.unbind(-1)
    w = qw.squeeze(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(B, S, 3, 3)
    Cw = torch.randn(B, S, 3, generator=g, dtype=torch.float64) * spread if position is None else torch.tensor(position, dtype=torch.float64).expand(B, S, 3)
    t = -(R @ Cw.unsqueeze(-1))
    intr = torch.zeros(B, S, 3, 3)
    intr[..., 0, 0] = 400 + 300 * torch.rand(B, S, generator=g)
    intr[..., 1, 1] = 250 + 100 * torch.rand(B, S, generator=g)
    intr[..., 0, 2], intr[..., 1, 2], intr[..., 2, 2] = 259.0, 196.0, 1.0
    return torch.cat([R, t], -1).float(), intr


#                          B  S    selected views                       camera_case arguments
CAMERA_CASES = {
    "branches_fx_ne_fy": (1, 5, [0, 1, 2, 3, 4], dict(flips=True)),                         # every quaternion branch; non-square frame, fx != fy (all cases)
    "subset_two_batches": (2, 5, [1, 0, 4], dict()),
    "one_camera": (1, 4, [2], dict()),                                                       # Sc = 1: no scale
    "coincident_at_origin": (1, 4, [0, 1, 2, 3], dict(position=(0.0, 0.0, 0.0))),            # every distance exactly 0: the 1e-6 clamp, t = 0 / 1e-6 = 0
    "coincident_near_origin": (2, 3, [2, 0, 1], dict(position=(0.004, -0.002, 0.003))),      # distances of rounding noise under the clamp
    "Sc300": (1, 300, [(7 * i) % 300 for i in range(300)], dict()),                          # the r += 256 loops; 5 row blocks of cam_adapt_kernel, the last partial
    "B2_Sc130": (2, 140, list(range(5, 135)), dict()),                                       # 260 camera rows: 5 row blocks, rows of batch 1 cross a block
}
CAMERA_HW = (392, 518)


def camera_inputs(case):
    B, S, idx, kw = CAMERA_CASES[case]
    ext, intr = camera_case(B, S, 2000 + sorted(CAMERA_CASES).index(case), **kw)
    return ext, intr, idx


def camera_weights(G=2):
    g = torch.Generator().manual_seed(1999)
    return (torch.randn(G * 1024, 9, generator=g) * 0.3, torch.randn(G * 1024, generator=g) * 0.1,
            torch.randn(G, 1024, 1024, generator=g) * 0.03, torch.randn(G, 1024, generator=g) * 0.1)


def check_camera_tables(name, enc, tables, Bd, quiet=False):
    """enc [B * Sc, 9] and tables [G, B * S, 1024] of a kernel against camera_tables_budget's result: the conditions on the inputs, every element
    of both within its bound, rows without a camera exactly adapt_b. -> (used fraction of enc, of tables)."""
    assert Bd["gap"] >= 0.1 and Bd["w"] >= 0.02 and Bd["es_rel"] <= 0.5, "%s: the cameras sit on a discontinuity of the encoding: %s" % (
        name, {k: Bd[k] for k in ("gap", "w", "es_rel")})
    zero = torch.zeros(())
    a = elementwise_budget(name + ".enc", enc.reshape(Bd["enc"].shape), Bd["enc"], zero, U_OUT["f32"], 0.0, extra=Bd["e_enc"], quiet=quiet)
    b = elementwise_budget(name + ".tables", tables, Bd["tables"], zero, U_OUT["f32"], 0.0, extra=Bd["e_tab"], quiet=quiet)
    free = torch.ones(Bd["tables"].shape[1], dtype=torch.bool)
    free[Bd["rows"]] = False
    assert torch.equal(tables.detach().double().cpu()[:, free], Bd["tables"][:, free]), name + ": a view without a camera must hold adapt_b exactly"
    return a, b


# ---- ovg_camera_head (csrc/ovg_camhead.hip), stage by stage -----------------------------------
# The entry leaves its intermediates in the caller's workspace, so every stage is gated against a float64 reference computed from the
# kernel's OWN stored input of that stage: tok <- tokens, e <- pose, x0 <- tok, e, qkv <- x0, attn <- qkv, x_mid <- x0, attn, hid <- x_mid,
# x <- x_mid, hid (and <- tok, e, attn, hid through all three GEMMs), xn <- x, out <- xn. With iters = 1 and one trunk block the workspace
# holds all of these but three after the call: the 16-bit xn buffer is overwritten twice (LN_n1(x0), LN_n2(x_mid), trunk_norm(x)), and x
# is updated in place. Two ways round that, both used:
#  * carried: x0 / x_mid are recomputed in float64 from tok, e, attn with their f32 error bounds (the GEMM budgets folded in), the LayerNorm
#    carries the bound, and an xn element whose float64 value lies within that bound of a rounding midpoint may be stored one ulp away:
#    rounding_window() turns that into a per-element delta which the next GEMM carries as `extra` = delta |w|^T. In the f32 mode there is no
#    rounding point and the bound itself is carried. In the 16-bit modes the worst-case bound of a K = 2048 accumulation (gemm_c, ~2.5e-4 of
#    sum |x||w|) is as large as a 16-bit ulp of xn, i.e. EVERY element would count as ambiguous and the gate would see nothing;
#  * stored: the same call with ls1 = ls2 = 0 leaves x = x0 in the workspace, with ls2 = 0 it leaves x = x_mid (x += 0 * y is exact), and its
#    qkv / attn / hid are bit-identical to the real call's (asserted by the caller). Then only the LayerNorm's own f32 budget (~70 u_acc) decides
#    which xn elements are ambiguous: about 2 % of a row in f16, 0.2 % in bf16, capped at CAMERA_AMBIGUOUS_CAP per row.
CAM_C, CAM_HEADS, CAM_HD, CAM_HID, CAM_MOD, CAM_PB, CAM_T = 2048, 16, 128, 8192, 6144, 1024, 9
CAM_PART_COLS, CAM_MAX_S = 32768, 4096
CAMERA_GEMMS = {"mod": (CAM_MOD, CAM_C), "qkv": (3 * CAM_C, CAM_C), "proj": (CAM_C, CAM_C), "fc1": (CAM_HID, CAM_C), "fc2": (CAM_C, CAM_HID),
                "pb1": (CAM_PB, CAM_C)}            # name -> (N, K)
CAMERA_AMBIGUOUS_CAP = 0.05
CAMERA_TOL_TWIN = {"bf16": 1.5e-2, "f16": 2e-3, "f32": 1e-5}       # gpu_selftest.test_camera_head's global gates against the rounding twin
CAMERA_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def camera_ws_views(ws, S, dtype):
    """ws: the uint8 workspace tensor of an ovg_camera_head call -> dict of typed views in the order of carve(): tok, x [S, 2048] f32,
    pose [S, 9] f32, part [S, 32768] f32 (the split-K partials, [ksplit][S][N] of the last GEMM), xn, e [S, 2048], qkv [S, 6144],
    attn [S, 2048], hid [S, 8192] in the compute dtype; every buffer starts on a multiple of 256 bytes."""
    from omnivggt_official_amd import ops
    f32 = torch.float32
    plan = (("tok", f32, CAM_C), ("x", f32, CAM_C), ("pose", f32, CAM_T), ("part", f32, CAM_PART_COLS), ("xn", dtype, CAM_C), ("e", dtype, CAM_C),
            ("qkv", dtype, 3 * CAM_C), ("attn", dtype, CAM_C), ("hid", dtype, CAM_HID))
    off, views = 0, {}
    for name, dt, cols in plan:
        nbytes = S * cols * torch.empty((), dtype=dt).element_size()
        views[name] = ws[off:off + nbytes].view(dt).view(S, cols)
        off += (nbytes + 255) // 256 * 256
    assert off == ops.camera_head_workspace_bytes(S, dtype), (off, ops.camera_head_workspace_bytes(S, dtype))
    return views


def camera_ksplit(S, N, K):
    """pick_ksplit, restated: doubled until the grid has 512 workgroups, never above 16, never below 256 k per slot, never more than
    32768 partial columns."""
    zs, ks = (S + 63) // 64, 1
    while (N // 64) * zs * ks < 512 and ks < 16 and K // (ks * 2) >= 256 and ks * 2 * N <= CAM_PART_COLS:
        ks *= 2
    return ks


def camera_ksplit_table(S):
    return {name: camera_ksplit(S, N, K) for name, (N, K) in CAMERA_GEMMS.items()}


def camera_gemm_c(name, mode):
    """gemm_c for the K of that GEMM + one addition per split-K slot (the consumer folds the slots one after the other onto the bias), with
    the largest ksplit the plan can pick for it (S = 1)."""
    N, K = CAMERA_GEMMS[name]
    return gemm_c(K, mode) + MARGIN * camera_ksplit(1, N, K)


def camera_w64(W, dev):
    """The packed weights (heads_hip.HipCameraHead._pack) as float64 on `dev`."""
    cv = lambda v: v.detach().to(dev, torch.float64) if torch.is_tensor(v) else v
    out = {k: cv(v) for k, v in W.items() if k != "blocks"}
    out["blocks"] = [{k: cv(v) for k, v in blk.items()} for blk in W["blocks"]]
    return out


def rounding_window(v, b, mode):
    """v float64, b >= 0 the f32 budget of the value a kernel holds before its store -> (r, delta, ambiguous): r = the reference's stored
    value, delta = how far the kernel's stored value may be from r (rounding is monotone: it lies between the roundings of v - b and
    v + b; zero wherever both equal r), ambiguous = the two ends round differently. f32: nothing is rounded below the arithmetic's own
    precision, delta = b + one f32 rounding."""
    if mode == "f32":
        return v, b + U_ACC * v.abs(), torch.zeros_like(v, dtype=torch.bool)
    r, lo, hi = round16(v, mode), round16(v - b, mode), round16(v + b, mode)
    return r, torch.maximum(hi - r, r - lo), lo != hi


def _ln_abs(x, w, b, eps):
    ref, mag, c, extra = layernorm_budget(x, w, b, eps)
    return ref, c * U_ACC * mag + extra


def ln_carry(x, ex, w, eps):
    """An absolute error ex of x through y = (x - mean) rstd w + b, first order as in qk_norm_rope_error."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    zh = (x - mean) * rstd
    return w.abs() * rstd * (ex + ex.mean(-1, keepdim=True) + zh.abs() * (zh.abs() * ex).mean(-1, keepdim=True))


# row_layernorm (2048 values on 256 threads): a thread adds its 8 values one after the other (7), a 6-level butterfly, the four wave sums
# (3): depth 16 <= the 3 + 2048 / 256 + 6 = 17 layernorm_budget charges for n = 2048. Covered; no depth of its own.
CAMERA_LN_DEPTH = 7 + 6 + 3
assert CAMERA_LN_DEPTH <= 3 + CAM_C // 256 + 6


# e = SiLU(v), v = b + sum_9 w_i p_i in f32: nine products and nine sums, a term passes through at most 10 roundings -> ev = 10 u mag_v,
# mag_v = |b| + sum |w||p|. s(v) = v / (1 + exp(-v)): |s'| <= 1.0999 carries ev; expf within 3 ulp (6 u, C_EXP's bound) moves the denominator
# by at most 6 u of itself, the sum 1, the division 1 -> 8 u |s|, and |s(v)| <= |v| <= mag_v: c = 1.1 x 10 + 8 on mag_v (x margin).
def camera_embed_budget(pose, W, mode):
    """pose [S, 9] (or [9]: the empty pose, one row for all) float64 -> (ref [S, 2048], mag, c, extra)."""
    pose = pose.double()
    w, b = W["embed_w"], W["embed_b"]
    v = pose @ w.t() + b
    mag = pose.abs() @ w.abs().t() + b.abs()
    ref = v * torch.sigmoid(v)
    return ref, mag, MARGIN * (1.1 * 10 + 8), f16_subnormal_floor(mode)


# x0 = gate (ln (1 + scale) + shift) + tok, (shift, scale, gate) = e mod_w^T + mod_b folded from the split-K slots, ln = LayerNorm(tok) without
# affine parameters, eps 1e-6. Each of the three GEMM values within em = c_gemm u mag_mod, ln within layernorm_budget's bound; 1 + scale, the
# two products and the two sums: 5 roundings on |gate| (|ln||1 + scale| + |shift|) + |tok|.
def camera_x0(tok, e, W, mode):
    """tok [S, 2048], e [S, 2048] float64 (the stored buffers) -> (x0, e_x0) float64."""
    tok, e = tok.double(), e.double()
    mod = e @ W["mod_w"].t() + W["mod_b"]
    em = camera_gemm_c("mod", mode) * U_ACC * (e.abs() @ W["mod_w"].abs().t() + W["mod_b"].abs())
    (h, s, g), (eh, es, eg) = mod.chunk(3, -1), em.chunk(3, -1)
    one, zero = torch.ones(CAM_C, dtype=torch.float64, device=tok.device), torch.zeros(CAM_C, dtype=torch.float64, device=tok.device)
    l, el = _ln_abs(tok, one, zero, 1e-6)
    inner = l * (1 + s) + h
    e_inner = (1 + s).abs() * el + l.abs() * es + eh
    x0 = g * inner + tok
    e_x0 = g.abs() * e_inner + inner.abs() * eg + eg * e_inner + MARGIN * 5 * U_ACC * (g.abs() * (l.abs() * (1 + s).abs() + h.abs()) + tok.abs())
    return x0, e_x0


def camera_residual(x, ex, a, w, bias, ls, name, mode):
    """x' = x + ls (a w^T + bias), the partials folded onto the bias by the consumer: the GEMM's budget through |ls| + three roundings (res_c).
    -> (x', e_x')."""
    a = a.double()
    y, mg = a @ w.t() + bias, a.abs() @ w.abs().t() + bias.abs()
    return x + ls * y, ex + ls.abs() * camera_gemm_c(name, mode) * U_ACC * mg + MARGIN * 3 * U_ACC * (x.abs() + ls.abs() * mg)


# gelu_c carries z's error through the global bound |gelu'| <= 1.13. At K = 2048 that error (c_gemm u mag, mag ~ 30 |z|) is ~5e-3, more than
# the whole difference between the erf form and its tanh approximation (4.7e-4). The mean value theorem gives the same bound with the
# LOCAL supremum of |gelu'| over [z - ez, z + ez]: gelu'(t) = Phi(t) + t phi(t), its derivative phi(t) (2 - t^2) vanishes at +-sqrt 2 only, so
# the supremum is attained at an end of the interval or at +-sqrt 2 (|gelu'| = 1.129 / 0.129) where the interval holds it. Never above 1.13 ez;
# in the negative tail, where gelu' ~ 1e-2, two orders tighter. The evaluation's own 8 roundings stay on mag as in gelu_c.
def gelu_carry(z, ez):
    d = lambda t: 0.5 * (1 + torch.erf(t / math.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    lo, hi = z - ez, z + ez
    sup = torch.maximum(d(lo).abs(), d(hi).abs())
    for t0, v in ((math.sqrt(2.0), 1.13), (-math.sqrt(2.0), 0.13)):
        sup = torch.where((lo <= t0) & (hi >= t0), sup.clamp_min(v), sup)
    return sup * ez


def camera_ln_gemm(x, ex, nw, nb, w, bias, name, mode, gelu=False):
    """LayerNorm (eps 1e-5) of x (known within ex), stored in the mode's dtype, then the GEMM `name` (+ exact-erf GELU) and the store.
    -> dict(ref, mag, c, extra, share): extra = the stored xn's rounding window carried through |w| (and, with the GEMM's own budget, through
    gelu_carry, which never exceeds |gelu'| <= 1.13), share = the fraction of ambiguous xn elements per row."""
    v, b = _ln_abs(x, nw, nb, 1e-5)
    b = b + ln_carry(x, ex, nw, 1e-5)
    r, delta, amb = rounding_window(v, b, mode)
    z, mg = r @ w.t() + bias, r.abs() @ w.abs().t() + bias.abs()
    extra = delta @ w.abs().t()
    cg = camera_gemm_c(name, mode)
    if gelu:
        return {"ref": torch.nn.functional.gelu(z), "mag": mg, "c": MARGIN * 8, "extra": gelu_carry(z, cg * U_ACC * mg + extra) + f16_subnormal_floor(mode),
                "share": amb.double().mean(-1)}
    return {"ref": z, "mag": mg, "c": cg, "extra": extra + f16_subnormal_floor(mode), "share": amb.double().mean(-1)}


# attention of the trunk (ch_attn_kernel): head dim 128, everything f32, P never rounded. qs = q / sqrt(128) (1 rounding), s = sum_128 qs k
# one after the other (a product and a sum per term: a term passes through at most 128 + 1 roundings) -> e_s = 130 u A, A = max_k sum_d |qs||k|;
# s - max: one rounding on |s - max| <= 2 Smax; expf 3 ulp -> p relative (130 A + 2 Smax + 6) u, numerator and denominator both (x 2).
# The row sum: a thread adds ceil(S / 128) values, a 6-level butterfly, the two wave sums, then the reciprocal -> ceil(S / 128) + 8;
# PV: S products and S sums one key after the other -> S + 1; the product with the reciprocal 1. mag = sum p |v| / sum p.
def camera_attn_budget(qkv, mode):
    """qkv [S, 6144] float64 (the stored buffer) -> (ref [S, 2048], mag, c [S, 2048])."""
    S = qkv.shape[0]
    q, k, v = qkv.double().view(S, 3, CAM_HEADS, CAM_HD).permute(1, 2, 0, 3)
    scale = CAM_HD ** -0.5
    ref, mag, c = (torch.empty(S, CAM_HEADS, CAM_HD, dtype=torch.float64, device=qkv.device) for _ in range(3))
    for h in range(0, CAM_HEADS, 4):
        qq, kk, vv = q[h:h + 4] * scale, k[h:h + 4], v[h:h + 4]
        s = qq @ kk.transpose(-1, -2)
        A = (qq.abs() @ kk.abs().transpose(-1, -2)).amax(-1)
        p = torch.softmax(s, -1)
        ch = MARGIN * (2 * (130 * A + 2 * s.abs().amax(-1) + 6) + (S + 127) // 128 + 8 + S + 1 + 1)
        ref[:, h:h + 4], mag[:, h:h + 4] = (p @ vv).permute(1, 0, 2), (p @ vv.abs()).permute(1, 0, 2)
        c[:, h:h + 4] = ch.t().unsqueeze(-1)
    return ref.reshape(S, CAM_C), mag.reshape(S, CAM_C), c.reshape(S, CAM_C)


# pose branch. pb1 is the LAST GEMM of a call, so its split-K partials part[ks][S][1024] are still in the workspace afterwards: the GEMM
# and its consumer are gated apart.
#  * every slot against xn[:, slot] pb1_w[:, slot]^T: gemm_c for the slot's K / ksplit products, on sum |xn||w| over the slot;
#  * ch_pose_kernel against the STORED partials: z = b1 + the slots one after the other (ksplit roundings on |b1| + sum |part|),
#    g = GELU(z) in f32 (gelu_carry of that + the evaluation's 8 roundings on |z|; never stored), delta = g pb2^T + b2 with f32 operands:
#    a product (1), a thread adds 4 terms (3), a 6-level butterfly, the four wave sums (3), the bias (1) -> 14 + 1 = 15 on |g||pb2|^T + |b2|;
#    pose = previous + delta (one more rounding from the second round on), out = pose with ReLU on the two FoV components (1-Lipschitz).
#    Nothing of the K = 2048 accumulation's worst case enters: the budget is of order 1e-6 of a component.
def camera_part_view(part, S, ks, N=CAM_PB):
    """The [S, 32768] partial buffer of camera_ws_views -> the [ks, S, N] partials the last GEMM left at its start."""
    return part.reshape(-1)[:ks * S * N].view(ks, S, N)


def check_camera_pb1(name, part, xn, W, mode, quiet=False):
    """part [ks, S, 1024] (stored) against the stored xn, slot by slot. -> the worst used fraction."""
    xn, w = xn.double(), W["pb1_w"]
    ks = part.shape[0]
    kc = CAM_C // ks
    used = 0.0
    for k in range(ks):
        xs, ws = xn[:, k * kc:(k + 1) * kc], w[:, k * kc:(k + 1) * kc]
        used = max(used, elementwise_budget("%s.pb1_slot%d" % (name, k), part[k], xs @ ws.t(), xs.abs() @ ws.abs().t(), U_OUT["f32"], gemm_c(kc, mode), quiet=True))
    if not quiet:
        print("[PASS] %-52s budget used %.3f" % (name + ".pb1_slots(%d).elementwise" % ks, used), flush=True)
    return used


def camera_pose_budget(part, W, mode, prev=None):
    """part [ks, S, 1024] float64 (the stored partials), prev [S, 9] the carried pose or None -> (pose [S, 9] un-activated, out [S, 9],
    e [S, 9] absolute)."""
    part = part.double()
    z, mz = W["pb1_b"] + part.sum(0), W["pb1_b"].abs() + part.abs().sum(0)
    eg = gelu_carry(z, MARGIN * part.shape[0] * U_ACC * mz) + MARGIN * 8 * U_ACC * z.abs()
    g = torch.nn.functional.gelu(z)
    delta = g @ W["pb2_w"].t() + W["pb2_b"]
    e = eg @ W["pb2_w"].abs().t() + MARGIN * 15 * U_ACC * (g.abs() @ W["pb2_w"].abs().t() + W["pb2_b"].abs())
    pose = delta
    if prev is not None:
        pose = prev.double() + delta
        e = e + MARGIN * U_ACC * (prev.double().abs() + delta.abs())
    out = torch.cat([pose[:, :7], torch.relu(pose[:, 7:])], -1)
    return pose, out, e


CAMERA_COMPONENTS = ("tx", "ty", "tz", "qx", "qy", "qz", "qw", "fov_h", "fov_w")


def _abs_gate(name, got, ref, err, quiet=False):
    return elementwise_budget(name, got, ref, torch.zeros_like(ref), U_OUT["f32"], 0.0, extra=err, quiet=quiet)


def check_camera_pose(name, out, pose, part, W, mode, prev=None, quiet=False):
    """out [S, 9] (the activated encodings of the round) and pose [S, 9] or None (the carried, un-activated pose in the workspace) against
    the stored pb1 partials, each of the nine components gated on its own. -> the worst used fraction."""
    rp, ro, e = camera_pose_budget(part, W, mode, prev)
    used = 0.0
    for i, comp in enumerate(CAMERA_COMPONENTS):
        used = max(used, _abs_gate("%s.out.%s" % (name, comp), out[:, i:i + 1], ro[:, i:i + 1], e[:, i:i + 1], quiet=quiet))
        if pose is not None:
            used = max(used, _abs_gate("%s.pose.%s" % (name, comp), pose[:, i:i + 1], rp[:, i:i + 1], e[:, i:i + 1], quiet=True))
    return used


def check_camera_embed(name, e, pose, W, mode, quiet=False):
    ref, mag, c, extra = camera_embed_budget(pose, W, mode)
    return elementwise_budget(name, e, ref.expand(e.shape), mag.expand(e.shape), U_OUT[mode], c, extra=extra, quiet=quiet)


def check_camera_stages(tag, B, tokens, W, mode, quiet=False):
    """Every stage gate of an iters = 1, one-block call. B: the buffers after the call (camera_ws_views' keys tok, x, pose, xn, e, qkv, attn,
    hid, part as camera_part_view gives it + out: [S, 9]) and, where the caller has them, x0 and xmid (the stored residual stream after the modulation / after the attention
    update, see above); without them, or in the f32 mode, qkv and hid are gated with the carried bounds. tokens [S, 2048] f32; W: camera_w64
    on the device of the buffers. Asserts every budget and the cap on the ambiguous xn elements; -> ({stage: used fraction}, the largest ambiguous share of a row)."""
    dev = B["tok"].device
    d = lambda t: t.detach().to(dev, torch.float64)
    blk = W["blocks"][0]
    u, uT = U_OUT["f32"], U_OUT[mode]
    floor = f16_subnormal_floor(mode)
    used, shares = {}, {}

    def gate(stage, got, ref, mag, u_out, c, extra=None):
        used[stage] = max(used.get(stage, 0.0), elementwise_budget("%s.%s" % (tag, stage), got, ref, mag, u_out, c, extra=extra, quiet=quiet))

    def abs_gate(stage, got, ref, err):
        used[stage] = max(used.get(stage, 0.0), _abs_gate("%s.%s" % (tag, stage), got, ref, err, quiet=quiet))

    # (c) tok <- tokens
    ref, mag, c, extra = layernorm_budget(d(tokens), W["token_norm_w"], W["token_norm_b"], 1e-5)
    gate("tok", B["tok"], ref, mag, u, c, extra)
    # (d) e <- empty_pose
    used["e"] = check_camera_embed(tag + ".e", B["e"], W["empty_pose"].view(1, CAM_T), W, mode, quiet=quiet)
    # x0 <- stored tok, e
    tok, e, attn, hid = d(B["tok"]), d(B["e"]), d(B["attn"]), d(B["hid"])
    x0, e_x0 = camera_x0(tok, e, W, mode)
    zero = torch.zeros_like(x0)
    if "x0" in B:
        abs_gate("x0", B["x0"], x0, e_x0)
    # (e) qkv: carried in the f32 mode (and where no stored x0 exists), from the stored x0 otherwise
    carried = mode == "f32" or "x0" not in B
    G = camera_ln_gemm(x0, e_x0, blk["n1_w"], blk["n1_b"], blk["qkv_w"], blk["qkv_b"], "qkv", mode) if carried else \
        camera_ln_gemm(d(B["x0"]), zero, blk["n1_w"], blk["n1_b"], blk["qkv_w"], blk["qkv_b"], "qkv", mode)
    gate("qkv", B["qkv"], G["ref"], G["mag"], uT, G["c"], G["extra"])
    shares["xn_n1"] = float(G["share"].max())
    if mode == "f32" and "x0" in B:
        G = camera_ln_gemm(d(B["x0"]), zero, blk["n1_w"], blk["n1_b"], blk["qkv_w"], blk["qkv_b"], "qkv", mode)
        gate("qkv", B["qkv"], G["ref"], G["mag"], uT, G["c"], G["extra"])
    del G
    # (f) attn <- stored qkv
    ref, mag, c = camera_attn_budget(d(B["qkv"]), mode)
    gate("attn", B["attn"], ref, mag, uT, c, floor)
    # x_mid <- x0, stored attn
    xm, e_xm = camera_residual(x0, e_x0, attn, blk["proj_w"], blk["proj_b"], blk["ls1"], "proj", mode)
    if "xmid" in B:
        if "x0" in B:
            r2, e2 = camera_residual(d(B["x0"]), zero, attn, blk["proj_w"], blk["proj_b"], blk["ls1"], "proj", mode)
            abs_gate("xmid", B["xmid"], r2, e2)
        else:
            abs_gate("xmid", B["xmid"], xm, e_xm)
    # (g) hid
    carried = mode == "f32" or "xmid" not in B
    G = camera_ln_gemm(xm, e_xm, blk["n2_w"], blk["n2_b"], blk["fc1_w"], blk["fc1_b"], "fc1", mode, gelu=True) if carried else \
        camera_ln_gemm(d(B["xmid"]), zero, blk["n2_w"], blk["n2_b"], blk["fc1_w"], blk["fc1_b"], "fc1", mode, gelu=True)
    gate("hid", B["hid"], G["ref"], G["mag"], uT, G["c"], G["extra"])
    shares["xn_n2"] = float(G["share"].max())
    if mode == "f32" and "xmid" in B:
        G = camera_ln_gemm(d(B["xmid"]), zero, blk["n2_w"], blk["n2_b"], blk["fc1_w"], blk["fc1_b"], "fc1", mode, gelu=True)
        gate("hid", B["hid"], G["ref"], G["mag"], uT, G["c"], G["extra"])
    del G
    # (h) x <- stored tok, e, attn, hid: three GEMM budgets and the residual roundings (and <- the stored x_mid, hid where there is one)
    xf, e_xf = camera_residual(xm, e_xm, hid, blk["fc2_w"], blk["fc2_b"], blk["ls2"], "fc2", mode)
    abs_gate("x", B["x"], xf, e_xf)
    if "xmid" in B:
        r2, e2 = camera_residual(d(B["xmid"]), zero, hid, blk["fc2_w"], blk["fc2_b"], blk["ls2"], "fc2", mode)
        abs_gate("x", B["x"], r2, e2)
        if not quiet:       # how wide this gate is: the fc2 accumulation's worst case (K = 8192) against the size of the stream it is added to
            print("%s: the budget of x from the stored x_mid is at most %.2f%% of the row's rms" % (tag, 100 * float((e2 / r2.pow(2).mean(-1, keepdim=True).sqrt()).max())), flush=True)
    # (i) xn <- stored x
    ref, mag, c, extra = layernorm_budget(d(B["x"]), W["trunk_norm_w"], W["trunk_norm_b"], 1e-5)
    gate("xn", B["xn"], ref, mag, uT, c, extra + floor)
    # (j) the pb1 partials <- stored xn, slot by slot; out, pose <- the stored partials
    used["pb1"] = check_camera_pb1(tag, d(B["part"]), d(B["xn"]), W, mode, quiet=quiet)
    used["out"] = check_camera_pose(tag, B["out"], B["pose"], d(B["part"]), W, mode, quiet=quiet)
    # (l) the ambiguous share of the two overwritten xn buffers
    if not quiet:
        print("%s: ambiguous xn elements per row at most %.2f%% (n1), %.2f%% (n2)" % (tag, 100 * shares["xn_n1"], 100 * shares["xn_n2"]), flush=True)
    if mode != "f32":
        assert max(shares.values()) < CAMERA_AMBIGUOUS_CAP, "%s: %s of a row's xn elements count as ambiguous: the gate would hide failures" % (tag, shares)
    return used, max(shares.values())


def camera_group_gate(name, got, ref, tol):
    """The global gate per component group: translation, quaternion and field of view each normalised by their own maximum.
    got / ref [..., 9] -> True when all three hold (printed through gpu_selftest.report)."""
    import gpu_selftest as st
    ok = True
    for grp, sl in (("T", slice(0, 3)), ("quat", slice(3, 7)), ("fov", slice(7, 9))):
        ok = st.report("%s.%s" % (name, grp), got[..., sl].detach().double().cpu(), ref[..., sl].detach().double().cpu(), tol) and ok
    return ok


def check_camera_round2(tag, B1, B2, W, mode, positive, quiet=False):
    """The round transition. B1 / B2: the buffers after an iters = 1 / iters = 2 call on the same input (pose, e, xn, part [ks, S, 1024], out [iters, S, 9]).
    The pose after round 1 is read from out[0] where both FoV components are positive (ReLU the identity); where they are negative out[0]
    holds zeros there and the un-activated pose is the one the iters = 1 call left in its workspace. Gates round 2's e against
    SiLU(embed(pose)), the pb1 partials against the stored xn, out[1] and the carried pose against pose + the delta from the stored partials. -> the worst used fraction."""
    dev = B2["xn"].device
    o1, o2 = B1["out"].detach().to(dev), B2["out"].detach().to(dev)
    p1 = B1["pose"].detach().to(dev)
    assert torch.equal(o1[0], o2[0]), tag + ": round 1 of the two-round call differs from the one-round call"
    assert torch.equal(o2[0][:, :7], p1[:, :7]), tag + ": translation and quaternion are stored un-activated"
    if positive:
        assert float(o2[0][:, 7:].min()) > 0 and torch.equal(o2[0], p1), tag + ": the FoV components were to be positive after round 1"
        pose1 = o2[0].double()
    else:
        assert float(p1[:, 7:].max()) < 0 and float(o2[0][:, 7:].abs().max()) == 0, tag + ": the FoV components were to be negative after round 1, and clamped in out[0]"
        pose1 = p1.double()
    a = check_camera_embed(tag + ".e_round2", B2["e"], pose1, W, mode, quiet=quiet)
    b = max(check_camera_pb1(tag + ".round2", B2["part"].to(dev), B2["xn"].to(dev), W, mode, quiet=quiet),
            check_camera_pose(tag + ".round2", o2[1], B2["pose"], B2["part"].to(dev), W, mode, prev=pose1, quiet=quiet))
    if not positive:
        rp, _, e = camera_pose_budget(B2["part"].to(dev), W, mode, pose1)
        assert float((rp[:, 7:] + e[:, 7:]).max()) < 0, tag + ": the FoV components were to stay negative after round 2"
        assert float(B2["pose"][:, 7:].max()) < 0 and float(o2[1][:, 7:].abs().max()) == 0, tag + ": out[1] clamped, the carried pose not"
    return max(a, b)


# Token counts at which every GEMM takes every ksplit value the rule can give it (test_camera_head_budget_host.py asserts that), the last
# z slice holds 1, 2, 3 or 4 16-row blocks, z slices are ragged and the attention's 128-key loops make 2 .. 32 trips.
CAMERA_S_SET = (1, 17, 40, 65, 129, 193, 321, 513, 961, 1985, 4096)


def camera_tokens(S, seed):
    """[S, 2048] f32 camera tokens for the stage gates: 1.3 (1 + 0.3 n) with a random sign, n normal. Values away from zero keep the
    share of tiny LayerNorm outputs low: an xn element counts as ambiguous when the LayerNorm's budget -- dominated, for small elements,
    by the error of the row mean, an absolute term -- reaches a rounding midpoint, which in f16 is 3.3 % of a normal row on average and up
    to 4.6 % in a few hundred rows, too close to the cap of 5 % for 4096 rows; with these tokens 1.4 % and 2.4 %."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.sign(torch.randn(S, CAM_C, generator=g))
    return sign * (1.0 + 0.3 * torch.randn(S, CAM_C, generator=g)) * 1.3
