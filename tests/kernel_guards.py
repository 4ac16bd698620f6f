"""Guard bands, poisoned padding and a per-element error budget for the kernel tests (a plain helper module like gpu_selftest;
the host test test_kernel_guards_host.py proves on the CPU that each helper catches what it is for).

guarded()            an output view inside a larger byte buffer pre-filled with a finite non-zero pattern + a checker that every byte
                     outside the view is bit-unchanged afterwards (front / back guard, row gaps, spare rows)
poison_*()           large finite values of alternating sign in the padding a kernel must not depend on
elementwise_budget() |got - ref| <= u_out |ref| + c u_acc mag for EVERY element (gpu_selftest.report gates the tensor-global maximum only)
*_budget()           the constants c, each derived from the rounding points of its kernel (never fitted to a kernel's output)
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
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
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
