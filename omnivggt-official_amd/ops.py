"""Torch-tensor front ends of the C ABI entries (one function per `ovg_*` kernel entry).

They only marshal device pointers, shapes and the current HIP stream into the parameter
structs of include/omnivggt_hip.h; every byte of compute happens in libomnivggt_hip.so.
"""
import collections
import math

import torch

from . import lib as L

C, H, D, HID = 1024, 16, 64, 4096
KV_TILE = L.KV_TILE


def _stream():
    return torch.cuda.current_stream().cuda_stream


def pad_to(n, m):
    return (n + m - 1) // m * m


def nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.OvgError("expected a HIP device tensor (the hot path has no CPU fallback)")


class HiLo:
    """A split-f16 tensor (L.F32X mode): two f16 planes of one allocation, value ~ hi + lo (include/omnivggt_hip.h, OVG_F16X2)."""
    def __init__(self, planes):
        self.planes, self.hi, self.lo = planes, planes[0], planes[1]      # planes: f16 [2, ...] contiguous

    @property
    def shape(self):
        return self.hi.shape

    @property
    def device(self):
        return self.hi.device

    def stride(self, i):
        return self.hi.stride(i)

    def float(self):
        """f32 value of the pair (tests)."""
        return self.hi.float() + self.lo.float()


def empty_like_dtype(shape, dtype, device, zero=False):
    """Activation / weight storage for `dtype`: a plain tensor, or a HiLo pair of f16 planes in the split-f16 mode."""
    mk = torch.zeros if zero else torch.empty
    if L.is_split(dtype):
        return HiLo(mk((2,) + tuple(shape), device=device, dtype=torch.float16))
    return mk(tuple(shape), device=device, dtype=dtype)


def hi_lo(t):
    """(tensor whose pointer goes into the ordinary field, tensor for the *_lo field or None)."""
    return (t.hi, t.lo) if isinstance(t, HiLo) else (t, None)


def to_hilo(x32):
    """f32 tensor -> HiLo on the same device with the library's rounding (hi = f16(sat(x)), lo = f16(x - hi)); tests / tools."""
    hi = x32.clamp(-65504.0, 65504.0).to(torch.float16)
    lo = (x32 - hi.float()).clamp(-65504.0, 65504.0).to(torch.float16)
    return HiLo(torch.stack([hi, lo]).contiguous())


def layernorm(x, weight, bias, eps, dtype, out=None, out_f32=False):
    """x: f32 [rows, 1024] (row-strided view allowed) -> [rows,1024] in dtype (or f32)."""
    _chk_dev(x, weight, bias)
    rows = x.shape[0]
    if out is None:
        out = torch.empty(rows, C, device=x.device, dtype=torch.float32) if out_f32 else empty_like_dtype((rows, C), dtype, x.device)
    o_hi, o_lo = hi_lo(out)
    p = L.LayerNormParams(L.ptr(x), x.stride(0), L.ptr(o_hi), o_hi.stride(0), L.ptr(weight), L.ptr(bias), rows, eps,
                          L.dtype_code(dtype), 1 if out_f32 else 0, L.ptr(o_lo))
    L.call("ovg_layernorm", p, _stream())
    return out


def linear(x, w, bias, dtype, epilogue=L.EPI_STORE, out=None, out_f32=False, res=None, gamma=None, inject=None,
           inj_period=0, table=None, p0=0, p1=0, row_off=0, out_rows=None, tile=L.TILE_AUTO):
    """y = epilogue(x @ w.T + bias); x [M,K], w [N,K] in dtype."""
    (x, x_lo), (w, w_lo) = hi_lo(x), hi_lo(w)
    _chk_dev(x, w, bias, res, gamma, inject, table)
    M, K = x.shape
    N = w.shape[0]
    f32_out = out_f32 or epilogue in (L.EPI_RES, L.EPI_PATCH)
    if out is None:
        rows = out_rows if out_rows is not None else M
        out = torch.empty(rows, N, device=x.device, dtype=torch.float32) if f32_out else empty_like_dtype((rows, N), dtype, x.device)
    o_hi, o_lo = hi_lo(out)
    _chk_dev(o_hi)
    p = L.LinearParams()
    p.x, p.ldx, p.w, p.ldw, p.bias = L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(bias)
    p.y, p.ldy, p.M, p.N, p.K = L.ptr(o_hi), o_hi.stride(0), M, N, K
    p.x_lo, p.w_lo, p.y_lo = L.ptr(x_lo), L.ptr(w_lo), L.ptr(o_lo)
    p.dtype, p.epilogue, p.out_f32 = L.dtype_code(dtype), epilogue, 1 if f32_out else 0
    if res is not None:
        p.res, p.ldres = L.ptr(res), res.stride(0)
    p.gamma, p.inject, p.inj_period = L.ptr(gamma), L.ptr(inject), inj_period
    p.table, p.p0, p.p1, p.row_off, p.tile = L.ptr(table), p0, p1, row_off, tile
    L.call("ovg_linear", p, _stream())
    return out


def vt_index(n_pad, dtype, device="cpu"):
    """Column permutation of a V^T row: idx[pos] = key stored at column pos. 16-bit dtypes: inside every block of 32 keys
    pos = 8 g + 4 h + i holds key 16 h + 4 g + i (the PV fragment order, csrc/ovg_common.h vt_pos16); f32: identity."""
    pos = torch.arange(n_pad, device=device)
    if dtype is torch.float32:
        return pos
    k = pos & 31
    return (pos & ~31) | (((k >> 2) & 1) << 4) | (((k >> 3) & 3) << 2) | (k & 3)


def set_vt(vt, v_nat):
    """Fill a V^T buffer [BH,64,nk_pad] from natural-order values v_nat [BH,64,n] (n <= nk_pad; the rest is zeroed)."""
    BH, d, n_pad = vt.shape
    full = torch.zeros(BH, d, n_pad, device=vt.device, dtype=vt.dtype)
    full[:, :, : v_nat.shape[2]] = v_nat.to(device=vt.device, dtype=vt.dtype)
    vt.copy_(full[:, :, vt_index(n_pad, vt.dtype, vt.device)])
    return vt


def get_vt(vt):
    """Natural-order view (a copy) of a V^T buffer [BH,64,nk_pad] written by ovg_qkv."""
    idx = vt_index(vt.shape[2], vt.dtype, vt.device)
    out = torch.empty_like(vt)
    out[:, :, idx] = vt
    return out


def alloc_qkv(BH, nq, nk, dtype, device):
    """Zero-filled head-major buffers q [BH,nq_pad,64], k [BH,nk_pad,64], vt [BH,64,nk_pad] (16-bit vt rows hold their keys in
    the vt_index order: fill / read them with set_vt / get_vt when they do not come from ovg_qkv)."""
    nq_pad, nk_pad = pad_to(nq, KV_TILE), pad_to(nk, KV_TILE)
    q = empty_like_dtype((BH, nq_pad, D), dtype, device, zero=True)      # split-f16 mode: HiLo pairs
    k = empty_like_dtype((BH, nk_pad, D), dtype, device, zero=True)
    vt = empty_like_dtype((BH, D, nk_pad), dtype, device, zero=True)
    return q, k, vt


def qkv(x, w, bias, seq, dtype, q, k, vt, qk_norm=None, rope=None, tokens_per_view=1374, grid_w=37, n_special=5,
        q_scale=0.125 * 1.4426950408889634, qk_eps=1e-5, part=0, tile=L.TILE_AUTO):
    """Fused QKV projection.  qk_norm = (qn_w, qn_b, kn_w, kn_b) or None; rope = (cos, sin) or None."""
    (x, x_lo), (w, w_lo), (q, q_lo), (k, k_lo), (vt, vt_lo) = hi_lo(x), hi_lo(w), hi_lo(q), hi_lo(k), hi_lo(vt)
    _chk_dev(x, w, bias, q, k, vt)
    p = L.QkvParams()
    p.x, p.ldx, p.w, p.bias = L.ptr(x), x.stride(0), L.ptr(w), L.ptr(bias)
    p.q, p.k, p.vt = L.ptr(q), L.ptr(k), L.ptr(vt)
    p.x_lo, p.w_lo, p.q_lo, p.k_lo, p.vt_lo = L.ptr(x_lo), L.ptr(w_lo), L.ptr(q_lo), L.ptr(k_lo), L.ptr(vt_lo)
    p.M, p.seq, p.nq_pad, p.nk_pad, p.dtype = x.shape[0], seq, q.shape[1], k.shape[1], L.dtype_code(dtype)
    if qk_norm is not None:
        p.qk_norm = 1
        p.qn_w, p.qn_b, p.kn_w, p.kn_b = (L.ptr(t) for t in qk_norm)
    p.qk_eps = qk_eps
    if rope is not None:
        p.rope = 1
        p.rope_cos, p.rope_sin, p.max_pos = L.ptr(rope[0]), L.ptr(rope[1]), rope[0].shape[0]
    p.tokens_per_view, p.grid_w, p.n_special, p.q_scale = tokens_per_view, grid_w, n_special, q_scale
    p.part, p.tile = part, tile
    L.call("ovg_qkv", p, _stream())


def attn_plan(BH, nq, nks, dtype, variant=0, kv_splits=0, nq_pad=None, cus=0):
    """How ovg_flash_attn would run this shape (host-only query): dict(splits, q_tile, part_bytes, lse_bytes, main_rows, tail_q_tile).
    nq_pad: row count of the q buffer the call will use (default: nq padded to 64); the partial buffers are sized with it."""
    p = L.AttnParams()
    p.nq, p.nq_pad, p.BH, p.nseg = nq, (pad_to(nq, KV_TILE) if nq_pad is None else nq_pad), BH, len(nks)
    for i, nk in enumerate(nks):
        p.seg[i].nk = nk
    p.dtype, p.variant, p.kv_splits, p.cus = L.dtype_code(dtype), variant, kv_splits, cus
    out = L.AttnPlanOut()
    L.check(L.load().ovg_attn_plan(L.C.byref(p), L.C.byref(out)), "ovg_attn_plan")
    return {"splits": out.splits, "q_tile": out.q_tile, "part_bytes": out.part_bytes, "lse_bytes": out.lse_bytes,
            "main_rows": out.main_rows, "tail_q_tile": out.tail_q_tile}


def alloc_split_ws(plan, device):
    """(ws_part, ws_lse) byte/f32 buffers for a plan with splits > 1, else (None, None)."""
    if plan["splits"] <= 1:
        return None, None
    return (torch.empty(plan["part_bytes"], device=device, dtype=torch.uint8),
            torch.empty(plan["lse_bytes"] // 4, device=device, dtype=torch.float32))


AttnKnobs = collections.namedtuple("AttnKnobs", "variant kv_splits cus fallback_counter")


def attn_knobs(owner, dtype, cus=None):
    """The attention knobs of `owner` (the aggregator, or any object with some of .attn_variant / .f32x_fast_pv / .attn_kv_splits / .attn_cus /
    .fallback_counter; None = library defaults), read at call time, as the launch will carry them. cus: the caller's own CU budget instead of
    owner.attn_cus (the sharded run plans against what RCCL leaves)."""
    variant = int(getattr(owner, "attn_variant", 0))
    if L.is_split(dtype) and variant == L.ATTN_AUTO and getattr(owner, "f32x_fast_pv", False):
        variant = L.ATTN_F32X_FAST_PV                 # split-f16 mode without the P_lo x V_hi product of the PV contraction (opt-in)
    return AttnKnobs(variant, int(getattr(owner, "attn_kv_splits", 0)), int(getattr(owner, "attn_cus", 0) if cus is None else cus),
                     getattr(owner, "fallback_counter", None))


def attn_split_ws(BH, nq, nks, dtype, knobs, nq_pad, device, alloc=alloc_split_ws):
    """(ws_part, ws_lse) for the attention launch of this shape under `knobs` (attn_knobs) if ovg_attn_plan -- asked with the SAME variant,
    split factor and CU budget the launch will carry -- cuts it along the keys, else (None, None): only the 16-bit kernels split, and
    kv_splits == 1 forbids it. The buffers' sizes travel with the pointers (ovg_attn_params.ws_part_bytes / ws_lse_bytes), so a plan / launch
    mismatch is an error code, not an overrun. alloc(plan, device): where the buffers come from (tests: guarded ones). Callers cache."""
    if dtype not in (torch.bfloat16, torch.float16) or knobs.kv_splits == 1:
        return None, None
    return alloc(attn_plan(BH, nq, nks, dtype, knobs.variant, knobs.kv_splits, nq_pad=nq_pad, cus=knobs.cus), device)


def flash_attn(q, segments, nq, dtype, out=None, variant=0, kv_heads=0, head_major=False, lse=None, kv_splits=0, split_ws=None, fallback_count=None, cus=0):
    """q [BH,nq_pad,64]; segments: list of (k [BHkv,nk_pad,64], vt [BHkv,64,nk_pad], nk).
    Returns out [B*nq, 1024] token-major, or with head_major=True out [BH, nq_pad, 64].
    kv_heads > 0: the segments hold kv_heads heads and batch entry bh attends to head bh % kv_heads
    (head-parallel sharding: the BH entries are (source rank, head) pairs).
    lse: optional f32 [BH, nq_pad] receiving log2(sum_k exp2(logit)) over the keys of this call (see attn_merge).
    kv_splits / split_ws = (ws_part, ws_lse) from alloc_split_ws(attn_plan(...)): split-KV for launches that do not fill the
    chip evenly (kv_splits 0 = library decides, and only splits when split_ws is given; 1 = never; 2..8 = force).
    fallback_count: optional int32 device tensor [1]: workgroups of the speculative bf16 kernels that re-ran (telemetry).
    Split-f16 mode (dtype = L.F32X): q / k / vt / out are HiLo pairs."""
    q, q_lo = hi_lo(q)
    _chk_dev(q)
    BH = q.shape[0]
    if out is None:
        out = empty_like_dtype((BH, q.shape[1], D) if head_major else ((BH // H) * nq, C), dtype, q.device)
    ret = out
    out, out_lo = hi_lo(out)
    p = L.AttnParams()
    p.q, p.nq, p.nq_pad, p.nseg = L.ptr(q), nq, q.shape[1], len(segments)
    p.q_lo, p.out_lo = L.ptr(q_lo), L.ptr(out_lo)
    for i, (k, vt, nk) in enumerate(segments):
        (k, k_lo), (vt, vt_lo) = hi_lo(k), hi_lo(vt)
        _chk_dev(k, vt)
        p.seg[i].k, p.seg[i].vt, p.seg[i].nk, p.seg[i].nk_pad = L.ptr(k), L.ptr(vt), nk, k.shape[1]
        p.seg[i].k_lo, p.seg[i].vt_lo = L.ptr(k_lo), L.ptr(vt_lo)
    p.out, p.BH, p.dtype, p.variant, p.kv_heads = L.ptr(out), BH, L.dtype_code(dtype), variant, kv_heads
    if head_major:
        p.ldo, p.out_bh_stride = out.stride(1), out.stride(0)
    else:
        p.ldo = out.stride(0)
    if lse is not None:
        _chk_dev(lse)
        if lse.dtype != torch.float32 or tuple(lse.shape) != (BH, q.shape[1]) or not lse.is_contiguous():
            raise L.OvgError("lse must be a contiguous f32 [BH, nq_pad] tensor")
        p.lse = L.ptr(lse)
    p.kv_splits, p.cus = kv_splits, cus            # cus: CUs the launch plan may count on (0 = all; sharded runs leave some to RCCL)
    if split_ws is not None and split_ws[0] is not None:
        _chk_dev(*split_ws)
        p.ws_part, p.ws_lse = L.ptr(split_ws[0]), L.ptr(split_ws[1])
        p.ws_part_bytes, p.ws_lse_bytes = nbytes(split_ws[0]), nbytes(split_ws[1])
    if fallback_count is not None:
        _chk_dev(fallback_count)
        p.fallback_count = L.ptr(fallback_count)
    L.call("ovg_flash_attn", p, _stream())
    return ret


def attn_merge(a, lse_a, b, lse_b, dtype, out=None):
    """Exact merge of two token-major attention results [n, 1024] over disjoint key sets (B = 1);
    lse_a / lse_b f32 [16, n_pad] from flash_attn(..., lse=...). out may alias a or b."""
    if out is None:
        out = empty_like_dtype(tuple(a.shape), dtype, a.device)
    ret = out
    (a, a_lo), (b, b_lo), (out, out_lo) = hi_lo(a), hi_lo(b), hi_lo(out)
    _chk_dev(a, b, lse_a, lse_b, out)
    p = L.AttnMergeParams(L.ptr(a), a.stride(0), L.ptr(lse_a), L.ptr(b), b.stride(0), L.ptr(lse_b), L.ptr(out), out.stride(0),
                          a.shape[0], lse_a.shape[1], L.dtype_code(dtype), L.ptr(a_lo), L.ptr(b_lo), L.ptr(out_lo))
    L.call("ovg_attn_merge", p, _stream())
    return ret


def pack_weights(src, dtype, k_pad=None, out=None):
    """f32 [rows, k] (any trailing dims flattened) -> dtype [rows, k_pad] on the device, zero padded (out: optional caller storage, row stride allowed)."""
    _chk_dev(src)
    s2 = src.detach().reshape(src.shape[0], -1).float().contiguous()
    rows, k = s2.shape
    k_pad = k if k_pad is None else k_pad
    if out is None:
        out = empty_like_dtype((rows, k_pad), dtype, src.device)
    o_hi, o_lo = hi_lo(out)
    p = L.PackWeightsParams(L.ptr(s2), s2.stride(0), L.ptr(o_hi), o_hi.stride(0), rows, k, k_pad, L.dtype_code(dtype), L.ptr(o_lo))
    L.call("ovg_pack_weights", p, _stream())
    return out


def block_workspace_bytes(M, seq, dtype, nq_pad=None, nk_pad=None, BH=None):
    """dict of scratch bytes an ovg_block_forward call with these shapes needs (host-only query; split-f16 mode: of ONE plane of
    each tensor). nq_pad / nk_pad: rows of the q / k buffers (default: seq padded to 64); BH: default (M // seq) * 16."""
    p = L.BlockParams()
    p.M, p.seq, p.BH = M, seq, ((M // seq) * H if BH is None else BH)
    p.nq_pad = pad_to(seq, KV_TILE) if nq_pad is None else nq_pad
    p.nk_pad = pad_to(seq, KV_TILE) if nk_pad is None else nk_pad
    p.dtype = dtype if isinstance(dtype, int) else L.dtype_code(dtype)
    ws = L.BlockWorkspace()
    L.check(L.load().ovg_block_workspace_bytes(L.C.byref(p), L.C.byref(ws)), "ovg_block_workspace_bytes")
    return {f: getattr(ws, f) for f, _ in L.BlockWorkspace._fields_}


def block_extra_segments(p, segments, local_seg_index=0):
    """Fill the remote K / V^T segments of an L.BlockParams: segments = list of (k [BH,nk_pad,64], vt [BH,64,nk_pad], nk) as flash_attn
    takes them (HiLo pairs in the split-f16 mode); the block's own keys become segment `local_seg_index` of the 1 + len(segments)
    the attention step runs over, the others keep their order. More than OVG_MAX_SEG - 1 segments cannot be stored: the count is
    passed on as it is and the entry refuses it."""
    for i, (k, vt, nk) in enumerate(segments[:L.OVG_MAX_SEG]):
        (k, k_lo), (vt, vt_lo) = hi_lo(k), hi_lo(vt)
        _chk_dev(k, vt)
        p.extra[i].k, p.extra[i].vt, p.extra[i].nk, p.extra[i].nk_pad = L.ptr(k), L.ptr(vt), nk, k.shape[1]
        p.extra[i].k_lo, p.extra[i].vt_lo = L.ptr(k_lo), L.ptr(vt_lo)
    p.nseg_extra, p.local_seg_index = len(segments), local_seg_index
    return p


def heads_to_tokens(x, n, dtype, out=None):
    """x [heads, n_pad, 64] head-major -> out [n, heads*64] token-major (16-bit dtypes)."""
    _chk_dev(x, out)
    heads, n_pad = x.shape[0], x.shape[1]
    if out is None:
        out = torch.empty(n, heads * D, device=x.device, dtype=dtype)
    p = L.HeadsToTokensParams(L.ptr(x), n_pad, L.ptr(out), out.stride(0), n, heads, L.dtype_code(dtype))
    L.call("ovg_heads_to_tokens", p, _stream())
    return out


def copy_rows(x, y):
    """y[r, :n] = x[r, :n] for f32 row-strided views x, y [rows, n] (ovg_copy_rows)."""
    _chk_dev(x, y)
    p = L.CopyRowsParams(L.ptr(x), x.stride(0), L.ptr(y), y.stride(0), x.shape[0], x.shape[1])
    L.call("ovg_copy_rows", p, _stream())
    return y


def im2col_rgb(images, dtype, k_pad=640, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=None):
    """images f32 [V,3,H,W] -> [V*gh*gw, k_pad] normalised patches."""
    _chk_dev(images)
    V, Cc, Hp, Wp = images.shape
    if out is None:            # caller storage must be dense [V*gh*gw, k_pad]
        out = empty_like_dtype((V * (Hp // 14) * (Wp // 14), k_pad), dtype, images.device)
    o_hi, o_lo = hi_lo(out)
    p = L.Im2colParams()
    p.img, p.out, p.k_pad, p.V, p.C, p.Hpx, p.Wpx = L.ptr(images), L.ptr(o_hi), k_pad, V, Cc, Hp, Wp
    p.out_lo = L.ptr(o_lo)
    p.dtype, p.mode = L.dtype_code(dtype), 0
    for i in range(3):
        p.mean[i], p.std[i] = mean[i], std[i]
    L.call("ovg_im2col", p, _stream())
    return out


def depth_stats(depth, mask):
    """depth, mask f32 [B, n] -> f64 [B,2] = {masked sum, count} (deterministic two-stage)."""
    _chk_dev(depth, mask)
    B, n = depth.shape
    nblocks = 256
    stats = torch.empty(B, 2, device=depth.device, dtype=torch.float64)
    partial = torch.empty(B * nblocks * 2, device=depth.device, dtype=torch.float64)
    p = L.DepthStatsParams(L.ptr(depth), L.ptr(mask), B, n, L.ptr(stats), L.ptr(partial), nblocks)
    L.call("ovg_depth_stats", p, _stream())
    return stats


def im2col_depth(depth, mask, stats, views_per_batch, dtype, k_pad=448, out=None):
    """depth, mask f32 [V,H,W]; stats f64 [B,2] -> [V*gh*gw, k_pad] (channels: normalised depth, mask)."""
    _chk_dev(depth, mask, stats)
    V, Hp, Wp = depth.shape
    if out is None:
        out = empty_like_dtype((V * (Hp // 14) * (Wp // 14), k_pad), dtype, depth.device)
    o_hi, o_lo = hi_lo(out)
    p = L.Im2colParams()
    p.img, p.img2, p.out, p.k_pad, p.V, p.C, p.Hpx, p.Wpx = L.ptr(depth), L.ptr(mask), L.ptr(o_hi), k_pad, V, 2, Hp, Wp
    p.out_lo = L.ptr(o_lo)
    p.dtype, p.mode, p.depth_stats, p.views_per_batch = L.dtype_code(dtype), 1, L.ptr(stats), views_per_batch
    L.call("ovg_im2col", p, _stream())
    return out


def dino_specials(x, V, tokens_per_view, cls, pos0, reg):
    _chk_dev(x, cls, pos0, reg)
    p = L.DinoSpecialsParams(L.ptr(x), x.stride(0), V, tokens_per_view, L.ptr(cls), L.ptr(pos0), L.ptr(reg), reg.shape[0])
    L.call("ovg_dino_specials", p, _stream())


def assemble_tokens(xd, norm_w, norm_b, eps, camera_token, register_token, cam_add, depth_tok, depth_row, placeholder,
                    out, V, S, tokens_per_view=1374, n_special=5, view0=0):
    _chk_dev(xd, out)
    p = L.AssembleParams()
    p.xd, p.ldxd, p.norm_w, p.norm_b, p.eps = L.ptr(xd), xd.stride(0), L.ptr(norm_w), L.ptr(norm_b), eps
    p.camera_token, p.register_token, p.cam_add = L.ptr(camera_token), L.ptr(register_token), L.ptr(cam_add)
    p.depth_tok, p.depth_row, p.placeholder = L.ptr(depth_tok), L.ptr(depth_row), L.ptr(placeholder)
    p.out, p.ldo, p.V, p.S, p.tokens_per_view, p.n_special = L.ptr(out), out.stride(0), V, S, tokens_per_view, n_special
    p.view0 = view0
    L.call("ovg_assemble_tokens", p, _stream())


def probe_mfma(a_frag, b_frag, dtype_code):
    """a_frag, b_frag: int32 [64,4] raw fragments -> f32 [64,4] accumulator of one 16x16 MFMA."""
    out = torch.empty(64, 4, device=a_frag.device, dtype=torch.float32)
    rc = L.load().ovg_probe_mfma(L.ptr(a_frag), L.ptr(b_frag), L.ptr(out), dtype_code, _stream())
    L.check(rc, "ovg_probe_mfma")
    return out


# ---------------------------------------------------------------------------------------------
# DPT head entries (NHWC activations, 16-bit modes)
# ---------------------------------------------------------------------------------------------
def head_layernorm(x, weight, bias, eps, dtype, views, tokens_per_view=1374, n_special=5, out=None):
    """x: f32 aggregator output [views*tokens_per_view, 2048] (row stride allowed) -> [views*(tokens_per_view-n_special), 2048]."""
    _chk_dev(x, weight, bias)
    p0 = tokens_per_view - n_special
    if out is None:
        out = torch.empty(views * p0, 2048, device=x.device, dtype=dtype)
    p = L.HeadLayerNormParams(L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), L.ptr(weight), L.ptr(bias),
                              views * p0, p0, tokens_per_view, n_special, eps, L.dtype_code(dtype))
    L.call("ovg_head_layernorm", p, _stream())
    return out


def conv(x, w, bias, dtype, cout, ksize=1, stride=1, upshuffle=0, relu=False, add1=None, add2=None, pos=None, out_f32=False, out=None):
    """NHWC convolution. x [n,H,W,Cin] dtype (contiguous), w [w_rows, k*k*Cin] dtype (taps-major), bias f32 [cout] or None.
    upshuffle = s: ConvTranspose2d(kernel = stride = s) -> [n, H*s, W*s, cout]. pos = (pos_x [OW,cout/2], pos_y [OH,cout/2])."""
    _chk_dev(x, w, bias, add1, add2)
    n, H, W, cin = x.shape
    pad = ksize // 2
    OH, OW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    s = upshuffle if upshuffle > 1 else 1
    if out is None:            # caller storage: [n, OH*s, OW*s, cout] with a pixel stride >= cout
        out = torch.empty(n, OH * s, OW * s, cout, device=x.device, dtype=torch.float32 if out_f32 else dtype)
    p = L.ConvParams()
    p.x, p.ldx, p.w, p.bias, p.y, p.ldy = L.ptr(x), x.stride(2), L.ptr(w), L.ptr(bias), L.ptr(out), out.stride(2)
    if add1 is not None:
        p.add1, p.ld1 = L.ptr(add1), add1.stride(2)
    if add2 is not None:
        p.add2, p.ld2 = L.ptr(add2), add2.stride(2)
    if pos is not None:
        p.pos_x, p.pos_y = L.ptr(pos[0]), L.ptr(pos[1])
    p.n_img, p.H, p.W, p.Cin, p.Cout, p.w_rows = n, H, W, cin, cout, w.shape[0]
    p.ksize, p.stride, p.upshuffle, p.relu, p.out_f32, p.dtype = ksize, stride, upshuffle, 1 if relu else 0, 1 if out_f32 else 0, L.dtype_code(dtype)
    L.call("ovg_conv", p, _stream())
    return out


def upsample(x, OH, OW, dtype, pos=None, out=None):
    """Bilinear align_corners=True resize of NHWC x [n,H,W,C] -> [n,OH,OW,C] (+ UV position embedding tables)."""
    _chk_dev(x)
    n, H, W, c = x.shape
    if out is None:
        out = torch.empty(n, OH, OW, c, device=x.device, dtype=dtype)
    p = L.UpsampleParams()
    p.x, p.ldx, p.y, p.ldy = L.ptr(x), x.stride(2), L.ptr(out), out.stride(2)
    if pos is not None:
        p.pos_x, p.pos_y = L.ptr(pos[0]), L.ptr(pos[1])
    p.n_img, p.H, p.W, p.OH, p.OW, p.C, p.dtype = n, H, W, OH, OW, c, L.dtype_code(dtype)
    L.call("ovg_upsample", p, _stream())
    return out


def dpt_tail_supported(x, dtype, OH=None, OW=None):
    """The one-launch output stage (ovg_dpt_tail) exists for the plain 16-bit dtypes and the model's 128-channel map. Mirrors every
    host-side limit of the C entry (csrc/ovg_head.hip: ovg_dpt_tail) that answers OVG_E_UNSUPPORTED / OVG_E_ARG for a shape the three-launch
    form still serves -- one source image within 32-bit element offsets, an output of at least 2 x 2 pixels, 16-byte aligned rows --
    so that callers fall back to upsample -> conv -> dpt_out instead of raising (round-5 advisor)."""
    if dtype not in (torch.bfloat16, torch.float16) or x.dim() != 4 or x.shape[-1] != 128:
        return False
    n, H, W, c = x.shape
    ldx = x.stride(2)
    if H * W * ldx >= (1 << 31) or ldx % 8 or (x.data_ptr() & 15):
        return False
    if OH is not None and (OH <= 1 or OW <= 1):
        return False
    return True


def dpt_tail(x, OH, OW, dtype, pos, w1, b1, w2, b2, activation, out=None):
    """x [n,H,W,128] dtype -> upsample to (OH, OW) + pos -> conv3x3(128->32)+ReLU -> conv1x1 -> activation: (val [n,OH,OW,od-1], conf [n,OH,OW]).
    w1 [>=32, 9*128] dtype taps-major (the zero-padded matrix of the ovg_conv form is fine)."""
    _chk_dev(x, w1, b1, w2, b2)
    n, H, W, c = x.shape
    od = w2.shape[0]
    val, conf = out if out is not None else (torch.empty(n, OH, OW, od - 1, device=x.device, dtype=torch.float32),
                                             torch.empty(n, OH, OW, device=x.device, dtype=torch.float32))      # caller storage must be dense
    p = L.DptTailParams()
    p.x, p.ldx, p.w1, p.ldw1, p.b1, p.w2, p.b2, p.val, p.conf = L.ptr(x), x.stride(2), L.ptr(w1), w1.stride(0), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(val), L.ptr(conf)
    if pos is not None:
        p.pos_x, p.pos_y = L.ptr(pos[0]), L.ptr(pos[1])
    p.n_img, p.H, p.W, p.OH, p.OW, p.C, p.out_dim, p.activation, p.dtype = n, H, W, OH, OW, c, od, 0 if activation == "exp" else 1, L.dtype_code(dtype)
    L.call("ovg_dpt_tail", p, _stream())
    return val, conf


def dpt_out(h, w2, b2, activation, out=None):
    """h f32 [n,H,W,32] (post-ReLU) -> (val [n,H,W,out_dim-1], conf [n,H,W]); activation 'exp' | 'inv_log'."""
    _chk_dev(h, w2, b2)
    n, H, W, _ = h.shape
    od = w2.shape[0]
    val, conf = out if out is not None else (torch.empty(n, H, W, od - 1, device=h.device, dtype=torch.float32),
                                             torch.empty(n, H, W, device=h.device, dtype=torch.float32))
    p = L.DptOutParams(L.ptr(h), L.ptr(w2), L.ptr(b2), L.ptr(val), L.ptr(conf), n * H * W, od, 0 if activation == "exp" else 1)
    L.call("ovg_dpt_out", p, _stream())
    return val, conf


def camera_head_workspace_bytes(S, dtype):
    n = L.load().ovg_camera_head_workspace_bytes(S, L.dtype_code(dtype))
    if n < 0:
        raise L.OvgError("ovg_camera_head_workspace_bytes: unsupported (S=%d, dtype=%s)" % (S, dtype))
    return int(n)


def camera_head(tokens, W, dtype, iters=4, ws=None, out=None):
    """Whole CameraHead.forward (camera_head.py:84-154) of one batch element in one call.
    tokens: f32 [S, 2048] view of the camera tokens (row stride allowed, e.g. out[-1][b, :, 0]); W: packed weights
    (heads_hip.HipCameraHead._pack: GEMM matrices in `dtype`, everything else f32); -> [iters, S, 9] f32."""
    _chk_dev(tokens, ws)
    S = tokens.shape[0]
    if tokens.dtype != torch.float32 or tokens.shape[1] != 2048 or tokens.stride(1) != 1:
        raise L.OvgError("camera_head: tokens must be f32 [S, 2048] with unit inner stride")
    need = camera_head_workspace_bytes(S, dtype)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, device=tokens.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(iters, S, 9, device=tokens.device, dtype=torch.float32)
    p = L.CameraHeadParams()
    p.tokens, p.ld_tokens, p.S, p.iters, p.dtype = L.ptr(tokens), tokens.stride(0), S, iters, L.dtype_code(dtype)
    p.trunk_depth, p.dim, p.heads = len(W["blocks"]), 2048, W["heads"]
    for name in ("token_norm_w", "token_norm_b", "trunk_norm_w", "trunk_norm_b", "empty_pose", "embed_w", "embed_b", "mod_w", "mod_b",
                 "pb1_w", "pb1_b", "pb2_w", "pb2_b"):
        _chk_dev(W[name])
        setattr(p, name, L.ptr(W[name]))
    for i, blk in enumerate(W["blocks"]):
        for name, _ in L.CameraBlockWeights._fields_:
            _chk_dev(blk[name])
            setattr(p.blk[i], name, L.ptr(blk[name]))
    p.ws, p.ws_bytes, p.out = L.ptr(ws), ws.numel() * ws.element_size(), L.ptr(out)
    L.call("ovg_camera_head", p, _stream())
    return out


def camera_tables(extrinsics, intrinsics, index, S, hw, pose_w, pose_b, adapt_w, adapt_b, out=None):
    """Camera-modality injection tables [G, B*S, 1024] f32 built on the device in <= 3 launches, no host round trip
    (ovg_camera_tables). extrinsics [B,S,3,4] / intrinsics [B,S,3,3] f32 device tensors (ignored when index is None);
    index: int32 DEVICE tensor [Sc] of the views that carry a GT camera, or None; pose_w [G*1024, 9], pose_b [G*1024],
    adapt_w [G,1024,1024], adapt_b [G,1024] f32."""
    _chk_dev(pose_w, pose_b, adapt_w, adapt_b, index, out)
    G = adapt_b.shape[0]
    Sc = 0 if index is None else int(index.numel())
    B = 1 if Sc == 0 else extrinsics.shape[0]
    dev = adapt_b.device
    if out is None:
        out = torch.empty(G, B * S, C, device=dev, dtype=torch.float32)
    p = L.CameraTablesParams()
    p.B, p.S, p.Sc, p.H, p.W, p.G = B, S, Sc, int(hw[0]), int(hw[1]), G
    p.pose_w, p.pose_b, p.adapt_w, p.adapt_b, p.tables = L.ptr(pose_w), L.ptr(pose_b), L.ptr(adapt_w), L.ptr(adapt_b), L.ptr(out)
    keep = None
    if Sc:
        _chk_dev(extrinsics, intrinsics)
        if index.dtype != torch.int32 or not index.is_contiguous():
            raise L.OvgError("camera_tables: index must be a contiguous int32 device tensor")
        ext = extrinsics.detach().to(torch.float32).contiguous()
        intr = intrinsics.detach().to(torch.float32).contiguous()
        if tuple(ext.shape[1:]) != (S, 3, 4) or tuple(intr.shape) != (B, S, 3, 3):
            raise L.OvgError("camera_tables: extrinsics must be [B,S,3,4] and intrinsics [B,S,3,3]")
        enc = torch.empty(B * Sc, 9, device=dev, dtype=torch.float32)
        emb = torch.empty(G, B * Sc, C, device=dev, dtype=torch.float32)
        keep = (ext, intr, enc, emb)
        p.extrinsics, p.intrinsics, p.index, p.enc, p.emb = L.ptr(ext), L.ptr(intr), L.ptr(index), L.ptr(enc), L.ptr(emb)
    L.call("ovg_camera_tables", p, _stream())
    del keep          # the caching allocator keeps freed blocks valid for work already queued on this stream
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry wrappers (unproject .. mesh_smooth). Each reads as: what it checks, what it allocates, how it fills the struct; the
# checks below are the one implementation of each kind. The older wrappers (.. knn_normals) test the device first, the newer ones
# test shapes first and the device last.
# ---------------------------------------------------------------------------------------------------------------------------------
_F32, _F64, _U8, _I32, _I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
_F32_MAX = 3.4028234663852886e38


def _ws_query(symbol, **dims):
    """A host-only `*_workspace_bytes` query of the library -> bytes. Every integer must fit its C argument type (int32 / int64,
    from L.SYMBOLS) and the library must not answer with a negative value."""
    ctypes_ = L.SYMBOLS[symbol][1]
    if all(-(1 << 8 * L.C.sizeof(ct) - 1) <= int(v) < 1 << 8 * L.C.sizeof(ct) - 1 for ct, v in zip(ctypes_, dims.values())):
        b = getattr(L.load(), symbol)(*(int(v) for v in dims.values()))
        if b >= 0:
            return int(b)
    raise L.OvgError("%s: unsupported (%s)" % (symbol, ", ".join("%s=%d" % kv for kv in dims.items())))


def _tensor(what, t, name, dtype, shape=None, numel=None, min_numel=None, optional=False):
    """t must be a contiguous `dtype` tensor of exactly `shape`, or of any shape with exactly `numel` / at least `min_numel` elements
    (none of the three: any size). None passes only when optional."""
    if t is None and optional:
        return
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()
    if ok and shape is not None:
        ok = tuple(t.shape) == tuple(shape)
    if ok and numel is not None:
        ok = t.numel() == numel
    if ok and min_numel is not None:
        ok = t.numel() >= min_numel
    if not ok:
        size = " %r" % (list(shape),) if shape is not None else " of %s elements" % numel if numel is not None else \
            " of at least %s elements" % min_numel if min_numel is not None else ""
        raise L.OvgError("%s: %s must be a contiguous %s tensor%s" % (what, name, str(dtype).replace("torch.", ""), size))


def _rows(what, t, name, dtype, width):
    """t must be a contiguous `dtype` tensor of any shape that holds `width` values per row -> the number of rows."""
    _tensor(what, t, name, dtype)
    if t.numel() % width:
        raise L.OvgError("%s: %s must be a contiguous %s tensor of %d values per row" % (what, name, str(dtype).replace("torch.", ""), width))
    return t.numel() // width


def _table(what, t, name, dtype, width, min_rows=0, max_rows=None):
    """t must be a contiguous `dtype` tensor [n, width] with min_rows <= n (< max_rows) -> n."""
    _tensor(what, t, name, dtype)
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < min_rows or (max_rows is not None and t.shape[0] >= max_rows):
        bound = (", %d <= n" % min_rows if min_rows else "") + (" < %d" % max_rows if max_rows is not None else "")
        raise L.OvgError("%s: %s must be a contiguous %s tensor [n, %d]%s" % (what, name, str(dtype).replace("torch.", ""), width, bound))
    return int(t.shape[0])


def _points(what, t, name, min_rows=0, max_rows=None):
    """t must be a contiguous f32 tensor [n, 3] with min_rows <= n (< max_rows) -> n."""
    return _table(what, t, name, _F32, 3, min_rows, max_rows)


def _query_reference(what, query, reference, query_valid, reference_valid, exclude_self, origin=None, out_stats=None):
    """The arguments the nearest-neighbour and grid searches share -> (nq, nr)."""
    nq, nr = _points(what, query, "query"), _points(what, reference, "reference")
    _tensor(what, query_valid, "query_valid", _U8, (nq,), optional=True)
    _tensor(what, reference_valid, "reference_valid", _U8, (nr,), optional=True)
    _tensor(what, origin, "origin", _F32, numel=3, optional=True)
    if exclude_self and nq != nr:
        raise L.OvgError("%s: exclude_self needs nq == nr (got %d, %d)" % (what, nq, nr))
    _tensor(what, out_stats, "out_stats", _I64, numel=4, optional=True)
    return nq, nr


def _out(what, t, name, dtype, shape, device, any_shape=False):
    """An output: allocated when None, else checked (any_shape: only for the element count of `shape`)."""
    if t is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if any_shape:
        _tensor(what, t, name, dtype, numel=math.prod(shape))
    else:
        _tensor(what, t, name, dtype, shape)
    return t


def _workspace(ws, need, device):
    """The caller's workspace when it holds `need` bytes, else a fresh one."""
    return torch.empty(need, device=device, dtype=_U8) if ws is None or nbytes(ws) < need else ws


def _number(what, name, value, lo=None, hi=None, strict=False, f32=True):
    """A host number (not a bool, not NaN) with lo <= value <= hi (strict: lo < value) -> float(value). f32: it is passed on as a
    float32 and must be finite there; otherwise +-inf and any magnitude pass."""
    ok = not isinstance(value, bool) and isinstance(value, (int, float)) and value == value
    if ok and lo is not None:
        ok = value > lo if strict else value >= lo
    if ok and hi is not None:
        ok = value <= hi
    if ok and f32:
        ok = abs(value) <= _F32_MAX
    if ok:
        try:
            return float(value)
        except OverflowError:                                                # an integer beyond float64
            pass
    rule = ("" if lo is None else " %s %r" % (">" if strict else ">=", lo)) + ("" if hi is None else " <= %r" % (hi,))
    raise L.OvgError("%s: %s must be a %s%s, got %r" % (what, name, "finite float32 number" if f32 else "number (not NaN)", rule, value))


def _int_in(what, name, value, lo, hi):
    """A host integer (not a bool) with lo <= value < hi."""
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value < hi:
        raise L.OvgError("%s: %s must be an integer in [%d, %d), got %r" % (what, name, lo, hi, value))
    return value


def _capacity_buffers(what, buffers):
    """The outputs of a SCATTER stage, buffers = (tensor, name, dtype, elements it must hold, required): nothing is asked of the
    buffers of a zero capacity, and a buffer that is not required may be None."""
    for t, name, dtype, need, required in buffers:
        if need:
            _tensor(what, t, name, dtype, min_numel=need, optional=not required)


def unproject(depth, cam):
    """depth f32 [S,H,W], cam f32 [S,16] (cam-to-world R row-major, t, fu, fv, cu, cv) -> world points [S,H,W,3] f32."""
    _chk_dev(depth, cam)
    S, H, W = depth.shape
    out = torch.empty(S, H, W, 3, device=depth.device, dtype=torch.float32)
    p = L.UnprojectParams(L.ptr(depth), L.ptr(cam), L.ptr(out), S, H, W)
    L.call("ovg_unproject", p, _stream())
    return out


def percentile_workspace_bytes(n, ncols):
    return _ws_query("ovg_percentile_workspace_bytes", n=n, ncols=ncols)


def percentile(x, n, stride, col_stride, ncols, qs, mask=None, norm=False, ws=None):
    """numpy-2 linear percentiles `qs` (<= 4, in [0, 100]) of `ncols` (<= 4) f32 columns of x: key i of column c at element
    c * col_stride + i * stride (element offsets from x's data pointer). mask: optional contiguous f32 [n] (key * (mask > 0.1)).
    -> out [ncols, len(qs)] f32 on the device (and, with norm=True and two percentiles, the 0-d f32 norm of out[:, 1] - out[:, 0])."""
    what = "percentile"
    _chk_dev(x, mask, ws)
    if x.dtype != torch.float32:
        raise L.OvgError("%s: x must be f32" % what)
    _tensor(what, mask, "mask", _F32, optional=True)
    last = (ncols - 1) * col_stride + (n - 1) * stride
    if n < 1 or stride < 1 or col_stride < 0 or x.storage_offset() + last >= x.untyped_storage().nbytes() // 4 or \
            (mask is not None and mask.numel() < n):
        raise L.OvgError("%s: the strided columns (or the mask) reach outside the tensor" % what)
    ws = _workspace(ws, percentile_workspace_bytes(n, ncols), x.device)
    out = torch.empty(ncols, len(qs), device=x.device, dtype=torch.float32)
    nrm = torch.empty((), device=x.device, dtype=torch.float32) if norm else None
    p = L.PercentileParams()
    p.x, p.n, p.stride, p.col_stride, p.ncols, p.nq = L.ptr(x), int(n), int(stride), int(col_stride), int(ncols), len(qs)
    for j, q in enumerate(qs[:L.PCT_MAX_Q]):
        p.q[j] = float(q)
    p.mask, p.out, p.norm_out, p.ws, p.ws_bytes = L.ptr(mask), L.ptr(out), L.ptr(nrm), L.ptr(ws), nbytes(ws)
    L.call("ovg_percentile", p, _stream())
    return (out, nrm) if norm else out


def point_filter_workspace_bytes(n):
    return _ws_query("ovg_point_filter_workspace_bytes", n=n)


def point_filter(stage, conf, images, points, hw, ws, threshold=None, mask=None, min_conf=1e-5, flags=0, index_base=0,
                 out_count=None, capacity=0, out_points=None, out_colors=None, out_index=None):
    """ovg_point_filter on contiguous device tensors: conf f32 [n], images f32 NCHW [n / hw, 3, hw], points f32 [n, 3], threshold a
    0-d / 1-element f32 device tensor or None (0), mask f32 [n] or None. stage L.PF_COUNT writes the int64 cloud size to out_count;
    L.PF_SCATTER writes the first `capacity` kept pixels (in pixel order) to out_points / out_colors / out_index from what the COUNT
    stage left in ws."""
    what = "point_filter"
    _chk_dev(conf, images, points, ws, threshold, mask, out_count, out_points, out_colors, out_index)
    _tensor(what, conf, "conf", _F32)
    n = conf.numel()
    _tensor(what, images, "images", _F32, numel=3 * n)
    _tensor(what, points, "points", _F32, numel=3 * n)
    _tensor(what, threshold, "threshold", _F32, optional=True)
    _tensor(what, mask, "mask", _F32, numel=n, optional=True)
    if hw <= 0 or n % hw:
        raise L.OvgError("%s: hw must be positive and divide the pixel count" % what)
    if stage & L.PF_SCATTER:
        _tensor(what, out_points, "out_points", _F32, min_numel=3 * capacity, optional=True)
        _tensor(what, out_colors, "out_colors", _U8, min_numel=3 * capacity, optional=True)
        _tensor(what, out_index, "out_index", _I64, min_numel=capacity, optional=True)
    if out_count is not None and (out_count.dtype != torch.int64 or out_count.numel() < 1):
        raise L.OvgError("%s: out_count must be an int64 device tensor" % what)
    p = L.PointFilterParams()
    p.conf, p.mask, p.threshold, p.min_conf, p.flags = L.ptr(conf), L.ptr(mask), L.ptr(threshold), float(min_conf), int(flags)
    p.images, p.hw, p.points, p.n, p.stage = L.ptr(images), int(hw), L.ptr(points), n, int(stage)
    p.index_base, p.capacity = int(index_base), int(capacity)
    p.out_points, p.out_colors, p.out_index, p.out_count = L.ptr(out_points), L.ptr(out_colors), L.ptr(out_index), L.ptr(out_count)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_point_filter", p, _stream())


def voxel_downsample_workspace_bytes(n):
    return _ws_query("ovg_voxel_downsample_workspace_bytes", n=n)


def voxel_downsample(stage, points, voxel, ws, conf=None, colors=None, out_count=None, capacity=0, out_points=None, out_colors=None,
                     out_index=None):
    """ovg_voxel_downsample on contiguous device tensors: points f32 [n, 3], voxel a 0-d / 1-element f32 device tensor, conf f32 [n] or
    None, colors u8 [n, 3] or None. stage L.VG_COUNT writes (M', flags) to the two int64 of out_count; L.VG_SCATTER writes the first
    `capacity` winners (in input order) to out_points / out_colors / out_index from what the COUNT stage left in ws."""
    what = "voxel_downsample"
    _chk_dev(points, voxel, ws, conf, colors, out_count, out_points, out_colors, out_index)
    n = _rows(what, points, "points", _F32, 3)
    _tensor(what, voxel, "voxel", _F32, numel=1)
    _tensor(what, conf, "conf", _F32, numel=n, optional=True)
    _tensor(what, colors, "colors", _U8, numel=3 * n, optional=True)
    if stage & L.VG_SCATTER:
        _tensor(what, out_points, "out_points", _F32, min_numel=3 * capacity, optional=True)
        _tensor(what, out_colors, "out_colors", _U8, min_numel=3 * capacity, optional=True)
        _tensor(what, out_index, "out_index", _I64, min_numel=capacity, optional=True)
    _tensor(what, out_count, "out_count", _I64, min_numel=2, optional=True)
    p = L.VoxelDownsampleParams()
    p.points, p.conf, p.colors, p.voxel, p.n, p.stage = L.ptr(points), L.ptr(conf), L.ptr(colors), L.ptr(voxel), n, int(stage)
    p.capacity = int(capacity)
    p.out_points, p.out_colors, p.out_index, p.out_count = L.ptr(out_points), L.ptr(out_colors), L.ptr(out_index), L.ptr(out_count)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_voxel_downsample", p, _stream())


def render_workspace_bytes(V, H, W):
    return _ws_query("ovg_render_workspace_bytes", V=V, H=H, W=W)


def render_points(points, colors, cams, H, W, radius=1, near=1e-3, background=(255, 255, 255), depth=True, index=False, ws=None,
                  flags=0):
    """ovg_render_points on contiguous device tensors: points f32 [n, 3], colors u8 [n, 3], cams f32 [V, 16] (world-to-camera rotation
    row-major, translation, fx, fy, cx, cy). -> (rgb u8 [V, H, W, 3], depth f32 [V, H, W] or None, index int64 [V, H, W] or None),
    allocated here; ws: an optional uint8 device tensor of at least render_workspace_bytes(V, H, W) bytes. Nothing is read back."""
    what = "render_points"
    _chk_dev(points, colors, cams, ws)
    n, V = _rows(what, points, "points", _F32, 3), _rows(what, cams, "cams", _F32, 16)
    _tensor(what, colors, "colors", _U8, numel=3 * n)
    ws = _workspace(ws, render_workspace_bytes(V, H, W), cams.device)
    rgb = torch.empty(V, H, W, 3, device=cams.device, dtype=torch.uint8)
    dep = torch.empty(V, H, W, device=cams.device, dtype=torch.float32) if depth else None
    idx = torch.empty(V, H, W, device=cams.device, dtype=torch.int64) if index else None
    p = L.RenderParams()
    p.points, p.colors, p.n, p.cams = L.ptr(points) if n else None, L.ptr(colors) if n else None, n, L.ptr(cams)
    p.V, p.H, p.W, p.radius, p.near, p.flags = V, int(H), int(W), int(radius), float(near), int(flags)
    for k in range(3):
        p.background[k] = int(background[k])
    p.ws, p.ws_bytes, p.out_rgb, p.out_depth, p.out_index = L.ptr(ws), nbytes(ws), L.ptr(rgb), L.ptr(dep), L.ptr(idx)
    L.call("ovg_render_points", p, _stream())
    return rgb, dep, idx


def render_mesh_workspace_bytes(V, H, W):
    return _ws_query("ovg_render_mesh_workspace_bytes", V=V, H=H, W=W)


def render_mesh(vertices, faces, cams, H, W, normals=None, colors=None, shading=L.MESH_SHADE_HEADLIGHT, cull=L.MESH_CULL_NONE, near=1e-3,
                background=(255, 255, 255), depth=True, index=False, coop_threshold=0, ws=None, out=None, flags=0):
    """ovg_render_mesh on contiguous device tensors: vertices f32 [M, 3], faces int32 [F, 3], optional normals f32 [M, 3] and colors u8
    [M, 3], cams f32 [V, 16] (as for render_points). -> (rgb u8 [V, H, W, 3], depth f32 [V, H, W] or None, index int64 [V, H, W] or
    None), allocated here unless out = (rgb, depth or None, index or None) gives them; ws: an optional uint8 device tensor of at
    least render_mesh_workspace_bytes(V, H, W) bytes. Nothing is read back."""
    what = "render_mesh"
    _chk_dev(vertices, faces, cams, normals, colors, ws)
    M, F, V = _rows(what, vertices, "vertices", _F32, 3), _rows(what, faces, "faces", _I32, 3), _rows(what, cams, "cams", _F32, 16)
    _tensor(what, normals, "normals", _F32, numel=3 * M, optional=True)
    _tensor(what, colors, "colors", _U8, numel=3 * M, optional=True)
    ws = _workspace(ws, render_mesh_workspace_bytes(V, H, W), cams.device)
    if out is not None:
        rgb, dep, idx = out
    else:
        rgb = torch.empty(V, H, W, 3, device=cams.device, dtype=torch.uint8)
        dep = torch.empty(V, H, W, device=cams.device, dtype=torch.float32) if depth else None
        idx = torch.empty(V, H, W, device=cams.device, dtype=torch.int64) if index else None
    p = L.RenderMeshParams()
    p.vertices, p.faces = L.ptr(vertices) if M else None, L.ptr(faces) if F else None
    p.normals, p.colors = L.ptr(normals) if M else None, L.ptr(colors) if M else None
    p.M, p.F, p.cams = M, F, L.ptr(cams)
    p.V, p.H, p.W, p.shading, p.cull, p.coop_threshold = V, int(H), int(W), int(shading), int(cull), int(coop_threshold)
    p.near, p.flags = float(near), int(flags)
    for k in range(3):
        p.background[k] = int(background[k])
    p.ws, p.ws_bytes, p.out_rgb, p.out_depth, p.out_index = L.ptr(ws), nbytes(ws), L.ptr(rgb), L.ptr(dep), L.ptr(idx)
    L.call("ovg_render_mesh", p, _stream())
    return rgb, dep, idx


def consistency_workspace_bytes(S, H, W):
    return _ws_query("ovg_consistency_workspace_bytes", S=S, H=H, W=W)


def multiview_consistency(points, cams, tol, near=1e-3, valid=None, src_first=0, src_count=None, occluded=False, ws=None,
                          tile=L.MVC_TILE_DEFAULT, flags=0):
    """ovg_multiview_consistency on contiguous device tensors: points f32 [S, H, W, 3], cams f32 [S, 16] (packed as for render_points),
    valid u8 [S, H, W] or None. -> (support, violations, occluded or None), int16 [src_count, H, W] for the source views src_first ..
    src_first + src_count - 1 (all S by default), allocated here; ws: an optional uint8 device tensor of at least
    consistency_workspace_bytes(S, H, W) bytes (with L.MVC_KEEP_MAP in flags: the one an earlier call on the same inputs filled).
    Nothing is read back."""
    what = "multiview_consistency"
    _chk_dev(points, cams, valid, ws)
    _tensor(what, points, "points", _F32)
    if points.dim() != 4 or points.shape[3] != 3:
        raise L.OvgError("%s: points must be [S, H, W, 3]" % what)
    S, H, W = (int(v) for v in points.shape[:3])
    _tensor(what, cams, "cams", _F32, numel=16 * S)
    _tensor(what, valid, "valid", _U8, (S, H, W), optional=True)
    n = S - src_first if src_count is None else int(src_count)
    if not (0 <= src_first < S and 0 < n <= S - src_first):
        raise L.OvgError("%s: source views %d .. %d outside [0, %d)" % (what, src_first, src_first + n - 1, S))
    need = consistency_workspace_bytes(S, H, W)
    if (ws is None or nbytes(ws) < need) and flags & L.MVC_KEEP_MAP:
        raise L.OvgError("%s: MVC_KEEP_MAP needs the workspace of the call that computed the maps" % what)
    ws = _workspace(ws, need, points.device)
    sup = torch.empty(n, H, W, device=points.device, dtype=torch.int16)
    vio = torch.empty(n, H, W, device=points.device, dtype=torch.int16)
    occ = torch.empty(n, H, W, device=points.device, dtype=torch.int16) if occluded else None
    p = L.ConsistencyParams()
    p.points, p.cams, p.valid, p.S, p.H, p.W = L.ptr(points), L.ptr(cams), L.ptr(valid), S, H, W
    p.src_first, p.src_count, p.tol, p.near, p.tile, p.flags = int(src_first), n, float(tol), float(near), int(tile), int(flags)
    p.ws, p.ws_bytes, p.support, p.violations, p.occluded = L.ptr(ws), nbytes(ws), L.ptr(sup), L.ptr(vio), L.ptr(occ)
    L.call("ovg_multiview_consistency", p, _stream())
    return sup, vio, occ


def nn_workspace_bytes(nq, nr):
    return _ws_query("ovg_nn_workspace_bytes", nq=nq, nr=nr)


def nearest_neighbours(query, reference, query_valid=None, reference_valid=None, exclude_self=False, splits=0, ws=None, index=None,
                       sqdist=None):
    """ovg_nearest_neighbours on contiguous device tensors: query f32 [nq, 3], reference f32 [nr, 3], query_valid / reference_valid
    u8 [nq] / [nr] or None. -> (index int32 [nq], sqdist f32 [nq]): for every query the nearest usable reference (lowest index on
    ties; with exclude_self, nq == nr and reference i is skipped for query i), -1 / +inf where there is none. splits: 0 lets the
    library choose, any other value gives the same bytes; ws: an optional uint8 device tensor of at least nn_workspace_bytes(nq, nr)
    bytes; index / sqdist: optional outputs to write into. Nothing is read back."""
    what = "nearest_neighbours"
    _chk_dev(query, reference, query_valid, reference_valid, ws, index, sqdist)
    nq, nr = _query_reference(what, query, reference, query_valid, reference_valid, exclude_self)
    ws = _workspace(ws, nn_workspace_bytes(nq, nr), query.device)
    index = _out(what, index, "index", _I32, (nq,), query.device, any_shape=True)
    sqdist = _out(what, sqdist, "sqdist", _F32, (nq,), query.device, any_shape=True)
    p = L.NnParams()
    p.query, p.reference, p.query_valid, p.reference_valid = L.ptr(query), L.ptr(reference), L.ptr(query_valid), L.ptr(reference_valid)
    p.nq, p.nr, p.flags, p.splits = nq, nr, L.NN_EXCLUDE_SAME_INDEX if exclude_self else 0, int(splits)
    p.ws, p.ws_bytes, p.index, p.sqdist = L.ptr(ws), nbytes(ws), L.ptr(index), L.ptr(sqdist)
    L.call("ovg_nearest_neighbours", p, _stream())
    return index, sqdist


def fps_workspace_bytes(batch, n, npoint):
    return _ws_query("ovg_fps_workspace_bytes", batch=batch, n=n, npoint=npoint)


def farthest_point_sample(points, npoint, valid=None, first=0, include_last=False, path=0, ws=None, index=None, sqdist=None, distance=None):
    """ovg_farthest_point_sample on contiguous device tensors: points f32 [B, N, 3], valid u8 [B, N] or None. -> (index int32
    [B, npoint], sqdist f32 [B, npoint], distance): sample i of a cloud is the usable point farthest from samples 0 .. i - 1 (lowest index
    on ties; sample 0 is `first`, sample 1 is N - 1 with include_last), sqdist its squared distance to them (1e10 for the first), -1 /
    +inf where a cloud has no usable point. path: L.FPS_PATH_AUTO lets the library choose, L.FPS_PATH_ONE_WORKGROUP / L.FPS_PATH_PER_STEP
    force a form; all give the same bytes. ws: an optional uint8 device tensor of at least fps_workspace_bytes(B, N, npoint) bytes;
    index / sqdist: optional outputs to write into; distance: None, or True to allocate, or an f32 [B, N] tensor to fill with every
    point's squared distance to the nearest sample (returned as the third value, else None). Nothing is read back."""
    what = "farthest_point_sample"
    _chk_dev(points, valid, ws, index, sqdist, None if isinstance(distance, bool) else distance)
    _tensor(what, points, "points", _F32)
    if points.dim() != 3 or points.shape[2] != 3:
        raise L.OvgError("%s: points must be [B, N, 3]" % what)
    B, N, npoint = int(points.shape[0]), int(points.shape[1]), int(npoint)
    _tensor(what, valid, "valid", _U8, (B, N), optional=True)
    ws = _workspace(ws, fps_workspace_bytes(B, N, npoint), points.device)
    index = _out(what, index, "index", _I32, (B, npoint), points.device, any_shape=True)
    sqdist = _out(what, sqdist, "sqdist", _F32, (B, npoint), points.device, any_shape=True)
    if distance is None or distance is False:
        distance = None
    else:
        distance = _out(what, None if distance is True else distance, "distance", _F32, (B, N), points.device, any_shape=True)
    p = L.FpsParams()
    p.points, p.valid, p.batch, p.n, p.npoint, p.first = L.ptr(points), L.ptr(valid), B, N, npoint, int(first)
    p.flags, p.path = L.FPS_INCLUDE_LAST if include_last else 0, int(path)
    p.ws, p.ws_bytes, p.index, p.sqdist, p.distance = L.ptr(ws), nbytes(ws), L.ptr(index), L.ptr(sqdist), L.ptr(distance)
    L.call("ovg_farthest_point_sample", p, _stream())
    return index, sqdist, distance


def radius_reach(radius_sq):
    """REACH of include/omnivggt_hip.h for a float32 radius_sq: the float32 just above sqrt((double)radius_sq) (1 + 2^-20). The box of
    cells a query scans spans +-REACH per axis, and REACH is the smallest cell edge ovg_radius_search accepts."""
    import struct
    r2 = struct.unpack("f", struct.pack("f", float(radius_sq)))[0]
    v = math.sqrt(r2) * (1.0 + 2.0 ** -20)
    bits = struct.unpack("I", struct.pack("f", v))[0]                        # rounded to nearest
    if struct.unpack("f", struct.pack("I", bits))[0] <= v:
        bits += 1                                                            # positive and finite: the next float up
    return struct.unpack("f", struct.pack("I", bits))[0]


def radius_workspace_bytes(nq, nr):
    return _ws_query("ovg_radius_workspace_bytes", nq=nq, nr=nr)


def radius_search(stage, query, reference, radius_sq, cell, ws, query_valid=None, reference_valid=None, origin=None, exclude_self=False,
                  max_pairs=0, out_stats=None, count=None, index=None, sqdist=None):
    """ovg_radius_search on contiguous device tensors: query f32 [nq, 3], reference f32 [nr, 3], query_valid / reference_valid u8 [nq] /
    [nr] or None, origin f32 [3] or None (zeros); radius_sq and cell are host floats (taken as float32; cell >= radius_reach(radius_sq)),
    ws a uint8 device tensor of at least radius_workspace_bytes(nq, nr) bytes that carries the grid from one stage to the next.
    stage L.RS_BUILD bins the references and writes (flags, occupied cells, largest cell, candidate pairs) to out_stats (int64 [4],
    allocated when None); L.RS_SEARCH writes count int32 [nq], index int32 [nq] and sqdist f32 [nq] (allocated when None) -- or nothing
    at all when the candidate pairs exceed max_pairs, which out_stats (if given) then reports as L.RS_OVER_BUDGET.
    -> (out_stats, count, index, sqdist), None for what the stage does not write. Nothing is read back."""
    what = "radius_search"
    _chk_dev(query, reference, ws, query_valid, reference_valid, origin, out_stats, count, index, sqdist)
    nq, nr = _query_reference(what, query, reference, query_valid, reference_valid, exclude_self, origin, out_stats)
    stage = int(stage)
    if stage & L.RS_BUILD and out_stats is None:
        out_stats = torch.empty(4, device=query.device, dtype=torch.int64)
    if stage & L.RS_SEARCH:
        count = _out(what, count, "count", _I32, (nq,), query.device, any_shape=True)
        index = _out(what, index, "index", _I32, (nq,), query.device, any_shape=True)
        sqdist = _out(what, sqdist, "sqdist", _F32, (nq,), query.device, any_shape=True)
    else:
        count = index = sqdist = None
    p = L.RadiusParams()
    p.query, p.reference, p.query_valid, p.reference_valid = L.ptr(query), L.ptr(reference), L.ptr(query_valid), L.ptr(reference_valid)
    p.origin, p.nq, p.nr, p.radius_sq, p.cell = L.ptr(origin), nq, nr, float(radius_sq), float(cell)
    p.flags, p.stage, p.max_pairs = L.RS_EXCLUDE_SAME_INDEX if exclude_self else 0, stage, int(max_pairs)
    p.ws, p.ws_bytes, p.out_stats = L.ptr(ws), nbytes(ws), L.ptr(out_stats)
    p.count, p.index, p.sqdist = L.ptr(count), L.ptr(index), L.ptr(sqdist)
    L.call("ovg_radius_search", p, _stream())
    return out_stats, count, index, sqdist


def knn_search(query, reference, radius_sq, cell, ws, k, query_valid=None, reference_valid=None, origin=None, exclude_self=False,
               max_pairs=0, out_stats=None, count=None, index=None, sqdist=None):
    """ovg_knn_search on contiguous device tensors, with the arguments of radius_search's L.RS_SEARCH stage and 1 <= k <= L.KNN_MAX_K:
    ws must hold what radius_search(L.RS_BUILD, ...) left there for the same reference, radius_sq, cell and origin. Writes count int32
    [nq], index int32 [nq, k] and sqdist f32 [nq, k] (allocated when None): the k nearest references within the radius, nearest
    first, equal distances in ascending index, -1 / +inf from rank min(k, count) on -- or nothing at all when the candidate pairs
    exceed max_pairs or ws holds no grid, which out_stats (int64 [4], if given) then reports as L.RS_OVER_BUDGET / L.RS_NOT_BUILT.
    -> (out_stats, count, index, sqdist). Nothing is read back."""
    what = "knn_search"
    _chk_dev(query, reference, ws, query_valid, reference_valid, origin, out_stats, count, index, sqdist)
    nq, nr = _query_reference(what, query, reference, query_valid, reference_valid, exclude_self, origin, out_stats)
    k = int(k)
    if not 1 <= k <= L.KNN_MAX_K:
        raise L.OvgError("%s: k must be in [1, %d], got %d" % (what, L.KNN_MAX_K, k))
    count = _out(what, count, "count", _I32, (nq,), query.device, any_shape=True)
    index = _out(what, index, "index", _I32, (nq, k), query.device, any_shape=True)
    sqdist = _out(what, sqdist, "sqdist", _F32, (nq, k), query.device, any_shape=True)
    p = L.KnnParams()
    p.query, p.reference, p.query_valid, p.reference_valid = L.ptr(query), L.ptr(reference), L.ptr(query_valid), L.ptr(reference_valid)
    p.origin, p.nq, p.nr, p.radius_sq, p.cell = L.ptr(origin), nq, nr, float(radius_sq), float(cell)
    p.flags, p.k, p.max_pairs = L.RS_EXCLUDE_SAME_INDEX if exclude_self else 0, k, int(max_pairs)
    p.ws, p.ws_bytes, p.out_stats = L.ptr(ws), nbytes(ws), L.ptr(out_stats)
    p.count, p.index, p.sqdist = L.ptr(count), L.ptr(index), L.ptr(sqdist)
    L.call("ovg_knn_search", p, _stream())
    return out_stats, count, index, sqdist


def cluster(points, radius_sq, cell, ws, min_neighbours, valid=None, origin=None, max_pairs=0, out_stats=None, root=None, kind=None,
            degree=None):
    """ovg_cluster on contiguous device tensors: points f32 [n, 3], valid u8 [n] or None, origin f32 [3] or None; min_neighbours >= 0
    (0: plain Euclidean connected components). ws must hold what radius_search(L.RS_BUILD, points, points, ..., query_valid=valid,
    reference_valid=valid) left there for the same radius_sq, cell and origin. Writes root int32 [n] (the lowest index of the point's
    cluster, -1 for noise and unusable points), kind u8 [n] (L.CL_UNUSABLE / CL_NOISE / CL_BORDER / CL_CORE) and degree int32 [n]
    (the neighbours within the radius, the point itself not counted) -- allocated when None; degree=False: not written -- or nothing
    at all when the candidate pairs exceed max_pairs or ws holds no grid, which out_stats (int64 [4], if given) then reports as
    L.RS_OVER_BUDGET / L.RS_NOT_BUILT; L.CL_INTERNAL there means the union-find broke its own bounds (a bug: no result).
    -> (out_stats, root, kind, degree). Nothing is read back."""
    what = "cluster"
    _chk_dev(points, ws, valid, origin, out_stats, root, kind, None if isinstance(degree, bool) else degree)
    n = _points(what, points, "points")
    _int_in(what, "min_neighbours", min_neighbours, 0, 1 << 31)
    _tensor(what, valid, "valid", _U8, (n,), optional=True)
    _tensor(what, origin, "origin", _F32, numel=3, optional=True)
    _tensor(what, out_stats, "out_stats", _I64, numel=4, optional=True)
    root = _out(what, root, "root", _I32, (n,), points.device, any_shape=True)
    kind = _out(what, kind, "kind", _U8, (n,), points.device, any_shape=True)
    deg = None if degree is False else _out(what, None if degree is True else degree, "degree", _I32, (n,), points.device, any_shape=True)
    p = L.ClusterParams()
    p.points, p.valid, p.origin, p.n, p.radius_sq, p.cell = L.ptr(points), L.ptr(valid), L.ptr(origin), n, float(radius_sq), float(cell)
    p.min_neighbours, p.flags, p.max_pairs = min_neighbours, 0, int(max_pairs)
    p.ws, p.ws_bytes, p.out_stats = L.ptr(ws), nbytes(ws), L.ptr(out_stats)
    p.root, p.kind, p.degree = L.ptr(root), L.ptr(kind), L.ptr(deg)
    L.call("ovg_cluster", p, _stream())
    return out_stats, root, kind, deg


def knn_normals(query, reference, index, viewpoint=None, normal=None, curvature=None, covariance=None, used=None):
    """ovg_knn_normals on contiguous device tensors: query f32 [nq, 3], reference f32 [nr, 3], index int32 [nq, k] (a neighbour table
    as knn_search writes it), viewpoint None, f32 [3] (shared) or f32 [nq, 3] (one per query). -> (normal f32 [nq, 3], curvature,
    covariance, used): the unit normal of the plane through every row's neighbours (zeros where fewer than three), towards the
    viewpoint. curvature (f32 [nq]), covariance (f64 [nq, 6]: xx xy xz yy yz zz) and used (int32 [nq]: neighbours per row) are
    written when given as tensors or True (allocated), else returned as None. Nothing is read back."""
    what = "knn_normals"
    opt = lambda t: None if isinstance(t, bool) else t
    _chk_dev(query, reference, index, viewpoint, normal, opt(curvature), opt(covariance), opt(used))
    nq, nr = _points(what, query, "query"), _points(what, reference, "reference")
    _tensor(what, index, "index", _I32)
    if index.dim() != 2 or index.shape[0] != nq or index.shape[1] < 1:
        raise L.OvgError("%s: index must be [%d, k], k >= 1" % (what, nq))
    k = int(index.shape[1])
    if viewpoint is not None:
        _tensor(what, viewpoint, "viewpoint", _F32, (nq, 3) if isinstance(viewpoint, torch.Tensor) and viewpoint.dim() == 2 else (3,))
    stride = 3 if viewpoint is not None and viewpoint.dim() == 2 else 0
    outs = [_out(what, normal, "normal", _F32, (nq, 3), query.device)]
    for t, name, dt, shape in ((curvature, "curvature", _F32, (nq,)), (covariance, "covariance", _F64, (nq, 6)), (used, "used", _I32, (nq,))):
        outs.append(None if t is None or t is False else _out(what, opt(t), name, dt, shape, query.device))
    p = L.KnnNormalsParams()
    p.query, p.reference, p.index, p.viewpoint = L.ptr(query), L.ptr(reference), L.ptr(index), L.ptr(viewpoint)
    p.nq, p.nr, p.k, p.viewpoint_stride = nq, nr, k, stride
    p.normal, p.curvature, p.covariance, p.used = (L.ptr(t) for t in outs)
    L.call("ovg_knn_normals", p, _stream())
    return tuple(outs)


def align_workspace_bytes(n):
    return _ws_query("ovg_align_workspace_bytes", n=n)


def align_moments(source, target, index=None, source_valid=None, target_valid=None, sqdist=None, max_sqdist=None, centre=None, ws=None,
                  count=None, sums=None):
    """ovg_align_moments on contiguous device tensors: source f32 [n, 3], target f32 [m, 3], index int32 [n] or None (pair i <-> i, n == m),
    source_valid / target_valid u8 [n] / [m] or None, sqdist f32 [n] with the host float max_sqdist (both or neither: the inclusive gate),
    centre f64 [6] (cp, cq) or None. -> (count int64 [1], sums f64 [18]) (allocated when None): the number of used pairs and the float64
    sums of a, b, a b^T, |a|^2, |b|^2 and |q - p|^2 over them in the fixed order of include/omnivggt_hip.h, so two calls give identical
    bytes. ws: an optional uint8 device tensor of at least align_workspace_bytes(n) bytes. Nothing is read back."""
    what = "align_moments"
    n, m = _points(what, source, "source", 1), _points(what, target, "target", 1)
    _tensor(what, index, "index", _I32, (n,), optional=True)
    if index is None and n != m:
        raise L.OvgError("%s: without an index the pairs are i <-> i and need n == m (got %d, %d)" % (what, n, m))
    _tensor(what, source_valid, "source_valid", _U8, (n,), optional=True)
    _tensor(what, target_valid, "target_valid", _U8, (m,), optional=True)
    _tensor(what, sqdist, "sqdist", _F32, (n,), optional=True)
    if (sqdist is None) != (max_sqdist is None):
        raise L.OvgError("%s: the gate needs both sqdist and max_sqdist" % what)
    if max_sqdist is not None and not float(max_sqdist) == float(max_sqdist):
        raise L.OvgError("%s: max_sqdist must be a number, not NaN" % what)
    _tensor(what, centre, "centre", _F64, (6,), optional=True)
    _tensor(what, count, "count", _I64, (1,), optional=True)
    _tensor(what, sums, "sums", _F64, (L.ALIGN_SUMS,), optional=True)
    _tensor(what, ws, "ws", _U8, optional=True)
    _chk_dev(source, target, index, source_valid, target_valid, sqdist, centre, ws, count, sums)
    ws = _workspace(ws, align_workspace_bytes(n), source.device)
    count = _out(what, count, "count", _I64, (1,), source.device)
    sums = _out(what, sums, "sums", _F64, (L.ALIGN_SUMS,), source.device)
    p = L.AlignMomentsParams()
    p.source, p.target, p.index, p.source_valid, p.target_valid = L.ptr(source), L.ptr(target), L.ptr(index), L.ptr(source_valid), L.ptr(target_valid)
    p.sqdist, p.centre, p.n, p.m = L.ptr(sqdist), L.ptr(centre), n, m
    p.max_sqdist, p.flags = (0.0, 0) if sqdist is None else (float(max_sqdist), L.ALIGN_GATE)
    p.ws, p.ws_bytes, p.out_count, p.out_sums = L.ptr(ws), nbytes(ws), L.ptr(count), L.ptr(sums)
    L.call("ovg_align_moments", p, _stream())
    return count, sums


def align_solve(count, sums, transform, centre=None, with_scale=True, compose=False, scale=None, rms=None, out_count=None, status=None):
    """ovg_align_solve on device tensors: the moments (count int64 [1], sums f64 [18], and the centre f64 [6] they were computed with, or
    None) -> the least-squares similarity (with_scale) or rigid step q ~ s R p + t, written to transform f64 [4, 4], or multiplied onto
    it from the left with compose=True. scale f64 [1], rms f64 [1] (of the used pairs before the step), out_count int64 [1] and status
    int32 [1] (L.ALIGN_FEW_PAIRS | L.ALIGN_NO_SPREAD | L.ALIGN_NOT_FINITE: the step is then the identity) are written when given.
    -> transform. Nothing is read back."""
    what = "align_solve"
    _tensor(what, count, "count", _I64, (1,))
    _tensor(what, sums, "sums", _F64, (L.ALIGN_SUMS,))
    _tensor(what, transform, "transform", _F64, (4, 4))
    _tensor(what, centre, "centre", _F64, (6,), optional=True)
    _tensor(what, scale, "scale", _F64, (1,), optional=True)
    _tensor(what, rms, "rms", _F64, (1,), optional=True)
    _tensor(what, out_count, "out_count", _I64, (1,), optional=True)
    _tensor(what, status, "status", _I32, (1,), optional=True)
    _chk_dev(count, sums, transform, centre, scale, rms, out_count, status)
    p = L.AlignSolveParams()
    p.count, p.sums, p.centre, p.transform = L.ptr(count), L.ptr(sums), L.ptr(centre), L.ptr(transform)
    p.flags = (L.ALIGN_SCALE if with_scale else 0) | (L.ALIGN_COMPOSE if compose else 0)
    p.out_scale, p.out_rms, p.out_count, p.out_status = L.ptr(scale), L.ptr(rms), L.ptr(out_count), L.ptr(status)
    L.call("ovg_align_solve", p, _stream())
    return transform


def align_apply(points, transform, out=None):
    """ovg_align_apply on contiguous device tensors: points f32 [n, 3], transform f64 [4, 4] -> out f32 [n, 3] (allocated when None; may
    be `points` itself): out[i] = f32(T p[i]) with every coordinate ((T0 x + T1 y) + T2 z) + T3 in float64. Nothing is read back."""
    what = "align_apply"
    n = _points(what, points, "points", 1)
    _tensor(what, transform, "transform", _F64, (4, 4))
    _tensor(what, out, "out", _F32, (n, 3), optional=True)
    _chk_dev(points, transform, out)
    out = _out(what, out, "out", _F32, (n, 3), points.device)
    p = L.AlignApplyParams()
    p.points, p.transform, p.n, p.out = L.ptr(points), L.ptr(transform), n, L.ptr(out)
    L.call("ovg_align_apply", p, _stream())
    return out


def align_wmoments_workspace_bytes(n):
    return _ws_query("ovg_align_wmoments_workspace_bytes", n=n)


def align_wmoments(source, target, weight=None, source_valid=None, target_valid=None, transform=None, delta=None, delta_scale=1.0,
                   cauchy=False, centre=None, ws=None, count=None, sums=None):
    """ovg_align_wmoments on contiguous device tensors: source, target f32 [n, 3] (pair i <-> i), weight f32 [n] or None, source_valid /
    target_valid u8 [n] or None, transform f64 [4, 4] or None, centre f64 [6] or None. cauchy=True reweights every pair by
    1 / (1 + r^2 / delta^2), r its residual under `transform`, delta = delta_scale (a host float, not NaN) times the device scalar
    `delta` (f64 [1], or None: 1); a delta that is not finite and positive reweights nothing. -> (count int64 [1], sums f64 [20])
    (allocated when None): the used pairs and the weighted sums of include/omnivggt_hip.h in its fixed order, so two calls give
    identical bytes. ws: an optional uint8 device tensor of at least align_wmoments_workspace_bytes(n) bytes. Nothing is read back."""
    what = "align_wmoments"
    n = _points(what, source, "source", 1)
    _tensor(what, target, "target", _F32, (n, 3))
    _tensor(what, weight, "weight", _F32, (n,), optional=True)
    _tensor(what, source_valid, "source_valid", _U8, (n,), optional=True)
    _tensor(what, target_valid, "target_valid", _U8, (n,), optional=True)
    _tensor(what, transform, "transform", _F64, (4, 4), optional=True)
    _tensor(what, delta, "delta", _F64, (1,), optional=True)
    delta_scale = _number(what, "delta_scale", delta_scale, f32=False)
    _tensor(what, centre, "centre", _F64, (6,), optional=True)
    _tensor(what, count, "count", _I64, (1,), optional=True)
    _tensor(what, sums, "sums", _F64, (L.WALIGN_SUMS,), optional=True)
    _tensor(what, ws, "ws", _U8, optional=True)
    _chk_dev(source, target, weight, source_valid, target_valid, transform, delta, centre, ws, count, sums)
    ws = _workspace(ws, align_wmoments_workspace_bytes(n), source.device)
    count = _out(what, count, "count", _I64, (1,), source.device)
    sums = _out(what, sums, "sums", _F64, (L.WALIGN_SUMS,), source.device)
    p = L.AlignWMomentsParams()
    p.source, p.target, p.weight, p.source_valid, p.target_valid = L.ptr(source), L.ptr(target), L.ptr(weight), L.ptr(source_valid), L.ptr(target_valid)
    p.transform, p.delta, p.centre, p.delta_scale, p.n = L.ptr(transform), L.ptr(delta), L.ptr(centre), delta_scale, n
    p.flags = L.WALIGN_CAUCHY if cauchy else 0
    p.ws, p.ws_bytes, p.out_count, p.out_sums = L.ptr(ws), nbytes(ws), L.ptr(count), L.ptr(sums)
    L.call("ovg_align_wmoments", p, _stream())
    return count, sums


def align_wsolve(count, sums, transform, centre=None, with_scale=True, keep=False, scale=None, rms=None, fit_rms=None, weight=None,
                 out_count=None, status=None):
    """ovg_align_wsolve on device tensors: the weighted moments (count int64 [1], sums f64 [20], and the centre f64 [6] they were computed
    with, or None) -> the weighted least-squares similarity (with_scale) or rigid transform q ~ s R p + t, written to transform f64
    [4, 4]. keep=True: a degenerate solve leaves transform and scale as they are instead of writing the identity and 1. scale, rms
    (weighted, under the transform the weights came from), fit_rms (weighted, after this fit), weight (the weight sum), all f64 [1],
    out_count int64 [1] and status int32 [1] (the L.ALIGN_* bits) are written when given. -> transform. Nothing is read back."""
    what = "align_wsolve"
    _tensor(what, count, "count", _I64, (1,))
    _tensor(what, sums, "sums", _F64, (L.WALIGN_SUMS,))
    _tensor(what, transform, "transform", _F64, (4, 4))
    _tensor(what, centre, "centre", _F64, (6,), optional=True)
    for t, name in ((scale, "scale"), (rms, "rms"), (fit_rms, "fit_rms"), (weight, "weight")):
        _tensor(what, t, name, _F64, (1,), optional=True)
    _tensor(what, out_count, "out_count", _I64, (1,), optional=True)
    _tensor(what, status, "status", _I32, (1,), optional=True)
    _chk_dev(count, sums, transform, centre, scale, rms, fit_rms, weight, out_count, status)
    p = L.AlignWSolveParams()
    p.count, p.sums, p.centre, p.transform = L.ptr(count), L.ptr(sums), L.ptr(centre), L.ptr(transform)
    p.flags = (L.ALIGN_SCALE if with_scale else 0) | (L.WALIGN_KEEP if keep else 0)
    p.out_scale, p.out_rms, p.out_fit_rms, p.out_weight = L.ptr(scale), L.ptr(rms), L.ptr(fit_rms), L.ptr(weight)
    p.out_count, p.out_status = L.ptr(out_count), L.ptr(status)
    L.call("ovg_align_wsolve", p, _stream())
    return transform


def align_move_maps(n, transform=None, scale=None, points=None, depth=None, points_conf=None, depth_conf=None, out_points=None,
                    out_depth=None, out_points_conf=None, out_depth_conf=None):
    """ovg_align_move_maps on contiguous device tensors of n pixels (any shape with that many elements: [n], [V, H, W], [V, H, W, 1];
    points 3 n), every map optional (at least one): points f32 -> out_points = f32(transform p) as align_apply (transform f64
    [4, 4]); depth f32 -> out_depth = f32(depth * scale) (scale f64 [1] on the device); points_conf / depth_conf f32 are copied.
    Outputs are allocated in the input's shape when None and may be their own inputs.
    -> (out_points, out_depth, out_points_conf, out_depth_conf), None for an absent map. Nothing is read back."""
    what = "align_move_maps"
    n = _int_in(what, "n", n, 1, 1 << 31)
    maps = ((points, out_points, "points", (n, 3)), (depth, out_depth, "depth", (n,)), (points_conf, out_points_conf, "points_conf", (n,)),
            (depth_conf, out_depth_conf, "depth_conf", (n,)))
    if all(m[0] is None for m in maps):
        raise L.OvgError("%s: at least one of points, depth, points_conf, depth_conf is needed" % what)
    for t, o, name, shape in maps:                                           # maps come as [V, H, W(, 3)] or flat: the element count is the rule
        _tensor(what, t, name, _F32, numel=math.prod(shape), optional=True)
        _tensor(what, o, "out_" + name, _F32, numel=math.prod(shape), optional=True)
        if t is None and o is not None:
            raise L.OvgError("%s: out_%s without %s" % (what, name, name))
    _tensor(what, transform, "transform", _F64, (4, 4), optional=points is None)
    _tensor(what, scale, "scale", _F64, (1,), optional=depth is None)
    _chk_dev(transform, scale, *(t for m in maps for t in m[:2]))
    dev = next(m[0] for m in maps if m[0] is not None).device
    outs = [None if t is None else _out(what, o, "out_" + name, _F32, tuple(t.shape), dev) for t, o, name, shape in maps]
    p = L.AlignMoveMapsParams()
    p.points, p.depth, p.points_conf, p.depth_conf = L.ptr(points), L.ptr(depth), L.ptr(points_conf), L.ptr(depth_conf)
    p.transform, p.scale, p.n = L.ptr(transform), L.ptr(scale), n
    p.out_points, p.out_depth, p.out_points_conf, p.out_depth_conf = (L.ptr(o) for o in outs)
    L.call("ovg_align_move_maps", p, _stream())
    return tuple(outs)


def align_move_cameras(extrinsic, transform, scale, out=None):
    """ovg_align_move_cameras on contiguous device tensors: extrinsic f32 [V, 3, 4] (world-to-camera in the frame the points were in),
    transform f64 [4, 4] = [s R, t] that moved the points, scale f64 [1] = s -> out f32 [V, 3, 4] (allocated when None; may be
    `extrinsic` itself): the cameras that see the moved points at s times the old depth. Nothing is read back."""
    what = "align_move_cameras"
    _tensor(what, extrinsic, "extrinsic", _F32)
    if extrinsic.dim() != 3 or tuple(extrinsic.shape[1:]) != (3, 4) or not 1 <= extrinsic.shape[0] < 1 << 31:
        raise L.OvgError("%s: extrinsic must be a contiguous float32 tensor [V, 3, 4], V >= 1" % what)
    V = int(extrinsic.shape[0])
    _tensor(what, transform, "transform", _F64, (4, 4))
    _tensor(what, scale, "scale", _F64, (1,))
    _tensor(what, out, "out", _F32, (V, 3, 4), optional=True)
    _chk_dev(extrinsic, transform, scale, out)
    out = _out(what, out, "out", _F32, (V, 3, 4), extrinsic.device)
    p = L.AlignMoveCamerasParams()
    p.extrinsic, p.transform, p.scale, p.views, p.out = L.ptr(extrinsic), L.ptr(transform), L.ptr(scale), V, L.ptr(out)
    L.call("ovg_align_move_cameras", p, _stream())
    return out


def deptheval_median_workspace_bytes(groups, n):
    return _ws_query("ovg_deptheval_median_workspace_bytes", groups=groups, n=n)


def deptheval_sums_workspace_bytes(groups, n):
    return _ws_query("ovg_deptheval_sums_workspace_bytes", groups=groups, n=n)


def _deptheval_maps(what, pred, gt, valid, min_depth, max_depth):
    """-> (G, n, stride) of the f32 [G, n] maps (rows contiguous, one row stride shared by pred, gt and valid)."""
    for t, name in ((pred, "pred"), (gt, "gt")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1:
            raise L.OvgError("%s: %s must be an f32 tensor [G, n] with contiguous rows, G >= 1, n >= 1" % (what, name))
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or valid.dim() != 2 or valid.stride(1) != 1):
        raise L.OvgError("%s: valid must be a uint8 tensor [G, n] with contiguous rows" % what)
    G, n = int(pred.shape[0]), int(pred.shape[1])
    stride = int(pred.stride(0)) if G > 1 else n
    for t, name in ((gt, "gt"), (valid, "valid")):
        if t is not None and (tuple(t.shape) != (G, n) or (G > 1 and int(t.stride(0)) != stride)):
            raise L.OvgError("%s: %s must be shaped %r with the row stride of pred (%d)" % (what, name, (G, n), stride))
    if G > L.DEPTHEVAL_MAX_GROUPS or G * n >= (1 << 31) or stride < n:
        raise L.OvgError("%s: the maps must be at most %d groups, fewer than 2^31 pixels, row stride >= n" % (what, L.DEPTHEVAL_MAX_GROUPS))
    _number(what, "min_depth", min_depth, lo=0, f32=False)
    _number(what, "max_depth", max_depth, f32=False)
    return G, n, stride


def deptheval_median(pred, gt, valid=None, min_depth=0.0, max_depth=float("inf"), ws=None, count=None, median=None):
    """ovg_deptheval_median on device tensors: pred, gt f32 [G, n] (rows contiguous, one shared row stride), valid u8 [G, n] or None.
    -> (count int64 [G], median f32 [G, 2, 2]) (allocated when None): per group the number of used pixels and, for pred ([g, 0]) and
    gt ([g, 1]), the lower and upper middle order statistics over them -- a function of the multiset of used values alone. ws: an
    optional uint8 device tensor of at least deptheval_median_workspace_bytes(G, n) bytes (the call zeroes it). Nothing is read back."""
    what = "deptheval_median"
    G, n, stride = _deptheval_maps(what, pred, gt, valid, min_depth, max_depth)
    _tensor(what, count, "count", _I64, (G,), optional=True)
    _tensor(what, median, "median", _F32, (G, 2, 2), optional=True)
    _tensor(what, ws, "ws", _U8, optional=True)
    _chk_dev(pred, gt, valid, ws, count, median)
    ws = _workspace(ws, deptheval_median_workspace_bytes(G, n), pred.device)
    count = _out(what, count, "count", _I64, (G,), pred.device)
    median = _out(what, median, "median", _F32, (G, 2, 2), pred.device)
    p = L.DepthEvalMedianParams()
    p.pred, p.gt, p.valid, p.groups, p.n, p.stride = L.ptr(pred), L.ptr(gt), L.ptr(valid), G, n, stride
    p.min_depth, p.max_depth = float(min_depth), float(max_depth)
    p.ws, p.ws_bytes, p.out_count, p.out_median = L.ptr(ws), nbytes(ws), L.ptr(count), L.ptr(median)
    L.call("ovg_deptheval_median", p, _stream())
    return count, median


def deptheval_sums(pred, gt, valid=None, min_depth=0.0, max_depth=float("inf"), coeff=None, clip_min=1e-3, clip_max=float("inf"), ws=None,
                   counts=None, sums=None):
    """ovg_deptheval_sums on device tensors shaped as for deptheval_median. coeff None: the MOMENTS of a fit (sums of p, g, p p, p g,
    g g); coeff f64 [G, 2] = (s, t): the METRICS terms of q = clip(s p + t) against g (|e| / g, e e / g, e e, |e|, (log q - log g)^2)
    and the delta counts. -> (counts int64 [G, 4], sums f64 [G, 5]) (allocated when None): counts[:, 0] the used pixels, [:, 1:] those
    with max(q / g, g / q) < 1.25, 1.25^2, 1.25^3 (0 for the moments); the sums in the fixed order of include/omnivggt_hip.h, so two
    calls give identical bytes. ws: optional, at least deptheval_sums_workspace_bytes(G, n) bytes. Nothing is read back."""
    what = "deptheval_sums"
    G, n, stride = _deptheval_maps(what, pred, gt, valid, min_depth, max_depth)
    _tensor(what, coeff, "coeff", _F64, (G, 2), optional=True)
    _tensor(what, counts, "counts", _I64, (G, L.DEPTHEVAL_COUNTS), optional=True)
    _tensor(what, sums, "sums", _F64, (G, L.DEPTHEVAL_SUMS), optional=True)
    if coeff is not None:
        _number(what, "clip_min", clip_min, f32=False)
        _number(what, "clip_max", clip_max, f32=False)
        if not 0 < clip_min < float("inf") or clip_max < clip_min:
            raise L.OvgError("%s: clip_min must be positive and finite, clip_max >= clip_min" % what)
    _tensor(what, ws, "ws", _U8, optional=True)
    _chk_dev(pred, gt, valid, coeff, ws, counts, sums)
    ws = _workspace(ws, deptheval_sums_workspace_bytes(G, n), pred.device)
    counts = _out(what, counts, "counts", _I64, (G, L.DEPTHEVAL_COUNTS), pred.device)
    sums = _out(what, sums, "sums", _F64, (G, L.DEPTHEVAL_SUMS), pred.device)
    p = L.DepthEvalSumsParams()
    p.pred, p.gt, p.valid, p.groups, p.n, p.stride = L.ptr(pred), L.ptr(gt), L.ptr(valid), G, n, stride
    p.min_depth, p.max_depth = float(min_depth), float(max_depth)
    p.mode, p.coeff = (L.DEPTHEVAL_MOMENTS, None) if coeff is None else (L.DEPTHEVAL_METRICS, L.ptr(coeff))
    p.clip_min, p.clip_max = (0.0, 0.0) if coeff is None else (float(clip_min), float(clip_max))
    p.ws, p.ws_bytes, p.out_counts, p.out_sums = L.ptr(ws), nbytes(ws), L.ptr(counts), L.ptr(sums)
    L.call("ovg_deptheval_sums", p, _stream())
    return counts, sums


def deptheval_solve(mode, count, sums=None, median=None, coeff=None, status=None):
    """ovg_deptheval_solve on device tensors: mode L.DEPTHEVAL_NONE / MEDIAN / SCALE / SCALE_SHIFT; count int64 [G] (deptheval_median's)
    or [G, 4] (deptheval_sums': column 0 is read); sums f64 [G, 5] (the moments: SCALE, SCALE_SHIFT), median f32 [G, 2, 2] (MEDIAN).
    -> (coeff f64 [G, 2] = (s, t) with gt ~ s pred + t, status int32 [G]) (allocated when None). A degenerate group gets (1, 0) and
    L.DEPTHEVAL_FEW / NOT_FINITE / NO_SPREAD / BAD_FIT in its status. Nothing is read back."""
    what = "deptheval_solve"
    if isinstance(mode, bool) or mode not in (L.DEPTHEVAL_NONE, L.DEPTHEVAL_MEDIAN, L.DEPTHEVAL_SCALE, L.DEPTHEVAL_SCALE_SHIFT):
        raise L.OvgError("%s: mode must be one of L.DEPTHEVAL_NONE / MEDIAN / SCALE / SCALE_SHIFT, got %r" % (what, mode))
    _tensor(what, count, "count", _I64)
    if count.dim() not in (1, 2) or not 1 <= count.shape[0] <= L.DEPTHEVAL_MAX_GROUPS or (count.dim() == 2 and count.shape[1] != L.DEPTHEVAL_COUNTS):
        raise L.OvgError("%s: count must be [G] or [G, %d], 1 <= G <= %d" % (what, L.DEPTHEVAL_COUNTS, L.DEPTHEVAL_MAX_GROUPS))
    G = int(count.shape[0])
    _tensor(what, sums, "sums", _F64, (G, L.DEPTHEVAL_SUMS), optional=mode not in (L.DEPTHEVAL_SCALE, L.DEPTHEVAL_SCALE_SHIFT))
    _tensor(what, median, "median", _F32, (G, 2, 2), optional=mode != L.DEPTHEVAL_MEDIAN)
    _tensor(what, coeff, "coeff", _F64, (G, 2), optional=True)
    _tensor(what, status, "status", _I32, (G,), optional=True)
    _chk_dev(count, sums, median, coeff, status)
    coeff = _out(what, coeff, "coeff", _F64, (G, 2), count.device)
    status = _out(what, status, "status", _I32, (G,), count.device)
    p = L.DepthEvalSolveParams()
    p.count, p.count_stride, p.sums, p.median = L.ptr(count), 1 if count.dim() == 1 else L.DEPTHEVAL_COUNTS, L.ptr(sums), L.ptr(median)
    p.groups, p.mode, p.coeff, p.status = G, int(mode), L.ptr(coeff), L.ptr(status)
    L.call("ovg_deptheval_solve", p, _stream())
    return coeff, status


def plane_hypotheses(points, hypotheses, seed=0, valid=None, candidates=None, axis=None, min_abs_cos=0.0, planes=None, index=None):
    """ovg_plane_hypotheses on contiguous device tensors: points f32 [n, 3], valid u8 [n] or None, candidates int32 [m] or None (draw
    from all n points), axis f32 [3] or None (a unit vector: used as given) with min_abs_cos in [0, 1]; hypotheses = H, seed in
    [0, 2^64). -> (planes f32 [H, 4], index int32 [H, 3]) (allocated when None): hypothesis h through the three points its seeded
    draws name, four NaNs where the rule of include/omnivggt_hip.h voids it; index holds the draws either way. Nothing is read back."""
    what = "plane_hypotheses"
    n = _points(what, points, "points", 1, 1 << 31)
    _int_in(what, "hypotheses", hypotheses, 1, 1 << 31)
    _int_in(what, "seed", seed, 0, 1 << 64)
    _tensor(what, valid, "valid", _U8, (n,), optional=True)
    _tensor(what, candidates, "candidates", _I32, optional=True)
    if candidates is not None and (candidates.dim() != 1 or not 1 <= candidates.shape[0] < 1 << 31):
        raise L.OvgError("%s: candidates must be [m], 1 <= m < 2^31" % what)
    _tensor(what, axis, "axis", _F32, (3,), optional=True)
    _number(what, "min_abs_cos", min_abs_cos, lo=0.0, hi=1.0)
    if axis is None and min_abs_cos != 0:
        raise L.OvgError("%s: min_abs_cos needs an axis" % what)
    _chk_dev(points, valid, candidates, axis, planes, index)
    planes = _out(what, planes, "planes", _F32, (hypotheses, 4), points.device)
    index = _out(what, index, "index", _I32, (hypotheses, 3), points.device)
    p = L.PlaneHypothesesParams()
    p.points, p.valid, p.candidates, p.axis = L.ptr(points), L.ptr(valid), L.ptr(candidates), L.ptr(axis)
    p.n, p.m, p.H, p.seed = n, n if candidates is None else int(candidates.shape[0]), hypotheses, seed
    p.min_abs_cos, p.pad, p.planes, p.index = float(min_abs_cos), 0, L.ptr(planes), L.ptr(index)
    L.call("ovg_plane_hypotheses", p, _stream())
    return planes, index


def plane_score(points, planes, threshold, valid=None, splits=0, count=None):
    """ovg_plane_score on contiguous device tensors: points f32 [n, 3], planes f32 [H, 4], valid u8 [n] or None, threshold a host float
    (finite, >= 0; used as float32). -> count int32 [H] (allocated when None): the points with |((nx x + ny y) + nz z) + w| <= threshold
    per plane, usable points only; a void (NaN) plane counts 0. splits: 0 lets the entry choose, otherwise the number of point splits
    of its grid -- the bytes are the same for every value. Nothing is read back."""
    what = "plane_score"
    n = _points(what, points, "points", 1, 1 << 31)
    H = _table(what, planes, "planes", _F32, 4, 1, 1 << 31)
    threshold = _number(what, "threshold", threshold, lo=0)
    _tensor(what, valid, "valid", _U8, (n,), optional=True)
    _int_in(what, "splits", splits, 0, 1 << 31)
    _chk_dev(points, planes, valid, count)
    count = _out(what, count, "count", _I32, (H,), points.device)
    p = L.PlaneScoreParams()
    p.points, p.valid, p.planes, p.n, p.H = L.ptr(points), L.ptr(valid), L.ptr(planes), n, H
    p.threshold, p.splits, p.count = threshold, splits, L.ptr(count)
    L.call("ovg_plane_score", p, _stream())
    return count


def plane_select(count, planes, min_inliers=3, best=None, plane=None, best_count=None, status=None):
    """ovg_plane_select on device tensors: count int32 [H], planes f32 [H, 4] -> (best int32 [1], plane f32 [4], best_count int32 [1],
    status int32 [1]) (allocated when None): the hypothesis with the most inliers, ties to the lowest index, or -1 / four zeros /
    L.PLANE_NONE when that count is below min_inliers (>= 3). Nothing is read back."""
    what = "plane_select"
    _tensor(what, count, "count", _I32)
    if count.dim() != 1 or not 1 <= count.shape[0] < 1 << 31:
        raise L.OvgError("%s: count must be [H], 1 <= H < 2^31" % what)
    H = int(count.shape[0])
    _tensor(what, planes, "planes", _F32, (H, 4))
    _int_in(what, "min_inliers", min_inliers, 3, 1 << 31)
    _chk_dev(count, planes, best, plane, best_count, status)
    dev = count.device
    best = _out(what, best, "best", _I32, (1,), dev)
    plane = _out(what, plane, "plane", _F32, (4,), dev)
    best_count = _out(what, best_count, "best_count", _I32, (1,), dev)
    status = _out(what, status, "status", _I32, (1,), dev)
    p = L.PlaneSelectParams()
    p.count, p.planes, p.H, p.min_inliers, p.pad = L.ptr(count), L.ptr(planes), H, min_inliers, 0
    p.best, p.plane, p.best_count, p.status = L.ptr(best), L.ptr(plane), L.ptr(best_count), L.ptr(status)
    L.call("ovg_plane_select", p, _stream())
    return best, plane, best_count, status


def plane_mask(points, plane, threshold, valid=None, gate=None, inlier=None, distance=None, out_count=None):
    """ovg_plane_mask on contiguous device tensors: points f32 [n, 3], plane f32 [4] (read on the device), valid u8 [n] or None, gate
    int32 [1] or None (a status: with L.PLANE_NONE in it nothing is an inlier). -> (inlier u8 [n], distance, out_count int64 [1]):
    the inlier mask of the plane at the threshold, the signed residual f32 [n] (NaN for unusable points) when distance is a tensor or
    True (allocated), else None, and the number of inliers. Nothing is read back."""
    what = "plane_mask"
    n = _points(what, points, "points", 1, 1 << 31)
    _tensor(what, plane, "plane", _F32, (4,))
    threshold = _number(what, "threshold", threshold, lo=0)
    _tensor(what, valid, "valid", _U8, (n,), optional=True)
    _tensor(what, gate, "gate", _I32, (1,), optional=True)
    _chk_dev(points, plane, valid, gate, inlier, None if isinstance(distance, bool) else distance, out_count)
    inlier = _out(what, inlier, "inlier", _U8, (n,), points.device)
    dist = None if distance is None or distance is False else \
        _out(what, None if distance is True else distance, "distance", _F32, (n,), points.device)
    out_count = _out(what, out_count, "out_count", _I64, (1,), points.device)
    p = L.PlaneMaskParams()
    p.points, p.valid, p.plane, p.gate, p.n = L.ptr(points), L.ptr(valid), L.ptr(plane), L.ptr(gate), n
    p.threshold, p.pad, p.inlier, p.distance, p.out_count = threshold, 0, L.ptr(inlier), L.ptr(dist), L.ptr(out_count)
    L.call("ovg_plane_mask", p, _stream())
    return inlier, dist, out_count


def plane_fit(count, sums, plane, centre=None, axis=None, rms=None, eigen=None, status=None):
    """ovg_plane_fit on device tensors: the moments of the inliers (count int64 [1], sums f64 [18] and the centre f64 [6] they were
    computed with, or None: align_moments with source == target == the points and source_valid = the inlier mask) -> the
    least-squares plane through them, written over plane f32 [4]; axis f32 [3] or None orients it. A degenerate step (fewer than three
    inliers, collinear inliers, non-finite sums) leaves the plane as it was. rms f64 [1], eigen f64 [3] (ascending) and status int32 [1]
    (L.PLANE_FEW | L.PLANE_NO_SPREAD | L.PLANE_NOT_FINITE) are written when given. -> plane. Nothing is read back."""
    what = "plane_fit"
    _tensor(what, count, "count", _I64, (1,))
    _tensor(what, sums, "sums", _F64, (L.ALIGN_SUMS,))
    _tensor(what, plane, "plane", _F32, (4,))
    _tensor(what, centre, "centre", _F64, (6,), optional=True)
    _tensor(what, axis, "axis", _F32, (3,), optional=True)
    _tensor(what, rms, "rms", _F64, (1,), optional=True)
    _tensor(what, eigen, "eigen", _F64, (3,), optional=True)
    _tensor(what, status, "status", _I32, (1,), optional=True)
    _chk_dev(count, sums, plane, centre, axis, rms, eigen, status)
    p = L.PlaneFitParams()
    p.count, p.sums, p.centre, p.axis, p.plane = L.ptr(count), L.ptr(sums), L.ptr(centre), L.ptr(axis), L.ptr(plane)
    p.out_rms, p.out_eigen, p.status = L.ptr(rms), L.ptr(eigen), L.ptr(status)
    L.call("ovg_plane_fit", p, _stream())
    return plane


def _map_shape(what, t, name, trailing=()):
    """t must be a tensor [S, H, W] + trailing with 1 <= S H W < 2^31 -> (S, H, W)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 + len(trailing) or tuple(t.shape[3:]) != tuple(trailing) or 0 in t.shape or \
            t.numel() // max(1, math.prod(trailing)) >= 1 << 31:
        raise L.OvgError("%s: %s must be a tensor [S, H, W%s], 1 <= S H W < 2^31" % (what, name, "".join(", %d" % v for v in trailing)))
    return tuple(int(v) for v in t.shape[:3])


def _tsdf_volume(what, tsdf, weight, color, origin):
    """The volume and its origin as the two TSDF entries take them -> (nx, ny, nz, origin as three floats)."""
    nz, ny, nx = _map_shape(what, tsdf, "tsdf")
    _tensor(what, tsdf, "tsdf", _F32, (nz, ny, nx))
    _tensor(what, weight, "weight", _F32, (nz, ny, nx))
    _tensor(what, color, "color", _F32, (nz, ny, nx, 4), optional=True)
    try:
        origin = [float(v) for v in origin]
    except (TypeError, ValueError):
        origin = []
    if len(origin) != 3 or not all(abs(v) <= _F32_MAX for v in origin):
        raise L.OvgError("%s: origin must be three finite float32 numbers" % what)
    return nx, ny, nz, origin


def tsdf_integrate(tsdf, weight, depth, cams, origin, voxel, trunc, max_weight=64.0, near=1e-3, color=None, valid=None, obs_weight=None,
                   colors=None, view_first=0, view_count=None, tile=L.TSDF_TILE_DEFAULT):
    """ovg_tsdf_integrate on contiguous device tensors, in place: tsdf, weight f32 [nz, ny, nx] and color f32 [nz, ny, nx, 4] or None
    (the volume; fresh: tsdf 1, the rest 0), depth f32 [S, H, W] z-depth, cams f32 [S, 16] (packed as for render_points), valid u8
    [S, H, W], obs_weight f32 [S, H, W] and colors u8 [S, H, W, 3] or None; origin three host floats, voxel / trunc / max_weight / near
    host floats (positive, finite; used as float32). The views view_first .. view_first + view_count - 1 (all S by default) are
    averaged into every lattice point in ascending order by the rule of include/omnivggt_hip.h; a range and then the rest give the
    bytes of one call. tile: L.TSDF_TILE_*, speed only. -> (tsdf, weight, color). Nothing is read back."""
    what = "tsdf_integrate"
    nx, ny, nz, origin = _tsdf_volume(what, tsdf, weight, color, origin)
    S, H, W = _map_shape(what, depth, "depth")
    _tensor(what, depth, "depth", _F32, (S, H, W))
    _tensor(what, cams, "cams", _F32, (S, 16))
    _tensor(what, valid, "valid", _U8, (S, H, W), optional=True)
    _tensor(what, obs_weight, "obs_weight", _F32, (S, H, W), optional=True)
    _tensor(what, colors, "colors", _U8, (S, H, W, 3), optional=True)
    if colors is not None and color is None:
        raise L.OvgError("%s: colors need a colour volume" % what)
    voxel, trunc = _number(what, "voxel", voxel, lo=0, strict=True), _number(what, "trunc", trunc, lo=0, strict=True)
    max_weight, near = _number(what, "max_weight", max_weight, lo=0, strict=True), _number(what, "near", near, lo=0, strict=True)
    _int_in(what, "view_first", view_first, 0, S)
    n = _int_in(what, "view_count", S - view_first if view_count is None else view_count, 1, S - view_first + 1)
    _int_in(what, "tile", tile, L.TSDF_TILE_DEFAULT, L.TSDF_TILE_32x8x1 + 1)
    _chk_dev(tsdf, weight, color, depth, cams, valid, obs_weight, colors)
    p = L.TsdfIntegrateParams()
    p.tsdf, p.weight, p.color, p.nx, p.ny, p.nz = L.ptr(tsdf), L.ptr(weight), L.ptr(color), nx, ny, nz
    for k in range(3):
        p.origin[k] = origin[k]
    p.voxel, p.trunc, p.max_weight, p.near = voxel, trunc, max_weight, near
    p.depth, p.cams, p.valid, p.obs_weight, p.colors = L.ptr(depth), L.ptr(cams), L.ptr(valid), L.ptr(obs_weight), L.ptr(colors)
    p.S, p.H, p.W, p.view_first, p.view_count, p.tile = S, H, W, view_first, n, tile
    L.call("ovg_tsdf_integrate", p, _stream())
    return tsdf, weight, color


def tsdf_extract_workspace_bytes(nx, ny, nz):
    return _ws_query("ovg_tsdf_extract_workspace_bytes", nx=nx, ny=ny, nz=nz)


def tsdf_extract(stage, tsdf, weight, origin, voxel, ws, min_weight=1.0, color=None, out_count=None, vertex_capacity=0, quad_capacity=0,
                 vertices=None, normals=None, colors=None, faces=None):
    """ovg_tsdf_extract on contiguous device tensors: the volume as for tsdf_integrate; ws a uint8 tensor of at least
    tsdf_extract_workspace_bytes(nx, ny, nz) bytes. stage L.TSDF_COUNT writes (vertices M, quads Q) to the two int64 of out_count;
    L.TSDF_SCATTER writes the first vertex_capacity vertices to vertices / normals f32 [., 3] and colors u8 [., 3] and the first
    quad_capacity quads to faces int32 [2 ., 3] (two triangles each) from what the COUNT stage left in ws."""
    what = "tsdf_extract"
    nx, ny, nz, origin = _tsdf_volume(what, tsdf, weight, color, origin)
    voxel, min_weight = _number(what, "voxel", voxel, lo=0, strict=True), _number(what, "min_weight", min_weight, lo=0, strict=True)
    if stage not in (L.TSDF_COUNT, L.TSDF_SCATTER, L.TSDF_COUNT | L.TSDF_SCATTER):
        raise L.OvgError("%s: unknown stage %r" % (what, stage))
    _int_in(what, "vertex_capacity", vertex_capacity, 0, 1 << 62)
    _int_in(what, "quad_capacity", quad_capacity, 0, 1 << 62)
    _tensor(what, ws, "ws", _U8)
    if stage & L.TSDF_SCATTER:
        _capacity_buffers(what, ((vertices, "vertices", _F32, 3 * vertex_capacity, True), (normals, "normals", _F32, 3 * vertex_capacity, True),
                                 (colors, "colors", _U8, 3 * vertex_capacity, True), (faces, "faces", _I32, 6 * quad_capacity, True)))
    _tensor(what, out_count, "out_count", _I64, min_numel=2)
    _chk_dev(tsdf, weight, color, ws, out_count, vertices, normals, colors, faces)
    p = L.TsdfExtractParams()
    p.tsdf, p.weight, p.color, p.nx, p.ny, p.nz = L.ptr(tsdf), L.ptr(weight), L.ptr(color), nx, ny, nz
    for k in range(3):
        p.origin[k] = origin[k]
    p.voxel, p.min_weight, p.stage, p.pad = voxel, min_weight, int(stage), 0
    p.vertex_capacity, p.quad_capacity = vertex_capacity, quad_capacity
    p.vertices, p.normals, p.colors, p.faces, p.out_count = L.ptr(vertices), L.ptr(normals), L.ptr(colors), L.ptr(faces), L.ptr(out_count)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_tsdf_extract", p, _stream())


# ---------------------------------------------------------------------------------------------------------------------------------
# image-space map geometry (ovg_map_depth, ovg_map_normals, ovg_map_edges, ovg_map_triangulate)
# ---------------------------------------------------------------------------------------------------------------------------------
def map_depth(points=None, cams=None, depth=None, valid=None, near=1e-3, out=None):
    """ovg_map_depth on contiguous device tensors: exactly one of points f32 [S, H, W, 3] with cams f32 [S, 16] (packed as for
    render_points) or depth f32 [S, H, W]; valid u8 [S, H, W] or None. -> z f32 [S, H, W] (`out`, or allocated here): the camera depth
    of a usable pixel (valid, finite, > near), NaN otherwise. Nothing is read back."""
    what = "map_depth"
    if (points is None) == (depth is None):
        raise L.OvgError("%s: exactly one of points / depth" % what)
    if points is not None:
        S, H, W = _map_shape(what, points, "points", (3,))
        _tensor(what, points, "points", _F32, (S, H, W, 3))
        _tensor(what, cams, "cams", _F32, (S, 16))
    else:
        S, H, W = _map_shape(what, depth, "depth")
        _tensor(what, depth, "depth", _F32, (S, H, W))
    _tensor(what, valid, "valid", _U8, (S, H, W), optional=True)
    near = _number(what, "near", near, lo=0, strict=True)
    src = points if points is not None else depth
    out = _out(what, out, "out", _F32, (S, H, W), src.device)
    _chk_dev(points, cams, depth, valid, out)
    p = L.MapDepthParams()
    p.points, p.cams, p.depth, p.valid = L.ptr(points), L.ptr(cams) if points is not None else None, L.ptr(depth), L.ptr(valid)
    p.S, p.H, p.W, p.near, p.z = S, H, W, near, L.ptr(out)
    L.call("ovg_map_depth", p, _stream())
    return out


def map_normals(points, z, rel_tol=0.03, out=None):
    """ovg_map_normals on contiguous device tensors: points f32 [S, H, W, 3], z f32 [S, H, W] (map_depth's). -> normals f32
    [S, H, W, 3] (`out`, or allocated here), unit vectors towards the camera, (0, 0, 0) where the rule gives none."""
    what = "map_normals"
    S, H, W = _map_shape(what, points, "points", (3,))
    _tensor(what, points, "points", _F32, (S, H, W, 3))
    _tensor(what, z, "z", _F32, (S, H, W))
    rel_tol = _number(what, "rel_tol", rel_tol, lo=0, f32=False)             # +inf switches the test off
    out = _out(what, out, "out", _F32, (S, H, W, 3), points.device)
    _chk_dev(points, z, out)
    p = L.MapNormalsParams()
    p.points, p.z, p.S, p.H, p.W, p.rel_tol, p.normals = L.ptr(points), L.ptr(z), S, H, W, rel_tol, L.ptr(out)
    L.call("ovg_map_normals", p, _stream())
    return out


def map_edges(z, normals=None, radius=1, rel_tol=0.03, min_cos=float("-inf"), tile=L.MAP_TILE_DEFAULT, out=None):
    """ovg_map_edges on contiguous device tensors: z f32 [S, H, W], normals f32 [S, H, W, 3] or None; radius 1, 2 or 3; min_cos a
    float32 value (not NaN). -> flags u8 [S, H, W] (`out`, or allocated here), bits L.MAP_UNUSABLE / MAP_DEPTH_EDGE /
    MAP_NORMAL_EDGE / MAP_NO_NORMAL. tile: L.MAP_TILE_*, speed only."""
    what = "map_edges"
    S, H, W = _map_shape(what, z, "z")
    _tensor(what, z, "z", _F32, (S, H, W))
    _tensor(what, normals, "normals", _F32, (S, H, W, 3), optional=True)
    _int_in(what, "radius", radius, 1, L.MAP_MAX_RADIUS + 1)
    rel_tol = _number(what, "rel_tol", rel_tol, lo=0, f32=False)             # +inf switches the test off
    min_cos = _number(what, "min_cos", min_cos, f32=False)
    _int_in(what, "tile", tile, L.MAP_TILE_DEFAULT, L.MAP_TILE_64x4 + 1)
    out = _out(what, out, "out", _U8, (S, H, W), z.device)
    _chk_dev(z, normals, out)
    p = L.MapEdgesParams()
    p.z, p.normals, p.S, p.H, p.W, p.radius = L.ptr(z), L.ptr(normals), S, H, W, radius
    p.rel_tol, p.min_cos, p.tile, p.pad, p.flags = rel_tol, min_cos, tile, 0, L.ptr(out)
    L.call("ovg_map_edges", p, _stream())
    return out


def map_triangulate_workspace_bytes(S, H, W):
    return _ws_query("ovg_map_triangulate_workspace_bytes", S=S, H=H, W=W)


def map_triangulate(stage, z, points, ws, rel_tol=0.03, keep=None, normals=None, colors=None, out_count=None, vertex_capacity=0,
                    face_capacity=0, vertices=None, out_normals=None, out_colors=None, pixel_index=None, faces=None):
    """ovg_map_triangulate on contiguous device tensors: z f32 [S, H, W], points f32 [S, H, W, 3], keep u8 [S, H, W], normals f32
    [S, H, W, 3] and colors u8 [S, H, W, 3] or None; ws a uint8 tensor of at least map_triangulate_workspace_bytes(S, H, W) bytes.
    stage L.MAP_COUNT writes (vertices M, faces F) to the two int64 of out_count; L.MAP_SCATTER writes the first vertex_capacity
    vertices to vertices / out_normals f32 [., 3], out_colors u8 [., 3] and pixel_index int64 [.] and the first face_capacity faces to
    faces int32 [., 3] from what the COUNT stage left in ws."""
    what = "map_triangulate"
    S, H, W = _map_shape(what, z, "z")
    _tensor(what, z, "z", _F32, (S, H, W))
    _tensor(what, points, "points", _F32, (S, H, W, 3))
    _tensor(what, keep, "keep", _U8, (S, H, W), optional=True)
    _tensor(what, normals, "normals", _F32, (S, H, W, 3), optional=True)
    _tensor(what, colors, "colors", _U8, (S, H, W, 3), optional=True)
    rel_tol = _number(what, "rel_tol", rel_tol, lo=0, f32=False)             # +inf switches the test off
    if stage not in (L.MAP_COUNT, L.MAP_SCATTER, L.MAP_COUNT | L.MAP_SCATTER):
        raise L.OvgError("%s: unknown stage %r" % (what, stage))
    _int_in(what, "vertex_capacity", vertex_capacity, 0, 1 << 62)
    _int_in(what, "face_capacity", face_capacity, 0, 1 << 62)
    _tensor(what, ws, "ws", _U8)
    if stage & L.MAP_SCATTER:
        _capacity_buffers(what, ((vertices, "vertices", _F32, 3 * vertex_capacity, True), (out_normals, "out_normals", _F32, 3 * vertex_capacity, True),
                                 (out_colors, "out_colors", _U8, 3 * vertex_capacity, True), (pixel_index, "pixel_index", _I64, vertex_capacity, True),
                                 (faces, "faces", _I32, 3 * face_capacity, True)))
    _tensor(what, out_count, "out_count", _I64, min_numel=2)
    _chk_dev(z, points, keep, normals, colors, ws, out_count, vertices, out_normals, out_colors, pixel_index, faces)
    p = L.MapTriangulateParams()
    p.z, p.points, p.keep, p.normals, p.colors = L.ptr(z), L.ptr(points), L.ptr(keep), L.ptr(normals), L.ptr(colors)
    p.S, p.H, p.W, p.rel_tol, p.stage, p.pad = S, H, W, rel_tol, int(stage), 0
    p.vertex_capacity, p.face_capacity = vertex_capacity, face_capacity
    p.out_vertices, p.out_normals, p.out_colors = L.ptr(vertices), L.ptr(out_normals), L.ptr(out_colors)
    p.out_pixel_index, p.out_faces, p.out_count = L.ptr(pixel_index), L.ptr(faces), L.ptr(out_count)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_map_triangulate", p, _stream())


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes: simplification by vertex clustering (ovg_mesh_simplify); cleaning: components and edge statistics, ordered sub-meshes,
# Laplacian / Taubin smoothing (ovg_mesh_topology / _select / _smooth)
# ---------------------------------------------------------------------------------------------------------------------------------
def _meshops_mesh(what, vertices, faces, ws, max_faces=1 << 31):
    """The checks the mesh entries share -> (M, F)."""
    M = _points(what, vertices, "vertices", 1, 1 << 31)
    F = _table(what, faces, "faces", _I32, 3, 1, max_faces)
    _tensor(what, ws, "ws", _U8)
    return M, F


def mesh_simplify_workspace_bytes(vertices, faces):
    return _ws_query("ovg_mesh_simplify_workspace_bytes", vertices=vertices, faces=faces)


def mesh_simplify(stage, vertices, faces, voxel, ws, normals=None, colors=None, position=L.MS_POS_MEAN, out_count=None, vertex_capacity=0,
                  face_capacity=0, out_vertices=None, out_normals=None, out_colors=None, source_index=None, vertex_count=None, out_faces=None):
    """ovg_mesh_simplify on contiguous device tensors: vertices f32 [M, 3], faces int32 [F, 3], voxel a 0-d / 1-element f32 device
    tensor, normals f32 [M, 3] and colors u8 [M, 3] or None; ws a uint8 tensor of at least mesh_simplify_workspace_bytes(M, F) bytes.
    stage L.MS_COUNT writes (M', F', flags, cells, degenerate, duplicates) to the six int64 of out_count; L.MS_SCATTER writes the
    first vertex_capacity vertices to out_vertices f32 [., 3] (out_normals f32 [., 3] / out_colors u8 [., 3] exactly when normals /
    colors are given; source_index int64 [.] and vertex_count int32 [.] optional) and the first face_capacity faces to out_faces int32
    [., 3] from what the COUNT stage left in ws. position: L.MS_POS_MEAN or L.MS_POS_FIRST."""
    what = "mesh_simplify"
    M, F = _meshops_mesh(what, vertices, faces, ws, (1 << 32) - 1)
    _tensor(what, normals, "normals", _F32, (M, 3), optional=True)
    _tensor(what, colors, "colors", _U8, (M, 3), optional=True)
    _tensor(what, voxel, "voxel", _F32, numel=1)
    if stage not in (L.MS_COUNT, L.MS_SCATTER, L.MS_COUNT | L.MS_SCATTER):
        raise L.OvgError("%s: unknown stage %r" % (what, stage))
    if position not in (L.MS_POS_MEAN, L.MS_POS_FIRST):
        raise L.OvgError("%s: unknown position %r" % (what, position))
    _int_in(what, "vertex_capacity", vertex_capacity, 0, 1 << 62)
    _int_in(what, "face_capacity", face_capacity, 0, 1 << 62)
    if stage & L.MS_SCATTER:
        if vertex_capacity and ((normals is None) != (out_normals is None) or (colors is None) != (out_colors is None)):
            raise L.OvgError("%s: out_normals / out_colors go with normals / colors" % what)
        _capacity_buffers(what, ((out_vertices, "out_vertices", _F32, 3 * vertex_capacity, True), (out_normals, "out_normals", _F32, 3 * vertex_capacity, False),
                                 (out_colors, "out_colors", _U8, 3 * vertex_capacity, False), (source_index, "source_index", _I64, vertex_capacity, False),
                                 (vertex_count, "vertex_count", _I32, vertex_capacity, False), (out_faces, "out_faces", _I32, 3 * face_capacity, True)))
    _tensor(what, out_count, "out_count", _I64, min_numel=6, optional=not stage & L.MS_COUNT)
    _chk_dev(vertices, faces, voxel, ws, normals, colors, out_count, out_vertices, out_normals, out_colors, source_index, vertex_count, out_faces)
    p = L.MeshSimplifyParams()
    p.vertices, p.faces, p.normals, p.colors, p.voxel = L.ptr(vertices), L.ptr(faces), L.ptr(normals), L.ptr(colors), L.ptr(voxel)
    p.num_vertices, p.num_faces, p.stage, p.position = M, F, int(stage), int(position)
    p.vertex_capacity, p.face_capacity = vertex_capacity, face_capacity
    p.out_vertices, p.out_normals, p.out_colors = L.ptr(out_vertices), L.ptr(out_normals), L.ptr(out_colors)
    p.out_source_index, p.out_vertex_count, p.out_faces = L.ptr(source_index), L.ptr(vertex_count), L.ptr(out_faces)
    p.out_count, p.ws, p.ws_bytes = L.ptr(out_count), L.ptr(ws), nbytes(ws)
    L.call("ovg_mesh_simplify", p, _stream())


def mesh_topology_workspace_bytes(vertices, faces):
    return _ws_query("ovg_mesh_topology_workspace_bytes", vertices=vertices, faces=faces)


def mesh_select_workspace_bytes(vertices, faces):
    return _ws_query("ovg_mesh_select_workspace_bytes", vertices=vertices, faces=faces)


def mesh_smooth_workspace_bytes(vertices, faces):
    return _ws_query("ovg_mesh_smooth_workspace_bytes", vertices=vertices, faces=faces)


def mesh_topology(vertices, faces, ws, vertex_root, face_root, vertex_flags, out_count):
    """ovg_mesh_topology on contiguous device tensors: vertices f32 [M, 3], faces int32 [F, 3]; ws a uint8 tensor of at least
    mesh_topology_workspace_bytes(M, F) bytes. Writes vertex_root int32 [M], face_root int32 [F], vertex_flags u8 [M] (the L.MT_* bits)
    and the eight int64 of out_count: live faces, referenced vertices, edges, boundary edges, non-manifold edges, boundary vertices,
    non-manifold vertices, status flags (L.MT_INTERNAL)."""
    what = "mesh_topology"
    M, F = _meshops_mesh(what, vertices, faces, ws)
    _tensor(what, vertex_root, "vertex_root", _I32, (M,))
    _tensor(what, face_root, "face_root", _I32, (F,))
    _tensor(what, vertex_flags, "vertex_flags", _U8, (M,))
    _tensor(what, out_count, "out_count", _I64, (8,))
    _chk_dev(vertices, faces, ws, vertex_root, face_root, vertex_flags, out_count)
    p = L.MeshTopologyParams()
    p.vertices, p.faces, p.num_vertices, p.num_faces = L.ptr(vertices), L.ptr(faces), M, F
    p.vertex_root, p.face_root, p.vertex_flags, p.out_count = L.ptr(vertex_root), L.ptr(face_root), L.ptr(vertex_flags), L.ptr(out_count)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_mesh_topology", p, _stream())


def mesh_select(stage, vertices, faces, ws, face_keep=None, vertex_keep=None, out_count=None, vertex_capacity=0, face_capacity=0,
                out_vertices=None, source_index=None, out_faces=None, face_index=None):
    """ovg_mesh_select on contiguous device tensors: vertices f32 [M, 3], faces int32 [F, 3], face_keep u8 [F] and vertex_keep u8 [M]
    or None; ws a uint8 tensor of at least mesh_select_workspace_bytes(M, F) bytes. stage L.MSEL_COUNT writes (M', F') to the two
    int64 of out_count; L.MSEL_SCATTER writes the first vertex_capacity vertices to out_vertices f32 [., 3] (source_index int64 [.]
    optional) and the first face_capacity faces to out_faces int32 [., 3] (face_index int64 [.] optional) from what the COUNT stage
    left in ws."""
    what = "mesh_select"
    M, F = _meshops_mesh(what, vertices, faces, ws)
    _tensor(what, face_keep, "face_keep", _U8, (F,), optional=True)
    _tensor(what, vertex_keep, "vertex_keep", _U8, (M,), optional=True)
    if stage not in (L.MSEL_COUNT, L.MSEL_SCATTER, L.MSEL_COUNT | L.MSEL_SCATTER):
        raise L.OvgError("%s: unknown stage %r" % (what, stage))
    _int_in(what, "vertex_capacity", vertex_capacity, 0, 1 << 62)
    _int_in(what, "face_capacity", face_capacity, 0, 1 << 62)
    if stage & L.MSEL_SCATTER:
        _capacity_buffers(what, ((out_vertices, "out_vertices", _F32, 3 * vertex_capacity, True), (source_index, "source_index", _I64, vertex_capacity, False),
                                 (out_faces, "out_faces", _I32, 3 * face_capacity, True), (face_index, "face_index", _I64, face_capacity, False)))
    _tensor(what, out_count, "out_count", _I64, min_numel=2, optional=not stage & L.MSEL_COUNT)
    _chk_dev(vertices, faces, ws, face_keep, vertex_keep, out_count, out_vertices, source_index, out_faces, face_index)
    p = L.MeshSelectParams()
    p.vertices, p.faces, p.face_keep, p.vertex_keep = L.ptr(vertices), L.ptr(faces), L.ptr(face_keep), L.ptr(vertex_keep)
    p.num_vertices, p.num_faces, p.stage, p.pad = M, F, int(stage), 0
    p.vertex_capacity, p.face_capacity = vertex_capacity, face_capacity
    p.out_vertices, p.out_source_index, p.out_faces, p.out_face_index = L.ptr(out_vertices), L.ptr(source_index), L.ptr(out_faces), L.ptr(face_index)
    p.out_count, p.ws, p.ws_bytes = L.ptr(out_count), L.ptr(ws), nbytes(ws)
    L.call("ovg_mesh_select", p, _stream())


def mesh_smooth(vertices, faces, ws, iterations, lam, mu, out_vertices, out_status, fixed=None, fix_boundary=True, out_normals=None):
    """ovg_mesh_smooth on contiguous device tensors: vertices f32 [M, 3], faces int32 [F, 3], fixed u8 [M] or None; ws a uint8 tensor of
    at least mesh_smooth_workspace_bytes(M, F) bytes. `iterations` steps with factor f32(lam), each followed by one with f32(mu) when
    mu != 0. Writes out_vertices f32 [M, 3] (not the input tensor), out_normals f32 [M, 3] when given, and the L.MSM_* flags to the
    one int64 of out_status."""
    what = "mesh_smooth"
    M, F = _meshops_mesh(what, vertices, faces, ws)
    _tensor(what, fixed, "fixed", _U8, (M,), optional=True)
    _tensor(what, out_vertices, "out_vertices", _F32, (M, 3))
    _tensor(what, out_normals, "out_normals", _F32, (M, 3), optional=True)
    _tensor(what, out_status, "out_status", _I64, (1,))
    _int_in(what, "iterations", iterations, 0, 65537)
    lam, mu = _number(what, "lam", lam), _number(what, "mu", mu)
    if not isinstance(fix_boundary, bool):
        raise L.OvgError("%s: fix_boundary must be True or False, got %r" % (what, fix_boundary))
    if out_vertices.data_ptr() == vertices.data_ptr():
        raise L.OvgError("%s: out_vertices must not be the input tensor" % what)
    _chk_dev(vertices, faces, ws, fixed, out_vertices, out_normals, out_status)
    p = L.MeshSmoothParams()
    p.vertices, p.faces, p.fixed, p.num_vertices, p.num_faces = L.ptr(vertices), L.ptr(faces), L.ptr(fixed), M, F
    p.iterations, p.fix_boundary, p.lam, p.mu = iterations, int(fix_boundary), lam, mu
    p.out_vertices, p.out_normals, p.out_status = L.ptr(out_vertices), L.ptr(out_normals), L.ptr(out_status)
    p.ws, p.ws_bytes = L.ptr(ws), nbytes(ws)
    L.call("ovg_mesh_smooth", p, _stream())
