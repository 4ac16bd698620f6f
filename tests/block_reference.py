"""Shared pieces of the block-entry tests (a plain helper module like kernel_guards; test_block_reference_host.py pins the reference
against the oracle on the CPU before test_gpu_block_entries.py holds a kernel against it).

draw_weights()      one block's parameters, variance-preserving GEMM weights, LayerScale gammas of order 1 (0.5 + 0.1 randn: the model's
                    own 0.01 would let the residual hide a wrong branch under a tensor-global gate)
positions()         the (y, x) patch coordinates ovg_qkv derives from tokens_per_view / grid_w (header: t < 5 -> (0, 0))
block_reference()   the block in float64: LN -> qkv + q/k-norm + RoPE -> softmax attention (optionally over extra K / V segments)
                    -> proj, LayerScale, residual -> LN -> fc1, GELU (erf) -> fc2, LayerScale, residual -> inject every inj_period rows
expected_workspace_bytes()   the header's documented formula, restated
"""
import torch
import torch.nn.functional as F

import gpu_selftest as st

C, H, D, HID = 1024, 16, 64, 4096
GEMM = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
# frame-mode shapes (tokens_per_view, grid_w): 5 special tokens + patches; they cross OVG_KV_TILE = 64, the 16 / 64 / 128 row edges of the
# GEMM tiles, one query tile, and (3 views as one sequence: 18, 75, 192, 195, 387 keys) attention over more than one key tile
SHAPES = ((6, 1), (25, 5), (64, 10), (65, 10), (129, 31))
GATE = {"bf16": 3e-2, "f16": 6e-3, "f32": 5e-5, "f32x": 5e-5}       # gpu_selftest.test_block's gates; split-f16 at the f32 gate
ROPE_ROWS = 38


def draw_weights(seed=11):
    """{state-dict key without prefix: f32 CPU tensor}."""
    g = torch.Generator().manual_seed(seed)

    def r(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=g) * scale + shift

    return {
        "norm1.weight": r(C, scale=0.1, shift=1.0), "norm1.bias": r(C, scale=0.1),
        "attn.qkv.weight": r(3 * C, C, scale=C ** -0.5), "attn.qkv.bias": r(3 * C, scale=0.1),
        "attn.q_norm.weight": r(D, scale=0.1, shift=1.0), "attn.q_norm.bias": r(D, scale=0.1),
        "attn.k_norm.weight": r(D, scale=0.1, shift=1.0), "attn.k_norm.bias": r(D, scale=0.1),
        "attn.proj.weight": r(C, C, scale=C ** -0.5), "attn.proj.bias": r(C, scale=0.1),
        "ls1.gamma": r(C, scale=0.1, shift=0.5),
        "norm2.weight": r(C, scale=0.1, shift=1.0), "norm2.bias": r(C, scale=0.1),
        "mlp.fc1.weight": r(HID, C, scale=C ** -0.5), "mlp.fc1.bias": r(HID, scale=0.1),
        "mlp.fc2.weight": r(C, HID, scale=HID ** -0.5), "mlp.fc2.bias": r(C, scale=0.1),
        "ls2.gamma": r(C, scale=0.1, shift=0.5),
    }


def rope_tables():
    """The oracle's cos / sin [ROPE_ROWS, 32] (f32): the reference takes them as they are, the kernels their 16 unique columns."""
    return st.orc.rope_tables(ROPE_ROWS)


def positions(M, tokens_per_view, grid_w, n_special=5):
    """int64 [M, 2]: (y, x) of row m from t = m % tokens_per_view."""
    t = torch.arange(M) % tokens_per_view
    pp = (t - n_special).clamp(min=0)
    py = torch.where(t >= n_special, pp // grid_w + 1, torch.zeros_like(t))
    px = torch.where(t >= n_special, pp % grid_w + 1, torch.zeros_like(t))
    return torch.stack([py, px], -1)


def inject_rows(M, inject, inj_period):
    """[M, 1024] float64: row m = inject[m / inj_period] where m % inj_period == 0, else zero (ovg_linear's RES epilogue)."""
    full = torch.zeros(M, inject.shape[1], dtype=torch.float64)
    n = full[::inj_period].shape[0]
    full[::inj_period] = inject[:n].double()
    return full


def block_reference(x, W, seq, tokens_per_view, grid_w, rope, inject=None, inj_period=0, segments=None, local_seg_index=0, eps=1e-5):
    """x [M, 1024]; W: draw_weights() keys -> the values the device holds (any float dtype; taken to float64); rope: (cos, sin)
    [max_pos, 32]. segments: extra (k [16, nk, 64], v [16, nk, 64]) pairs (B = 1: seq == M), the block's own keys are inserted at
    `local_seg_index` of the concatenation. -> float64 [M, 1024]."""
    W = {k: v.double() for k, v in W.items()}
    x = x.double()
    M = x.shape[0]
    B = M // seq
    xn = F.layer_norm(x, (C,), W["norm1.weight"], W["norm1.bias"], eps)
    qn = [W["attn.q_norm.weight"], W["attn.q_norm.bias"], W["attn.k_norm.weight"], W["attn.k_norm.bias"]]
    q, k, v = st.qkv_reference(xn, W["attn.qkv.weight"], W["attn.qkv.bias"], seq, qn, (rope[0].double(), rope[1].double()),
                               tokens_per_view, grid_w)                                    # [B, 16, seq, 64], q pre-scaled for exp2
    if segments:
        assert B == 1
        ks, vs = [s[0].double().unsqueeze(0) for s in segments], [s[1].double().unsqueeze(0) for s in segments]
        ks.insert(local_seg_index, k)
        vs.insert(local_seg_index, v)
        k, v = torch.cat(ks, 2), torch.cat(vs, 2)
    o = st.attn_reference(q, k, v).transpose(1, 2).reshape(M, C)
    x1 = x + W["ls1.gamma"] * (o @ W["attn.proj.weight"].t() + W["attn.proj.bias"])
    h = F.gelu(F.layer_norm(x1, (C,), W["norm2.weight"], W["norm2.bias"], eps) @ W["mlp.fc1.weight"].t() + W["mlp.fc1.bias"])
    x2 = x1 + W["ls2.gamma"] * (h @ W["mlp.fc2.weight"].t() + W["mlp.fc2.bias"])
    if inject is not None:
        x2 = x2 + inject_rows(M, inject, inj_period)
    return x2


def expected_workspace_bytes(M, seq, esz, nq_pad=None, nk_pad=None):
    """include/omnivggt_hip.h: xn / attn [M, 1024], hid [M, 4096], q [BH, nq_pad, 64], k [BH, nk_pad, 64], vt [BH, 64, nk_pad] in the
    compute dtype (esz bytes; split-f16: one f16 plane), BH = (M / seq) 16, paddings default to seq rounded up to 64."""
    pad = (seq + 63) // 64 * 64
    nq_pad = pad if nq_pad is None else nq_pad
    nk_pad = pad if nk_pad is None else nk_pad
    BH = (M // seq) * H
    out = {"xn": M * C * esz, "attn": M * C * esz, "hid": M * HID * esz, "q": BH * nq_pad * D * esz, "k": BH * nk_pad * D * esz,
           "vt": BH * nk_pad * D * esz}
    out["total"] = sum(out.values())
    return out
