"""CPU-only proof of the stage budgets of the camera head (kernel_guards.check_camera_stages and what it is built from): torch's own f32
arithmetic, split where ovg_camera_head stores (head_ops_emul.camera_head_buffers), stays inside every stage's budget in all three modes,
with the share of ambiguous xn elements under its cap; planted defects -- each confined to what the tensor-global gate on the final pose
cannot see: one split-K slot of one 16-row block, two keys, one row, one (head, query), four columns -- go over their stage's budget while
that global gate accepts them. Every figure is printed."""
import contextlib
import io
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_selftest as st
import head_ops_emul as emul
import kernel_guards as kg
from omnivggt_official_amd import ops

MODES = ("bf16", "f16", "f32")


def _global_ok(got, ref, tol):
    keep = list(st.results)
    with contextlib.redirect_stdout(io.StringIO()):
        ok = st.report("x", got, ref, tol)
    st.results[:] = keep
    return ok


_W32 = {}


def _weights(mode, fov_bias=None, fov_rows=1.0):
    """One trunk block of random weights in the layout of heads_hip.HipCameraHead._pack, at the scales of the sensitised head of the GPU
    tests (matrices 1.5 x the nn.Linear default, LayerScale 0.7, biases within 0.1, a non-zero empty pose)."""
    if not _W32:
        g = torch.Generator().manual_seed(77)
        mat = lambda n, k: torch.randn(n, k, generator=g) * (1.5 / math.sqrt(3 * k))
        vec = lambda n: torch.rand(n, generator=g) * 0.2 - 0.1
        lnw = lambda n: 1.0 + 0.1 * torch.randn(n, generator=g)
        _W32.update({"token_norm_w": lnw(2048), "token_norm_b": vec(2048), "trunk_norm_w": lnw(2048), "trunk_norm_b": vec(2048),
                     "empty_pose": torch.randn(9, generator=g) * 0.5, "embed_w": mat(2048, 9), "embed_b": vec(2048), "mod_w": mat(6144, 2048), "mod_b": vec(6144),
                     "pb1_w": mat(1024, 2048), "pb1_b": vec(1024), "pb2_w": mat(9, 1024), "pb2_b": vec(9), "heads": 16,
                     "blocks": [{"n1_w": lnw(2048), "n1_b": vec(2048), "n2_w": lnw(2048), "n2_b": vec(2048), "ls1": torch.full((2048,), 0.7), "ls2": torch.full((2048,), 0.7),
                                 "qkv_w": mat(6144, 2048), "qkv_b": vec(6144), "proj_w": mat(2048, 2048), "proj_b": vec(2048),
                                 "fc1_w": mat(8192, 2048), "fc1_b": vec(8192), "fc2_w": mat(2048, 8192), "fc2_b": vec(2048)}]})
    dt = kg.CAMERA_DT[mode]
    cv = lambda k, v: v.to(dt) if k in ("mod_w", "pb1_w", "qkv_w", "proj_w", "fc1_w", "fc2_w") else v
    W = {k: cv(k, v) for k, v in _W32.items() if k != "blocks"}
    W["blocks"] = [{k: cv(k, v) for k, v in _W32["blocks"][0].items()}]
    if fov_bias is not None:
        W["pb2_b"] = W["pb2_b"].clone()
        W["pb2_b"][7:] = fov_bias
        W["pb2_w"] = W["pb2_w"].clone()
        W["pb2_w"][7:] *= fov_rows                   # quiet FoV rows: the delta stays next to its bias
    return W


def _tokens(S, seed=5):
    return torch.randn(S, 2048, generator=torch.Generator().manual_seed(seed)) * 1.3


def _buffers(toks, W, dt, iters=1, hooks=None):
    """The twin's buffers, with the pose branch's partials split as the kernel's plan splits them at this token count."""
    return emul.camera_head_buffers(toks, W, dt, iters=iters, hooks=hooks, pb1_slots=kg.camera_ksplit(toks.shape[0], *kg.CAMERA_GEMMS["pb1"]))


def _stages(tag, B, toks, W64, mode, keep=("x0", "xmid"), quiet=False):
    Bc = {k: v for k, v in B.items() if k not in ("x0", "xmid") or k in keep}
    Bc["out"] = B["out"][0]
    return kg.check_camera_stages(tag, Bc, toks, W64, mode, quiet=quiet)


def test_workspace_views_restate_the_entrys_layout():
    for mode in MODES:
        for S in (1, 3, 17, 130):
            dt = kg.CAMERA_DT[mode]
            ws = torch.zeros(ops.camera_head_workspace_bytes(S, dt), dtype=torch.uint8)
            V = kg.camera_ws_views(ws, S, dt)
            assert list(V) == ["tok", "x", "pose", "part", "xn", "e", "qkv", "attn", "hid"]
            assert all(v.data_ptr() % 256 == ws.data_ptr() % 256 for v in V.values())
            assert V["hid"].shape == (S, 8192) and V["hid"].dtype == dt and V["pose"].shape == (S, 9) and V["part"].shape == (S, 32768)


def test_ksplit_rule_and_the_token_counts_that_exhaust_it():
    """The restated rule gives each GEMM the split-K factors listed below, and CAMERA_S_SET of the GPU test makes every GEMM take every value it can."""
    every = {name: {kg.camera_ksplit(S, N, K) for S in range(1, kg.CAM_MAX_S + 1)} for name, (N, K) in kg.CAMERA_GEMMS.items()}
    assert every == {"mod": {4, 2, 1}, "qkv": {4, 2, 1}, "proj": {8, 4, 2, 1}, "fc1": {4, 2, 1}, "fc2": {16, 8, 4, 2, 1}, "pb1": {8, 4, 2, 1}}
    for name, (N, K) in kg.CAMERA_GEMMS.items():
        assert {kg.camera_ksplit(S, N, K) for S in kg.CAMERA_S_SET} == every[name], name
        assert all(kg.camera_ksplit(S, N, K) * N <= kg.CAM_PART_COLS and K % (256 * kg.camera_ksplit(S, N, K)) == 0 for S in range(1, kg.CAM_MAX_S + 1))
        assert kg.camera_ksplit(1, N, K) == max(every[name])
    nmb = {min((S - (S - 1) // 64 * 64 + 15) // 16, 4) for S in kg.CAMERA_S_SET}
    assert nmb == {1, 2, 3, 4}
    assert any(S % 64 for S in kg.CAMERA_S_SET if S > 64) and sum(S > 128 for S in kg.CAMERA_S_SET) >= 2


def test_the_split_twin_is_the_twin_of_the_global_gates():
    """camera_head_buffers with one pb1 product is head_ops_emul.camera_head bit for bit, at four rounds (and as many blocks as the weights have:
    the GPU tests run it with four), so the twin the budgets are proven on and the twin of the global gates cannot drift apart."""
    W = _weights("bf16")
    W["blocks"] = W["blocks"] * 4
    toks = _tokens(5)
    with torch.no_grad():
        assert torch.equal(emul.camera_head_buffers(toks, W, torch.bfloat16, iters=4)["out"], emul.camera_head(toks, W, torch.bfloat16, iters=4))


@pytest.mark.parametrize("mode", MODES)
def test_f32_twin_meets_every_stage_budget(mode):
    W = _weights(mode)
    W64 = kg.camera_w64(W, "cpu")
    worst, worst_share = {}, 0.0
    for S in (1, 17, 20):
        toks = _tokens(S) if S < 20 else kg.camera_tokens(S, 5)            # normal tokens, and the GPU test's
        with torch.no_grad():
            B = _buffers(toks, W, kg.CAMERA_DT[mode])
        for keep in (("x0", "xmid"), ()) if mode == "f32" else (("x0", "xmid"),):
            used, share = _stages("twin_%s_S%d%s" % (mode, S, "" if keep else "_carried"), B, toks, W64, mode, keep=keep)
            worst_share = max(worst_share, share)
            for k, v in used.items():
                worst[k] = max(worst.get(k, 0.0), v)
        if mode != "f32":
            # what the carried form would leave of the gate in a 16-bit mode: printed, the reason the stored x0 / x_mid are used there
            x0, e_x0 = kg.camera_x0(B["tok"].double(), B["e"].double(), W64, mode)
            blk = W64["blocks"][0]
            sh = kg.camera_ln_gemm(x0, e_x0, blk["n1_w"], blk["n1_b"], blk["qkv_w"], blk["qkv_b"], "qkv", mode)["share"]
            print("twin_%s_S%d: with the modulation GEMM's budget carried, %.1f%% of a row's xn elements would count as ambiguous" % (mode, S, 100 * float(sh.max())), flush=True)
    print("camera head f32 twin %s: worst used budget per stage: %s; ambiguous xn elements per row at most %.2f%%" % (
        mode, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), 100 * worst_share), flush=True)
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fov", [2.0, -2.0])
def test_round_transition_of_the_twin(mode, fov):
    """iters = 2: the second round's e against SiLU(embed(pose after round 1)) and out[1] against that pose + the delta from the stored xn;
    FoV positive (ReLU the identity, the pose read from out[0]) and negative (out clamped, the carried pose not)."""
    W = _weights(mode, fov_bias=fov)
    W64 = kg.camera_w64(W, "cpu")
    toks = _tokens(17)
    with torch.no_grad():
        B1 = _buffers(toks, W, kg.CAMERA_DT[mode], iters=1)
        B2 = _buffers(toks, W, kg.CAMERA_DT[mode], iters=2)
    kg.check_camera_round2("twin_round2_%s_fov%+.1f" % (mode, fov), B1, B2, W64, mode, positive=fov > 0)


# ---------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------
def _drop_slot(name_, rows, cols, ks):
    def lin(name, x, w, b):
        y = x @ w.float().t() + b.float()
        if name == name_:
            K = x.shape[1] // ks
            y[rows, cols] -= x[rows, :K] @ w.float()[cols, :K].t()
        return y
    return lin


def _clamped_row(name_, cols):
    def lin(name, x, w, b):
        y = x @ w.float().t() + b.float()
        if name == name_:
            S = x.shape[0]
            y[S - 1, cols] = y[S - 2, cols]
        return y
    return lin


def _one_pass_ln(name_):
    def ln(name, x, w, b, eps):
        if name != name_:
            return F.layer_norm(x, (x.shape[-1],), None if w is None else w.float(), None if b is None else b.float(), eps)
        mean = x.mean(-1, keepdim=True)
        var = (x * x).mean(-1, keepdim=True) - mean * mean
        return (x - mean) * torch.rsqrt(var + eps) * w.float() + b.float()
    return ln


def _tanh_gelu(name_):
    return lambda name, z: F.gelu(z, approximate="tanh") if name == name_ else F.gelu(z)


def _no_one_plus(row, cols):
    def modulate(l, shift, scale, gate, tok):
        x = gate * (l * (1 + scale) + shift) + tok
        x[row, cols] = (gate * (l * scale + shift) + tok)[row, cols]
        return x
    return modulate


def _wrong_v(head, query):
    def attn(q, k, v):
        a = torch.softmax(q @ k.transpose(1, 2) * q.shape[-1] ** -0.5, dim=-1)
        o = a @ v
        o[head, query] = a[head, query] @ v[head + 1]
        return o
    return attn


def _drop_term(comp, k):
    def pb2(hb, w2, b2):
        d = hb @ w2.t() + b2
        d[:, comp] -= hb[:, k] * w2[comp, k]
        return d
    return pb2


def _relu_carry(pose):
    return torch.cat([pose[:, :7], F.relu(pose[:, 7:])], -1)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_planted_defects_pass_the_global_gate_and_fail_their_stage(mode):
    dt = kg.CAMERA_DT[mode]
    S = 20
    W = _weights(mode)
    toks = _tokens(S)
    toks[7] += 300.0                       # a row whose mean dwarfs its spread (the one-pass variance defect lives there; the others do not care)
    toks[S - 1] = toks[S - 2] + 0.02 * _tokens(1, seed=6)[0]      # the last two rows 2 % apart: served from the wrong one, a row is subtly off
    # head 6's V projection = head 5's + 2 %: V taken from the neighbouring head is subtly off
    vw = W["blocks"][0]["qkv_w"].float()
    vw[4096 + 768:4096 + 896] = vw[4096 + 640:4096 + 768] + 0.02 * vw[4096 + 768:4096 + 896]
    W["blocks"][0]["qkv_w"] = vw.to(dt)
    W["blocks"][0]["qkv_b"] = W["blocks"][0]["qkv_b"].clone()
    W["blocks"][0]["qkv_b"][4096 + 768:4096 + 896] = W["blocks"][0]["qkv_b"][4096 + 640:4096 + 768]
    W64 = kg.camera_w64(W, "cpu")
    with torch.no_grad():
        good = _buffers(toks, W, dt)
    _stages("defect_base_%s" % mode, good, toks, W64, mode, quiet=True)
    ks = kg.camera_ksplit_table(S)
    defects = (
        ("one_split_k_slot_dropped_for_a_16_row_block", "x0", dict(lin=_drop_slot("mod", slice(16, 20), slice(64, 80), ks["mod"]))),
        ("one_pass_variance_on_a_row_with_a_large_mean", "tok", dict(ln=_one_pass_ln("token_norm"))),
        ("tanh_gelu_in_fc1", "hid", dict(gelu=_tanh_gelu("fc1"))),
        ("scale_without_one_plus_in_one_threads_columns", "x0", dict(modulate=_no_one_plus(13, slice(1024 + 4 * 250, 1024 + 4 * 251)))),
        ("last_row_served_by_another_rows_clamp", "qkv", dict(lin=_clamped_row("qkv", slice(4096 + 16, 4096 + 32)))),
        ("one_heads_v_from_its_neighbour_for_one_query", "attn", dict(attn=_wrong_v(5, 11))),
        ("tanh_gelu_in_the_pose_kernel", "out.tx", dict(gelu=_tanh_gelu("pb1"))),
        ("one_small_term_of_fov_w_dropped_from_the_pb2_dot", "out.fov_w", dict(pb2=_drop_term(8, int(W["pb2_w"][8].abs().argsort()[100])))),
    )
    wrong = []
    for name, stage, hooks in defects:
        with torch.no_grad():
            bad = _buffers(toks, W, dt, hooks=hooks)
        g_ok = _global_ok(bad["out"], good["out"], kg.CAMERA_TOL_TWIN[mode])
        try:
            _stages("defect_%s_%s" % (mode, name), bad, toks, W64, mode, quiet=True)
            said = "ACCEPTED"
        except AssertionError as exc:
            said = str(exc).split(";")[0]
        print("%-52s global gate %s, stage budget REJECTS (%s)" % (name, "accepts" if g_ok else "REJECTS", said), flush=True)
        where = said.split(":")[0][len("defect_%s_%s." % (mode, name)):]          # the gate that raised: "x0", "qkv", "out.fov_w", ...
        if not g_ok or where != stage:
            wrong.append((name, g_ok, said))
    assert not wrong, "each defect was built to pass the global gate on the pose and to be caught at its stage: %s" % wrong


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_relu_on_the_carried_pose_is_rejected_by_the_round_transition(mode):
    dt = kg.CAMERA_DT[mode]
    W = _weights(mode, fov_bias=-0.005, fov_rows=0.002)
    W64 = kg.camera_w64(W, "cpu")
    toks = _tokens(17)
    with torch.no_grad():
        B1 = _buffers(toks, W, dt, iters=1)
        good = _buffers(toks, W, dt, iters=2)
        bad = _buffers(toks, W, dt, iters=2, hooks=dict(carry=_relu_carry))
    assert float(B1["pose"][:, 7:].max()) < 0, "the FoV components were to be negative after round 1"
    kg.check_camera_round2("relu_carry_base_" + mode, B1, good, W64, mode, positive=False, quiet=True)
    g_ok = _global_ok(bad["out"], good["out"], kg.CAMERA_TOL_TWIN[mode])
    with pytest.raises(AssertionError) as exc:
        kg.check_camera_round2("relu_carry_" + mode, B1, bad, W64, mode, positive=False, quiet=True)
    assert ".e_round2:" in str(exc.value), "the carried pose was to be caught where round 2 embeds it: %s" % exc.value
    print("relu_on_the_carried_pose: global gate %s, round transition REJECTS (%s)" % ("accepts" if g_ok else "REJECTS", str(exc.value).split(";")[0]), flush=True)
    assert g_ok


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_keys_from_128_on_ignored_at_S130_is_rejected_by_the_attention_budget(mode):
    """On the attention stage alone (a qkv buffer of its own, no weight matrices): the two keys of the second trip of the `j += 128` loops
    carry about 1.5e-3 of every row's weight; without them the output stays inside the global gate's tolerance, taken on this stage's
    output, and goes over camera_attn_budget."""
    S, dt = 130, kg.CAMERA_DT[mode]
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(S, 3, 16, 128, generator=g)
    qkv[:, 0] *= 0.3                                              # flat-ish attention: about 1 / S per key
    d = F.normalize(torch.randn(16, 128, generator=g), dim=-1)
    qkv[:, 0] += 4.0 * d                                          # a common query component ...
    qkv[128:, 1] = -6.0 * d                                       # ... that the last two keys oppose: their weight drops by e^(-24 / sqrt(128))
    qkv[:, 2, :, :8] += 12.0                                      # eight large channels per head set the tensor maximum the global gate divides by
    qkv = qkv.reshape(S, 6144).to(dt)
    q, k, v = qkv.float().view(S, 3, 16, 128).permute(1, 2, 0, 3)
    p = torch.softmax(q @ k.transpose(1, 2) * 128 ** -0.5, -1)
    good = (p @ v).permute(1, 0, 2).reshape(S, 2048).to(dt)
    p2 = torch.softmax(q @ k[:, :128].transpose(1, 2) * 128 ** -0.5, -1)
    bad = (p2 @ v[:, :128]).permute(1, 0, 2).reshape(S, 2048).to(dt)
    ref, mag, c = kg.camera_attn_budget(qkv.double(), mode)
    print("weight of keys 128, 129: %.2e .. %.2e of a row" % (float(p[..., 128:].sum(-1).min()), float(p[..., 128:].sum(-1).max())), flush=True)
    assert kg.elementwise_budget("attn_S130_twin_" + mode, good, ref, mag, kg.U_OUT[mode], c, extra=kg.f16_subnormal_floor(mode)) <= 1.0
    g_ok = _global_ok(bad.double(), ref, kg.CAMERA_TOL_TWIN[mode])
    with pytest.raises(AssertionError) as exc:
        kg.elementwise_budget("attn_S130_keys_ignored_" + mode, bad, ref, mag, kg.U_OUT[mode], c, extra=kg.f16_subnormal_floor(mode), quiet=True)
    print("keys_from_128_on_ignored: global gate %s, attention budget REJECTS (%s)" % ("accepts" if g_ok else "REJECTS", str(exc.value).split(";")[0]), flush=True)
    assert g_ok
