"""-m gpu: ovg_camera_head (csrc/ovg_camhead.hip) stage by stage. The entry leaves its intermediates in the caller's workspace; every stage is
gated per element against a float64 reference computed from the kernel's own stored input of that stage (kernel_guards.check_camera_stages;
test_camera_head_budget_host.py proves on the CPU that these budgets hold for f32 arithmetic and reject planted defects which the global gate
on the pose accepts) -- at token counts that make every GEMM take every split-K factor its plan can pick, up to the entry's limit of 4096,
in all three modes, with one trunk block and one round; the hand-over between two rounds; the refusals at the limits; and the whole head
(four rounds of four blocks) above 128 tokens against the rounding twin, per component group. Outputs and workspaces sit inside guard bands."""
import importlib

import pytest
import torch

import head_ops_emul as emul
import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops
from test_gpu_edges import DEV, MODES, Slot, _global, _need_gpu, _strided_input, _sync_check, _val  # noqa: F401 (_need_gpu: the autouse fixture)

pytestmark = pytest.mark.gpu
WORST, SHARE = {}, {}
CPU_REFERENCE_UP_TO = 257                 # above it the float64 references are computed on the device
KEYS = ("tok", "x", "pose", "xn", "e", "qkv", "attn", "hid", "part")


class _Cam:
    """The sensitised head of test_camera_head_every_row_block_edge_guarded, its weights packed once per dtype, and what the tests derive
    from them (one-block views, float64 copies per device)."""

    def __init__(self):
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
                elif p.dim() > 1:
                    p.mul_(1.5)
                elif "bias" in name:
                    p.uniform_(-0.1, 0.1)
        hip = heads_hip.HipCameraHead(head.to(DEV))
        with torch.no_grad():
            self.W = {mode: hip._pack(MODES[mode], torch.device(DEV)) for mode in ("bf16", "f16", "f32")}
        self._w64, self._cpu = {}, {}

    def one_block(self, mode, ls1=None, ls2=None, fov_bias=None):
        W = dict(self.W[mode])
        blk = dict(W["blocks"][0])
        for key, v in (("ls1", ls1), ("ls2", ls2)):
            if v is not None:
                blk[key] = torch.full_like(blk[key], v)
        W["blocks"] = [blk]
        if fov_bias is not None:
            W["pb2_b"] = W["pb2_b"].clone()
            W["pb2_b"][7:] = fov_bias
        return W

    def w64(self, mode, dev, fov_bias=None):
        key = (mode, dev)
        if key not in self._w64:
            self._w64 = {k: v for k, v in self._w64.items() if k[0] == mode}       # one mode's float64 copies at a time
            self._w64[key] = kg.camera_w64(self.one_block(mode), dev)
        W = self._w64[key]
        if fov_bias is not None:
            W = dict(W)
            W["pb2_b"] = W["pb2_b"].clone()
            W["pb2_b"][7:] = fov_bias
        return W

    def cpu(self, mode):
        if mode not in self._cpu:
            W = self.W[mode]
            Wc = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in W.items() if k != "blocks"}
            Wc["blocks"] = [{k: v.cpu() for k, v in blk.items()} for blk in W["blocks"]]
            self._cpu = {mode: Wc}
        return self._cpu[mode]


@pytest.fixture(scope="module")
def cam():
    L.require_gpu()
    c = _Cam()
    yield c
    Slot.cache.clear()


def _run(W, toks, S, mode, iters, keys=KEYS, tag="camst"):
    """One guarded call from a strided, poisoned token view into an exact-size guarded workspace -> clones of the named workspace buffers + out."""
    dt = MODES[mode]
    slot = Slot.get((iters * S, 9), torch.float32, None, tag=tag)
    wsb = Slot.get((1, ops.camera_head_workspace_bytes(S, dt)), torch.uint8, None, spare_rows=0, tag=tag + "ws")
    ops.camera_head(toks, W, dt, iters=iters, ws=wsb.view.view(-1), out=slot.view.view(iters, S, 9))
    _sync_check(slot.check, wsb.check)
    V = kg.camera_ws_views(wsb.view.view(-1), S, dt)
    B = {k: V[k].clone() for k in keys if k != "part"}
    if "part" in keys:                    # pb1 is the last GEMM of the call: its split-K partials are still there
        B["part"] = kg.camera_part_view(V["part"], S, kg.camera_ksplit(S, *kg.CAMERA_GEMMS["pb1"])).clone()
    B["out"] = slot.view.view(iters, S, 9).clone()
    return B


def _note(mode, used):
    for stage, v in used.items():
        WORST[(mode, stage)] = max(WORST.get((mode, stage), 0.0), v)
    print("worst used budget so far, %s: %s" % (mode, ", ".join("%s %.3f" % (k[1], v) for k, v in sorted(WORST.items()) if k[0] == mode)), flush=True)


@pytest.mark.parametrize("S", kg.CAMERA_S_SET)
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_every_stage_within_its_budget_at_every_split_k_plan(cam, mode, S):
    table = kg.camera_ksplit_table(S)
    zs = (S + 63) // 64
    print("camera head S=%d: %d z slices, last one %d rows (%d 16-row blocks), %d attention trips, ksplit %s" % (
        S, zs, S - 64 * (zs - 1), min((S - 64 * (zs - 1) + 15) // 16, 4), (S + 127) // 128, table), flush=True)
    toks = kg.camera_tokens(S, 1000 + S)
    td = _strided_input(toks, True)
    A = _run(cam.one_block(mode), td, S, mode, 1)
    # the same call without the LayerScales leaves x0 / x_mid where x is: x += 0 * y is exact, and what it computes before is bit-identical
    B0 = _run(cam.one_block(mode, ls1=0.0, ls2=0.0), td, S, mode, 1, keys=("tok", "e", "x", "qkv"))
    Bm = _run(cam.one_block(mode, ls2=0.0), td, S, mode, 1, keys=("x", "qkv", "attn", "hid"))
    for k in ("tok", "e", "qkv"):
        assert torch.equal(A[k], B0[k]), "%s differs between the call and the call without LayerScales" % k
    for k in ("qkv", "attn", "hid"):
        assert torch.equal(A[k], Bm[k]), "%s differs between the call and the call without ls2" % k
    A["x0"], A["xmid"] = B0["x"], Bm["x"]
    A["out"] = A["out"][0]
    del B0, Bm
    dev = DEV if S > CPU_REFERENCE_UP_TO else "cpu"
    A = {k: v.to(dev) for k, v in A.items()}
    used, share = kg.check_camera_stages("camera_%s_S%d" % (mode, S), A, toks.to(dev), cam.w64(mode, dev), mode)
    _note(mode, used)
    SHARE[mode] = max(SHARE.get(mode, 0.0), share)
    print("largest ambiguous share of an xn row so far, %s: %.2f%%" % (mode, 100 * SHARE[mode]), flush=True)
    Slot.cache.clear()


@pytest.mark.parametrize("positive", [True, False])
@pytest.mark.parametrize("S", [17, 129])
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_round_transition(cam, mode, S, positive):
    """Two rounds of one block: round 2's e from the pose of round 1, the pb1 partials from the stored xn, out[1] = that pose + the delta from the stored partials; with pb2_b pushing both
    FoV components positive (ReLU the identity: the pose is out[0]) and negative (out clamped to zero, the carried pose un-activated, as
    CameraHead.forward keeps pred_pose_enc apart from its activated copy)."""
    fov = 3.0 if positive else -3.0
    W = cam.one_block(mode, fov_bias=fov)
    toks = kg.camera_tokens(S, 2000 + S)
    td = _strided_input(toks, True)
    B1 = _run(W, td, S, mode, 1, keys=("pose",))
    B2 = _run(W, td, S, mode, 2, keys=("pose", "e", "xn", "part"))
    B1, B2 = ({k: v.cpu() for k, v in B.items()} for B in (B1, B2))
    used = kg.check_camera_round2("camera_round2_%s_S%d_fov%+d" % (mode, S, fov), B1, B2, cam.w64(mode, "cpu", fov_bias=fov), mode, positive)
    _note(mode, {"round2": used})
    Slot.cache.clear()


def _entry(tokens, W, dtype, S, iters, trunk_depth, ws, out):
    """ops.camera_head's parameter block with S and trunk_depth set freely (the wrapper takes them from its arguments' shapes)."""
    p = L.CameraHeadParams()
    p.tokens, p.ld_tokens, p.S, p.iters, p.dtype = L.ptr(tokens), tokens.stride(0), S, iters, L.dtype_code(dtype)
    p.trunk_depth, p.dim, p.heads = trunk_depth, 2048, W["heads"]
    for name in ("token_norm_w", "token_norm_b", "trunk_norm_w", "trunk_norm_b", "empty_pose", "embed_w", "embed_b", "mod_w", "mod_b",
                 "pb1_w", "pb1_b", "pb2_w", "pb2_b"):
        setattr(p, name, L.ptr(W[name]))
    for i, blk in enumerate(W["blocks"][:L.CAMERA_MAX_TRUNK]):
        for name, _ in L.CameraBlockWeights._fields_:
            setattr(p.blk[i], name, L.ptr(blk[name]))
    p.ws, p.ws_bytes, p.out = L.ptr(ws), ws.numel() * ws.element_size(), L.ptr(out)
    L.call("ovg_camera_head", p, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_refusals_at_the_limits_write_nothing(cam, mode):
    dt = MODES[mode]
    W = cam.W[mode]
    toks = torch.zeros(4097, 2048, device=DEV)
    for what, S, depth in (("S = 4097", 4097, 4), ("trunk_depth = 5", 8, 5), ("trunk_depth = 0", 8, 0)):
        slot = Slot.get((4 * S, 9), torch.float32, None, tag="camref")
        wsb = Slot.get((1, ops.camera_head_workspace_bytes(min(S, 4096), dt)), torch.uint8, None, spare_rows=0, tag="camrefws")
        with pytest.raises(L.OvgError, match="UNSUPPORTED"):
            _entry(toks[:S], W, dt, S, 4, depth, wsb.view.view(-1), slot.view.view(4, S, 9))
        _sync_check(slot.check, wsb.check)
        for s in (slot, wsb):
            assert bool((s.check.buffer == kg.GUARD_BYTE).all()), "camera_head %s %s: a refused call wrote to its output or workspace" % (mode, what)
        kg.STATS["refusals"] += 1
        print("[REFUSED] camera_head %s %s" % (mode, what), flush=True)
    with pytest.raises(L.OvgError, match="unsupported"):
        ops.camera_head_workspace_bytes(4097, dt)
    Slot.cache.clear()


@pytest.mark.parametrize("S", [129, 321])
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_full_depth_above_128_tokens(cam, mode, S):
    """Four rounds of four blocks against the rounding twin: gpu_selftest.test_camera_head's gates, on the whole tensor and per component group."""
    dt = MODES[mode]
    toks = torch.randn(S, 2048, generator=torch.Generator().manual_seed(3000 + S)) * 1.3
    B = _run(cam.W[mode], _strided_input(toks, True), S, mode, 4, keys=(), tag="camfull")
    with torch.no_grad():
        twin = emul.camera_head(toks, cam.cpu(mode), dt)
    tag = "camera_head_%s_S%d_vs_twin" % (mode, S)
    _global(tag, _val(B["out"]), twin.double(), kg.CAMERA_TOL_TWIN[mode])
    assert kg.camera_group_gate(tag, _val(B["out"]), twin.double(), kg.CAMERA_TOL_TWIN[mode])
    Slot.cache.clear()
