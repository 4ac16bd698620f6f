"""HIP-backed replacement of the reference's ZeroAggregator
(omnivggt/models/omnivggt_aggregator.py:18-305, base omnivggt/models/aggregator.py:26-366).

Same constructor keywords that matter for inference, same parameter names (state-dict keys),
same forward signature and return value `(list[depth] of (B,S,P,2C) f32, patch_start_idx)`.
All compute goes through libomnivggt_hip.so (ops.py / lib.py); there is no PyTorch fallback.

Data layout in HBM (B=1 shown; DESIGN.md has the full table):
  residual stream   f32, rows = tokens (view-major), lives INSIDE the output list: after
                    frame block i it is out[i][..., :C], after global block i out[i][..., C:]
                    (row stride 2C) -- the reference's torch.cat (omnivggt_aggregator.py:250)
                    and the zero-padded injection add (:284-301) cost nothing here.
  activations       compute dtype (bf16/f16/f32): LN output [T,C], attention output [T,C],
                    MLP hidden [T,4C]
  q,k               head-major [B'*16, N_pad, 64];  v transposed [B'*16, 64, N_pad]
"""
import ctypes as C_

import torch
import torch.nn as nn

from . import camera_math
from . import lib as L
from . import ops

C, HEADS, D = 1024, 16, 64
RESNET_MEAN = (0.485, 0.456, 0.406)
RESNET_STD = (0.229, 0.224, 0.225)
ROPE_MAX_POS = 128      # RoPE table rows: patch coordinates 1..127 -> inputs up to 1778 px per side


# ----------------------------------------------------------------------------
# parameter containers (names = reference state-dict keys; never called as modules)
# ----------------------------------------------------------------------------
class _Gamma(nn.Module):
    def __init__(self, dim, init):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))


class _AttnParams(nn.Module):
    def __init__(self, dim, qk_norm):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        if qk_norm:
            self.q_norm = nn.LayerNorm(dim // HEADS)
            self.k_norm = nn.LayerNorm(dim // HEADS)


class _MlpParams(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class BlockParamsModule(nn.Module):
    """Parameters of one Block (layers/block.py:27-79)."""
    def __init__(self, dim, qk_norm, ln_eps, ls_init):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=ln_eps)
        self.attn = _AttnParams(dim, qk_norm)
        self.ls1 = _Gamma(dim, ls_init)
        self.norm2 = nn.LayerNorm(dim, eps=ln_eps)
        self.mlp = _MlpParams(dim, 4 * dim)
        self.ls2 = _Gamma(dim, ls_init)


class _ConvProj(nn.Module):
    def __init__(self, in_chans, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, kernel_size=14, stride=14)


class DinoParams(nn.Module):
    """Parameters of the DINOv2 ViT-L/14-reg backbone (layers/vision_transformer.py:42-175)."""
    def __init__(self, dim, depth, n_patches, n_reg):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n_patches + 1, dim))
        self.register_tokens = nn.Parameter(torch.zeros(1, n_reg, dim))
        self.patch_embed = _ConvProj(3, dim)
        self.blocks = nn.ModuleList([BlockParamsModule(dim, False, 1e-6, 1.0) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)


# ----------------------------------------------------------------------------
# device-side runners
# ----------------------------------------------------------------------------
class Workspace:
    """Scratch for one (tokens, sequence length) shape."""
    def __init__(self, M, seq, dtype, device, share=None, kv_rows=None):
        """share: another Workspace with the same M whose LN / attention / hidden scratch is reused (nothing is
        allocated twice); kv_rows: pad q / k / v^T to this many rows instead of `seq` (sharded path: all ranks
        gather equal-sized buffers). Sizes equal ovg_block_workspace_bytes() for (M, seq, dtype)."""
        self.M, self.seq, self.dtype = M, seq, dtype
        self.BH = (M // seq) * HEADS
        if share is not None:
            self.xn, self.attn, self.hid = share.xn, share.attn, share.hid
        else:                                   # split-f16 mode (L.F32X): ops.HiLo pairs of f16 planes
            self.xn = ops.empty_like_dtype((M, C), dtype, device)
            self.attn = ops.empty_like_dtype((M, C), dtype, device)
            self.hid = ops.empty_like_dtype((M, 4 * C), dtype, device)
        rows = seq if kv_rows is None else kv_rows
        self.q, self.k, self.vt = ops.alloc_qkv(self.BH, rows, rows, dtype, device)
        self.device, self._split = device, {}

    def split_ws(self, variant=0, kv_splits=0, cus=0):
        """(ws_part, ws_lse) for this shape's self-attention launch with these knobs if the launch plan cuts it along the keys (launches
        that would leave CUs idle: 8-view global attention = 688 workgroups on 512 slots), else (None, None)."""
        key = (variant, kv_splits, cus)
        if key not in self._split:
            self._split[key] = ops.attn_split_ws(self.BH, self.seq, [self.seq], self.dtype, ops.AttnKnobs(*key, None), self.q.shape[1], self.device)
        return self._split[key]

    def share_from(self, other):
        """Reuse the LN / attention / hidden scratch of another workspace with the same M."""
        self.xn, self.attn, self.hid = other.xn, other.attn, other.hid
        return self


class BlockRunner:
    """Packed weights of one block + the ovg_block_forward call."""
    _GEMM = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")

    def __init__(self, sd, prefix, dtype, device, qk_norm, rope, ln_eps, rope_tables=None, knobs=None):
        self.dtype, self.qk_norm, self.rope, self.ln_eps = dtype, qk_norm, rope, ln_eps
        # `knobs`: any object with .attn_variant / .gemm_tile, read at CALL time (the aggregator itself), so that
        # changing agg.attn_variant after pack() takes effect; None = library defaults
        self.knobs = knobs
        t = {}

        def grab(name, dt):
            src = sd["%s.%s" % (prefix, name)].detach()
            if name in self._GEMM and dt is not torch.float32 and src.dtype == torch.float32:
                t[name] = ops.pack_weights(src.to(device), dt)       # ovg_pack_weights: f32 checkpoint -> compute dtype (split-f16: a HiLo pair)
            elif L.is_split(dt):
                raise L.OvgError("the split-f16 mode packs its (hi, lo) weight planes from f32 masters: load the f32 checkpoint")
            else:
                t[name] = src.to(device=device, dtype=dt).contiguous()
            return L.ptr(ops.hi_lo(t[name])[0])

        lo = lambda name: L.ptr(ops.hi_lo(t[name])[1])

        w = L.BlockWeights()
        w.n1_w, w.n1_b = grab("norm1.weight", torch.float32), grab("norm1.bias", torch.float32)
        w.qkv_w, w.qkv_b = grab("attn.qkv.weight", dtype), grab("attn.qkv.bias", torch.float32)
        if qk_norm:
            w.qn_w, w.qn_b = grab("attn.q_norm.weight", torch.float32), grab("attn.q_norm.bias", torch.float32)
            w.kn_w, w.kn_b = grab("attn.k_norm.weight", torch.float32), grab("attn.k_norm.bias", torch.float32)
        w.proj_w, w.proj_b = grab("attn.proj.weight", dtype), grab("attn.proj.bias", torch.float32)
        w.ls1 = grab("ls1.gamma", torch.float32)
        w.n2_w, w.n2_b = grab("norm2.weight", torch.float32), grab("norm2.bias", torch.float32)
        w.fc1_w, w.fc1_b = grab("mlp.fc1.weight", dtype), grab("mlp.fc1.bias", torch.float32)
        w.fc2_w, w.fc2_b = grab("mlp.fc2.weight", dtype), grab("mlp.fc2.bias", torch.float32)
        w.ls2 = grab("ls2.gamma", torch.float32)
        w.qkv_w_lo, w.proj_w_lo, w.fc1_w_lo, w.fc2_w_lo = lo("attn.qkv.weight"), lo("attn.proj.weight"), lo("mlp.fc1.weight"), lo("mlp.fc2.weight")
        self.tensors, self.weights = t, w
        if rope:
            if rope_tables is None:
                rope_tables = make_rope_tables(ROPE_MAX_POS, device)
            self.rope_tables = rope_tables

    def params(self, ws, x_in, x_out, inject=None, inj_period=0, tokens_per_view=1374, grid_w=37, n_special=5):
        p = L.BlockParams()
        p.w = self.weights
        p.x_in, p.ld_in, p.x_out, p.ld_out = L.ptr(x_in), x_in.stride(0), L.ptr(x_out), x_out.stride(0)
        p.M, p.seq, p.BH = ws.M, ws.seq, ws.BH
        p.nq_pad, p.nk_pad = ws.q.shape[1], ws.k.shape[1]
        p.dtype, p.ln_eps, p.qk_norm, p.rope, p.qk_eps = L.dtype_code(self.dtype), self.ln_eps, int(self.qk_norm), int(self.rope), 1e-5
        if self.rope:
            p.rope_cos, p.rope_sin, p.max_pos = L.ptr(self.rope_tables[0]), L.ptr(self.rope_tables[1]), self.rope_tables[0].shape[0]
        p.tokens_per_view, p.grid_w, p.n_special = tokens_per_view, grid_w, n_special
        if inject is not None:
            p.inject, p.inj_period = L.ptr(inject), inj_period
        for name in ("xn", "q", "k", "vt", "attn", "hid"):
            hi, lo = ops.hi_lo(getattr(ws, name))
            setattr(p, "ws_" + name, L.ptr(hi))
            setattr(p, "ws_%s_lo" % name, L.ptr(lo))
        knobs = ops.attn_knobs(self.knobs, self.dtype)
        p.attn_variant, p.attn_kv_splits, p.attn_cus = knobs.variant, knobs.kv_splits, knobs.cus
        p.attn_fallback_count = L.ptr(knobs.fallback_counter)
        p.gemm_tile = int(getattr(self.knobs, "gemm_tile", 0))
        if hasattr(ws, "split_ws"):
            part, lse = ws.split_ws(knobs.variant, knobs.kv_splits, knobs.cus)
            p.ws_attn_part, p.ws_attn_lse = L.ptr(part), L.ptr(lse)
            p.ws_attn_part_bytes, p.ws_attn_lse_bytes = ops.nbytes(part), ops.nbytes(lse)
        return p

    def forward(self, ws, x_in, x_out, inject=None, inj_period=0, events=None, **kw):
        """x_in/x_out: f32 [M,1024] row-strided views (x_out may alias x_in).
        events: optional (start, stop) torch.cuda.Event pair recorded around the attention launch."""
        p = self.params(ws, x_in, x_out, inject, inj_period, **kw)
        if events is not None:
            p.ev_attn_start, p.ev_attn_stop = events[0].cuda_event, events[1].cuda_event
        L.call("ovg_block_forward", p, torch.cuda.current_stream().cuda_stream)


def make_rope_tables(max_pos, device, base=100.0, half_dim=32):
    """cos/sin [max_pos,16] f32, computed exactly like layers/rope.py:86-117 (16 unique freqs)."""
    exponents = torch.arange(0, half_dim, 2).float() / half_dim
    inv_freq = 1.0 / (base ** exponents)
    angles = torch.einsum("i,j->ij", torch.arange(max_pos, dtype=inv_freq.dtype), inv_freq)
    return angles.cos().contiguous().to(device), angles.sin().contiguous().to(device)


# ----------------------------------------------------------------------------
class ZeroAggregator(nn.Module):
    """Drop-in for omnivggt.models.omnivggt_aggregator.ZeroAggregator (inference only)."""

    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                 num_register_tokens=4, pose_hidden_dim=512, patch_embed="dinov2_vitl14_reg", aa_order=("frame", "global"),
                 aa_block_size=1, qk_norm=True, rope_freq=100, init_values=0.01, dino_depth=24,
                 compute_dtype=torch.float32, **unused):
        super().__init__()
        if embed_dim != C or num_heads != HEADS or patch_size != 14 or mlp_ratio != 4:
            raise ValueError("the gfx950 kernels are built for embed_dim=1024, 16 heads, patch 14, mlp_ratio 4")
        if pose_hidden_dim <= 0:
            raise ValueError("pose_hidden_dim must be positive")
        if patch_embed != "dinov2_vitl14_reg" or tuple(aa_order) != ("frame", "global") or aa_block_size != 1 or not qk_norm or rope_freq <= 0:
            raise ValueError("unsupported aggregator configuration for the HIP path")
        self.img_size, self.patch_size, self.depth, self.dino_depth = img_size, patch_size, depth, dino_depth
        self.rope_freq = float(rope_freq)
        self.patch_start_idx = 1 + num_register_tokens
        self.aa_block_num = depth
        grid = img_size // patch_size
        self.grid = grid                                  # the TRAINED (square) patch grid = pos_embed geometry
        self.set_geometry(img_size, img_size)             # per-call geometry; forward() resets it from the input

        self.patch_embed = DinoParams(embed_dim, dino_depth, grid * grid, num_register_tokens)
        self.frame_blocks = nn.ModuleList([BlockParamsModule(embed_dim, True, 1e-5, init_values) for _ in range(depth)])
        self.global_blocks = nn.ModuleList([BlockParamsModule(embed_dim, True, 1e-5, init_values) for _ in range(depth)])
        self.camera_token = nn.Parameter(torch.randn(1, 2, 1, embed_dim) * 1e-6)
        self.register_token = nn.Parameter(torch.randn(1, 2, num_register_tokens, embed_dim) * 1e-6)
        self.depth_placeholder = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pose_embeddings = nn.ModuleList([nn.Linear(pose_hidden_dim, embed_dim) for _ in range(depth + 1)])
        self.camera_adapters = nn.ModuleList([nn.Linear(embed_dim, embed_dim) for _ in range(depth + 1)])
        for a in self.camera_adapters:
            nn.init.zeros_(a.weight)
            nn.init.zeros_(a.bias)
        self.depth_patch_embed = _ConvProj(2, embed_dim)
        self.pose_hidden_dim = pose_hidden_dim
        self.compute_dtype = L.F32X if compute_dtype == "f32x" else compute_dtype
        self.attn_variant = 0       # ovg_attn_params.variant of every attention call (0 = library default); read per call
        self.gemm_tile = 0          # OVG_TILE_* forced on the block GEMMs (tests); 0 = shape heuristic
        self.attn_kv_splits = 0     # ovg_attn_params.kv_splits: 0 = library decides per launch, 1 = never split
        self.f32x_fast_pv = False   # split-f16 mode, opt-in (round 6): True = attention's PV contraction without P_lo x V_hi: +16 % (64 views 28.1 -> 32.6 frames/s) at 3e-5 of the f32 mode at full depth but up to 1.0e-4 on single rows (64-view depth-1 camera token) -- outside the mode's <= 1e-4 contract
        self.attn_cus = 0           # ovg_attn_params.cus of the BlockRunner launches (0 = the whole device). The sharded run leaves it at 0: frame / DINOv2 attention never overlaps an exchange; the global-attention launches that DO take their budget from sharding.HipExecutor.cus
        self.max_workspaces = 4     # scratch shapes kept alive (frame + global of the two most recent geometries)
        self.layer_hook = None      # callable(layer index, outs[layer]) invoked after every global block of the single-GPU forward (OmniVGGT.forward: early DPT pyramid levels)
        self.shard = None           # set by sharding.ViewSharding for the multi-GPU path
        self.fallback_counter = None    # enable_fallback_counter(): device int32 the attention launches count their re-run workgroups into
        self._packed = None
        self._ws = {}
        self.register_load_state_dict_post_hook(lambda m, k: m.invalidate())

    # ------------------------------------------------------------------
    # live per-kernel timing of the global-attention launches (bench.py roofline)
    def enable_attention_events(self, n):
        """Pre-create n HIP event pairs; every global-attention launch takes the next pair (None when exhausted)."""
        self._events = []
        for _ in range(n):
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            pair[0].record()
            pair[1].record()          # materialise the hipEvent_t handles
            self._events.append(pair)
        self._event_i, self._event_flop = 0, []
        return self._events

    def reset_attention_events(self):
        self._event_i, self._event_flop = 0, []

    def next_attention_events(self, flop=0.0):
        """Event pair for the next global-attention launch; `flop` = algorithmic FLOP of that launch (4 * BH * nq * nk * 64)."""
        ev = getattr(self, "_events", None)
        if not ev or self._event_i >= len(ev):
            return None
        self._event_i += 1
        self._event_flop.append(float(flop))
        return ev[self._event_i - 1]

    def attention_event_times(self):
        """ms of every recorded global-attention launch since reset (device must be synchronised)."""
        return [a.elapsed_time(b) for a, b in getattr(self, "_events", [])[: getattr(self, "_event_i", 0)]]

    def attention_event_flops(self):
        return list(getattr(self, "_event_flop", []))

    def disable_attention_events(self):
        self._events, self._event_i, self._event_flop = [], 0, []

    # ------------------------------------------------------------------
    # telemetry of the speculative bf16 softmax (ovg_attn_params.fallback_count): how many workgroups of the attention launches since
    # the last reset failed the verification of their speculative pass and re-ran with the lazy-rescale body (results are exact either way)
    def enable_fallback_counter(self, device):
        self.fallback_counter = torch.zeros(1, dtype=torch.int32, device=device)
        return self.fallback_counter

    def read_fallback_counter(self, reset=True):
        """Workgroups that paid the second pass since the last reset (synchronises the device); None when not enabled."""
        c = getattr(self, "fallback_counter", None)
        if c is None:
            return None
        n = int(c.item())
        if reset:
            c.zero_()
        return n

    def invalidate(self):
        self._packed = None
        self._ws = {}

    # ------------------------------------------------------------------
    def set_geometry(self, H, W):
        """Patch-grid geometry of the current input (any H, W that are multiples of the patch size, like the
        reference: layers/patch_embed.py:72-73). Non-518x518 inputs get a resampled pos_embed (pos_table)."""
        ps = self.patch_size
        if H % ps or W % ps:
            raise AssertionError(f"Input image height {H} / width {W} is not a multiple of patch size {ps}")
        gh, gw = H // ps, W // ps
        if max(gh, gw) + 1 > ROPE_MAX_POS:
            raise ValueError("inputs larger than %d px per side are not supported" % ((ROPE_MAX_POS - 1) * ps))
        self.grid_hw = (gh, gw)
        self.n_patches = gh * gw
        self.tokens_per_view = self.n_patches + self.patch_start_idx
        return gh, gw

    def pos_table(self, pk, gh, gw):
        """f32 [1 + gh*gw, 1024] on the device: the cls position row, then the patch position rows for this
        grid -- pos_embed itself for the trained square grid, otherwise DINOv2's bicubic + antialias
        resampling (layers/vision_transformer.py:180-212 with interpolate_offset=0.0, aggregator.py:156-157),
        evaluated once per geometry with the same ATen CPU op the reference calls, then cached."""
        if (gh, gw) == (self.grid, self.grid):
            return pk["pos_embed"]
        key = ("pos", gh, gw)
        if key not in pk:
            pe = pk["pos_embed"].detach().float().cpu().unsqueeze(0)      # the packed copy: the module parameter may be on meta (from_packed)
            M = self.grid
            patch = torch.nn.functional.interpolate(pe[:, 1:].reshape(1, M, M, C).permute(0, 3, 1, 2), mode="bicubic",
                                                    antialias=True, size=(gh, gw))
            patch = patch.permute(0, 2, 3, 1).reshape(-1, C)
            pk[key] = torch.cat((pe[0, :1], patch), dim=0).contiguous().to(pk["device"])
        return pk[key]

    def set_compute_dtype(self, dtype):
        if dtype == "f32x":
            dtype = L.F32X
        if dtype not in (torch.bfloat16, torch.float16, torch.float32) and dtype is not L.F32X:
            raise ValueError("compute dtype must be bf16, f16, f32 or the split-f16 mode lib.F32X ('f32x')")
        if dtype is not self.compute_dtype:
            self.compute_dtype = dtype
            self.invalidate()

    def pack(self, device, sd=None):
        """One-time pre-pack after load_state_dict: GEMM weights -> compute dtype, the rest f32.
        sd: use this state dict instead of the module's parameters -- export_packed() output read back from disk, whose
        GEMM weights are already in the compute dtype (and the two Conv2d patch weights already 2-D, zero padded)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:          # "cuda" and "cuda:<current>" are the same pack
            device = torch.device("cuda", torch.cuda.current_device())
        if sd is None and self._packed is not None and self._packed["device"] == device and self._packed["dtype"] is self.compute_dtype:
            return self._packed
        L.require_gpu()
        dt = self.compute_dtype
        if sd is None:
            sd = {k: v for k, v in self.state_dict().items()}
            if any(v.is_meta for v in sd.values()):
                raise L.OvgError("this aggregator's parameters live on the meta device (OmniVGGT.from_packed keeps only the packed "
                                 "weights): it can run its packed dtype on the device it was loaded to, but it cannot be re-packed "
                                 "for another dtype / device -- load the original checkpoint (from_safetensors) for that")
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        rope = make_rope_tables(ROPE_MAX_POS, device, self.rope_freq)
        pk = {"device": device, "dtype": dt, "rope": rope}
        pk["dino"] = [BlockRunner(sd, "patch_embed.blocks.%d" % i, dt, device, False, False, 1e-6, knobs=self) for i in range(self.dino_depth)]
        pk["frame"] = [BlockRunner(sd, "frame_blocks.%d" % i, dt, device, True, True, 1e-5, rope, knobs=self) for i in range(self.depth)]
        pk["global"] = [BlockRunner(sd, "global_blocks.%d" % i, dt, device, True, True, 1e-5, rope, knobs=self) for i in range(self.depth)]

        def conv_as_gemm(w, k_pad):          # Conv2d(k=14, s=14) weight [1024, C_in, 14, 14] -> GEMM rows [1024, k_pad]
            if w.dim() == 2 and w.shape[1] == k_pad and w.dtype is dt:      # already packed (load_packed)
                return w.detach().to(device).contiguous()
            return ops.pack_weights(w.detach().to(device), dt, k_pad=k_pad)

        pk["patch_w"] = conv_as_gemm(sd["patch_embed.patch_embed.proj.weight"], 640)
        pk["patch_b"] = f32(sd["patch_embed.patch_embed.proj.bias"])
        pk["pos_embed"] = f32(sd["patch_embed.pos_embed"][0])                     # [1370,1024]
        pk["cls"] = f32(sd["patch_embed.cls_token"].reshape(-1))
        pk["reg"] = f32(sd["patch_embed.register_tokens"][0])                      # [4,1024]
        pk["dino_norm_w"], pk["dino_norm_b"] = f32(sd["patch_embed.norm.weight"]), f32(sd["patch_embed.norm.bias"])
        pk["depth_w"] = conv_as_gemm(sd["depth_patch_embed.proj.weight"], 448)
        pk["depth_b"] = f32(sd["depth_patch_embed.proj.bias"])
        pk["camera_token"] = f32(sd["camera_token"].reshape(2, C))
        pk["register_token"] = f32(sd["register_token"].reshape(2, -1, C))
        pk["placeholder"] = f32(sd["depth_placeholder"].reshape(-1))
        # camera modality tables (ovg_camera_tables, exact f32): the 25 pose embeddings and the 25 adapters stacked
        G = self.depth + 1
        pk["pose_w"] = torch.cat([sd["pose_embeddings.%d.weight" % i].detach().float().cpu() for i in range(G)]).contiguous().to(device)   # [G*1024, 9]
        pk["pose_b"] = torch.cat([sd["pose_embeddings.%d.bias" % i].detach().float().cpu() for i in range(G)]).contiguous().to(device)
        pk["adapt_w"] = torch.stack([f32(sd["camera_adapters.%d.weight" % i]) for i in range(G)]).contiguous()                              # [G,1024,1024]
        pk["adapt_b"] = torch.stack([f32(sd["camera_adapters.%d.bias" % i]) for i in range(G)]).contiguous()                                # [G,1024]
        self._packed = pk
        return pk

    # ------------------------------------------------------------------
    # persisted pre-packed weights: the reference converts nothing, it keeps f32 masters and starts every
    # process with a 25 s initialiser + a torch.hub call + a 5 GB f32 checkpoint read (inference.py:321-325). Here the
    # packed form -- GEMM weights in the compute dtype, conv patch weights as padded GEMM rows, everything else f32 -- can be
    # written once and mapped back without running pack_weights or holding f32 masters of the 1.2 G GEMM parameters.
    PACKED_GEMM_KEYS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")

    def export_packed(self, device):
        """{state-dict key: tensor} in packed form (device tensors; the caller moves / saves them)."""
        pk = self.pack(device)
        out = {k: v.detach() for k, v in self.state_dict().items()}
        for group, prefix in (("dino", "patch_embed.blocks"), ("frame", "frame_blocks"), ("global", "global_blocks")):
            for i, runner in enumerate(pk[group]):
                for name in self.PACKED_GEMM_KEYS:
                    out["%s.%d.%s" % (prefix, i, name)] = runner.tensors[name]
        out["patch_embed.patch_embed.proj.weight"] = pk["patch_w"]
        out["depth_patch_embed.proj.weight"] = pk["depth_w"]
        return out

    def load_packed(self, sd, device):
        """Install export_packed() output (any device) as this aggregator's packed weights; the module's own parameters are
        not touched (they may stay on the meta device: forward() only reads the packed form)."""
        want = next(v.dtype for k, v in sd.items() if k.endswith("global_blocks.0.attn.qkv.weight"))
        if L.is_split(self.compute_dtype):
            raise ValueError("packed files hold one 16-bit plane per weight; the split-f16 mode packs from the f32 checkpoint")
        if want != self.compute_dtype:
            raise ValueError("packed weights are %s but compute_dtype is %s" % (want, self.compute_dtype))
        self._packed = None
        pk = self.pack(device, sd=sd)
        return pk

    def workspace(self, M, seq, device):
        """Scratch for (tokens, sequence) -- cached, least-recently-used shapes beyond `max_workspaces` are dropped so a
        long-lived process serving scenes of varying S / geometry does not accumulate one 2 GB scratch set per shape."""
        key = (M, seq, self.compute_dtype, str(device))
        ws = self._ws.pop(key, None)
        if ws is None:
            while len(self._ws) >= max(2, int(self.max_workspaces)):
                self._ws.pop(next(iter(self._ws)))                  # dicts keep insertion order: first = least recently used
            share = next((o for (m2, _, dt2, dv2), o in self._ws.items() if m2 == M and dt2 is self.compute_dtype and dv2 == str(device)), None)
            ws = Workspace(M, seq, self.compute_dtype, device, share=share)
        self._ws[key] = ws                                           # (re)insert as most recently used
        return ws

    # ------------------------------------------------------------------
    def camera_tables(self, pk, extrinsics, intrinsics, camera_gt_index, B, S, hw, device):
        """f32 [depth+1, B*S, 1024]: camera_adapters[i](scatter(pose_embeddings[i](enc)))
        (omnivggt_aggregator.py:85-105,158-182,211,273-287). Views without a GT camera get the adapter bias (Linear of a
        zero row). Built by ONE C call (ovg_camera_tables: selection, normalisation, pose encoding, the stacked Linear(9 -> 1024),
        the 25 adapters as one batched exact-f32 GEMM over the camera rows, bias fill) from DEVICE extrinsics / intrinsics:
        no device -> host copy, no sync, <= 3 launches per forward. camera_math.py keeps the same arithmetic as host-side
        PyTorch (used by the post-processing helpers and as this entry's test twin)."""
        K = B * S
        if len(camera_gt_index) == 0:
            key = ("bias_tables", K)
            if key not in pk:               # Linear(0) = bias for every view; constant across calls
                cached = [k for k in pk if isinstance(k, tuple) and k and k[0] == "bias_tables"]
                if len(cached) >= 16:       # same cap as the index cache below: a long-lived process with ever-changing view counts
                    for k in cached:
                        del pk[k]
                pk[key] = ops.camera_tables(None, None, None, K, hw, pk["pose_w"], pk["pose_b"], pk["adapt_w"], pk["adapt_b"])
            return pk[key]                  # READ-ONLY: the same storage is handed to every forward without cameras (callers only slice it)
        if self.pose_hidden_dim != 9:
            raise ValueError("ovg_camera_tables encodes cameras as absT_quaR_FoV (9 values); pose_hidden_dim=%d" % self.pose_hidden_dim)
        idx_key = ("cam_index", tuple(int(i) for i in camera_gt_index))
        if idx_key not in pk:               # the index list reaches the device once per distinct list, not once per forward
            if min(idx_key[1]) < 0 or max(idx_key[1]) >= S:
                raise IndexError("camera_gt_index out of range for %d views" % S)
            # duplicate views are accepted like the reference accepts them (index_select + index assignment, omnivggt_aggregator.py:158-178):
            # the normalisation statistics run over the list AS GIVEN (a duplicate counts twice in the mean camera distance), and the
            # entries of one view describe one camera, so the table rows they scatter are byte-identical -- the concurrent writes are benign
            cached = [k for k in pk if isinstance(k, tuple) and k and k[0] == "cam_index"]
            if len(cached) >= 16:           # a long-lived process with ever-changing index lists: start over
                for k in cached:
                    del pk[k]
            pk[idx_key] = torch.tensor(idx_key[1], dtype=torch.int32).to(device)
        return ops.camera_tables(extrinsics.to(device), intrinsics.to(device), pk[idx_key], S, hw,
                                 pk["pose_w"], pk["pose_b"], pk["adapt_w"], pk["adapt_b"])

    def depth_tokens(self, pk, depth, mask, depth_gt_index, B, S, device):
        """(depth_tok [B*n*P0,1024] f32 or None, depth_row int32 [B*S])
        (omnivggt_aggregator.py:107-128,185-208)."""
        K = B * S
        row = torch.full((K,), -1, dtype=torch.int32)
        n = len(depth_gt_index)
        if n == 0:
            return None, row.to(device)
        if tuple(depth.shape[:4]) != tuple(mask.shape):
            raise AssertionError("mask and depth must have the same first four dimensions")
        idx = torch.tensor(list(depth_gt_index), device=device)
        H, W = depth.shape[2], depth.shape[3]
        d_sel = torch.index_select(depth.to(device).float(), 1, idx).reshape(B, n * H * W).contiguous()
        m_sel = torch.index_select(mask.to(device).float(), 1, idx).reshape(B, n * H * W).contiguous()
        stats = ops.depth_stats(d_sel, m_sel)
        cols = ops.im2col_depth(d_sel.view(B * n, H, W), m_sel.view(B * n, H, W), stats, n, self.compute_dtype)
        tok = ops.linear(cols, pk["depth_w"], pk["depth_b"], self.compute_dtype, out_f32=True)
        sel = torch.as_tensor(list(depth_gt_index), dtype=torch.long)
        row.view(B, S)[:, sel] = (torch.arange(B, dtype=torch.int32).unsqueeze(1) * n + torch.arange(n, dtype=torch.int32).unsqueeze(0))
        return tok, row.to(device)

    # ------------------------------------------------------------------
    def embed(self, pk, images, extrinsics, intrinsics, depth, mask, depth_gt_index, camera_gt_index, view_slice=None):
        """DINO backbone + modality fusion -> (tokens0 f32 [K*P,1024], camera tables).
        view_slice=(lo,hi) restricts the per-view work to a contiguous range of the B*S views
        (multi-GPU: each rank embeds its own views; global statistics still span all views)."""
        B, S, C_in, H, W = images.shape
        device = images.device
        P = self.tokens_per_view
        K = B * S
        lo, hi = (0, K) if view_slice is None else view_slice
        Kl = hi - lo
        dt = self.compute_dtype
        imgs = images.reshape(K, C_in, H, W)[lo:hi].float().contiguous()
        cols = ops.im2col_rgb(imgs, dt, mean=RESNET_MEAN, std=RESNET_STD)
        xd = torch.empty(Kl * P, C, device=device, dtype=torch.float32)
        pos = self.pos_table(pk, *self.grid_hw)
        ops.linear(cols, pk["patch_w"], pk["patch_b"], dt, epilogue=L.EPI_PATCH, out=xd, table=pos,
                   p0=self.n_patches, p1=P, row_off=self.patch_start_idx)
        ops.dino_specials(xd, Kl, P, pk["cls"], pos[0], pk["reg"])
        ws = self.workspace(Kl * P, P, device)
        for blk in pk["dino"]:
            blk.forward(ws, xd, xd)
        tables = self.camera_tables(pk, extrinsics, intrinsics, camera_gt_index, B, S, (H, W), device)
        dtok, drow = self.depth_tokens(pk, depth, mask, depth_gt_index, B, S, device)
        tokens0 = torch.empty(Kl * P, C, device=device, dtype=torch.float32)
        ops.assemble_tokens(xd, pk["dino_norm_w"], pk["dino_norm_b"], 1e-6, pk["camera_token"], pk["register_token"],
                            tables[0][lo:hi].contiguous(), dtok, drow[lo:hi].contiguous(), pk["placeholder"], tokens0, Kl, S,
                            P, self.patch_start_idx, view0=lo)
        return tokens0, tables

    def forward(self, images, extrinsics, intrinsics, depth, mask, depth_gt_index, camera_gt_index):
        B, S, C_in, H, W = images.shape
        if C_in != 3:
            raise ValueError(f"Expected 3 input channels, got {C_in}")
        if not images.is_cuda:
            raise L.OvgError("ZeroAggregator.forward needs HIP device tensors: there is no CPU fallback")
        # on every call and before anything is queued: the device kernels index the views with these lists unchecked, and a
        # cached index tensor (camera_tables) says nothing about the view count of THIS call
        for name, index in (("camera_gt_index", camera_gt_index), ("depth_gt_index", depth_gt_index)):
            if len(index) and (min(int(i) for i in index) < 0 or max(int(i) for i in index) >= S):
                raise IndexError("%s out of range for %d views" % (name, S))
        if self.shard is not None:
            return self.shard.forward(self, images, extrinsics, intrinsics, depth, mask, depth_gt_index, camera_gt_index)
        device = images.device
        pk = self.pack(device)
        gh, gw = self.set_geometry(H, W)
        P, K = self.tokens_per_view, B * S
        T = K * P
        geo = dict(tokens_per_view=P, grid_w=gw)
        with torch.no_grad():
            tokens0, tables = self.embed(pk, images, extrinsics, intrinsics, depth, mask, depth_gt_index, camera_gt_index)
            ws_f = self.workspace(T, P, device)
            ws_g = self.workspace(T, S * P, device)
            outs = [torch.empty(B, S, P, 2 * C, device=device, dtype=torch.float32) for _ in range(self.depth)]
            x = tokens0
            for i in range(self.depth):
                buf = outs[i].view(T, 2 * C)
                pk["frame"][i].forward(ws_f, x, buf[:, :C], inject=tables[i + 1], inj_period=P, **geo)
                pk["global"][i].forward(ws_g, buf[:, :C], buf[:, C:], events=self.next_attention_events(4.0 * B * (S * P) ** 2 * C), **geo)
                x = buf[:, C:]
                if self.layer_hook is not None:
                    self.layer_hook(i, outs[i])                  # outs[i] is final (queued on the current stream): OmniVGGT starts the DPT pyramid levels of layers 4 / 11 / 17 here
        return outs, self.patch_start_idx
