"""A launch tape of heads_hip.HipDPTHead and a per-element checker of every launch on it (a plain helper module like kernel_guards;
test_dpt_stages_host.py proves on the CPU that the checker accepts the f32 emulation of the chain and pins planted defects to their own
launch, test_gpu_dpt_head_stages.py runs it on the kernels).

recording()          replaces head_layernorm / conv / upsample / dpt_tail / dpt_out on the `ops` module object heads_hip uses for its duration:
                     every call lands on the tape with its scalar arguments, references to its input tensors and its output (the references
                     keep the memory from being handed out again); production code is untouched
expected_schedule()  the launches one pass must make, written from the structure of the reference DPT head (heads/dpt_head.py), not from
                     heads_hip.py: 39 with the fused output stage, 41 with the three-launch form
check_tape()         a float64 reference of EVERY launch from that launch's own recorded inputs (so that 16-bit roundings do not accumulate
                     across stages), under the tensor-global gate of gpu_selftest AND kernel_guards.elementwise_budget / the rounding window,
                     with the constants kernel_guards.py derives; launches of more than 4096 GEMM rows are referenced on sample_rows()
"""
import contextlib
import inspect
import types

import torch
import torch.nn.functional as F

import gpu_selftest as st
import head_ops_emul as emul
import kernel_guards as kg

OPS = ("head_layernorm", "conv", "upsample", "dpt_tail", "dpt_out")
MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
HEAD_GATE = {"bf16": 4e-2, "f16": 6e-3, "f32": 1e-4}        # gpu_selftest.test_heads' gates of the whole head against the f32 PyTorch head
HEADS = {"depth": (2, "exp"), "point": (4, "inv_log")}
WINDOW_CAP = 0.10                                            # the share of a 16-bit resized map that may sit inside its rounding window
SAMPLE_ABOVE = 4096                                          # GEMM rows above which a convolution is referenced on a sample
TILE = 256                                                   # rows of an M tile of the 256-pixel kernels (two of the 128-pixel kernel's)
#        views, patch rows, patch columns (x 14 pixels). One-line grids: an even N, so that the first resize (N / 2 -> N samples, ratio
#        (N / 2 - 1) / (N - 1)) is not dyadic; with an odd N ((N + 1) / 2 -> N, ratio 1 / 2) every other sample is an exact midpoint of two
#        16-bit values and the rounding window holds 11 - 14 % of the map (measured with the emulation for N = 7 and 9; 1 - 2 % for 6, 8, 10, 12)
GRIDS = {"4x7": (2, 4, 7), "1x6": (2, 1, 6), "6x1": (2, 6, 1), "19x18": (3, 19, 18)}
CHUNK_ELEMS = 1 << 23                                        # resized maps above this are referenced image by image (memory only)


# =============================================================================================
# the tape
# =============================================================================================
class Launch:
    """One recorded call: op, scalars {name: value} (absent tensors are None here), tensors {name: tensor or tuple of tensors}, out."""

    def __init__(self, op, scalars, tensors, out):
        self.op, self.scalars, self.tensors, self.out = op, scalars, tensors, out

    def arg(self, name):
        return self.tensors[name] if name in self.tensors else self.scalars.get(name)


def _is_tensors(v):
    return torch.is_tensor(v) or (isinstance(v, (tuple, list)) and len(v) > 0 and all(torch.is_tensor(t) for t in v))


@contextlib.contextmanager
def recording(ops_mod, impl=None, mutate=None):
    """-> the tape (a list of Launch, filled while the block runs). impl: an object whose attributes of the same names serve the calls
    (None: the module's own entries), + dpt_tail_supported if it has one. mutate: {tape index: f(entry, *args, **kwargs) -> out} serves that
    one launch instead (the host test plants its defects through it)."""
    tape = []
    names = list(OPS) + (["dpt_tail_supported"] if impl is not None and hasattr(impl, "dpt_tail_supported") else [])
    saved = {k: getattr(ops_mod, k) for k in names}

    def wrap(op):
        sig = inspect.signature(saved[op])               # arguments are named after the production entry, whatever serves the call
        fn = saved[op] if impl is None else getattr(impl, op)

        def call(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            idx = len(tape)
            out = mutate[idx](fn, *a, **kw) if (mutate and idx in mutate) else fn(*a, **kw)
            scalars, tensors = {}, {}
            for k, v in bound.arguments.items():
                if k != "out":
                    (tensors if _is_tensors(v) else scalars)[k] = v
            tape.append(Launch(op, scalars, tensors, out))
            return out
        return call

    try:
        for op in OPS:
            setattr(ops_mod, op, wrap(op))
        if "dpt_tail_supported" in names:
            setattr(ops_mod, "dpt_tail_supported", impl.dpt_tail_supported)
        yield tape
    finally:
        for k, v in saved.items():
            setattr(ops_mod, k, v)


def _emul_dpt_tail(x, OH, OW, dtype, pos, w1, b1, w2, b2, activation):
    """The fused output stage as the three emulated launches it stands for."""
    up = emul.upsample(x, OH, OW, dtype, pos=pos)
    return emul.dpt_out(emul.conv(up, w1, b1, dtype, 32, ksize=3, relu=True, out_f32=True), w2, b2, activation)


EMUL = types.SimpleNamespace(head_layernorm=emul.head_layernorm, conv=emul.conv, upsample=emul.upsample, dpt_out=emul.dpt_out, dpt_tail=_emul_dpt_tail,
                             dpt_tail_supported=lambda x, dtype, OH=None, OW=None: dtype in (torch.bfloat16, torch.float16))


def rand_head(heads_mod, which, device="cpu"):
    """The sensitised DPTHead of gpu_selftest.test_heads: matrices x 1.6, biases uniform +-0.2, the last weight scaled to 0.2."""
    od, act = HEADS[which]
    torch.manual_seed(11 + od)
    head = heads_mod.DPTHead(dim_in=2048, output_dim=od, activation=act, conf_activation="expp1", intermediate_layer_idx=(0, 1, 2, 3)).eval()
    with torch.no_grad():
        for name, p in head.named_parameters():
            if p.dim() > 1:
                p.mul_(1.6)
            elif "bias" in name:
                p.uniform_(-0.2, 0.2)
        last = head.scratch.output_conv2[2]
        last.weight.mul_(0.2 / float(last.weight.abs().max()))
    return head.to(device)


def rand_tokens(S, ph, pw, seed=9):
    g = torch.Generator().manual_seed(seed)
    toks = [torch.randn(1, S, ph * pw + 5, 2048, generator=g) * 0.7 for _ in range(4)]
    return toks, torch.zeros(1, S, 3, ph * 14, pw * 14)


# =============================================================================================
# the expected schedule
# =============================================================================================
def expected_schedule(ph, pw, out_dim, fused, patch=14, dim_in=2048, features=256, oc=(256, 512, 1024, 1024)):
    """One pass over a ph x pw patch grid, in launch order: a list of dicts (name, op, ksize, stride, upshuffle, cin, cout, relu, adds, pos,
    bias, out_f32, out = the output map's (OH, OW), or (rows per view,) for the LayerNorm). From heads/dpt_head.py: four levels of
    norm -> projects[i] + position embedding -> resize_layers[i] (ConvTranspose 4 | ConvTranspose 2 | identity | 3x3 stride 2) -> layer{i+1}_rn
    (no bias; ReLU'd for the ResidualConvUnits that read it); refinenet4 (RCU, out_conv, resize); refinenet3..1 (RCU1 on the skip + the path,
    RCU2, out_conv, resize); output_conv1; the output stage (resize + position embedding, output_conv2, activation)."""
    S = []

    def add(name, op, cin, cout, out, ksize=0, stride=1, upshuffle=0, relu=False, adds=0, pos=False, bias=True, out_f32=False):
        S.append(dict(name=name, op=op, ksize=ksize, stride=stride, upshuffle=upshuffle, cin=cin, cout=cout, relu=relu, adds=adds, pos=pos,
                      bias=bias, out_f32=out_f32, out=tuple(out)))

    size = [(4 * ph, 4 * pw), (2 * ph, 2 * pw), (ph, pw), ((ph - 1) // 2 + 1, (pw - 1) // 2 + 1)]
    for i in range(4):
        add("level%d.norm" % i, "head_layernorm", dim_in, dim_in, (ph * pw,))
        add("level%d.project" % i, "conv", dim_in, oc[i], (ph, pw), ksize=1, pos=True)
        if i == 0:
            add("level0.resize_convT4", "conv", oc[0], oc[0], size[0], ksize=1, upshuffle=4)
        elif i == 1:
            add("level1.resize_convT2", "conv", oc[1], oc[1], size[1], ksize=1, upshuffle=2)
        elif i == 3:
            add("level3.resize_3x3s2", "conv", oc[3], oc[3], size[3], ksize=3, stride=2)
        add("layer%d_rn" % (i + 1), "conv", oc[i], features, size[i], ksize=3, relu=True, bias=False)

    def rcu(name, hw, path):
        add(name + ".conv1", "conv", features, features, hw, ksize=3, relu=True)
        add(name + ".conv2", "conv", features, features, hw, ksize=3, adds=2 if path else 1, relu=path)     # RCU1: + skip + path, ReLU'd for RCU2

    rcu("refinenet4.rcu2", size[3], False)
    add("refinenet4.out_conv", "conv", features, features, size[3], ksize=1)
    add("refinenet4.resize", "upsample", features, features, size[2])
    for lvl, hw, to in ((3, size[2], size[1]), (2, size[1], size[0]), (1, size[0], (2 * size[0][0], 2 * size[0][1]))):
        rcu("refinenet%d.rcu1" % lvl, hw, True)
        rcu("refinenet%d.rcu2" % lvl, hw, False)
        add("refinenet%d.out_conv" % lvl, "conv", features, features, hw, ksize=1)
        add("refinenet%d.resize" % lvl, "upsample", features, features, to)
    full = (ph * patch, pw * patch)
    add("output_conv1", "conv", features, features // 2, (2 * size[0][0], 2 * size[0][1]), ksize=3)
    if fused:
        add("output_stage", "dpt_tail", features // 2, out_dim, full, pos=True)
    else:
        add("output_stage.resize", "upsample", features // 2, features // 2, full, pos=True)
        add("output_conv2.0", "conv", features // 2, 32, full, ksize=3, relu=True, out_f32=True)
        add("output_conv2.2", "dpt_out", 32, out_dim, full)
    return S


def signature(launch):
    """What a tape entry says about itself, in the schedule's terms (without the name)."""
    a, op = launch.arg, launch.op
    d = dict(op=op, ksize=0, stride=1, upshuffle=0, relu=False, adds=0, pos=False, bias=True, out_f32=False)
    if op == "head_layernorm":
        d.update(cin=a("x").shape[-1], cout=launch.out.shape[-1], out=(a("tokens_per_view") - a("n_special"),))
    elif op == "conv":
        d.update(ksize=a("ksize"), stride=a("stride"), upshuffle=a("upshuffle"), cin=a("x").shape[-1], cout=a("cout"), relu=bool(a("relu")),
                 adds=int(a("add1") is not None) + int(a("add2") is not None), pos=a("pos") is not None, bias=a("bias") is not None,
                 out_f32=bool(a("out_f32")), out=tuple(launch.out.shape[1:3]))
    elif op == "upsample":
        d.update(cin=a("x").shape[-1], cout=launch.out.shape[-1], pos=a("pos") is not None, out=(a("OH"), a("OW")))
    elif op == "dpt_tail":
        d.update(cin=a("x").shape[-1], cout=a("w2").shape[0], pos=a("pos") is not None, out=(a("OH"), a("OW")))
    else:
        d.update(cin=a("h").shape[-1], cout=a("w2").shape[0], out=tuple(a("h").shape[1:3]))
    return d


def assert_schedule(tape, schedule):
    got = [signature(l) for l in tape]
    assert len(got) == len(schedule), "the pass made %d launches, the schedule has %d" % (len(got), len(schedule))
    for i, (g, s) in enumerate(zip(got, schedule)):
        want = {k: v for k, v in s.items() if k != "name"}
        assert g == want, "launch %d (%s): recorded %s, expected %s" % (i, s["name"], g, want)


# =============================================================================================
# sampled references
# =============================================================================================
def sample_rows(n, OH, OW, seed=0, tile=TILE, per_tile=8):
    """Flat GEMM rows (image-major, then y, then x) of an [n, OH, OW] output to reference: `per_tile` rows of every M tile with the tile's
    first and last row among them, the four corners of every image, the first row and column of the first image and the last row and column
    of the last, both sides of every image seam, and the whole last tile. Sorted, unique, int64."""
    M, hw = n * OH * OW, OH * OW
    nt = (M + tile - 1) // tile
    g = torch.Generator().manual_seed(seed)
    starts = torch.arange(nt) * tile
    inner = starts[:, None] + 1 + torch.rand(nt, tile - 2, generator=g).argsort(1)[:, : per_tile - 2]
    img0 = torch.arange(n) * hw
    last = img0[-1]
    picks = [starts, (starts + tile - 1).clamp_max(M - 1), inner.flatten(),
             img0, img0 + OW - 1, img0 + hw - OW, img0 + hw - 1,
             torch.arange(OW), torch.arange(OH) * OW, last + hw - OW + torch.arange(OW), last + torch.arange(OH) * OW + OW - 1,
             img0[1:] - 1, img0[1:], torch.arange((nt - 1) * tile, M)]
    rows = torch.unique(torch.cat(picks))
    return rows[rows < M]


def assert_sample_conditions(rows, n, OH, OW, tile=TILE, per_tile=8):
    """The sample is a condition of the check, not a tuning knob: asserted wherever a sampled reference is used."""
    M, hw = n * OH * OW, OH * OW
    has = torch.zeros(M, dtype=torch.bool)
    has[rows] = True
    nt = (M + tile - 1) // tile
    padded = torch.zeros(nt * tile, dtype=torch.bool)
    padded[:M] = has
    live = torch.full((nt,), tile)
    live[-1] = M - (nt - 1) * tile
    assert bool((padded.view(nt, tile).sum(1) >= torch.minimum(live, torch.tensor(per_tile))).all()), "a tile with fewer than %d sampled rows" % per_tile
    starts = torch.arange(nt) * tile
    assert bool(has[starts].all()) and bool(has[(starts + tile - 1).clamp_max(M - 1)].all()), "a tile's first or last row is missing"
    img0 = torch.arange(n) * hw
    for c in (img0, img0 + OW - 1, img0 + hw - OW, img0 + hw - 1):
        assert bool(has[c].all()), "an image corner is missing"
    assert bool(has[:OW].all()) and bool(has[torch.arange(OH) * OW].all()), "no full border row and column"
    assert bool(has[img0[1:] - 1].all()) and bool(has[img0[1:]].all()), "an image seam is missing"
    assert bool(has[(nt - 1) * tile:].all()), "the last tile is not whole"


def conv_ref_rows(x, w, bias, cout, k, stride, up, relu, a1, a2, pos, rows, out=None):
    """kernel_guards.conv_ref for the GEMM rows `rows` alone: the patches are gathered from the stored tensors (any dtype, on their device),
    the products are float64 torch matmuls on that device. -> (ref, mag [m, s, s, cout] float64, got [m, s, s, cout] gathered from `out` or
    None), s = up or 1: every GEMM column of a sampled row, i.e. all output channels of all pixels it scatters to."""
    n, H, W, cin = x.shape
    pd, s = k // 2, (up if up > 1 else 1)
    OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
    rows = rows.to(x.device)
    img, r = rows // (OH * OW), rows % (OH * OW)
    oy, ox = r // OW, r % OW
    xp = F.pad(x, (0, 0, pd, pd, pd, pd)) if pd else x
    patches = torch.stack([xp[img, oy * stride + ky, ox * stride + kx] for ky in range(k) for kx in range(k)], 1).reshape(rows.numel(), k * k * cin).double()
    wd = w[: s * s * cout].double()
    ref = (patches @ wd.t()).view(-1, s, s, cout)
    mag = (patches.abs() @ wd.abs().t()).view(-1, s, s, cout)
    I = img[:, None, None]
    OY = oy[:, None, None] * s + torch.arange(s, device=x.device)[None, :, None]
    OX = ox[:, None, None] * s + torch.arange(s, device=x.device)[None, None, :]
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    for t in (a1, a2):
        if t is not None:
            v = t[I, OY, OX].double()
            ref, mag = ref + v, mag + v.abs()
    if pos is not None:
        tab = torch.cat([pos[0].double()[OX].expand(-1, s, s, -1), pos[1].double()[OY].expand(-1, s, s, -1)], -1)
        ref, mag = ref + tab, mag + tab.abs()
    got = None if out is None else out[I, OY, OX].double()
    return (torch.relu(ref) if relu else ref), mag, got


# =============================================================================================
# one checker per entry
# =============================================================================================
def _global(name, got, ref, tol):
    assert st.report(name, got.detach().double().cpu(), ref.detach().cpu(), tol), name + ": over the tensor-global gate"


def _cpu64(t):
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return tuple(_cpu64(v) for v in t)
    return t.detach().double().cpu()


def check_conv(name, mode, x, w, bias, cout, k, stride, up, relu, a1, a2, pos, out_f32, out, seed=0, sampled=None):
    """One ovg_conv launch from its stored operands: the global gate and the per-element budget of test_gpu_edges.test_conv_small_maps_guarded
    (an implicit GEMM over k k Cin products + bias / tables / adds: up to 4 more sums). -> (used fraction, rows referenced, GEMM rows)."""
    n, H, W, cin = x.shape
    pd = k // 2
    OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
    M = n * OH * OW
    f32 = out_f32 or mode == "f32"
    u_out = kg.U_OUT["f32"] if f32 else kg.U_OUT[mode]
    gate = 2e-5 if out_f32 else st.TOL[mode]
    c = kg.gemm_c(k * k * cin, mode) + 4 * kg.MARGIN
    if (M > SAMPLE_ABOVE) if sampled is None else sampled:
        rows = sample_rows(n, OH, OW, seed)
        assert_sample_conditions(rows, n, OH, OW)
        ref, mag, got = conv_ref_rows(x, w, bias, cout, k, stride, up, relu, a1, a2, pos, rows, out)
        m = rows.numel()
    else:
        ref, mag = kg.conv_ref(_cpu64(x), _cpu64(w), _cpu64(bias), cout, k, stride, up, relu, _cpu64(a1), _cpu64(a2), _cpu64(pos))
        got, m = _cpu64(out), M
    _global(name, got, ref, gate)
    used = kg.elementwise_budget(name, got, ref, mag, u_out, c, extra=kg.f16_subnormal_floor(mode), quiet=True)
    return used, m, M


def _check_layernorm(name, mode, L):
    a = L.arg
    x = _cpu64(a("x")).reshape(a("views"), a("tokens_per_view"), -1)[:, a("n_special"):]
    ref, mag, c, extra = kg.layernorm_budget(x.reshape(-1, x.shape[-1]), _cpu64(a("weight")), _cpu64(a("bias")), a("eps"))
    got = _cpu64(L.out)
    assert bool(torch.isfinite(got).all()), name
    # as test_gpu_edges._ln_check: the dtype's gate + the mean's own rounding relative to the tensor maximum
    _global(name, got, ref, st.TOL[mode] + float(extra.max() / ref.abs().max().clamp_min(1e-30)))
    return kg.elementwise_budget(name, got, ref, mag, kg.U_OUT[mode], c, extra=extra + kg.f16_subnormal_floor(mode), quiet=True)


def _check_upsample(name, mode, L):
    """-> (used fraction, window share or None). f32: the budget of test_gpu_edges.test_upsample_edges_guarded (+ one sum for the table);
    16-bit: kernel_guards.upsample_window, bit-equal to the specification's rounding outside the window, an admissible rounding inside; the used
    fraction is then the part of the window's elements that do not hold the specification's own rounding."""
    a = L.arg
    x, OH, OW, pos, got = _cpu64(a("x")), a("OH"), a("OW"), _cpu64(a("pos")), _cpu64(L.out)
    n, H, W, C = x.shape
    if mode == "f32":
        ref = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()
        mag = x.abs().amax((1, 2), keepdim=True).expand(n, OH, OW, C).contiguous()
        c = kg.MARGIN * (8 * max(H, W) + 8)
        if pos is not None:
            half = C // 2
            ref[..., :half] += pos[0][None, None]
            ref[..., half:] += pos[1][None, :, None]
            mag[..., :half] += pos[0].abs()[None, None]
            mag[..., half:] += pos[1].abs()[None, :, None]
            c += kg.MARGIN
        _global(name, got, ref, st.TOL[mode])
        return kg.elementwise_budget(name, got, ref, mag, kg.U_OUT[mode], c, quiet=True), None
    step = n if n * OH * OW * C <= CHUNK_ELEMS else 1
    inside, differs, scale, err = 0.0, 0.0, 0.0, 0.0
    for i in range(0, n, step):
        win = kg.upsample_window(x[i:i + step], OH, OW, pos, mode)
        share, dshare = kg.check_upsampled_map("%s[%d:%d]" % (name, i, i + step), got[i:i + step], win)
        inside, differs = inside + share * step / n, differs + dshare * step / n
        scale, err = max(scale, float(win["up"].abs().max())), max(err, float((got[i:i + step] - win["up"]).abs().max()))
    used = differs / inside if inside > 0 else 0.0
    assert err <= st.TOL[mode] * scale, "%s: over the tensor-global gate (%.3e of %.3e)" % (name, err, scale)
    return used, inside


def _check_dpt_tail(name, mode, L, images):
    a = L.arg
    x = a("x")
    sel = list(range(x.shape[0])) if images is None else list(images)
    val, conf = L.out
    B = kg.dpt_tail_budget(_cpu64(x[sel]), a("OH"), a("OW"), _cpu64(a("pos")), _cpu64(a("w1")), _cpu64(a("b1")), _cpu64(a("w2")), _cpu64(a("b2")),
                           a("activation"), mode)
    val, conf = _cpu64(val[sel]), _cpu64(conf[sel])
    _global(name + ".val", val, B["val"], kg.DPT_TAIL_GATE[mode])
    _global(name + ".conf", conf, B["conf"], kg.DPT_TAIL_GATE[mode])
    return kg.check_dpt_tail(name, val, conf, B, quiet=True), float(B["win"]["window"].double().mean())


def _check_dpt_out(name, L):
    """The formula of test_gpu_edges.test_dpt_out_and_dpt_tail_small_maps_guarded: o carries (32 + 1) u mag_o, which exp turns into a
    relative error; the f32 exp itself within 4 ulp."""
    a = L.arg
    h, w2, b2, act = _cpu64(a("h")), _cpu64(a("w2")), _cpu64(a("b2")), a("activation")
    o = h @ w2.t() + b2
    m = h.abs() @ w2.abs().t() + b2.abs()
    val = torch.exp(o[..., :-1]) if act == "exp" else torch.sign(o[..., :-1]) * torch.expm1(o[..., :-1].abs())
    conf = 1 + torch.exp(o[..., -1])
    gv, gc = _cpu64(L.out[0]), _cpu64(L.out[1])
    _global(name + ".val", gv, val, 2e-5)
    _global(name + ".conf", gc, conf, 2e-5)
    return max(kg.elementwise_budget(name + ".val", gv, val, (val.abs() + 1) * (1 + m[..., :-1]), kg.U_OUT["f32"], kg.MARGIN * 41, quiet=True),
               kg.elementwise_budget(name + ".conf", gc, conf, conf.abs() * (1 + m[..., -1]), kg.U_OUT["f32"], kg.MARGIN * 41, quiet=True))


def check_tape(tape, schedule, mode, tail_images=None, collect=False, tag=""):
    """Every launch of the tape against the float64 reference of its own inputs. -> dict: worst {launch kind: the largest used fraction of
    a budget}, shares [(tape index, name, window share)] of the 16-bit resizes and the fused output stage, failures [(tape index, name,
    message)] (collect=True; otherwise the first failure is raised, naming the launch's tape index and schedule name), sampled
    [(tape index, name, rows referenced, GEMM rows)]."""
    worst, shares, failures, sampled = {}, [], [], []
    for i, (L, s) in enumerate(zip(tape, schedule)):
        name = "%s#%02d_%s" % (tag, i, s["name"])
        try:
            share = None
            if L.op == "head_layernorm":
                kind, used = "head_layernorm", _check_layernorm(name, mode, L)
            elif L.op == "conv":
                a = L.arg
                used, m, M = check_conv(name, mode, a("x"), a("w"), a("bias"), a("cout"), a("ksize"), a("stride"), a("upshuffle"), bool(a("relu")),
                                        a("add1"), a("add2"), a("pos"), bool(a("out_f32")), L.out, seed=i)
                kind = "conv f32 out" if a("out_f32") and mode != "f32" else "conv"
                if m != M:
                    sampled.append((i, s["name"], m, M))
            elif L.op == "upsample":
                kind = "upsample"
                used, share = _check_upsample(name, mode, L)
            elif L.op == "dpt_tail":
                kind = "dpt_tail"
                used, share = _check_dpt_tail(name, mode, L, tail_images)
            else:
                kind, used = "dpt_out", _check_dpt_out(name, L)
            worst[kind] = max(worst.get(kind, 0.0), used)
            if share is not None:
                shares.append((i, s["name"], share))
        except AssertionError as e:
            if not collect:
                raise AssertionError("launch %d (%s), %s: %s" % (i, s["name"], mode, e)) from e
            failures.append((i, s["name"], str(e)))
    return {"worst": worst, "shares": shares, "failures": failures, "sampled": sampled}


def run_recorded(heads_hip, hip, toks, images, dtype, impl=None, mutate=None, chunk=None):
    """One forward of `hip` (a HipDPTHead) under the recorder -> (tape, val, conf)."""
    with torch.no_grad(), recording(heads_hip.ops, impl=impl, mutate=mutate) as tape:
        val, conf = hip(toks, images, 5, dtype=dtype, frames_chunk_size=chunk if chunk else images.shape[1])
    return tape, val, conf
