"""The menu of tiny and long patch grids shared by test_gpu_small_grids.py and test_gpu_call_history.py, and the helpers
that run one item through OmniVGGT.forward and keep everything the call produced.

A 14 x 14 input is one patch and 6 tokens per view; 14 x 1778 / 1778 x 14 is the 127-patch limit of the RoPE table.  m6, m7
and m8 all have M = 66 tokens with different sequence lengths (the workspaces that share xn / attn / hid); m12 is the
trained 518 x 518 grid, which takes the packed pos_embed itself (call-history tests only)."""
import torch

import aggregator_oracle as orc
from omnivggt_official_amd import lib as L
from omnivggt_official_amd.model import OmniVGGT

DEV = "cuda"
DENSE = ("depth", "depth_conf", "world_points", "world_points_conf")

# id: (B, S, (H, W), depth_gt_index, camera_gt_index)
MENU = {
    "m1": (1, 1, (14, 14), [], []),                                  # smallest legal forward: 1 x 1 patches, 6 tokens
    "m2": (1, 2, (14, 14), [1], [0]),
    "m3": (1, 3, (14, 70), [0], [1]),                                # one row: 1 x 5
    "m4": (1, 2, (70, 14), [], [0, 1]),                              # one column: 5 x 1
    "m5": (1, 3, (28, 42), [1], [0, 2]),                             # 2 x 3, 11 tokens
    "m6": (1, 6, (28, 42), list(range(6)), list(range(6))),          # M = 66
    "m7": (2, 3, (28, 42), [1], [0, 2]),                             # M = 66: m6's frame key, another global sequence
    "m8": (1, 2, (56, 98), [0, 1], [0, 1]),                          # M = 66 again (4 x 7, 33 tokens): other sequence lengths
    "m9": (1, 4, (28, 42), [], []),                                  # bias-table cache
    "m10": (1, 2, (14, 1778), [1], [0]),                             # last RoPE row, x axis: 1 x 127, 132 tokens
    "m11": (1, 2, (1778, 14), [0], [0, 1]),                          # last RoPE row, y axis
    "m12": (1, 2, (518, 518), [1], []),                              # the trained grid
}
SMALL = tuple("m%d" % i for i in range(1, 12))                       # the items held to the oracle
MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32x": "f32x", "f32": torch.float32}


def build(sd, dtype, depth=2, dino_depth=2):
    """As test_gpu_aggregator.build."""
    with torch.device("meta"):
        m = OmniVGGT(depth=depth, dino_depth=dino_depth, compute_dtype=dtype)
    m = m.to_empty(device="cpu")
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def cpu_inputs(B, S, hw):
    """B = 1: orc.synthetic_inputs; B = 2: two different scenes, as test_batch_of_two_scenes_depth2 builds them."""
    if B == 1:
        return orc.synthetic_inputs(S, hw=hw)
    parts = [orc.synthetic_inputs(S, seed=1234 + 1111 * b, hw=hw) for b in range(B)]
    return {k: torch.cat([q[k] for q in parts], 0) for k in parts[0]}


_DEVICE_INPUTS = {}


def device_inputs(B, S, hw):
    key = (B, S, tuple(hw))
    if key not in _DEVICE_INPUTS:
        _DEVICE_INPUTS[key] = {k: v.to(DEV) for k, v in cpu_inputs(B, S, hw).items()}
    return _DEVICE_INPUTS[key]


def forward_raw(m, inp, dgi, cgi):
    """One OmniVGGT.forward; -> (aggregator layers, the prediction dict). The layers are taken by a forward hook of the aggregator
    module: the call itself is the model's, heads and all. No synchronisation."""
    got = {}
    h = m.aggregator.register_forward_hook(lambda mod, args, out: got.update(toks=out[0]))
    try:
        with torch.no_grad():
            out = m(inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], list(dgi), list(cgi))
    finally:
        h.remove()
    return got["toks"], out


def forward(m, inp, dgi, cgi):
    """-> {name: DEVICE tensor} of everything the call produced: every aggregator layer, every entry of pose_enc_list and the four
    dense maps."""
    toks, out = forward_raw(m, inp, dgi, cgi)
    res = {"tok_L%d" % l: t for l, t in enumerate(toks)}
    res.update({"pose_%d" % i: p for i, p in enumerate(out["pose_enc_list"])})
    res.update({k: out[k] for k in DENSE})
    return res


def run_item(m, item):
    B, S, hw, dgi, cgi = MENU[item]
    return forward(m, device_inputs(B, S, hw), dgi, cgi)


def to_host(res):
    return {k: v.cpu() for k, v in res.items()}


def same_bytes(a, b):
    """Names of the tensors of two results that differ in any byte (shape, dtype or an int32 view of the payload)."""
    bad = [k for k in a if k not in b] + [k for k in b if k not in a]
    for k in a:
        if k in b and not (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
                           and torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32))):
            bad.append(k)
    return bad


def oracle_item(sd, item, depth=2, dino_depth=2):
    """The depth-2 CPU oracle's result of a menu item, under the names of forward()."""
    B, S, hw, dgi, cgi = MENU[item]
    inp = cpu_inputs(B, S, hw)
    with torch.no_grad():
        ref = orc.model_forward(sd, inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], list(dgi), list(cgi),
                                depth_layers=depth, dino_layers=dino_depth)
    res = {"tok_L%d" % l: t for l, t in enumerate(ref["_tokens"])}
    res.update({"pose_%d" % i: p for i, p in enumerate(ref["pose_enc_list"])})
    res.update({k: ref[k] for k in DENSE})
    return res


def mode_dtype(tag):
    return L.F32X if tag == "f32x" else MODES[tag]
