"""-m gpu: whole forwards at the smallest and the longest patch grids against the depth-2 CPU oracle.

Every GPU test of the model so far used 518^2, 392 x 518, 518 x 392 or 266^2.  set_geometry accepts any multiple of 14 up to
1778 px, and so does the reference.  At 14 x 14 (one patch, 6 tokens per view) frame attention sits inside one 64-row tile, the
pos_embed resample goes to 1 x 1 / 1 x 5 / 5 x 1, RoPE has gh = 1 or gw = 1, the DPT pyramid runs on 1 x 1 / 4 x 4 / 8 x 8 maps
(its bilinear steps then have a one-pixel output side), the fused DPT tail may fall back to its three-launch form and the
camera head sees S = 1; 14 x 1778 and 1778 x 14 read the last RoPE row (position 127).  The kernels are pinned alone at such
sizes elsewhere; this file pins the Python that sizes, pads and chains them: every call goes through OmniVGGT.forward with the
HIP heads, concurrent_heads and early_dpt_levels at their defaults.

Gates, per tensor as common.max_rel (every aggregator layer, its camera-token rows, the last patch row of the last view and the
last view as a whole, every entry of pose_enc_list, the four dense maps):
  f32, f32x : <= 1e-4 (the modes' contract, DESIGN sections 2 and 7)
  bf16, f16 : finite, <= 3e-2 / <= 5e-3 (the rule for 16-bit modes outside the full-depth twin cases)
"""
import os

import pytest
import torch
import torch.nn.functional as F

import common
import small_grids as sg
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops

pytestmark = pytest.mark.gpu
TOL = {"f32": 1e-4, "f32x": 1e-4, "bf16": 3e-2, "f16": 5e-3}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    L.require_gpu()
    torch.set_num_threads(min(32, os.cpu_count()))


@pytest.fixture(scope="module")
def sd():
    return common.reduced_state_dict(2, 2)


@pytest.fixture(scope="module")
def oracle(sd):
    """item -> the depth-2 oracle's result, computed once per item and shared by the four modes."""
    cache = {}

    def get(item):
        if item not in cache:
            cache[item] = sg.oracle_item(sd, item)
        return cache[item]
    return get


@pytest.fixture(scope="module")
def models(sd):
    """mode -> one depth-2 model per module: the items run on it one after the other, m1 first."""
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = sg.build(sd, sg.mode_dtype(tag))
        return cache[tag]
    return get


def gated_errors(got, ref):
    """{name: max-rel} of every gated tensor of one call."""
    errs = {}
    for k, r in ref.items():
        assert got[k].shape == r.shape and got[k].dtype == torch.float32, k
        errs[k] = common.max_rel(got[k], r)
        if k.startswith("tok_"):
            t = got[k]
            errs[k + ".camera_rows"] = common.max_rel(t[:, :, 0], r[:, :, 0])           # the camera token of every view
            errs[k + ".last_patch_row"] = common.max_rel(t[:, -1, -1], r[:, -1, -1])    # last patch of the last view: the last RoPE position
            errs[k + ".last_view"] = common.max_rel(t[:, -1], r[:, -1])
    return errs


@pytest.mark.parametrize("item", sg.SMALL)
@pytest.mark.parametrize("tag", ["f32", "f32x", "bf16", "f16"])
def test_menu_item_vs_depth2_oracle(models, oracle, tag, item):
    B, S, hw, dgi, cgi = sg.MENU[item]
    ref = oracle(item)
    m = models(tag)
    got = sg.to_host(sg.run_item(m, item))
    assert m.aggregator.layer_hook is None
    P = (hw[0] // 14) * (hw[1] // 14) + 5
    assert got["tok_L1"].shape == (B, S, P, 2048) and got["depth"].shape == (B, S, hw[0], hw[1], 1)
    for k, v in got.items():
        assert torch.isfinite(v).all(), (tag, item, k)
    errs = gated_errors(got, ref)
    worst = max(errs, key=errs.get)
    print("%s %s %s: worst %s %.2e; tokens %.2e pose %.2e depth %.2e points %.2e (gate %.0e)"
          % (item, sg.MENU[item], tag, worst, errs[worst], max(errs["tok_L0"], errs["tok_L1"]), errs["pose_3"], errs["depth"],
             errs["world_points"], TOL[tag]))
    assert errs[worst] <= TOL[tag], (tag, item, {k: "%.2e" % v for k, v in errs.items() if v > TOL[tag]})


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_geometry_limit_is_refused_and_changes_nothing(models, tag):
    """127 patches per side is the last RoPE row: 14 x 1792 and 1792 x 14 are refused with ValueError before anything is packed, sized or
    queued -- the geometry, the workspaces and the outputs of the call before stay as they were, and the next forward gives its bytes again."""
    m = models(tag)
    agg = m.aggregator
    before_dev = sg.run_item(m, "m5")
    before = sg.to_host(before_dev)
    state = (agg.grid_hw, agg.n_patches, agg.tokens_per_view, [(k, id(w), w.xn is not None) for k, w in agg._ws.items()],
             sorted(str(k) for k in agg._packed))
    for hw in ((14, 1792), (1792, 14)):
        with pytest.raises(ValueError, match="1778"):
            agg.set_geometry(*hw)
        inp = sg.device_inputs(1, 2, hw)
        with pytest.raises(ValueError, match="1778"):
            sg.forward(m, inp, [1], [0])
        assert agg.layer_hook is None
        now = (agg.grid_hw, agg.n_patches, agg.tokens_per_view, [(k, id(w), w.xn is not None) for k, w in agg._ws.items()],
               sorted(str(k) for k in agg._packed))
        assert now == state
    torch.cuda.synchronize()
    assert sg.same_bytes(sg.to_host(before_dev), before) == []          # the tensors the earlier call handed out
    assert sg.same_bytes(sg.to_host(sg.run_item(m, "m5")), before) == []
    assert agg.set_geometry(14, 1778) == (1, 127) and agg.set_geometry(1778, 14) == (127, 1)


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
def test_bilinear_resize_to_one_pixel_sides(tag):
    """ovg_upsample with OH == 1 or OW == 1 -- the fusion steps of the DPT pyramid on a one-row / one-column patch grid -- takes source
    row / column 0 like F.interpolate(align_corners=True); a 16-bit result is the rounding of one input value or of a lerp along the other axis."""
    dt = sg.MODES[tag]
    g = torch.Generator().manual_seed(5)
    for (H, W), (OH, OW) in (((1, 1), (1, 1)), ((1, 3), (1, 5)), ((3, 1), (5, 1)), ((2, 3), (1, 5)), ((3, 2), (5, 1)), ((1, 32), (1, 127))):
        x = torch.randn(2, H, W, 256, generator=g).to(dt)
        want = F.interpolate(x.double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        got = ops.upsample(x.to(sg.DEV), OH, OW, dt)
        torch.cuda.synchronize()
        assert got.shape == (2, OH, OW, 256)
        err = common.max_rel(got.cpu().double(), want)
        # the source coordinate ox * (W - 1) / (OW - 1) is formed in f32: two roundings of a value up to W - 1 move the lerp weight by
        # 2 (W - 1) 2^-24, which weighs a difference of up to 2 max|x|; the lerp itself adds a few roundings (8 allowed). The 16-bit
        # modes round the result once more (unit roundoff 2^-8 / 2^-11).
        f32_part = (4 * (max(H, W) - 1) + 8) * 2.0 ** -24
        assert err <= f32_part + {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[tag], ((H, W), (OH, OW), err)
