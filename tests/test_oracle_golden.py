"""The CPU oracle against the committed golden vectors (sub-sampled outputs of the REAL
reference, produced by oracle/gen_golden.py in the build container).  In that container the
oracle matched the reference bit-for-bit (tests/golden/oracle_vs_reference_report.json)."""
import json
import os

import pytest
import torch

import aggregator_oracle as orc
import common


def test_reference_report_says_bit_exact():
    rep = json.load(open(os.path.join(common.GOLD, "oracle_vs_reference_report.json")))
    assert set(rep) == set(common.CASES)
    for case in rep.values():
        assert max(case["oracle_vs_reference_max_rel"].values()) <= 2e-5


@pytest.mark.parametrize("name", ["s2_images_only", "s3_partial_aux", "s2_full_aux", "s2_392x518_aux"])
def test_oracle_reproduces_reference_golden(name):
    S, dgi, cgi, hw = common.case(name)
    sd = common.full_state_dict()
    inp = orc.synthetic_inputs(S, hw=hw)
    torch.set_num_threads(min(32, os.cpu_count()))   # 256-thread intra-op on the GPU box is far slower than 32
    with torch.no_grad():
        out = orc.model_forward(sd, inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], dgi, cgi)
    gold = common.load_golden(name)
    # same torch build + same thread-independent kernels => bit-exact here; leave slack for other hosts
    tol = 1e-5
    for l in common.TOK_LAYERS:
        assert common.max_rel(common.sample_tokens(out["_tokens"], l), gold["tok_L%d" % l]) <= tol
    assert common.max_rel(out["pose_enc"], gold["pose_enc"]) <= tol
    assert common.max_rel(out["depth"][0, :, ::37, ::37, 0], gold["depth"]) <= tol
    assert common.max_rel(out["world_points"][0, :, ::37, ::37], gold["world_points"]) <= tol
    assert common.max_rel(out["depth_conf"][0, :, ::37, ::37], gold["depth_conf"]) <= tol
    absmean = [float(t.abs().mean()) for t in out["_tokens"]]
    assert common.max_rel(torch.tensor(absmean), gold["tok_absmean"]) <= tol


def test_sensitised_weights_make_the_trunk_visible():
    """with sensitised weights the AA blocks change the tokens substantially,
    so a wrong kernel cannot hide behind LayerScale=0.01."""
    gold = common.load_golden("s2_full_aux")
    am = gold["tok_absmean"]
    assert am[-1] > 1.2 * am[0] or am[-1] < 0.8 * am[0] or abs(am[12] - am[0]) > 0.1 * am[0]


def test_bf16_twin_fixtures_are_present_and_sane():
    """SURVEY 8c Gate 2: the reference under torch.autocast('cpu', bfloat16) (oracle/gen_golden_bf16twin.py) moves the
    sampled tokens by 5e-3..2e-2 against its own f32 run on these weights -- the yard-stick of the 16-bit GPU gates."""
    rep = json.load(open(os.path.join(common.GOLD, "bf16twin_report.json")))
    for name in ("s2_images_only", "s3_partial_aux", "s2_392x518_aux"):
        twin, gold = common.load_golden(name + "_bf16twin"), common.load_golden(name)
        for l in common.TOK_LAYERS:
            e = common.max_rel(twin["tok_L%d" % l], gold["tok_L%d" % l])
            assert 1e-3 < e < 5e-2, (name, l, e)
            assert abs(e - rep[name]["twin_vs_f32_reference"]["tok_L%d" % l]["max_rel"]) < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# Tiny and long patch grids (oracle/gen_golden_tiny.py): 14 x 14 (one patch) ... 14 x 1778 (the 127-patch RoPE limit)
# ----------------------------------------------------------------------------------------------------------------------
def test_tiny_case_tables_agree():
    import gen_golden_tiny as gt
    assert {k: (v[0], list(v[1]), list(v[2]), tuple(v[3])) for k, v in gt.TINY_CASES.items()} == \
           {k: (v[0], list(v[1]), list(v[2]), tuple(v[3])) for k, v in common.TINY_CASES.items()}
    assert set(common.TINY_TWIN_CASES) == set(gt.TINY_CASES) - set(gt.NO_TWIN)
    assert not set(common.TINY_CASES) & set(common.CASES)


def test_tiny_reference_report_says_bit_exact():
    rep = json.load(open(os.path.join(common.GOLD, "oracle_vs_reference_tiny.json")))
    assert set(rep) == set(common.TINY_CASES)
    for case in rep.values():
        assert len(case["oracle_vs_reference_max_rel"]) == 24 + 5
        assert max(case["oracle_vs_reference_max_rel"].values()) <= 2e-5


@pytest.mark.parametrize("name", list(common.TINY_CASES))
def test_oracle_reproduces_tiny_reference_golden(name):
    """All token rows of TOK_LAYERS, pose_enc and every refinement step of it, and the four dense maps whole (thinned along a
    1778-px side only) at the 1e-5 of the 518-class cases."""
    import gen_golden_tiny as gt
    S, dgi, cgi, hw = common.case(name)
    sd = common.full_state_dict()
    inp = orc.synthetic_inputs(S, hw=hw)
    torch.set_num_threads(min(32, os.cpu_count()))
    with torch.no_grad():
        out = orc.model_forward(sd, inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], dgi, cgi)
    gold = common.load_golden(name)
    got = gt.sample(out["_tokens"], out, hw, with_list=True)
    got["tok_absmean"] = torch.tensor([float(t.abs().mean()) for t in out["_tokens"]])
    P = (hw[0] // 14) * (hw[1] // 14) + 5
    assert gold["tok_L23"].shape == (S, P, 2048 // gt.chan_step(hw)) and gold["pose_enc_list"].shape == (4, 1, S, 9)
    assert gold["world_points"].shape == (S, len(gt.thin(hw[0])), len(gt.thin(hw[1])), 3)
    assert set(got) == set(gold)
    for k in gold:
        assert got[k].shape == gold[k].shape, k
        assert common.max_rel(got[k], gold[k]) <= 1e-5, k


def test_tiny_bf16_twin_fixtures_are_finite_and_in_range():
    """The reference under torch.autocast('cpu', bfloat16) at the tiny / long grids moves every stored tensor by 1e-3 .. 5e-2 against its own
    f32 run, like at 518 x 518; the one-column case has no twin (the CPU autocast reference is not finite there)."""
    import numpy as np
    rep = json.load(open(os.path.join(common.GOLD, "bf16twin_report.json")))
    assert not os.path.exists(os.path.join(common.GOLD, "t2_70x14_cam_bf16twin.npz")) and "t2_70x14_cam" not in rep
    for name in common.TINY_TWIN_CASES:
        twin, gold = common.load_golden(name + "_bf16twin"), common.load_golden(name)
        assert set(twin) == set(gold) - {"tok_absmean", "pose_enc_list"}
        for k in twin:
            assert np.isfinite(twin[k]).all(), (name, k)
            e = common.max_rel(twin[k], gold[k])
            assert 1e-3 < e < 5e-2, (name, k, e)
            assert abs(e - rep[name]["twin_vs_f32_reference"][k]["max_rel"]) < 1e-9
