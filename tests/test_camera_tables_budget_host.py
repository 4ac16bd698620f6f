"""CPU-only proof of kernel_guards.camera_tables_budget: the f32 host arithmetic (camera_math + F.linear) meets it on every case the GPU
test runs, and the defects the symmetric inputs of the older tests cannot see -- fov_h taken from fx, a missing scale clamp, a table row
scattered to the wrong view -- go over it."""
import pytest
import torch
import torch.nn.functional as F

import kernel_guards as kg
from omnivggt_official_amd import camera_math


def _twin(ext, intr, idx, weights, hw=kg.CAMERA_HW, swap_fov=False, clamp=True, shift_rows=0):
    pose_w, pose_b, adapt_w, adapt_b = weights
    B, S = ext.shape[:2]
    sel = torch.tensor(idx)
    e, k = torch.index_select(ext, 1, sel), torch.index_select(intr, 1, sel)
    if swap_fov:
        k = k.clone()
        k[..., 0, 0], k[..., 1, 1] = k[..., 1, 1].clone(), k[..., 0, 0].clone()
    if clamp:
        rel = camera_math.normalize_extrinsics(e)
    else:
        last = torch.zeros(B, len(idx), 1, 4)
        last[..., 3] = 1.0
        full = torch.cat([e, last], -2)
        rel = torch.matmul(full, camera_math.se3_inverse(full[:, 0]).unsqueeze(1))
        c = rel[:, :, :3, 3]
        s = torch.norm(c - c[:, :1], dim=-1)[:, 1:].mean(1, keepdim=True)
        rel[:, :, :3, 3] = c / s.unsqueeze(-1)
        rel = rel[:, :, :3]
    enc = camera_math.pose_encoding(rel, k, hw).reshape(-1, 9)
    G = adapt_b.shape[0]
    tables = adapt_b.unsqueeze(1).repeat(1, B * S, 1)
    rows = (torch.arange(B).unsqueeze(1) * S + (sel.unsqueeze(0) + shift_rows) % S).reshape(-1)
    for g in range(G):
        emb = F.linear(enc, pose_w[g * 1024:(g + 1) * 1024], pose_b[g * 1024:(g + 1) * 1024])
        tables[g, rows] = F.linear(emb, adapt_w[g], adapt_b[g])
    return enc, tables


@pytest.mark.parametrize("case", list(kg.CAMERA_CASES))
def test_host_arithmetic_meets_the_camera_budget(case):
    weights = kg.camera_weights()
    ext, intr, idx = kg.camera_inputs(case)
    Bd = kg.camera_tables_budget(ext, intr, idx, kg.CAMERA_HW, *weights)
    enc, tables = _twin(ext, intr, idx, weights)
    a, b = kg.check_camera_tables("camera_twin_" + case, enc, tables, Bd)
    print("camera_twin_%s: used %.3f of the encoding's budget, %.3f of the tables'; gap %.2f, w >= %.3f, e_s / scale %.3f" % (
        case, a, b, Bd["gap"], Bd["w"], Bd["es_rel"]), flush=True)
    # fov_h from fx instead of fy: invisible on fx = fy inputs
    enc, tables = _twin(ext, intr, idx, weights, swap_fov=True)
    with pytest.raises(AssertionError, match="over their budget"):
        kg.check_camera_tables("camera_swapped_fov_" + case, enc, tables, Bd, quiet=True)
    if len(idx) < ext.shape[1]:
        enc, tables = _twin(ext, intr, idx, weights, shift_rows=1)
        with pytest.raises(AssertionError):
            kg.check_camera_tables("camera_shifted_rows_" + case, enc, tables, Bd, quiet=True)
    if case.startswith("coincident"):
        enc, tables = _twin(ext, intr, idx, weights, clamp=False)
        with pytest.raises(AssertionError, match="over their budget"):
            kg.check_camera_tables("camera_no_clamp_" + case, enc, tables, Bd, quiet=True)
