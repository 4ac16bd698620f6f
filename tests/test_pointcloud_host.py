"""Point-cloud extraction, host side: the CPU twin (tests/pointcloud_twin.py) against the golden outputs of the REAL reference export
(tools/gen_golden_pointcloud.py -> tests/golden/pointcloud.npz), the numpy index rule it restates, the C ABI without a device, the
Python API's argument checks and the PLY / GLB writers."""
import ctypes
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import common
import pointcloud_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")


def golden():
    g = dict(np.load(os.path.join(common.GOLD, "pointcloud.npz")))
    return g, json.loads(str(g["cases"]))


def case_inputs(g, case):
    """(points, conf, images, extrinsic, sky) of one golden case, batch dimension squeezed, as the reference saw them."""
    m = case["map"]
    if case["mode"] == "Predicted Depth":
        pts, conf = g[m + "_world_points_from_depth"], g[m + "_depth_conf"]
    else:
        pts, conf = g[m + "_world_points"], g[m + "_world_points_conf"]
    return pts, conf, g[m + "_images"], g[m + "_extrinsic"]


def test_twin_reproduces_reference_golden_bit_exactly():
    g, cases = golden()
    assert len(cases) >= 25
    for i, case in enumerate(cases):
        p = "c%d_" % i
        pts, conf, img, ext = case_inputs(g, case)
        tw = twin.select(pts, conf, img, ext, conf_thres=case["conf_thres"], frame=twin.parse_frame(case["filter_by_frames"]),
                         mask_black_bg=case["mask_black_bg"], mask_white_bg=case["mask_white_bg"], sky_mask=g.get(p + "sky"))
        name = case["name"]
        assert np.array_equal(tw["indices"], g[p + "indices"].astype(np.int64)), name
        assert np.array_equal(tw["colors"], g[p + "colors"]), name
        assert tw["conf_threshold"].tobytes() == g[p + "threshold"].tobytes() or \
            (np.isnan(tw["conf_threshold"]) and np.isnan(g[p + "threshold"])), name
        if case["empty"]:                                              # the reference's stand-in cloud has scene_scale = 1 (a Python int)
            assert float(tw["scene_scale"]) == float(g[p + "scene_scale"]) == 1.0, name
        else:
            assert np.asarray(tw["scene_scale"]).tobytes() == g[p + "scene_scale"].tobytes(), (name, tw["scene_scale"], g[p + "scene_scale"])
        assert np.abs(tw["transform"] - g[p + "transform"]).max() <= 1e-12, name
        assert case["empty"] == (tw["indices"].size == 0), name
    names = " ".join(c["name"] for c in cases)
    for needle in ("conf_thres=None", "ties", "min_conf", "inf 100", "nan", "black bg", "white bg", "sky", "frame", "depth"):
        assert needle in names, needle


def test_index_rule_is_numpys_f32_rule_not_the_f64_one():
    """numpy 2 forms the virtual index in f32 for f32 data: at 64 x 518^2 keys that picks other order statistics than the f64 rule."""
    n = 64 * 518 * 518
    rng = np.random.default_rng(7)
    x = rng.random(n, dtype=np.float32)
    f64_differs = False
    for p in (25.0, 37.3, 50.0, 99.9, 100.0):
        want = np.percentile(x, p)
        assert want.dtype == np.float32
        assert twin.percentile(x, [p])[0].tobytes() == want.tobytes(), p
        lo, hi, gamma = twin.index_rule(n, p)
        vi64 = (n - 1) * (p / 100.0)
        f64_differs |= (lo, float(gamma)) != (int(np.floor(vi64)), float(np.float32(vi64 - np.floor(vi64))))
    assert twin.index_rule(n, 50.0)[0::2] == (8586368, 0.0)           # the f64 rule says 8586367.5: lo 8586367, gamma 0.5
    assert f64_differs


def test_ctypes_struct_layout_matches_c_pointcloud():
    pairs = {"ovg_percentile_params": L.PercentileParams, "ovg_point_filter_params": L.PointFilterParams}
    src = '#include <stdio.h>\n#include "%s"\nint main(){\n' % HEADER
    for name in pairs:
        src += 'printf("%s %%zu\\n", sizeof(%s));\n' % (name, name)
    src += 'printf("maxcols %d\\nmaxq %d\\n", OVG_PCT_MAX_COLS, OVG_PCT_MAX_Q);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        sizes = dict(line.split() for line in subprocess.check_output([exe]).decode().strip().splitlines())
    for name, cls in pairs.items():
        assert int(sizes[name]) == ctypes.sizeof(cls), name
    assert int(sizes["maxcols"]) == L.PCT_MAX_COLS and int(sizes["maxq"]) == L.PCT_MAX_Q


def test_pointcloud_argument_validation_without_gpu():
    lib = L.load()
    big = 1 << 40                                                      # fake, never dereferenced: every call below fails its checks
    ws_need = lib.ovg_percentile_workspace_bytes(1000, 1)
    assert ws_need > 0 and lib.ovg_percentile_workspace_bytes(1000, 4) > ws_need
    assert lib.ovg_percentile_workspace_bytes((1 << 31) + 5, 3) == lib.ovg_percentile_workspace_bytes(10, 3) > 0
    for n, c in ((0, 1), (-1, 1), (10, 0), (10, 5)):
        assert lib.ovg_percentile_workspace_bytes(n, c) == -1
    pf = lib.ovg_point_filter_workspace_bytes
    n = (1 << 31) + 7
    assert pf(n) >= n + 2 * 8 * ((n + 4095) // 4096) and pf(0) == -1 and pf(-3) == -1

    def pct(**kw):
        p = L.PercentileParams(x=big, n=1000, stride=1, col_stride=0, ncols=1, nq=1, out=big, ws=big, ws_bytes=ws_need)
        p.q[0] = 50.0
        for k, v in kw.items():
            if k == "q":
                p.q[0] = v
            else:
                setattr(p, k, v)
        return lib.ovg_percentile(ctypes.byref(p), None)

    assert lib.ovg_percentile(None, None) == -1
    for bad in (dict(x=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=-5), dict(ncols=0), dict(ncols=5), dict(nq=0), dict(nq=5),
                dict(ws_bytes=ws_need - 1), dict(q=100.5), dict(q=-1.0), dict(q=float("nan")), dict(stride=0), dict(norm_out=big),
                dict(ws=big + 4)):
        assert pct(**bad) == -1, bad

    def filt(**kw):
        p = L.PointFilterParams(conf=big, images=big, points=big, n=4096, hw=1024, stage=L.PF_COUNT, out_count=big, ws=big,
                                ws_bytes=pf(4096))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_point_filter(ctypes.byref(p), None)

    assert lib.ovg_point_filter(None, None) == -1
    for bad in (dict(conf=None), dict(images=None), dict(points=None), dict(ws=None), dict(n=0), dict(hw=0), dict(hw=1000),
                dict(stage=0), dict(stage=4), dict(out_count=None), dict(flags=4), dict(ws_bytes=pf(4096) - 1),
                dict(stage=L.PF_SCATTER), dict(stage=L.PF_SCATTER, out_points=big, out_colors=big, capacity=-1)):
        assert filt(**bad) == -1, bad


def _cpu_predictions(S=2, H=6, W=8):
    return {"world_points": torch.zeros(1, S, H, W, 3), "world_points_conf": torch.ones(1, S, H, W), "images": torch.rand(1, S, 3, H, W),
            "extrinsic": torch.eye(4)[:3].repeat(1, S, 1, 1)}


def test_pointcloud_api_rejects_cpu_tensors_and_bad_arguments():
    pred = _cpu_predictions()
    with pytest.raises(L.OvgError):
        postprocess.predictions_to_point_cloud(pred)
    with pytest.raises(L.OvgError):
        postprocess.percentile(torch.rand(100), 50)
    with pytest.raises(L.OvgError):
        postprocess.get_world_points_from_depth({"depth": torch.ones(1, 2, 4, 4, 1), "pose_enc": torch.zeros(1, 2, 9),
                                                 "images": torch.zeros(1, 2, 3, 4, 4)})
    with pytest.raises(ValueError):
        postprocess.predictions_to_point_cloud(pred, sky_mask=torch.ones(2, 6, 7))
    with pytest.raises(ValueError):
        postprocess.predictions_to_point_cloud(pred, sky_mask=torch.ones(6, 8))
    for b in (1, -1, 0.0):
        with pytest.raises(ValueError):
            postprocess.predictions_to_point_cloud(pred, batch_index=b)
    with pytest.raises(ValueError):
        postprocess.predictions_to_point_cloud([pred])


class _HostCloud:
    def __init__(self, pts, col, transform):
        self.points, self.colors, self.transform = torch.from_numpy(pts), torch.from_numpy(col), transform


def _read_ply(path):
    data = open(path, "rb").read()
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    m = int(lines[2].split()[-1])
    assert lines[3:9] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                          "property uchar blue"]
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    assert rec.size == m and len(body) == 15 * m
    return np.stack([rec["x"], rec["y"], rec["z"]], 1), np.stack([rec["r"], rec["g"], rec["b"]], 1)


def _read_glb(path):
    data = open(path, "rb").read()
    magic, version, length = struct.unpack_from("<III", data, 0)
    assert magic == 0x46546C67 and version == 2 and length == len(data)
    jl, jt = struct.unpack_from("<II", data, 12)
    assert jt == 0x4E4F534A and jl % 4 == 0
    gltf = json.loads(data[20:20 + jl])
    binary = b""
    if 20 + jl < len(data):
        bl, bt = struct.unpack_from("<II", data, 20 + jl)
        assert bt == 0x004E4942 and bl % 4 == 0 and 28 + jl + bl == len(data)
        binary = data[28 + jl:28 + jl + bl]
    return gltf, binary


@pytest.mark.parametrize("M", [0, 1, 37])
def test_ply_and_glb_writers_round_trip(M, tmp_path):
    rng = np.random.default_rng(M)
    pts = rng.standard_normal((M, 3)).astype(np.float32)
    col = rng.integers(0, 256, (M, 3)).astype(np.uint8)
    ext = np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], 1)
    T = twin.alignment(ext)
    assert np.allclose(postprocess.scene_alignment(ext), T, rtol=0, atol=1e-12)
    cloud = _HostCloud(pts, col, T)
    postprocess.write_ply(str(tmp_path / "a.ply"), cloud, apply_transform=False)
    p, c = _read_ply(str(tmp_path / "a.ply"))
    assert np.array_equal(p, pts) and np.array_equal(c, col)
    postprocess.write_ply(str(tmp_path / "b.ply"), cloud)
    p, c = _read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(p, (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)) and np.array_equal(c, col)
    postprocess.write_glb(str(tmp_path / "c.glb"), cloud)
    gltf, binary = _read_glb(str(tmp_path / "c.glb"))
    assert gltf["asset"]["version"] == "2.0"
    node = gltf["nodes"][gltf["scenes"][gltf["scene"]]["nodes"][0]]
    assert np.array_equal(np.array(node["matrix"]).reshape(4, 4).T, T)          # column-major
    if M == 0:
        assert "mesh" not in node and binary == b""
        return
    prim = gltf["meshes"][node["mesh"]]["primitives"][0]
    assert prim["mode"] == 0
    pa, ca = gltf["accessors"][prim["attributes"]["POSITION"]], gltf["accessors"][prim["attributes"]["COLOR_0"]]
    assert pa["count"] == ca["count"] == M and pa["componentType"] == 5126 and pa["type"] == "VEC3"
    assert ca["componentType"] == 5121 and ca["normalized"] is True and ca["type"] == "VEC4"
    assert pa["min"] == [float(v) for v in pts.min(0)] and pa["max"] == [float(v) for v in pts.max(0)]
    pv, cv = gltf["bufferViews"][pa["bufferView"]], gltf["bufferViews"][ca["bufferView"]]
    assert pv["byteOffset"] % 4 == 0 and cv["byteOffset"] % 4 == 0 and gltf["buffers"][0]["byteLength"] <= len(binary)
    got_p = np.frombuffer(binary, "<f4", 3 * M, pv["byteOffset"]).reshape(M, 3)
    got_c = np.frombuffer(binary, "u1", 4 * M, cv["byteOffset"]).reshape(M, 4)
    assert np.array_equal(got_p, pts) and np.array_equal(got_c[:, :3], col) and (got_c[:, 3] == 255).all()
