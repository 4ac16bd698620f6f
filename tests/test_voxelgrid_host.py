"""Voxel-grid decimation, host side: the numpy twin (tests/voxelgrid_twin.py) on hand-made cases, the C ABI without a device (struct
layout, argument checks that return before any HIP call), the Python API's argument checks, and the camera frusta of write_glb."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

import abi_layout
import voxelgrid_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

F = np.float32


def _keep(points, v, conf=None):
    return twin.downsample(np.asarray(points, F), F(v), None if conf is None else np.asarray(conf, F)).tolist()


def test_twin_two_points_in_one_cell():
    pts = [[0.0, 0.0, 0.0], [0.1, 0.2, 0.3], [1.5, 0.0, 0.0]]
    assert _keep(pts, 1.0) == [0, 2]                                       # without conf: the earliest point of the cell
    assert _keep(pts, 1.0, [1.0, 2.0, 0.5]) == [1, 2]                      # the larger conf
    assert _keep(pts, 1.0, [2.0, 2.0, 0.5]) == [0, 2]                      # equal conf: the smaller index
    assert _keep(pts, 1.0, [-3.0, -2.0, 0.5]) == [1, 2]                    # negative values order as numbers
    assert _keep(pts, 1.0, [-0.0, 0.0, 0.5]) == [0, 2]                     # -0 == +0: a tie
    assert _keep(pts, 1.0, [-np.inf, -1e30, 0.5]) == [1, 2]


def test_twin_point_on_a_cell_face():
    # (p - o) / v an exact integer belongs to the upper cell: floor(2.0) = 2
    pts = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.4999999, 0.0, 0.0], [1.0, 0.0, 0.0], [0.75, 0.0, 0.0]]
    _, origin, c = twin.cells(np.asarray(pts, F), F(0.25))
    assert origin.tolist() == [0.0, 0.0, 0.0] and c[:, 0].tolist() == [0, 2, 1, 4, 3]
    assert _keep(pts, 0.5) == [0, 1, 3]                                    # cells 0, 1, 0, 2, 1
    # the quotient is numpy's own correctly rounded f32 division
    q = np.floor((F(0.3) - F(0.0)) / F(0.1))
    assert twin.cells(np.asarray([[0, 0, 0], [0.3, 0, 0]], F), F(0.1))[2][1, 0] == int(q)


def test_twin_non_finite_coordinates_and_nan_conf():
    pts = [[np.nan, 0, 0], [5.0, 5.0, 5.0], [np.inf, 5, 5], [5.2, 5.1, 5.0], [5, -np.inf, 5], [-1.0, -1.0, -1.0]]
    valid, origin, _ = twin.cells(np.asarray(pts, F), F(1.0))
    assert valid.tolist() == [False, True, False, True, False, True] and origin.tolist() == [-1.0, -1.0, -1.0]
    assert _keep(pts, 1.0) == [1, 5]
    assert _keep(pts, 1.0, [9, np.nan, 9, 0.5, 9, np.nan]) == [3, 5]       # NaN conf is the lowest; alone in its cell it still wins
    assert _keep(pts, 1.0, [9, np.nan, 9, np.nan, 9, 1]) == [1, 5]         # two NaN: the smaller index
    assert _keep(pts, 1.0, [9, np.nan, 9, -np.inf, 9, 1]) == [3, 5]        # -inf is above NaN
    assert _keep([[np.nan, 0, 0], [0, np.inf, 0]], 1.0) == []


def test_twin_negative_coordinates_single_point_and_empty():
    pts = [[-3.5, -2.0, -7.25], [-3.4, -1.9, -7.2], [-1.0, -2.0, -7.25], [-3.5, 4.0, -7.25]]
    assert _keep(pts, 0.5) == [0, 2, 3]
    assert _keep(pts, 100.0) == [0]
    assert _keep(pts, 0.01) == [0, 1, 2, 3]
    assert _keep([[1e30, -1e30, 0.0]], 1e-3) == [0]                        # a single point is its own origin: cell 0
    assert _keep(np.zeros((0, 3)), 1.0) == []
    with pytest.raises(twin.Overflow):
        _keep([[0, 0, 0], [3.0, 0, 0]], 1e-6)                              # 3e6 cells > 2^21 - 1
    assert _keep([[0, 0, 0], [2097151.0, 0, 0]], 1.0) == [0, 1]            # the last cell that fits
    with pytest.raises(twin.Overflow):
        _keep([[0, 0, 0], [2097152.0, 0, 0]], 1.0)
    with pytest.raises(twin.Overflow):
        _keep([[-3e38, 0, 0], [3e38, 0, 0]], 1.0)                          # the extent itself overflows f32
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            _keep(pts, bad)


def test_twin_properties_on_a_random_cloud():
    rng = np.random.default_rng(11)
    pts = (rng.standard_normal((5000, 3)) * 2).astype(F)
    pts[rng.integers(0, 5000, 40)] = pts[rng.integers(0, 5000, 40)]        # duplicates
    conf = np.floor(rng.random(5000) * 8).astype(F)                         # many ties
    v = F(0.37)
    keep = twin.downsample(pts, v, conf)
    _, _, c = twin.cells(pts, v)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    assert np.all(np.diff(keep) > 0) and len(np.unique(key[keep])) == len(keep) == len(np.unique(key))
    for i in keep[:200]:
        same = np.nonzero(key == key[i])[0]
        best = same[conf[same] == conf[same].max()][0]
        assert best == i
    assert twin.voxel_from_rel(0.01, F(3.7)).dtype == np.float32


def test_ctypes_struct_layout_matches_c_voxelgrid():
    enums, _ = abi_layout.check({"ovg_voxel_downsample_params": L.VoxelDownsampleParams},
                                ["OVG_VG_COUNT", "OVG_VG_SCATTER", "OVG_VG_OVERFLOW", "OVG_VG_BAD_VOXEL", "OVG_ABI_VERSION"])
    assert enums == [L.VG_COUNT, L.VG_SCATTER, L.VG_OVERFLOW, L.VG_BAD_VOXEL, L.ABI_VERSION]


def test_voxelgrid_argument_validation_without_gpu():
    lib = L.load()
    q = lib.ovg_voxel_downsample_workspace_bytes
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    assert q(0) == -1 and q(-4) == -1 and q(1 << 32) == -1 and q((1 << 32) + 5) == -1
    n = 64 * 518 * 518
    assert q(n) >= 2 * n * 16 + n and q(1) >= 1024 * 16 and q((1 << 32) - 1) > 0
    assert q(n + 1) >= q(n)

    def run(**kw):
        p = L.VoxelDownsampleParams(points=big, voxel=big, n=4096, stage=L.VG_COUNT, out_count=big, ws=big, ws_bytes=q(4096))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_voxel_downsample(ctypes.byref(p), None)

    assert lib.ovg_voxel_downsample(None, None) == -1
    scatter = dict(stage=L.VG_SCATTER, out_points=big)
    for bad in (dict(points=None), dict(voxel=None), dict(ws=None), dict(n=0), dict(n=-1), dict(n=1 << 32, ws_bytes=1 << 50),
                dict(n=(1 << 32) + 9, ws_bytes=1 << 50), dict(stage=0), dict(stage=4), dict(stage=-1), dict(out_count=None),
                dict(ws_bytes=q(4096) - 1), dict(ws_bytes=0), dict(ws=big + 4), dict(stage=L.VG_SCATTER),
                dict(scatter, capacity=-1), dict(scatter, colors=big), dict(scatter, out_colors=big),
                dict(stage=L.VG_COUNT | L.VG_SCATTER), dict(n=8192)):
        assert run(**bad) == -1, bad


class _Cloud:
    def __init__(self, M=10, S=3, seed=0):
        rng = np.random.default_rng(seed)
        self.points = torch.from_numpy(rng.standard_normal((M, 3)).astype(F))
        self.colors = torch.from_numpy(rng.integers(0, 256, (M, 3)).astype(np.uint8))
        rot = [np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(S)]
        ext = [np.concatenate([r, rng.standard_normal((3, 1))], 1) for r in rot]
        self.extrinsic = torch.from_numpy(np.stack(ext).astype(F)) if S else torch.zeros(0, 3, 4)
        self.transform = postprocess.scene_alignment(self.extrinsic[0].numpy()) if S else np.eye(4)
        self.scene_scale = torch.tensor(2.5)
        self.conf_threshold, self.indices, self.conf = torch.tensor(0.0), None, None


def test_voxel_downsample_size_arguments_and_cpu_tensors():
    cloud = _Cloud()
    for kw in (dict(), dict(voxel_size=0.1, rel_size=0.1), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(rel_size=0.0),
               dict(rel_size=-0.5), dict(voxel_size=float("nan")), dict(rel_size=float("inf")), dict(rel_size=torch.tensor(0.1))):
        with pytest.raises(ValueError):
            postprocess.voxel_downsample(cloud, **kw)
    for kw in (dict(voxel_size=0.1), dict(rel_size=0.01), dict(voxel_size=torch.tensor(0.1))):
        with pytest.raises(L.OvgError):
            postprocess.voxel_downsample(cloud, **kw)                       # CPU tensors: no fallback
    pc = postprocess.PointCloud(1, 2, 3, 4, 5, 6)
    assert pc.indices is None and pc.conf is None                          # the new slot defaults to None
    assert postprocess.PointCloud(1, 2, 3, 4, 5, 6, 7, 8).conf == 8


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


_COMP = {5126: ("<f4", 4), 5121: ("u1", 1), 5123: ("<u2", 2)}
_WIDTH = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}


def _accessor(gltf, binary, k):
    a = gltf["accessors"][k]
    view = gltf["bufferViews"][a["bufferView"]]
    dt, size = _COMP[a["componentType"]]
    w = _WIDTH[a["type"]]
    off = a.get("byteOffset", 0)
    assert off % size == 0 and view["byteOffset"] % 4 == 0
    assert off + a["count"] * w * size <= view["byteLength"]               # the accessor stays inside its view
    assert view["byteOffset"] + view["byteLength"] <= gltf["buffers"][0]["byteLength"] <= len(binary)
    arr = np.frombuffer(binary, dt, a["count"] * w, view["byteOffset"] + off).reshape(a["count"], w)
    if "min" in a:
        assert a["min"] == [float(v) for v in arr.min(0)] and a["max"] == [float(v) for v in arr.max(0)]
    return arr


@pytest.mark.parametrize("M,S", [(37, 3), (0, 2), (5, 11), (4, 0)])
def test_write_glb_cameras(M, S, tmp_path):
    cloud = _Cloud(M, S, seed=M + S)
    a, b, c = (str(tmp_path / n) for n in ("a.glb", "b.glb", "c.glb"))
    postprocess.write_glb(a, cloud)
    postprocess.write_glb(b, cloud, cameras=False, camera_scale=0.3)
    assert open(a, "rb").read() == open(b, "rb").read()                    # the default file does not change
    postprocess.write_glb(c, cloud, cameras=True, camera_scale=0.1)
    gltf, binary = _read_glb(c)
    node = gltf["nodes"][gltf["scenes"][gltf["scene"]]["nodes"][0]]
    assert np.array_equal(np.array(node["matrix"]).reshape(4, 4).T, cloud.transform)
    if M == 0 and S == 0:
        assert "mesh" not in node
        return
    prims = gltf["meshes"][node["mesh"]]["primitives"]
    assert len(gltf["meshes"]) == 1 and len(prims) == (1 if M else 0) + S  # cloud and cameras under the same aligned node
    spans = sorted((v["byteOffset"], v["byteOffset"] + v["byteLength"]) for v in gltf["bufferViews"])
    assert all(lo >= prev for (_, prev), (lo, _) in zip(spans, spans[1:]))  # views do not overlap
    if M:
        p0 = prims[0]
        assert p0["mode"] == 0 and np.array_equal(_accessor(gltf, binary, p0["attributes"]["POSITION"]), cloud.points.numpy())
        assert np.array_equal(_accessor(gltf, binary, p0["attributes"]["COLOR_0"])[:, :3], cloud.colors.numpy())
    ext = cloud.extrinsic.numpy().astype(np.float64)
    height = 0.1 * float(cloud.scene_scale)
    seen = set()
    for s, prim in enumerate(prims[1 if M else 0:]):
        assert prim["mode"] == 4
        pos = _accessor(gltf, binary, prim["attributes"]["POSITION"]).astype(np.float64)
        col = _accessor(gltf, binary, prim["attributes"]["COLOR_0"])
        idx = _accessor(gltf, binary, prim["indices"]).reshape(-1)
        R, t = ext[s, :, :3], ext[s, :, 3]
        centre = -R.T @ t
        assert np.array_equal(pos[0].astype(F), centre.astype(F))          # the apex is the camera centre -R^T t
        cam = (pos - centre) @ R.T                                         # the pyramid in the camera's frame
        assert np.abs(cam[0]).max() <= 1e-6
        assert np.allclose(cam[1:, 2], height, rtol=0, atol=1e-5)          # the base lies `height` along +z
        assert np.allclose(np.abs(cam[1:, :2]), height / 2 / np.sqrt(2), rtol=0, atol=1e-5) and np.abs(cam[1:, :2].sum(0)).max() <= 1e-5
        assert pos.shape == (5, 3) and idx.size == 18 and idx.max() == 4 and set(idx.tolist()) == {0, 1, 2, 3, 4}
        tris = idx.reshape(6, 3)
        assert all(len(set(t3)) == 3 for t3 in tris.tolist()) and (tris == 0).any(1).sum() == 4
        assert (col == col[0]).all() and col[0, 3] == 255                   # one flat colour per camera
        assert tuple(col[0, :3]) == postprocess.CAMERA_COLORS[s % len(postprocess.CAMERA_COLORS)]
        seen.add(tuple(col[0, :3]))
    assert len(seen) == min(S, len(postprocess.CAMERA_COLORS))
