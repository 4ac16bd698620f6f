"""k-nearest-neighbour search, PCA normals and the statistical filter, host side: the brute-force twin (tests/knn_twin.py) checked against
the radius twin and on crafted inputs, the C ABI without a device (struct layouts, argument checks that return before any HIP
call), the Python API's argument checks, and write_ply with normals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import knn_twin as twin
import nn_twin
import radius_twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def test_twin_k1_is_the_radius_twin_and_count_is_its_count():
    q, r, qv, rv = nn_twin.scene(300, 211, seed=3)
    for radius in (0.25, 0.5):
        r2 = radius_twin.radius_sq(radius)
        for kw in (dict(), dict(query_valid=qv, reference_valid=rv)):
            want = radius_twin.search(q, r, r2, **kw)
            got = twin.search(q, r, r2, 1, **kw)
            assert got[1].shape == got[2].shape == (300, 1)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.reshape(-1).tobytes() == w.tobytes()
            for k in (3, 16, 32):
                assert twin.search(q, r, r2, k, **kw)[0].tobytes() == want[0].tobytes()
    c, _, cv, _ = nn_twin.scene(260, 0, seed=1, same=True)
    want = radius_twin.search(c, c, F(0.25), cv, cv, exclude_self=True)
    got = twin.search(c, c, F(0.25), 1, cv, cv, exclude_self=True)
    assert all(g.reshape(-1).tobytes() == w.tobytes() for g, w in zip(got, want))


def test_twin_rows_are_sorted_padded_and_prefixes_of_each_other():
    q, r, qv, rv = nn_twin.scene(400, 1500, seed=2)
    r2 = radius_twin.radius_sq(0.75)
    count, index, sqdist = twin.search(q, r, r2, 32, qv, rv)
    found = np.minimum(count, 32)
    rank = np.arange(32)[None, :]
    pad = rank >= found[:, None]
    assert pad.any() and (~pad).any() and (count > 32).any() and (count == 0).any()
    assert (index[pad] == -1).all() and np.isposinf(sqdist[pad]).all()
    assert (index[~pad] >= 0).all() and (sqdist[~pad] <= r2).all()
    key = (sqdist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint32).astype(np.uint64)
    both = ~pad[:, 1:]
    assert (key[:, 1:][both] > key[:, :-1][both]).all()                        # ascending (bits(d), j), strictly
    ties = (sqdist[:, 1:] == sqdist[:, :-1]) & both
    assert ties.sum() > 10 and (index[:, 1:][ties] > index[:, :-1][ties]).all()            # equal distances: ascending index
    hit = np.nonzero(~pad)
    dx, dy, dz = (q[hit[0], a] - r[index[~pad], a] for a in range(3))
    assert ((dx * dx + dy * dy) + dz * dz).tobytes() == sqdist[~pad].tobytes()             # sqdist is the rule's d of the pair
    for k in (1, 5, 17):
        sub = twin.search(q, r, r2, k, qv, rv)
        assert sub[1].tobytes() == np.ascontiguousarray(index[:, :k]).tobytes() and sub[2].tobytes() == np.ascontiguousarray(sqdist[:, :k]).tobytes()
    rows = [7, 399, 0, 7]
    sub = twin.search(q, r, r2, 32, qv, rv, rows=rows, budget=1000)
    assert sub[0].tolist() == count[rows].tolist() and sub[1].tobytes() == index[rows].tobytes() and sub[2].tobytes() == sqdist[rows].tobytes()
    # k above the number of references; no reference at all
    few = twin.search(q[:9], r[:3], r2, 8)
    assert few[1].shape == (9, 8) and (few[1][:, 3:] == -1).all() and (few[0] <= 3).all()
    none = twin.search(q[:4], r[:0], r2, 4)
    assert (none[0] == 0).all() and (none[1] == -1).all() and np.isposinf(none[2]).all()


def test_twin_crafted_ties_duplicates_and_exclude_self():
    r = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, -1, 0], [0, 0, 1], [1e20, 0, 0]], F)
    count, index, sqdist = twin.search(r, r, F(1.0), 4)
    assert count.tolist() == [5, 3, 3, 1, 0, 2, 2, 1]
    assert index[0].tolist() == [0, 1, 2, 5] and sqdist[0].tolist() == [0, 1, 1, 1]          # three more at exactly 1: the lowest indices
    assert index[1].tolist() == [1, 2, 0, -1] and index[3].tolist() == [3, -1, -1, -1] and index[4].tolist() == [-1] * 4
    count, index, sqdist = twin.search(r, r, F(1.0), 4, exclude_self=True)
    assert count.tolist() == [4, 2, 2, 0, 0, 1, 1, 0]
    assert index[0].tolist() == [1, 2, 5, 6] and index[1].tolist() == [2, 0, -1, -1] and index[2].tolist() == [1, 0, -1, -1]
    rv = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    assert twin.search(r, r, F(1.0), 2, rv, rv)[1].tolist() == [[0, 2], [-1, -1], [2, 0], [3, -1], [-1, -1], [5, 0], [6, 0], [7, -1]]


def test_twin_covariance_and_normals():
    x, y = np.meshgrid(np.arange(5), np.arange(4), indexing="ij")
    plane = np.stack([x.reshape(-1) * 0.25, y.reshape(-1) * 0.5, np.full(20, 2.0)], 1).astype(F)
    idx = twin.search(plane, plane, F(1.0), 8)[1]
    c, m = twin.covariance(plane, plane, idx)
    assert (m >= 3).all() and (c[:, [2, 4, 5]] == 0).all() and (c[:, 0] > 0).all()
    n, lam, solved = twin.normals(plane, plane, idx)
    assert solved.all() and (np.abs(n) == np.array([0.0, 0.0, 1.0])).all() and (n[:, 2] == 1).all() and (lam[:, 0] == 0).all()
    n, _, _ = twin.normals(plane, plane, idx, viewpoint=(0.0, 0.0, -5.0))
    assert (n[:, 2] == -1).all()
    n, _, _ = twin.normals(plane, plane, idx, viewpoint=np.tile(np.array([[0, 0, 9.0]], F), (20, 1)))
    assert (n[:, 2] == 1).all()
    # skipped entries, rows of fewer than three, an empty row
    table = np.array([[0, 1, 5, -1], [0, 99, -1, 1], [-1, -1, -1, -1], [3, 3, 3, 3]], np.int32)
    c, m = twin.covariance(plane[:4], plane, table)
    assert m.tolist() == [3, 2, 0, 4] and (c[2] == 0).all() and (c[3] == 0).all()
    pts = plane[[0, 1, 5]].astype(np.float64)
    d = pts - pts.sum(0) / 3
    assert np.allclose(c[0], [(d[:, a] * d[:, b]).sum() / 3 for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], rtol=1e-15, atol=0)
    n, _, solved = twin.normals(plane[:4], plane, table)
    assert solved.tolist() == [True, False, False, True] and (n[1] == 0).all() and (n[2] == 0).all()
    assert (twin.matrices(c)[0] == twin.matrices(c)[0].T).all()


def _layout(struct, cname, extra):
    return abi_layout.check({cname: struct}, extra)[0]


def test_ctypes_struct_layouts_match_c_knn():
    assert _layout(L.KnnParams, "ovg_knn_params", ["OVG_KNN_MAX_K", "OVG_RS_QUERY_BLOCK", "OVG_ABI_VERSION"]) == [L.KNN_MAX_K, L.RS_QUERY_BLOCK, L.ABI_VERSION]
    assert _layout(L.KnnNormalsParams, "ovg_knn_normals_params", ["OVG_KNN_NORMALS_SWEEPS"]) == [L.KNN_NORMALS_SWEEPS]
    assert L.KNN_MAX_K == 32 and L.ABI_VERSION == 13
    # ovg_knn_params is ovg_radius_params with k in the place of stage; ovg_radius_params keeps its layout
    assert [(n, t) for n, t in L.KnnParams._fields_ if n != "k"] == [(n, t) for n, t in L.RadiusParams._fields_ if n != "stage"]
    assert L.KnnParams.k.offset == L.RadiusParams.stage.offset and ctypes.sizeof(L.KnnParams) == ctypes.sizeof(L.RadiusParams)
    text = open(HEADER).read()
    assert re.search(r"int\s+ovg_knn_search\s*\(\s*const\s+ovg_knn_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_knn_normals\s*\(\s*const\s+ovg_knn_normals_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_knn_search" in L.SYMBOLS and "ovg_knn_normals" in L.SYMBOLS


def test_argument_validation_of_both_entries_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    reach = ops.radius_reach(0.0625)
    need = lib.ovg_radius_workspace_bytes(1000, 1000)

    def run(**kw):
        p = L.KnnParams(query=big, reference=big, query_valid=big, reference_valid=big, origin=big, nq=1000, nr=1000, radius_sq=0.0625,
                        cell=reach, flags=0, k=16, max_pairs=1 << 40, ws=big, ws_bytes=need, out_stats=big, count=big, index=big, sqdist=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_knn_search(ctypes.byref(p), None)

    below = float(np.nextafter(F(reach), F(0)))
    assert lib.ovg_knn_search(None, None) == -1
    for bad in (dict(k=0), dict(k=-1), dict(k=33), dict(k=1 << 30), dict(k=-(1 << 31)),
                dict(query=None), dict(reference=None), dict(ws=None), dict(count=None), dict(index=None), dict(sqdist=None),
                dict(nq=0), dict(nr=0), dict(nq=-1), dict(nr=-7), dict(nq=1 << 31), dict(nr=1 << 31, ws_bytes=1 << 50), dict(nq=-(1 << 63)),
                dict(radius_sq=0.0), dict(radius_sq=-1.0), dict(radius_sq=2.0 ** -101), dict(radius_sq=float("inf")), dict(radius_sq=float("nan")),
                dict(cell=below), dict(cell=0.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(radius_sq=0.25),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=L.RS_EXCLUDE_SAME_INDEX, nr=999), dict(flags=L.RS_EXCLUDE_SAME_INDEX, nq=999),
                dict(max_pairs=-1), dict(max_pairs=-(1 << 63)),
                dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8), dict(ws=big + 4),
                dict(query=big + 2), dict(reference=big + 1), dict(origin=big + 2), dict(count=big + 1), dict(index=big + 2),
                dict(sqdist=big + 3), dict(out_stats=big + 4)):
        assert run(**bad) == -1, bad

    def normals(**kw):
        p = L.KnnNormalsParams(query=big, reference=big, index=big, viewpoint=big, nq=1000, nr=1000, k=16, viewpoint_stride=3, normal=big,
                               curvature=big, covariance=big, used=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_knn_normals(ctypes.byref(p), None)

    assert lib.ovg_knn_normals(None, None) == -1
    for bad in (dict(query=None), dict(reference=None), dict(index=None), dict(normal=None),
                dict(nq=0), dict(nr=0), dict(nq=-1), dict(nr=-1), dict(nq=1 << 31), dict(nr=1 << 31), dict(k=0), dict(k=-3),
                dict(viewpoint_stride=1), dict(viewpoint_stride=-3), dict(viewpoint_stride=6), dict(viewpoint=None),
                dict(viewpoint=None, viewpoint_stride=1),
                dict(query=big + 2), dict(reference=big + 1), dict(index=big + 2), dict(viewpoint=big + 1), dict(normal=big + 3),
                dict(curvature=big + 2), dict(covariance=big + 4), dict(used=big + 1)):
        assert normals(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    q, r = torch.zeros(5, 3), torch.zeros(2, 4, 3)
    base = dict(query=q, reference=r, k=4, radius=0.5)
    for kw in (dict(k=0), dict(k=33), dict(k=-1), dict(k=2.0), dict(k=True), dict(k="4"), dict(k=None),
               dict(query=torch.zeros(5, 4)), dict(query=torch.zeros(5, 3, dtype=torch.float64)), dict(reference=[[0.0, 0.0, 0.0]]),
               dict(query_valid=torch.ones(4, dtype=torch.bool)), dict(reference_valid=torch.ones(8, dtype=torch.bool)), dict(exclude_self=True),
               dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=None), dict(radius=True), dict(radius=1e20),
               dict(cell_size=0.4), dict(cell_size="x"), dict(origin=(0, 0)), dict(origin=torch.zeros(2)), dict(max_pairs=-1), dict(max_pairs=1.5)):
        with pytest.raises(ValueError):
            postprocess.knn_neighbours(**dict(base, **kw))
    for kw in (dict(), dict(k=1), dict(k=32), dict(query_valid=torch.ones(5, dtype=torch.bool)), dict(reference=torch.zeros(5, 3), exclude_self=True),
               dict(cell_size=1.0, origin=(1.0, 2.0, 3.0)), dict(max_pairs=10), dict(query=torch.zeros(0, 3)), dict(reference=torch.zeros(0, 3))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.knn_neighbours(**dict(base, **kw))
    with pytest.raises(TypeError):
        postprocess.knn_neighbours(q, r, 4)                                 # a radius is required
    cloud = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, torch.tensor(2.0), None, None)
    full = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, torch.tensor(2.0), np.eye(4), torch.zeros(2, 3, 4),
                                  torch.arange(5), torch.ones(5))
    for kw in (dict(), dict(radius=0.5, rel_radius=0.1), dict(radius=-1.0), dict(rel_radius=0.0), dict(rel_radius=float("nan")),
               dict(radius=0.5, k=0), dict(radius=0.5, k=33), dict(radius=0.5, k=1.5), dict(radius=0.5, k=True)):
        with pytest.raises(ValueError):
            postprocess.estimate_normals(cloud, **kw)
        with pytest.raises(ValueError):
            postprocess.statistical_outlier_mask(cloud, **kw)
        with pytest.raises(ValueError):
            postprocess.remove_statistical_outliers(cloud, **kw)
    for kw in (dict(viewpoint=(0, 0)), dict(viewpoint=(0, 0, float("inf"))), dict(viewpoint=1.0), dict(viewpoint="camera"),
               dict(viewpoint=torch.zeros(2)), dict(viewpoint=torch.zeros(3, dtype=torch.float64)), dict(viewpoint=torch.zeros(4, 3)),
               dict(viewpoint="cameras"), dict(viewpoint="cameras", image_hw=(4, 4)), dict(valid=torch.ones(4, dtype=torch.bool))):
        with pytest.raises(ValueError):
            postprocess.estimate_normals(cloud, radius=0.5, **kw)
    for kw in (dict(viewpoint="cameras"), dict(viewpoint="cameras", image_hw=(0, 4)), dict(viewpoint="cameras", image_hw=(4,)),
               dict(viewpoint="cameras", image_hw=4), dict(viewpoint="cameras", image_hw=(2.0, 2))):
        with pytest.raises(ValueError):
            postprocess.estimate_normals(full, radius=0.5, **kw)
    with pytest.raises(ValueError):
        postprocess.estimate_normals(q, rel_radius=0.1)                     # rel_radius needs a PointCloud
    for kw in (dict(std_ratio=-1.0), dict(std_ratio=float("nan")), dict(std_ratio="2"), dict(std_ratio=True), dict(std_ratio=None)):
        with pytest.raises(ValueError):
            postprocess.statistical_outlier_mask(cloud, radius=0.5, **kw)
        with pytest.raises(ValueError):
            postprocess.remove_statistical_outliers(cloud, radius=0.5, **kw)
    with pytest.raises(ValueError):
        postprocess.remove_statistical_outliers(q, radius=0.5)              # a PointCloud, not a tensor
    with pytest.raises(ValueError):
        postprocess.statistical_outlier_mask(torch.zeros(5, 2), radius=0.5)
    for kw in (dict(radius=0.5), dict(rel_radius=0.1), dict(radius=0.5, k=3)):
        for fn in (postprocess.estimate_normals, postprocess.statistical_outlier_mask, postprocess.remove_statistical_outliers):
            with pytest.raises(L.OvgError, match="no CPU fallback"):
                fn(cloud, **kw)
    for kw in (dict(viewpoint=(0.0, 1.0, 2.0)), dict(viewpoint=torch.zeros(3)), dict(viewpoint=torch.zeros(5, 3)), dict(return_curvature=True),
               dict(valid=torch.ones(5, dtype=torch.bool))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.estimate_normals(cloud, radius=0.5, **kw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.estimate_normals(full, radius=0.5, viewpoint="cameras", image_hw=(1, 3))
    with pytest.raises(L.OvgError):
        ops.knn_search(q, r.reshape(-1, 3), 0.25, 0.6, torch.zeros(1 << 16, dtype=torch.uint8), 4)   # CPU tensors at the thin wrappers
    with pytest.raises(L.OvgError):
        ops.knn_normals(q, q, torch.zeros(5, 4, dtype=torch.int32))
    res = postprocess.KNNResult(torch.tensor([2], dtype=torch.int32), torch.tensor([[1, 0, -1]], dtype=torch.int32), torch.tensor([[0.5, 1.0, float("inf")]]))
    assert res.count.tolist() == [2] and res.index.tolist() == [[1, 0, -1]] and res.sqdist[0, 1] == 1.0
    assert postprocess.KNN_MAX_K == L.KNN_MAX_K


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    props = [line.split()[1:] for line in head.decode().splitlines() if line.startswith("property")]
    dt = np.dtype([(name.decode() if isinstance(name, bytes) else name, {"float": "<f4", "uchar": "u1"}[t]) for t, name in props])
    return head.decode(), np.frombuffer(body, dt)


def test_write_ply_with_normals_and_without_them_the_old_bytes(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(7, 3)).astype(F)
    col = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    nrm = rng.normal(size=(7, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nrm[3] = 0
    ang = 0.7
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ np.diag([2.0, 1.0, 0.5])   # not orthogonal
    T[:3, 3] = [1.0, -2.0, 3.0]
    cloud = postprocess.PointCloud(torch.from_numpy(pts), torch.from_numpy(col), None, None, T, None)
    # without normals: the layout as it has always been, written here by hand
    for apply in (True, False):
        path = str(tmp_path / ("plain%d.ply" % apply))
        postprocess.write_ply(path, cloud, apply_transform=apply)
        want_pts = (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F) if apply else pts
        rec = np.empty(7, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
        rec["x"], rec["y"], rec["z"], rec["red"], rec["green"], rec["blue"] = (*want_pts.T, *col.T)
        head = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        assert open(path, "rb").read() == head.encode("ascii") + rec.tobytes()
        postprocess.write_ply(path + "n", cloud, apply_transform=apply, normals=None)
        assert open(path + "n", "rb").read() == open(path, "rb").read()
    path = str(tmp_path / "normals.ply")
    postprocess.write_ply(path, cloud, apply_transform=False, normals=torch.from_numpy(nrm))
    head, rec = _read_ply(path)
    assert rec.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue") and len(rec) == 7 and "element vertex 7" in head
    assert np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).tobytes() == nrm.tobytes() and np.stack([rec["x"], rec["y"], rec["z"]], 1).tobytes() == pts.tobytes()
    assert np.stack([rec["red"], rec["green"], rec["blue"]], 1).tobytes() == col.tobytes()
    postprocess.write_ply(path, cloud, normals=torch.from_numpy(nrm))
    _, rec = _read_ply(path)
    got = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float64)
    want = nrm.astype(np.float64) @ np.linalg.inv(T[:3, :3])
    want[[0, 1, 2, 4, 5, 6]] /= np.linalg.norm(want[[0, 1, 2, 4, 5, 6]], axis=1, keepdims=True)
    assert np.abs(got - want).max() <= 2.0 ** -23 and (got[3] == 0).all()
    assert np.abs(np.linalg.norm(got[[0, 1, 2, 4, 5, 6]], axis=1) - 1).max() <= 2.0 ** -22
    # a transformed normal stays perpendicular to transformed tangents: the inverse transpose, not the matrix itself
    tang = np.cross(nrm[0].astype(np.float64), [1.0, 0.0, 0.0])
    assert abs(got[0] @ (T[:3, :3] @ tang)) <= 1e-6 * np.linalg.norm(T[:3, :3] @ tang)
    empty = postprocess.PointCloud(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.uint8), None, None, T, None)
    postprocess.write_ply(path, empty, normals=torch.zeros(0, 3))
    head, rec = _read_ply(path)
    assert "element vertex 0" in head and len(rec) == 0 and "property float nz" in head
    for bad in (torch.zeros(6, 3), torch.zeros(7, 3, dtype=torch.float64), np.zeros((7, 3), F), torch.zeros(7, 2)):
        with pytest.raises(ValueError):
            postprocess.write_ply(path, cloud, normals=bad)
