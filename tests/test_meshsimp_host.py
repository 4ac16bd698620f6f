"""Mesh simplification, host side: the numpy twin (tests/meshsimp_twin.py) against its naive second form and against the properties
the rule promises, the C ABI without a device (struct layout, enums, the workspace query, the refusals that return before any HIP
call) and the argument checks of postprocess.simplify_mesh that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import meshsimp_twin as twin
import voxelgrid_twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
KEYS = ("vertices", "faces", "normals", "colors", "source_index", "vertex_count", "counts")


def _same(a, b, name):
    for k in KEYS:
        x, y = a[k], b[k]
        assert (x is None) == (y is None), (name, k)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (name, k, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (name, k)


def _scenes():
    v, f, n, c = twin.double_sheet()
    yield "double sheet 0.06 mean", (v, f, F(0.06), twin.odd_normals(v, n, F(0.06)), c, "mean")
    yield "double sheet 0.031 first", (v, f, F(0.031), n, c, "first")
    yield "double sheet 0.11 bare", (v, f, F(0.11), None, None, "mean")
    yield "bad input 0.06", twin.bad_input_sheet()[:2] + (F(0.06), n, c, "mean")
    hv, hf, hn, hc = twin.hot_cell_sheet(extra=600)
    yield "hot cell 0.06", (hv, hf, F(0.06), hn, hc, "mean")
    cv, cf, cn, cc = twin.collision_cloud(m=2500, faces=4000)
    yield "random cloud 0.08", (cv, cf, F(0.08), cn, cc, "mean")
    yield "one cell", (v, f, F(5.0), n, c, "mean")


def test_twin_equals_the_naive_form():
    for name, (v, f, edge, n, c, position) in _scenes():
        got = twin.simplify(v, f, edge, n, c, position)
        _same(got, twin.simplify_naive(v, f, edge, n, c, position), name)
        print("%-28s M' %5d F' %5d cells %5d degenerate %5d duplicates %5d" % ((name,) + tuple(int(x) for x in got["counts"][[0, 1, 3, 4, 5]])))
    one = twin.simplify(*list(_scenes())[-1][1][:3])
    assert one["counts"].tolist() == [0, 0, 0, 1, 4096, 0]


def test_double_sheet_exercises_both_face_rules():
    v, f, _, _ = twin.double_sheet()
    assert v.shape == (2178, 3) and f.shape == (4096, 3)
    # the sheet's 1 / 32 spacing is wider than the 0.031 edge: neighbours never share a cell there, so that edge has duplicates only
    # (4096 = survivors + duplicates); the two coarser edges exercise both rules
    for edge, degenerate in ((0.11, 100), (0.06, 100), (0.031, 0)):
        counts = twin.simplify(v, f, F(edge))["counts"]
        assert counts[4] >= degenerate and counts[5] >= 100 and counts[0] > 0, (edge, counts)
        assert counts[1] + counts[4] + counts[5] == 4096
    hv, hf, _, _ = twin.hot_cell_sheet()
    assert twin.simplify(hv, hf, F(0.06))["vertex_count"].max() >= 4096
    cv, cf, _, _ = twin.collision_cloud()
    cells, triples = twin.table_keys(cv, cf, F(0.04))
    assert 3000 < cells < 8000 and triples > 1000


def test_properties_of_the_output():
    for name, (v, f, edge, n, c, position) in _scenes():
        out = twin.simplify(v, f, edge, n, c, position)
        faces, src = out["faces"].astype(np.int64), out["source_index"]
        Mo = len(out["vertices"])
        assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])).all(), name       # no repeated corner
        assert len({frozenset(r) for r in faces.tolist()}) == len(faces), name                                           # no two with the same corner set
        assert sorted(set(faces.reshape(-1).tolist())) == list(range(Mo)), name                                          # every vertex referenced
        assert (np.diff(src) > 0).all(), name
        first = twin.simplify(v, f, edge, n, c, "first")
        assert np.array_equal(first["vertices"].view(np.uint32), v[src].view(np.uint32)), name
        for k in ("faces", "source_index", "vertex_count", "counts"):
            assert np.array_equal(first[k], out[k])                                                                       # position moves vertices only
        _, origin, _, cell = twin.grid(v, edge)
        if position == "mean" and Mo:                                                                                     # the mean lies in the closed cell
            lo = origin.astype(np.float64) + float(edge) * cell[src]
            got = out["vertices"].astype(np.float64)
            assert (got >= lo - 1e-6).all() and (got <= lo + float(edge) + 1e-6).all(), name
        if out["normals"] is not None:
            length = np.linalg.norm(out["normals"].astype(np.float64), axis=1)
            assert ((length == 0) | (np.abs(length - 1) < 1e-6)).all()
    v, f, n, c = twin.double_sheet()
    nrm = twin.odd_normals(v, n, F(0.06))
    out = twin.simplify(v, f, F(0.06), nrm, c)
    zero = (out["normals"] == 0).all(axis=1)
    assert zero.any() and (out["vertex_count"][zero] >= 3).all()                                                          # the cancelling pair


def test_permuting_the_faces_moves_nothing_but_the_faces():
    """Exact expectation: vertices, normals, colours, source_index, vertex_count and the counts keep their bytes; the survivors are, per
    set of three cells, the face that comes first in the NEW order, listed in the new order with their own corner order."""
    v, f, n, c = twin.double_sheet()
    edge = F(0.06)
    base = twin.simplify(v, f, edge, n, c)
    valid, _, _, cell = twin.grid(v, edge)
    cid = {tuple(r): k for k, r in enumerate(np.unique(cell[valid], axis=0).tolist())}
    cell_id = np.array([cid[tuple(r)] for r in cell.tolist()])
    for perm in (np.arange(len(f))[::-1], np.random.default_rng(2).permutation(len(f))):
        fp = np.ascontiguousarray(f[perm])
        out = twin.simplify(v, fp, edge, n, c)
        for k in ("vertices", "normals", "colors", "source_index", "vertex_count", "counts"):
            assert np.array_equal(out[k].view(np.uint8), base[k].view(np.uint8)), k
        seen, want = set(), []
        for j, row in enumerate(fp.tolist()):
            t = frozenset(int(cell_id[i]) for i in row)
            if len(t) == 3 and t not in seen:
                seen.add(t)
                want.append(j)
        assert out["face_index"].tolist() == want
        number = {int(s): k for k, s in enumerate(base["source_index"])}
        leader = {int(cell_id[s]): int(s) for s in base["source_index"]}
        rows = [[number[leader[int(cell_id[i])]] for i in fp[j]] for j in want]
        assert out["faces"].tolist() == rows
        assert {frozenset(r) for r in out["faces"].tolist()} == {frozenset(r) for r in base["faces"].tolist()}
    assert not np.array_equal(twin.simplify(v, np.ascontiguousarray(f[::-1]), edge)["faces"], base["faces"][::-1])       # a reversed copy won somewhere


def test_grid_is_the_grid_of_voxel_downsample_and_flags():
    v, _, _, _ = twin.bad_input_sheet()
    for edge in (0.11, 0.031, 0.0007):
        valid, origin, g, cell = twin.grid(v, F(edge))
        valid2, origin2, cell2 = voxelgrid_twin.cells(v, F(edge))
        assert np.array_equal(valid, valid2) and np.array_equal(origin, origin2) and np.array_equal(cell, cell2)
        assert len(np.unique(cell[valid], axis=0)) == len(voxelgrid_twin.downsample(v, F(edge)))
    f = twin.grid_faces(33)
    for bad, flag in ((0.0, twin.BAD_VOXEL), (-1.0, twin.BAD_VOXEL), (np.nan, twin.BAD_VOXEL), (np.inf, twin.BAD_VOXEL), (1.0 / (1 << 22), twin.OVERFLOW)):
        with pytest.raises(twin.Flagged) as e:
            twin.simplify(v, f, bad)
        assert e.value.flags == flag
    assert (twin.OVERFLOW, twin.BAD_VOXEL) == (L.MS_OVERFLOW, L.MS_BAD_VOXEL)


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_ctypes_struct_layout_and_enums_match_c_meshsimp():
    enums = ["OVG_MS_COUNT", "OVG_MS_SCATTER", "OVG_MS_OVERFLOW", "OVG_MS_BAD_VOXEL", "OVG_MS_POS_MEAN", "OVG_MS_POS_FIRST", "OVG_ABI_VERSION"]
    got, _ = abi_layout.check({"ovg_mesh_simplify_params": L.MeshSimplifyParams}, enums)
    assert got == [L.MS_COUNT, L.MS_SCATTER, L.MS_OVERFLOW, L.MS_BAD_VOXEL, L.MS_POS_MEAN, L.MS_POS_FIRST, L.ABI_VERSION] == [1, 2, 1, 2, 0, 1, 13]
    assert postprocess.MESH_POSITIONS == {"mean": L.MS_POS_MEAN, "first": L.MS_POS_FIRST}


def test_entries_are_declared_under_abi_13_and_built_exact():
    text = open(HEADER).read()
    assert re.search(r"int\s+ovg_mesh_simplify\s*\(\s*const\s+ovg_mesh_simplify_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"int64_t\s+ovg_mesh_simplify_workspace_bytes\s*\(\s*int64_t\s+vertices\s*,\s*int64_t\s+faces\s*\)\s*;", text)
    for entry in ("ovg_mesh_simplify", "ovg_mesh_simplify_workspace_bytes"):
        assert entry in L.SYMBOLS and text.index(entry) < text.index("#define OVG_ABI_VERSION")      # named in the ABI-13 list
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text) and L.load().ovg_abi_version() == 13 == L.ABI_VERSION
    from omnivggt_official_amd import build as B
    assert B.SOURCES[-1] == "ovg_meshsimp.hip" and B.EXTRA_FLAGS["ovg_meshsimp.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(B.CSRC, "ovg_meshsimp.hip")).read()
    assert re.search(r'^\s*#\s*include\s+"ovg_geom.h"', src, re.M)


def test_workspace_query_and_refusals_without_gpu():
    lib = L.load()
    q = lib.ovg_mesh_simplify_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256
    for m, f in ((1, 1), (2178, 4096), (20000, 30000), (511, 513), (64 * 518 * 518, 2 * 64 * 517 * 517)):
        C, T, tv, tf = max(1024, 2 * m), max(1024, 2 * f), -(-m // 4096), -(-f // 4096)
        parts = (256, 8 * C, 4 * C, 4 * C, 4 * C, 72 * C, 4 * m, m, 4 * T, f, 8 * tv, 8 * tv, 8 * tf, 8 * tf)
        assert q(m, f) == sum(r256(b) for b in parts) == ops.mesh_simplify_workspace_bytes(m, f)
    assert [q(*a) for a in ((0, 5), (5, 0), (0, 0), (-1, 5), (5, -3), (1 << 31, 5), (5, (1 << 32) - 1), (5, 1 << 40), (1 << 40, 5))] == [-1] * 9
    assert q((1 << 31) - 1, (1 << 32) - 2) > 0
    for bad in ((0, 5), (5, 0), (1 << 31, 5), (5, (1 << 32) - 1), (1 << 70, 5)):
        with pytest.raises(L.OvgError):
            ops.mesh_simplify_workspace_bytes(*bad)
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    need = q(4096, 8000)

    def run(**kw):
        p = L.MeshSimplifyParams(vertices=big, faces=big, normals=big, colors=big + 1, voxel=big, num_vertices=4096, num_faces=8000,
                                 stage=L.MS_COUNT | L.MS_SCATTER, position=L.MS_POS_MEAN, vertex_capacity=10, face_capacity=10, out_vertices=big,
                                 out_normals=big, out_colors=big + 1, out_source_index=big, out_vertex_count=big, out_faces=big, out_count=big,
                                 ws=big, ws_bytes=need)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_mesh_simplify(ctypes.byref(p), None)

    assert lib.ovg_mesh_simplify(None, None) == -1
    for bad in (dict(vertices=None), dict(faces=None), dict(ws=None), dict(voxel=None), dict(ws=big + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(ws_bytes=-5), dict(stage=0), dict(stage=4), dict(stage=-1), dict(position=2), dict(position=-1), dict(num_vertices=0),
                dict(num_vertices=-1), dict(num_faces=0), dict(num_vertices=1 << 31, ws_bytes=1 << 60), dict(num_faces=(1 << 32) - 1, ws_bytes=1 << 60),
                dict(num_vertices=8192), dict(num_faces=16000), dict(out_count=None), dict(vertex_capacity=-1), dict(face_capacity=-1),
                dict(out_vertices=None), dict(out_faces=None), dict(out_normals=None), dict(out_colors=None), dict(normals=None), dict(colors=None),
                dict(vertices=big + 2), dict(faces=big + 1), dict(normals=big + 2), dict(voxel=big + 2), dict(out_count=big + 4),
                dict(out_vertices=big + 2), dict(out_normals=big + 1), dict(out_source_index=big + 4), dict(out_vertex_count=big + 2),
                dict(out_faces=big + 2)):
        assert run(**bad) == -1, bad


# ---------------------------------------------------------------------------------------------
# the Python layers
# ---------------------------------------------------------------------------------------------
def _cpu_mesh(scene_scale=2.5, cls=postprocess.Mesh):
    v, f, n, c = twin.double_sheet(n=5)
    t = torch.from_numpy
    return cls(t(v), t(f), t(n), t(c), np.eye(4), None, None if scene_scale is None else torch.tensor(scene_scale))


def test_simplify_mesh_refusals_that_need_no_device():
    mesh = _cpu_mesh()
    for kw in (dict(), dict(voxel_size=0.1, rel_size=0.1), dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(rel_size=0.0), dict(rel_size=-0.5),
               dict(voxel_size=float("nan")), dict(voxel_size=float("inf")), dict(rel_size=float("inf")), dict(rel_size=torch.tensor(0.1)),
               dict(voxel_size=torch.ones(2)), dict(voxel_size=0.1, position="median"), dict(voxel_size=0.1, position=None),
               dict(rel_size=0.1, position=0)):
        with pytest.raises(ValueError):
            postprocess.simplify_mesh(mesh, **kw)
    with pytest.raises(ValueError):
        postprocess.simplify_mesh(_cpu_mesh(scene_scale=None), rel_size=0.01)      # no scene_scale to scale by
    with pytest.raises(ValueError):
        postprocess.simplify_mesh("mesh", voxel_size=0.1)
    for kw in (dict(voxel_size=0.1), dict(rel_size=0.01), dict(voxel_size=torch.tensor(0.1)), dict(voxel_size=0.1, position="first")):
        with pytest.raises(L.OvgError):
            postprocess.simplify_mesh(mesh, **kw)                                   # CPU tensors: no fallback
    with pytest.raises(L.OvgError):
        postprocess.simplify_mesh(_cpu_mesh(cls=postprocess.MapMesh), voxel_size=0.1)
    assert issubclass(postprocess.SimplifiedMesh, postprocess.Mesh)
    s = postprocess.SimplifiedMesh(1, 2, 3, 4, 5)
    assert s.source_index is None and s.pixel_index is None and (s.cells, s.degenerate_faces, s.duplicate_faces) == (0, 0, 0)


def test_ops_wrapper_checks_its_arguments_before_any_device_call():
    v, f, n, c = (torch.from_numpy(a) for a in twin.double_sheet(n=5))
    voxel, ws, count = torch.tensor(0.1), torch.zeros(1 << 20, dtype=torch.uint8), torch.zeros(6, dtype=torch.int64)
    good = dict(stage=L.MS_COUNT, vertices=v, faces=f, voxel=voxel, ws=ws, normals=n, colors=c, out_count=count)
    for bad in (dict(vertices=v[:, :2]), dict(vertices=v.double()), dict(faces=f.long()), dict(faces=f[:, :2]), dict(normals=n[:-1]),
                dict(colors=c.int()), dict(voxel=torch.ones(2)), dict(voxel=torch.tensor(0.1, dtype=torch.float64)), dict(stage=0), dict(stage=4),
                dict(position=2), dict(ws=ws.int()), dict(out_count=None), dict(out_count=count[:2]), dict(out_count=count.int()),
                dict(vertices=v[:0]), dict(faces=f[:0]), dict(stage=L.MS_SCATTER, vertex_capacity=-1),
                dict(stage=L.MS_SCATTER, vertex_capacity=4), dict(stage=L.MS_SCATTER, face_capacity=4),
                dict(stage=L.MS_SCATTER, vertex_capacity=4, out_vertices=torch.zeros(4, 3), out_normals=torch.zeros(4, 3)),
                dict(stage=L.MS_SCATTER, vertex_capacity=4, out_vertices=torch.zeros(3, 3), out_normals=torch.zeros(4, 3),
                     out_colors=torch.zeros(4, 3, dtype=torch.uint8))):
        with pytest.raises(L.OvgError) as e:
            ops.mesh_simplify(**{**good, **bad})
        assert "mesh_simplify" in str(e.value), bad
    with pytest.raises(L.OvgError) as e:
        ops.mesh_simplify(**good)                                                   # everything in order but the device
    assert "HIP device tensor" in str(e.value)
