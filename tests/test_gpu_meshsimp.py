"""ovg_mesh_simplify and postprocess.simplify_mesh on the device against tests/meshsimp_twin.py: every output byte for byte (vertices,
faces, normals, colours, source_index, vertex_count and the six counts) in guarded buffers of exactly the queried / counted sizes. The
double sheet at three edges (tests/test_meshsimp_host.py shows that it exercises the degenerate and the duplicate rule), bad input, one
cell, a hot cell, tables that really probe, every attribute combination, the grid against ovg_voxel_downsample, both flags, the glue
from the two mesh producers to the writers and the rasteriser, short capacities, and the gated cases for the stream contract's coverage
test. Every case runs twice."""
import functools
import json
import struct

import numpy as np
import pytest
import torch

import mapgeom_scenes
import mapgeom_twin
import meshsimp_twin as twin
import stream_contract as sc
import test_gpu_stream_contract as tsc
import tsdf_twin
from kernel_guards import GUARD_BYTE, guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
POS = {"mean": L.MS_POS_MEAN, "first": L.MS_POS_FIRST}
KEYS = ("vertices", "faces", "normals", "colors", "source_index", "vertex_count")


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    yield


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _g(shape, dtype):
    v, chk = guarded((1,) + tuple(shape), dtype, "cuda", guard_bytes=4096)
    return v[0], chk


def _same(got, want, name):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        bad = np.nonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))[0]
        raise AssertionError("%s: %d bytes differ, first at byte %d" % (name, len(bad), int(bad[0])))


def _count(v, f, edge, n=None, c=None, position="mean"):
    """The COUNT stage inside exactly the queried workspace -> (the six counts, the arguments for SCATTER, the guard checks)."""
    M, Fc = int(v.shape[0]), int(f.shape[0])
    (ws, c0), (count, c1) = _g((ops.mesh_simplify_workspace_bytes(M, Fc),), torch.uint8), _g((6,), torch.int64)
    voxel = edge if isinstance(edge, torch.Tensor) else torch.full((), float(edge), device="cuda", dtype=torch.float32)
    args = dict(vertices=v, faces=f, voxel=voxel, ws=ws, normals=n, colors=c, position=POS[position], out_count=count)
    ops.mesh_simplify(L.MS_COUNT, **args)
    torch.cuda.synchronize()
    c0("mesh_simplify COUNT ws")
    c1("mesh_simplify COUNT counts")
    return [int(x) for x in count.cpu()], args, (c0, c1)


def _device(v, f, edge, n=None, c=None, position="mean", short=(0, 0)):
    """COUNT, the counts, SCATTER into guarded buffers of exactly (M' - short[0], F' - short[1]) entries -> (counts, dict of tensors)."""
    counts, args, checks = _count(v, f, edge, n, c, position)
    Mo, Fo = counts[:2]
    cm, cf = max(Mo - short[0], 0), max(Fo - short[1], 0)
    (ov, c2), (on, c3), (oc, c4) = _g((max(cm, 1), 3), torch.float32), _g((max(cm, 1), 3), torch.float32), _g((max(cm, 1), 3), torch.uint8)
    (src, c5), (cnt, c6), (of, c7) = _g((max(cm, 1),), torch.int64), _g((max(cm, 1),), torch.int32), _g((max(cf, 1), 3), torch.int32)
    if not cm:                                                                # nothing may be written at all: one guarded element each
        ov, on, oc, src, cnt = ov[:0], on[:0], oc[:0], src[:0], cnt[:0]
    if not cf:
        of = of[:0]
    ops.mesh_simplify(L.MS_SCATTER, vertex_capacity=cm, face_capacity=cf, out_vertices=ov, out_normals=on if n is not None else None,
                      out_colors=oc if c is not None else None, source_index=src, vertex_count=cnt, out_faces=of, **args)
    torch.cuda.synchronize()
    for chk in checks + (c2, c3, c4, c5, c6, c7):
        chk("mesh_simplify SCATTER")
    untouched = ([c2, c3, c4, c5, c6] if not cm else []) + ([c7] if not cf else []) + ([c3] if n is None else []) + ([c4] if c is None else [])
    for chk in untouched:
        assert bool((chk.buffer == GUARD_BYTE).all())
    return counts, dict(vertices=ov, faces=of, normals=on if n is not None else None, colors=oc if c is not None else None, source_index=src,
                        vertex_count=cnt)


def _check(name, v, f, edge, n=None, c=None, position="mean", reps=2):
    """The device against the twin, `reps` times -> the twin's result."""
    want = twin.simplify(v, f, F(edge), n, c, position)
    dv, df, dn, dc = _dev(v), _dev(f), _dev(n), _dev(c)
    for rep in range(reps):
        counts, got = _device(dv, df, edge, dn, dc, position)
        assert counts == want["counts"].tolist(), (name, counts, want["counts"].tolist())
        for k in KEYS:
            assert (got[k] is None) == (want[k] is None), (name, k)
            if got[k] is not None:
                _same(got[k], want[k], "%s %s" % (name, k))
    return want


@functools.lru_cache(maxsize=None)
def _sheet():
    return twin.double_sheet()


# ---------------------------------------------------------------------------------------------
# every output equals the twin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,degenerate", [(0.11, 100), (0.06, 100), (0.031, 0)])
def test_double_sheet_equals_the_twin(edge, degenerate):
    """Condition: the twin reports at least 100 duplicates at every edge and at least 100 degenerate faces at 0.11 and 0.06, so the case
    cannot pass with either face rule idle. At 0.031 the sheet's 1 / 32 spacing is wider than the cell: neighbours never share one,
    there is no degenerate face to find (4096 = survivors + duplicates), and the duplicate rule carries that edge alone. The twin's
    figures for this seed: 0.11 -> 100 vertices, 162 faces, 3772 degenerate, 162 duplicates; 0.06 -> 289, 512, 3072, 512;
    0.031 -> 1153, 2314, 0, 1782."""
    v, f, n, c = _sheet()
    assert v.shape == (2178, 3) and f.shape == (4096, 3)
    for position in ("mean", "first"):
        want = _check("double sheet %g %s" % (edge, position), v, f, edge, n, c, position)
        counts = want["counts"]
        print("edge %g: %d vertices, %d faces, %d cells, %d degenerate, %d duplicates" % ((edge,) + tuple(int(x) for x in counts[[0, 1, 3, 4, 5]])))
        assert counts[5] >= 100 and counts[4] >= degenerate and counts[0] > 50 and counts[1] > 50, counts


def test_bad_input_one_cell_and_hot_cell():
    v, f, n, c = twin.bad_input_sheet()
    want = _check("bad input", v, f, 0.06, n, c)
    assert 40 not in want["source_index"] and 700 not in want["source_index"] and want["counts"][1] > 100
    for bad in (10, 2000, 3000):
        assert bad not in want["face_index"]
    v, f, n, c = _sheet()
    one = _check("one cell", v, f, 5.0, n, c)
    assert one["counts"].tolist() == [0, 0, 0, 1, 4096, 0]
    mesh = postprocess.simplify_mesh(postprocess.Mesh(_dev(v), _dev(f), _dev(n), _dev(c), np.eye(4)), voxel_size=5.0)
    assert isinstance(mesh, postprocess.SimplifiedMesh) and mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)
    assert mesh.faces.dtype == torch.int32 and mesh.source_index.shape == (0,) and (mesh.cells, mesh.degenerate_faces) == (1, 4096)
    hv, hf, hn, hc = twin.hot_cell_sheet()
    hot = _check("hot cell", hv, hf, 0.06, hn, hc)
    assert hot["vertex_count"].max() >= 4096                                 # thousands of vertices add into one slot's sums


def test_collisions_both_tables_probe_and_runs_are_identical():
    v, f, n, c = twin.collision_cloud()
    edge = 0.04
    cells, triples = twin.table_keys(v, f, F(edge))
    assert len(v) == 20000 and 3000 < cells < 8000 and triples > 1000        # both tables hold more than 1000 keys
    want = _check("collisions", v, f, edge, n, c)
    assert want["counts"][3] == cells and want["counts"][1] == triples and want["counts"][5] > 0
    dv, df, dn, dc = _dev(v), _dev(f), _dev(n), _dev(c)
    a, b = _device(dv, df, edge, dn, dc), _device(dv, df, edge, dn, dc)
    assert a[0] == b[0]
    for k in KEYS:
        assert torch.equal(a[1][k].contiguous().view(-1).view(torch.uint8), b[1][k].contiguous().view(-1).view(torch.uint8)), k
    rev = np.ascontiguousarray(f[::-1])
    want_rev = _check("collisions, faces reversed", v, rev, edge, n, c)
    for k in ("vertices", "normals", "colors", "source_index", "vertex_count", "counts"):
        assert np.array_equal(want_rev[k].view(np.uint8), want[k].view(np.uint8)), k
    assert not np.array_equal(want_rev["faces"], want["faces"][::-1])        # somewhere the other copy of a duplicate won


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_attributes(with_normals, with_colors):
    v, f, n, c = _sheet()
    n = twin.odd_normals(v, n, F(0.06)) if with_normals else None
    want = _check("attributes", v, f, 0.06, n, c if with_colors else None)
    if with_normals:
        zero = (want["normals"] == 0).all(axis=1)
        assert zero.any() and (want["vertex_count"][zero] >= 3).all()        # the cancelling pair: a zero sum gives (0, 0, 0)
        assert np.isfinite(want["normals"]).all()


# ---------------------------------------------------------------------------------------------
# the grid is ovg_voxel_downsample's; both flags
# ---------------------------------------------------------------------------------------------
def test_cells_match_voxel_downsample_and_both_flags_are_raised():
    v, f, n, c = twin.bad_input_sheet()
    dv, df = _dev(v), _dev(f)
    one = torch.ones((), device="cuda")
    cloud = postprocess.PointCloud(dv, _dev(c), torch.zeros((), device="cuda"), one, np.eye(4), None)
    for edge in (0.11, 0.06, 0.031):
        counts, got = _device(dv, df, edge)
        kept = postprocess.voxel_downsample(cloud, voxel_size=edge)
        assert counts[3] == len(kept.indices)                                 # occupied cells == the points the decimation keeps
        assert set(got["source_index"].cpu().tolist()) <= set(kept.indices.cpu().tolist())
    ok = np.isfinite(v).all(axis=1)
    extent = float((v[ok].max(axis=0) - v[ok].min(axis=0)).max())
    mesh = postprocess.Mesh(dv, df, _dev(n), _dev(c), np.eye(4), None, one)
    for edge, flag in ((torch.full((), extent / (1 << 22), device="cuda"), L.MS_OVERFLOW), (torch.zeros((), device="cuda"), L.MS_BAD_VOXEL)):
        counts, _ = _device(dv, df, edge)
        assert counts == [0, 0, flag, 0, 0, 0]
        with pytest.raises(ValueError):
            postprocess.simplify_mesh(mesh, voxel_size=edge)
    with pytest.raises(ValueError):
        postprocess.simplify_mesh(mesh, voxel_size=extent / (1 << 22))
    with pytest.raises(twin.Flagged):
        twin.simplify(v, f, F(extent / (1 << 22)))


# ---------------------------------------------------------------------------------------------
# the glue
# ---------------------------------------------------------------------------------------------
def _mesh_dict(mesh):
    return {k: getattr(mesh, k) for k in KEYS}


def test_glue_from_the_volume_to_the_rasteriser_and_the_writer(tmp_path):
    tsdf, weight, origin, voxel, _ = tsdf_twin.sdf_volume("sphere", 9)
    vol = postprocess.tsdf_volume([float(x) for x in origin], float(voxel), (9, 9, 9), color=False)
    vol.tsdf.copy_(_dev(tsdf))
    vol.weight.copy_(_dev(weight))
    vol.scene_scale = torch.full((), 2.0, device="cuda")
    full = postprocess.tsdf_extract(vol)
    reads = []
    names = ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__")
    orig = {k: getattr(torch.Tensor, k) for k in names}

    def spy(name):
        def fn(self, *a, **k):
            if self.is_cuda:
                reads.append((name, tuple(self.shape)))
            return orig[name](self, *a, **k)
        return fn
    for k in names:
        setattr(torch.Tensor, k, spy(k))
    try:
        mesh = postprocess.simplify_mesh(full, rel_size=0.15)                 # the edge is f32(0.15) * scene_scale, multiplied on the device
    finally:
        for k in names:
            setattr(torch.Tensor, k, orig[k])
    assert reads == [("cpu", (6,))]                                           # exactly one synchronisation: the six counts
    edge = F(0.15) * F(2.0)
    want = twin.simplify(full.vertices.cpu().numpy(), full.faces.cpu().numpy(), edge, full.normals.cpu().numpy(), full.colors.cpu().numpy())
    M, Fc = len(want["vertices"]), len(want["faces"])
    assert 40 <= M < full.vertices.shape[0] and 80 <= Fc < full.faces.shape[0]
    for k in KEYS:
        _same(getattr(mesh, k), want[k], "simplified sphere %s" % k)
    assert [mesh.cells, mesh.degenerate_faces, mesh.duplicate_faces] == want["counts"][3:].tolist()
    assert mesh.transform is full.transform and mesh.extrinsic is full.extrinsic and mesh.scene_scale is full.scene_scale and mesh.pixel_index is None
    ext = tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 2.0)[:2]
    res = postprocess.render_mesh(mesh, ext, tsdf_twin.pinhole(32, 32, 60.0), (32, 32), return_index=True)
    assert int((res.index >= 0).sum()) > 100 and int(res.index.max()) < Fc    # a non-empty image of the simplified faces
    path = str(tmp_path / "s.glb")
    postprocess.write_mesh_glb(path, mesh)
    raw = open(path, "rb").read()
    assert raw[:4] == b"glTF" and struct.unpack("<I", raw[8:12])[0] == len(raw)
    gltf = json.loads(raw[20:20 + struct.unpack("<I", raw[12:16])[0]])
    assert gltf["accessors"][0]["count"] == M and gltf["accessors"][3]["count"] == 3 * Fc
    postprocess.write_mesh_ply(str(tmp_path / "s.ply"), mesh)
    assert len(postprocess.mesh_to_point_cloud(mesh)) == M
    first = postprocess.simplify_mesh(full, voxel_size=float(edge), position="first")
    assert torch.equal(first.vertices, full.vertices[first.source_index]) and torch.equal(first.faces, mesh.faces)
    empty = postprocess.simplify_mesh(postprocess.tsdf_extract(postprocess.tsdf_volume((0, 0, 0), 0.1, (5, 4, 3))), voxel_size=0.1)
    assert isinstance(empty, postprocess.SimplifiedMesh) and empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)


def test_glue_from_the_map_mesh_keeps_the_pixels():
    s = mapgeom_scenes.box_scene()
    z = mapgeom_twin.map_depth(points=s["points"], cams=s["cams"], valid=s["valid"], near=mapgeom_scenes.NEAR)
    full = postprocess.triangulate_maps(_dev(s["points"]), _dev(z), keep=_dev(s["keep"]), images=_dev(s["colors"]),
                                        normals=_dev(mapgeom_twin.map_normals(s["points"], z, 0.03)))
    assert isinstance(full, postprocess.MapMesh) and full.vertices.shape[0] > 1000
    mesh = postprocess.simplify_mesh(full, rel_size=0.02)
    edge = F(0.02) * F(float(full.scene_scale))
    want = twin.simplify(full.vertices.cpu().numpy(), full.faces.cpu().numpy(), edge, full.normals.cpu().numpy(), full.colors.cpu().numpy())
    assert 50 < len(want["vertices"]) < full.vertices.shape[0] // 2 and len(want["faces"]) > 50
    for k in KEYS:
        _same(getattr(mesh, k), want[k], "simplified box %s" % k)
    assert torch.equal(mesh.pixel_index, full.pixel_index[mesh.source_index]) and mesh.pixel_index.dtype == torch.int64
    assert mesh.scene_scale is full.scene_scale and mesh.extrinsic is full.extrinsic


# ---------------------------------------------------------------------------------------------
# capacities
# ---------------------------------------------------------------------------------------------
def test_short_capacities_write_only_the_first_entries():
    v, f, n, c = _sheet()
    want = twin.simplify(v, f, F(0.06), n, c)
    M, Fc = len(want["vertices"]), len(want["faces"])
    dv, df, dn, dc = _dev(v), _dev(f), _dev(n), _dev(c)
    for short in ((3, 5), (M - 1, Fc - 1), (M, 0), (0, Fc)):
        counts, got = _device(dv, df, 0.06, dn, dc, short=short)
        assert counts == want["counts"].tolist()
        for k in KEYS:
            _same(got[k], want[k][:(Fc - short[1]) if k == "faces" else (M - short[0])], "short %r %s" % (short, k))


# ---------------------------------------------------------------------------------------------
# refusals on the device path write nothing
# ---------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    v, f, n, c = (_dev(a) for a in _sheet())
    need = ops.mesh_simplify_workspace_bytes(2178, 4096)
    (ws, c0), (count, c1) = _g((need,), torch.uint8), _g((6,), torch.int64)
    voxel = torch.full((), 0.06, device="cuda")
    with pytest.raises(L.OvgError):
        ops.mesh_simplify(L.MS_COUNT, v, f, voxel, ws[:-1], out_count=count)                    # one byte short
    with pytest.raises(L.OvgError):
        ops.mesh_simplify(L.MS_COUNT, v, f, voxel, ws[16:], out_count=count)
    with pytest.raises(L.OvgError):
        ops.mesh_simplify(L.MS_COUNT, v.cpu(), f, voxel, ws, out_count=count)
    torch.cuda.synchronize()
    assert bool((c0.buffer == GUARD_BYTE).all()) and bool((c1.buffer == GUARD_BYTE).all())


# ---------------------------------------------------------------------------------------------
# the stream and no-sync contract (recorded for test_gpu_stream_contract's coverage test)
# ---------------------------------------------------------------------------------------------
def test_mesh_simplify_entry_is_gated():
    v, f, n, c = _sheet()
    v2, f2, n2, c2 = twin.double_sheet(seed=4)                                # the decoy: the other seed, valid data of the same kind
    edge = F(0.06)
    want = twin.simplify(v, f, edge, n, c)
    M, Fc = len(want["vertices"]), len(want["faces"])
    t = torch.from_numpy

    def case(position):
        def build():
            cs = sc.Case("mesh_simplify COUNT then SCATTER, double sheet, normals + colors, %s" % position)
            dv, dn, dc = cs.inp(t(v), t(v2)), cs.inp(t(n), t(n2)), cs.inp(t(c), t(c2))
            df, voxel = cs.const(t(f)), cs.const(torch.full((), float(edge)))
            ws, count = cs.ws(ops.mesh_simplify_workspace_bytes(len(v), len(f))), cs.out((6,), torch.int64)
            ov, on, oc = cs.out((M, 3), torch.float32), cs.out((M, 3), torch.float32), cs.out((M, 3), torch.uint8)
            src, cnt, of = cs.out((M,), torch.int64), cs.out((M,), torch.int32), cs.out((Fc, 3), torch.int32)

            def call():
                args = dict(vertices=dv, faces=df, voxel=voxel, ws=ws, normals=dn, colors=dc, position=POS[position], out_count=count)
                ops.mesh_simplify(L.MS_COUNT, **args)
                ops.mesh_simplify(L.MS_SCATTER, vertex_capacity=M, face_capacity=Fc, out_vertices=ov, out_normals=on, out_colors=oc,
                                  source_index=src, vertex_count=cnt, out_faces=of, **args)
            cs.call = call
            return cs
        return build

    cases = tsc.family([case("mean"), case("first")], "mesh simplification")
    assert {e for cs in cases for e in cs.entries} == {"ovg_mesh_simplify"}
    assert "ovg_mesh_simplify" in tsc.COVERED
    _same(cases[0].outs[1], want["vertices"], "gated vertices")               # outs[0] is the counts
    _same(cases[0].outs[0], want["counts"], "gated counts")
