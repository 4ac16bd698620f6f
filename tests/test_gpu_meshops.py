"""ovg_mesh_topology, ovg_mesh_select, ovg_mesh_smooth and their postprocess API on the device against tests/meshops_twin.py: every output
byte for byte in guarded buffers of exactly the queried / counted sizes, every case twice. The zoo (two spheres, an open sheet, a triple
edge, a corner contact, a duplicated face, junk faces, loose vertices), the union-find under contention, a row of 10 000 neighbours, the
scan borders of the selection, smoothing in all its arguments, the glue from the two mesh producers to the reducer, the rasteriser and the
writer, refused calls, and the gated cases for the stream contract's coverage test."""
import functools

import numpy as np
import pytest
import torch

import mapgeom_scenes
import mapgeom_twin
import meshops_twin as twin
import meshsimp_twin
import stream_contract as sc
import test_gpu_stream_contract as tsc
import tsdf_twin
from kernel_guards import GUARD_BYTE, guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32


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


def _untouched(*checks):
    for chk in checks:
        assert bool((chk.buffer == GUARD_BYTE).all())


@functools.lru_cache(maxsize=None)
def _zoo(seed=0):
    return twin.zoo(seed)


@functools.lru_cache(maxsize=None)
def _sphere3():
    return twin.noisy_icosphere(3, noise=0.02, seed=1)


# ---------------------------------------------------------------------------------------------
# the three entries in guarded buffers of exactly the queried / counted sizes
# ---------------------------------------------------------------------------------------------
def _topology(v, f):
    M, Fc = int(v.shape[0]), int(f.shape[0])
    (ws, c0), (vr, c1), (fr, c2) = _g((ops.mesh_topology_workspace_bytes(M, Fc),), torch.uint8), _g((M,), torch.int32), _g((Fc,), torch.int32)
    (fl, c3), (cnt, c4) = _g((M,), torch.uint8), _g((8,), torch.int64)
    ops.mesh_topology(v, f, ws, vr, fr, fl, cnt)
    torch.cuda.synchronize()
    for chk in (c0, c1, c2, c3, c4):
        chk("mesh_topology")
    return dict(vertex_root=vr, face_root=fr, vertex_flags=fl, counts=cnt)


def _check_topology(name, v, f, reps=2):
    want = twin.topology(v, f)
    dv, df = _dev(v), _dev(f)
    for _ in range(reps):
        got = _topology(dv, df)
        for k in want:
            _same(got[k], want[k], "%s %s" % (name, k))
    return want


def _select(v, f, face_keep=None, vertex_keep=None, short=(0, 0), zero=False):
    """COUNT, the counts, SCATTER into buffers of exactly (M' - short[0], F' - short[1]) entries (zero: capacities 0) -> (counts, tensors)."""
    M, Fc = int(v.shape[0]), int(f.shape[0])
    (ws, c0), (cnt, c1) = _g((ops.mesh_select_workspace_bytes(M, Fc),), torch.uint8), _g((2,), torch.int64)
    args = dict(vertices=v, faces=f, ws=ws, face_keep=face_keep, vertex_keep=vertex_keep, out_count=cnt)
    ops.mesh_select(L.MSEL_COUNT, **args)
    torch.cuda.synchronize()
    c0("mesh_select COUNT ws")
    c1("mesh_select COUNT counts")
    counts = [int(x) for x in cnt.cpu()]
    cm, cf = (0, 0) if zero else (max(counts[0] - short[0], 0), max(counts[1] - short[1], 0))
    (ov, c2), (src, c3), (of, c4), (fi, c5) = (_g((max(cm, 1), 3), torch.float32), _g((max(cm, 1),), torch.int64), _g((max(cf, 1), 3), torch.int32),
                                               _g((max(cf, 1),), torch.int64))
    if not cm:                                                                # nothing may be written at all: one guarded element each
        ov, src = ov[:0], src[:0]
    if not cf:
        of, fi = of[:0], fi[:0]
    ops.mesh_select(L.MSEL_SCATTER, vertex_capacity=cm, face_capacity=cf, out_vertices=ov, source_index=src, out_faces=of, face_index=fi, **args)
    torch.cuda.synchronize()
    for chk in (c0, c1, c2, c3, c4, c5):
        chk("mesh_select SCATTER")
    _untouched(*(([c2, c3] if not cm else []) + ([c4, c5] if not cf else [])))
    return counts, dict(vertices=ov, source_index=src, faces=of, face_index=fi)


def _smooth(v, f, iterations, lam=0.5, mu=-0.53, fixed=None, fix_boundary=True, normals=True):
    M, Fc = int(v.shape[0]), int(f.shape[0])
    (ws, c0), (ov, c1), (on, c2), (st, c3) = (_g((ops.mesh_smooth_workspace_bytes(M, Fc),), torch.uint8), _g((M, 3), torch.float32),
                                              _g((M, 3), torch.float32), _g((1,), torch.int64))
    ops.mesh_smooth(v, f, ws, iterations, lam, mu, ov, st, fixed=fixed, fix_boundary=fix_boundary, out_normals=on if normals else None)
    torch.cuda.synchronize()
    for chk in (c0, c1, c2, c3):
        chk("mesh_smooth")
    if not normals:
        _untouched(c2)
    return dict(vertices=ov, normals=on if normals else None), int(st.cpu())


def _check_smooth(name, v, f, iterations, reps=2, **kw):
    want = twin.smooth(v, f, iterations, **kw)
    dv, df = _dev(v), _dev(f)
    dkw = {**kw, "fixed": _dev(kw["fixed"])} if kw.get("fixed") is not None else kw
    for _ in range(reps):
        got, status = _smooth(dv, df, iterations, **dkw)
        assert status == 0, (name, status)
        for k in ("vertices", "normals"):
            assert (got[k] is None) == (want[k] is None), (name, k)
            if got[k] is not None:
                _same(got[k], want[k], "%s %s" % (name, k))
    return want


def _moved(out, v):
    return ~(np.ascontiguousarray(out).view(np.uint32) == np.ascontiguousarray(v).view(np.uint32)).all(axis=1)


# ---------------------------------------------------------------------------------------------
# 1. the zoo
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_zoo_equals_the_twin(seed):
    z = _zoo(seed)
    v, f = z["vertices"], z["faces"]
    want = _check_topology("zoo", v, f)
    assert want["counts"].tolist() == [535, 298, 824, 44, 1, 42, 2, 0]
    mesh = postprocess.Mesh(_dev(v), _dev(f), None, None, np.eye(4))
    for order in ("size", "index"):
        lab = twin.labels(want["vertex_root"], want["face_root"], order)
        for _ in range(2):
            top = postprocess.mesh_topology(mesh, order=order)
            for k in ("vertex_root", "face_root", "vertex_flags"):
                _same(getattr(top, k), want[k], "mesh_topology %s" % k)
            for k in ("vertex_labels", "face_labels", "roots", "face_sizes", "vertex_sizes"):
                _same(getattr(top, k), lab[k], "mesh_topology %s %s" % (order, k))
            assert [top.live_faces, top.referenced_vertices, top.edges, top.boundary_edges, top.nonmanifold_edges, top.boundary_vertices,
                    top.nonmanifold_vertices] == want["counts"][:7].tolist()
            assert top.num_components == 6 and top.euler == 298 - 824 + 535 and not top.closed
    sv, sf = twin.icosphere(2)
    top = postprocess.mesh_topology(postprocess.Mesh(_dev(sv), _dev(sf), None, None, np.eye(4)))
    assert top.closed and top.euler == 2 and top.num_components == 1 and top.nonmanifold_edges == 0


# ---------------------------------------------------------------------------------------------
# 2. the union-find under contention
# ---------------------------------------------------------------------------------------------
def test_union_find_under_contention():
    v, f = twin.ribbon(35000)
    assert f.shape == (69998, 3)
    want = _check_topology("ribbon", v, f)
    assert (want["vertex_root"] == 0).all() and (want["face_root"] == 0).all() and want["counts"][7] == 0
    v, f, quad = twin.quads(3000)
    want = _check_topology("quads", v, f)
    lowest = np.empty(12000, np.int32)
    lowest[quad.reshape(-1)] = np.repeat(quad.min(axis=1), 4)
    assert np.array_equal(want["vertex_root"], lowest) and len(np.unique(want["vertex_root"])) == 3000


# ---------------------------------------------------------------------------------------------
# 3. the hot vertex
# ---------------------------------------------------------------------------------------------
def test_hot_vertex():
    v, f = twin.fan(5000)
    assert v.shape == (5001, 3) and f.shape == (5000, 3)
    want = _check_topology("fan", v, f)
    assert want["counts"].tolist() == [5000, 5001, 10000, 5000, 0, 5000, 0, 0]
    held = _check_smooth("fan, boundary fixed", v, f, 2)
    moved = _moved(held["vertices"], v)
    assert moved[0] and not moved[1:].any()                                   # vertex 0: one row of 10 000 neighbours
    free = _check_smooth("fan, boundary free", v, f, 2, fix_boundary=False)
    assert _moved(free["vertices"], v).all()


# ---------------------------------------------------------------------------------------------
# 4. scan borders of the selection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 65])
def test_select_at_the_scan_borders(nx):
    v, f = twin.grid_sheet(nx, 64)
    M, Fc = len(v), len(f)
    assert (M, Fc) == (nx * 64, 2 * (nx - 1) * 63) and (M == 4096) == (nx == 64)
    j = np.arange(Fc) % ((nx - 1) * 63)
    checker = (((j // (nx - 1)) + (j % (nx - 1))) % 2 == 0).astype(np.uint8)
    stripes = ((np.arange(M) % nx) % 8 != 3).astype(np.uint8)
    dv, df = _dev(v), _dev(f)
    for name, fk, vk in (("checkerboard", checker, None), ("stripes", None, stripes), ("both", checker, stripes), ("neither", None, None)):
        want = twin.select(v, f, fk, vk)
        Mo, Fo = (int(x) for x in want["counts"])
        assert 0 < Fo and (name == "neither" or Fo < Fc)
        for short in ((0, 0), (0, 0), (3, 5), (Mo - 1, Fo - 1), (Mo, 0), (0, Fo)):
            counts, got = _select(dv, df, _dev(fk), _dev(vk), short=short)
            assert counts == [Mo, Fo], (name, counts)
            for k in ("vertices", "source_index", "faces", "face_index"):
                n = (Fo - short[1]) if k in ("faces", "face_index") else (Mo - short[0])
                _same(got[k], want[k][:n], "%s %r %s" % (name, short, k))
        counts, _ = _select(dv, df, _dev(fk), _dev(vk), zero=True)            # capacities 0: nothing is written
        assert counts == [Mo, Fo]


# ---------------------------------------------------------------------------------------------
# 5. smoothing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [-0.53, 0.0])
@pytest.mark.parametrize("iterations", [1, 2, 10])
def test_smoothing_equals_the_twin(iterations, mu):
    v, f = _sphere3()
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    want = _check_smooth("sphere", v, f, iterations, mu=mu)
    assert _moved(want["vertices"], v).all()
    if iterations == 10:
        assert twin.radius_spread(want["vertices"]) < twin.radius_spread(v)


def test_smoothing_holds_what_it_must():
    sv, sf = twin.grid_sheet(9, 9)
    sv[:, 2] = (0.01 * np.random.default_rng(3).standard_normal(81)).astype(F)
    rim = twin.sheet_rim(9, 9)
    out = _check_smooth("sheet", sv, sf, 5)
    moved = _moved(out["vertices"], sv)
    assert not moved[rim].any() and moved[~rim].all()
    v, f = _sphere3()
    fixed = (np.arange(len(v)) % 5 == 0).astype(np.uint8)
    out = _check_smooth("fixed mask", v, f, 3, fixed=fixed)
    moved = _moved(out["vertices"], v)
    assert not moved[fixed != 0].any() and moved[fixed == 0].all()
    z = _zoo(0)                                                               # a face naming a NaN vertex, junk faces, loose vertices
    out = _check_smooth("zoo", z["vertices"], z["faces"], 3)
    nan = int(z["parts"]["nan"][0])
    assert np.isnan(out["vertices"][nan]).any() and not _moved(out["vertices"], z["vertices"])[z["parts"]["loose"]].any()
    assert (out["normals"][nan] == 0).all() and (out["normals"][z["parts"]["loose"]] == 0).all()
    _check_smooth("zoo without normals", z["vertices"], z["faces"], 2, normals=False)


def test_no_iteration_copies_and_computes_normals():
    v, f = _sphere3()
    want = _check_smooth("normals only", v, f, 0)
    assert not _moved(want["vertices"], v).any()
    cos = (want["normals"].astype(np.float64) * v / np.linalg.norm(v, axis=1, keepdims=True)).sum(axis=1)
    assert (cos > 0.9).all()                                                  # outward, near the radial direction
    mesh = postprocess.Mesh(_dev(v), _dev(f), None, None, np.eye(4))
    _same(postprocess.mesh_vertex_normals(mesh), want["normals"], "mesh_vertex_normals")
    z = _zoo(1)
    _check_smooth("zoo normals only", z["vertices"], z["faces"], 0)


def test_frame_is_laid_anew_in_every_step():
    """One strong inflate step takes the sphere outside the input's bounding box: a frame fixed at the start could not hold the second
    iteration's coordinates (q would leave [0, 2^30]); the twin lays the frame per step and the device agrees byte for byte."""
    v, f = _sphere3()
    once = twin.smooth(v, f, 1, 0.5, -4.0)["vertices"]
    assert (once.min(axis=0) < v.min(axis=0)).all() and (once.max(axis=0) > v.max(axis=0)).all()
    _check_smooth("inflating", v, f, 3, lam=0.5, mu=-4.0)
    big = (v.astype(np.float64) * 3e37).astype(F)
    with pytest.raises(twin.NonFinite):
        twin.smooth(big, f, 4, 1.0, -60.0)
    _, status = _smooth(_dev(big), _dev(f), 4, 1.0, -60.0)
    assert status == L.MSM_NONFINITE
    with pytest.raises(ValueError):
        postprocess.smooth_mesh(postprocess.Mesh(_dev(big), _dev(f), None, None, np.eye(4)), iterations=4, lam=1.0, mu=-60.0)


# ---------------------------------------------------------------------------------------------
# 6. the glue
# ---------------------------------------------------------------------------------------------
def _subset_equals(sub, want, name):
    for k in ("vertices", "faces", "source_index", "face_index"):
        _same(getattr(sub, k), want[k], "%s %s" % (name, k))


def test_keep_largest_on_the_zoo_is_the_sphere():
    z = _zoo(0)
    v, f = z["vertices"], z["faces"]
    nrm = np.random.default_rng(5).standard_normal((len(v), 3)).astype(F)
    col = np.random.default_rng(6).integers(0, 256, (len(v), 3)).astype(np.uint8)
    mesh = postprocess.Mesh(_dev(v), _dev(f), _dev(nrm), _dev(col), np.eye(4), None, torch.ones((), device="cuda"))
    top = twin.topology(v, f)
    big = int(z["parts"]["sphere2"][0])
    want = twin.select(v, f, face_keep=top["face_root"] == big)
    for kw in (dict(keep_largest=True), dict(min_faces=129), dict(rel_faces=0.5)):
        sub = postprocess.remove_small_components(mesh, **kw)
        assert isinstance(sub, postprocess.MeshSubset) and sub.vertices.shape == (162, 3) and sub.faces.shape == (320, 3), kw
        _subset_equals(sub, want, "largest %r" % (kw,))
        _same(sub.normals, nrm[want["source_index"]], "normals")
        _same(sub.colors, col[want["source_index"]], "colors")
        assert sub.transform is mesh.transform and sub.scene_scale is mesh.scene_scale and sub.pixel_index is None
    three = postprocess.remove_small_components(mesh, min_faces=80)
    keep = np.isin(top["face_root"], [int(z["parts"][k][0]) for k in ("sphere2", "sphere1", "sheet")])
    _subset_equals(three, twin.select(v, f, face_keep=keep), "three pieces")
    clean = postprocess.select_faces(mesh)
    _subset_equals(clean, twin.select(v, f), "live faces only")
    t2 = postprocess.mesh_topology(sub)
    assert t2.closed and t2.euler == 2 and t2.num_components == 1 and t2.live_faces == 320


def test_glue_from_the_volume_to_the_rasteriser_and_the_writer(tmp_path):
    tsdf, weight, origin, voxel, _ = tsdf_twin.sdf_volume("sphere", 9)
    vol = postprocess.tsdf_volume([float(x) for x in origin], float(voxel), (9, 9, 9), color=False)
    vol.tsdf.copy_(_dev(tsdf))
    vol.weight.copy_(_dev(weight))
    vol.scene_scale = torch.full((), 2.0, device="cuda")
    full = postprocess.tsdf_extract(vol)
    v, f = full.vertices.cpu().numpy(), full.faces.cpu().numpy()
    top = postprocess.mesh_topology(full)
    want_top = twin.topology(v, f)
    for k in ("vertex_root", "face_root", "vertex_flags"):
        _same(getattr(top, k), want_top[k], "fused %s" % k)
    assert top.live_faces == len(f) and top.num_components >= 1
    lab = twin.labels(want_top["vertex_root"], want_top["face_root"])
    largest = twin.select(v, f, face_keep=lab["face_labels"] == 0)
    for kw in (dict(keep_largest=True), dict(min_faces=int(lab["face_sizes"][0])), dict(rel_faces=(float(lab["face_sizes"][0]) - 0.5) / len(f))):
        sub = postprocess.remove_small_components(full, **kw)
        _subset_equals(sub, largest, "fused %r" % (kw,))
    assert sub.scene_scale is full.scene_scale and sub.extrinsic is full.extrinsic and sub.transform is full.transform
    smooth = postprocess.smooth_mesh(sub, iterations=3)
    want = twin.smooth(largest["vertices"], largest["faces"], 3)
    _same(smooth.vertices, want["vertices"], "smoothed fused vertices")
    _same(smooth.normals, want["normals"], "smoothed fused normals")
    assert type(smooth) is postprocess.MeshSubset and smooth.faces is sub.faces and smooth.colors is sub.colors and smooth.source_index is sub.source_index
    assert postprocess.smooth_mesh(sub, iterations=1, normals="keep").normals is sub.normals
    assert postprocess.smooth_mesh(sub, iterations=1, normals=None).normals is None
    small = postprocess.simplify_mesh(smooth, rel_size=0.15)
    ref = meshsimp_twin.simplify(want["vertices"], largest["faces"], F(0.15) * F(2.0), want["normals"], sub.colors.cpu().numpy())
    _same(small.vertices, ref["vertices"], "simplified after smoothing")
    ext = tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 2.0)[:2]
    res = postprocess.render_mesh(smooth, ext, tsdf_twin.pinhole(32, 32, 60.0), (32, 32), return_index=True)
    assert int((res.index >= 0).sum()) > 100 and int(res.index.max()) < smooth.faces.shape[0]
    postprocess.write_mesh_ply(str(tmp_path / "s.ply"), smooth)
    head = open(str(tmp_path / "s.ply"), "rb").read(400).decode("latin-1")
    assert "element vertex %d" % smooth.vertices.shape[0] in head and "element face %d" % smooth.faces.shape[0] in head
    empty = postprocess.tsdf_extract(postprocess.tsdf_volume((0, 0, 0), 0.1, (5, 4, 3)))
    assert postprocess.mesh_topology(empty).num_components == 0 and postprocess.smooth_mesh(empty).vertices.shape == (0, 3)
    gone = postprocess.remove_small_components(empty, keep_largest=True)
    assert isinstance(gone, postprocess.MeshSubset) and gone.vertices.shape == (0, 3) and gone.faces.shape == (0, 3)


def test_glue_from_the_map_mesh_keeps_the_pixels():
    s = mapgeom_scenes.box_scene()
    z = mapgeom_twin.map_depth(points=s["points"], cams=s["cams"], valid=s["valid"], near=mapgeom_scenes.NEAR)
    full = postprocess.triangulate_maps(_dev(s["points"]), _dev(z), keep=_dev(s["keep"]), images=_dev(s["colors"]),
                                        normals=_dev(mapgeom_twin.map_normals(s["points"], z, 0.03)))
    assert isinstance(full, postprocess.MapMesh) and full.vertices.shape[0] > 1000
    v, f = full.vertices.cpu().numpy(), full.faces.cpu().numpy()
    top = postprocess.mesh_topology(full)
    lab = twin.labels(*(twin.topology(v, f)[k] for k in ("vertex_root", "face_root")))
    _same(top.face_labels, lab["face_labels"], "map mesh face labels")
    _same(top.face_sizes, lab["face_sizes"], "map mesh face sizes")
    sub = postprocess.remove_small_components(full, keep_largest=True)
    want = twin.select(v, f, face_keep=lab["face_labels"] == 0)
    _subset_equals(sub, want, "map mesh largest")
    assert torch.equal(sub.pixel_index, full.pixel_index[sub.source_index]) and sub.pixel_index.dtype == torch.int64
    smooth = postprocess.smooth_mesh(full, iterations=2)
    assert type(smooth) is postprocess.MapMesh and smooth.pixel_index is full.pixel_index and smooth.conf_threshold is full.conf_threshold
    ref = twin.smooth(v, f, 2)
    _same(smooth.vertices, ref["vertices"], "smoothed map mesh")
    _same(smooth.normals, ref["normals"], "smoothed map mesh normals")
    small = postprocess.simplify_mesh(postprocess.smooth_mesh(sub, iterations=2), rel_size=0.02)
    assert torch.equal(small.pixel_index, sub.pixel_index[small.source_index])


# ---------------------------------------------------------------------------------------------
# 7. refused calls write nothing
# ---------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    z = _zoo(0)
    v, f = _dev(z["vertices"]), _dev(z["faces"])
    M, Fc = int(v.shape[0]), int(f.shape[0])
    i32, i64, u8, f32 = torch.int32, torch.int64, torch.uint8, torch.float32
    checks = []

    def g(shape, dtype):
        t, chk = _g(shape, dtype)
        checks.append(chk)
        return t
    ws = g((max(ops.mesh_topology_workspace_bytes(M, Fc), ops.mesh_select_workspace_bytes(M, Fc), ops.mesh_smooth_workspace_bytes(M, Fc)),), u8)
    vr, fr, fl, c8 = g((M,), i32), g((Fc,), i32), g((M,), u8), g((8,), i64)
    ov, on, st, c2, of = g((M, 3), f32), g((M, 3), f32), g((1,), i64), g((2,), i64), g((Fc, 3), i32)
    short_t, short_s, short_m = (ws[:ops.mesh_topology_workspace_bytes(M, Fc) - 1], ws[:ops.mesh_select_workspace_bytes(M, Fc) - 1],
                                 ws[:ops.mesh_smooth_workspace_bytes(M, Fc) - 1])
    refused = [lambda: ops.mesh_topology(v, f, short_t, vr, fr, fl, c8), lambda: ops.mesh_topology(v, f, ws[8:], vr, fr, fl, c8),
               lambda: ops.mesh_topology(v.cpu(), f, ws, vr, fr, fl, c8), lambda: ops.mesh_topology(v, f, ws, vr.cpu(), fr, fl, c8),
               lambda: ops.mesh_select(L.MSEL_COUNT, v, f, short_s, out_count=c2), lambda: ops.mesh_select(L.MSEL_COUNT, v, f, ws[8:], out_count=c2),
               lambda: ops.mesh_select(4, v, f, ws, out_count=c2), lambda: ops.mesh_select(L.MSEL_COUNT, v, f.cpu(), ws, out_count=c2),
               lambda: ops.mesh_smooth(v, f, short_m, 2, 0.5, -0.53, ov, st, out_normals=on),
               lambda: ops.mesh_smooth(v, f, ws[8:], 2, 0.5, -0.53, ov, st, out_normals=on),
               lambda: ops.mesh_smooth(v.cpu(), f, ws, 2, 0.5, -0.53, ov, st), lambda: ops.mesh_smooth(v, f, ws, 2, 0.5, -0.53, v, st)]
    for k, call in enumerate(refused):
        with pytest.raises(L.OvgError):
            call()
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream

    def topo(**kw):
        p = L.MeshTopologyParams(vertices=v.data_ptr(), faces=f.data_ptr(), num_vertices=M, num_faces=Fc, vertex_root=vr.data_ptr(),
                                 face_root=fr.data_ptr(), vertex_flags=fl.data_ptr(), out_count=c8.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        for name, val in kw.items():
            setattr(p, name, val)
        return lib.ovg_mesh_topology(p, stream)

    def sel(**kw):
        p = L.MeshSelectParams(vertices=v.data_ptr(), faces=f.data_ptr(), num_vertices=M, num_faces=Fc, stage=L.MSEL_COUNT | L.MSEL_SCATTER,
                               vertex_capacity=M, face_capacity=Fc, out_vertices=ov.data_ptr(), out_faces=of.data_ptr(), out_count=c2.data_ptr(),
                               ws=ws.data_ptr(), ws_bytes=ws.numel())
        for name, val in kw.items():
            setattr(p, name, val)
        return lib.ovg_mesh_select(p, stream)

    def smo(**kw):
        p = L.MeshSmoothParams(vertices=v.data_ptr(), faces=f.data_ptr(), num_vertices=M, num_faces=Fc, iterations=2, fix_boundary=1, lam=0.5, mu=-0.53,
                               out_vertices=ov.data_ptr(), out_normals=on.data_ptr(), out_status=st.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        for name, val in kw.items():
            setattr(p, name, val)
        return lib.ovg_mesh_smooth(p, stream)
    for fn, bads in ((topo, (dict(vertices=None), dict(face_root=None), dict(vertex_root=vr.data_ptr() + 2), dict(out_count=c8.data_ptr() + 4),
                            dict(num_faces=0), dict(num_vertices=1 << 31))),
                     (sel, (dict(faces=None), dict(stage=0), dict(stage=8), dict(out_vertices=None), dict(out_faces=of.data_ptr() + 1),
                            dict(vertex_capacity=-1), dict(out_count=None))),
                     (smo, (dict(out_vertices=None), dict(out_status=None), dict(out_normals=on.data_ptr() + 2), dict(iterations=-1),
                            dict(fix_boundary=3), dict(lam=float("nan")), dict(ws_bytes=16)))):
        for bad in bads:
            assert fn(**bad) == -1, bad
    torch.cuda.synchronize()
    _untouched(*checks)
    assert topo() == 0 and sel() == 0 and smo() == 0                          # the same structs, unbroken, run
    torch.cuda.synchronize()
    for chk in checks:
        chk("after the good calls")


# ---------------------------------------------------------------------------------------------
# 8. the stream and no-sync contract (recorded for test_gpu_stream_contract's coverage test)
# ---------------------------------------------------------------------------------------------
def test_mesh_cleaning_entries_are_gated():
    z0, z1 = _zoo(0), _zoo(1)
    v, f = _sphere3()
    v2 = twin.noisy_icosphere(3, noise=0.02, seed=2)[0]                       # the decoy: another noise, valid data of the same kind
    t = torch.from_numpy
    M, Fc = len(v), len(f)
    keep, keep2 = (np.arange(Fc) % 3 != 0).astype(np.uint8), (np.arange(Fc) % 3 != 1).astype(np.uint8)
    sel = twin.select(v, f, face_keep=keep)
    Mo, Fo = (int(x) for x in sel["counts"])

    def topology():
        cs = sc.Case("mesh_topology, zoo")
        dv, df = cs.inp(t(z0["vertices"]), t(z1["vertices"])), cs.inp(t(z0["faces"]), t(z1["faces"]))
        m, nf = len(z0["vertices"]), len(z0["faces"])
        ws = cs.ws(ops.mesh_topology_workspace_bytes(m, nf))
        cnt, vr, fr, fl = cs.out((8,), torch.int64), cs.out((m,), torch.int32), cs.out((nf,), torch.int32), cs.out((m,), torch.uint8)
        cs.call = lambda: ops.mesh_topology(dv, df, ws, vr, fr, fl, cnt)
        return cs

    def select():
        cs = sc.Case("mesh_select COUNT then SCATTER, sphere, face_keep")
        dv, dk, df = cs.inp(t(v), t(v2)), cs.inp(t(keep), t(keep2)), cs.const(t(f))
        ws, cnt = cs.ws(ops.mesh_select_workspace_bytes(M, Fc)), cs.out((2,), torch.int64)
        ov, src, of, fi = cs.out((Mo, 3), torch.float32), cs.out((Mo,), torch.int64), cs.out((Fo, 3), torch.int32), cs.out((Fo,), torch.int64)

        def call():
            args = dict(vertices=dv, faces=df, ws=ws, face_keep=dk, out_count=cnt)
            ops.mesh_select(L.MSEL_COUNT, **args)
            ops.mesh_select(L.MSEL_SCATTER, vertex_capacity=Mo, face_capacity=Fo, out_vertices=ov, source_index=src, out_faces=of, face_index=fi, **args)
        cs.call = call
        return cs

    def smooth(mu):
        def build():
            cs = sc.Case("mesh_smooth, sphere, 3 iterations, mu %g, normals" % mu)
            dv, df = cs.inp(t(v), t(v2)), cs.const(t(f))
            ws = cs.ws(ops.mesh_smooth_workspace_bytes(M, Fc))
            ov, on, st = cs.out((M, 3), torch.float32), cs.out((M, 3), torch.float32), cs.out((1,), torch.int64)
            cs.call = lambda: ops.mesh_smooth(dv, df, ws, 3, 0.5, mu, ov, st, out_normals=on)
            return cs
        return build

    cases = tsc.family([topology, select, smooth(-0.53), smooth(0.0)], "mesh cleaning")
    assert {e for cs in cases for e in cs.entries} == {"ovg_mesh_topology", "ovg_mesh_select", "ovg_mesh_smooth"}
    for e in ("ovg_mesh_topology", "ovg_mesh_select", "ovg_mesh_smooth"):
        assert e in tsc.COVERED
    want = twin.topology(z0["vertices"], z0["faces"])
    _same(cases[0].outs[0], want["counts"], "gated counts")
    _same(cases[0].outs[1], want["vertex_root"], "gated vertex_root")
    _same(cases[1].outs[1], sel["vertices"], "gated selected vertices")
    _same(cases[2].outs[0], twin.smooth(v, f, 3)["vertices"], "gated smoothed vertices")
