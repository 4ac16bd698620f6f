"""Mesh cleaning, host side: the numpy twin (tests/meshops_twin.py) against its naive second form, against scipy's connected components and
against closed-form facts of the test meshes; the properties Taubin smoothing promises; the C ABI without a device (struct layouts, enums,
the workspace queries, the refusals that return before any HIP call) and the argument checks of the Python layers that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import meshops_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
ENTRIES = ("ovg_mesh_topology", "ovg_mesh_select", "ovg_mesh_smooth")


def _bytes_equal(a, b, name):
    for k in a:
        x, y = a[k], b[k]
        assert (x is None) == (y is None), (name, k)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (name, k, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (name, k)


# ---------------------------------------------------------------------------------------------
# the twin against its naive form, scipy and closed-form facts
# ---------------------------------------------------------------------------------------------
def test_zoo_is_what_it_says():
    z = twin.zoo(0)
    v, f, parts = z["vertices"], z["faces"], z["parts"]
    assert {k: len(i) for k, i in parts.items()} == dict(sphere2=162, sphere1=42, sheet=81, triple=5, corner=5, double=3, loose=5, nan=1)
    assert len(v) == 304 and len(f) == 320 + 80 + 128 + 3 + 2 + 2 + 1 + 3
    assert (f == -1).any() and (f == len(v)).any() and (f[:, 0] == f[:, 1]).any() and np.isnan(v[parts["nan"][0]]).any()
    assert not np.array_equal(twin.zoo(1)["faces"], f)                       # the seed shuffles


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_equals_the_naive_form(seed):
    z = twin.zoo(seed)
    v, f = z["vertices"], z["faces"]
    _bytes_equal(twin.topology(v, f), twin.topology_naive(v, f), "topology")
    fixed = np.zeros(len(v), np.uint8)
    fixed[z["parts"]["sphere1"][:7]] = 1
    for kw in (dict(), dict(mu=0.0), dict(iterations=3, fix_boundary=False), dict(iterations=2, fixed=fixed), dict(iterations=0),
               dict(iterations=1, normals=False)):
        _bytes_equal(twin.smooth(v, f, **kw), twin.smooth_naive(v, f, **kw), "smooth %r" % (kw,))


def test_components_match_scipy_and_the_parts():
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    z = twin.zoo(0)
    v, f, parts = z["vertices"], z["faces"], z["parts"]
    top = twin.topology(v, f)
    _, fc, _, live = twin.live_faces(v, f)
    lf = fc[live]
    rows, cols = np.concatenate([lf[:, 0], lf[:, 1]]), np.concatenate([lf[:, 1], lf[:, 2]])
    graph = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(len(v), len(v)))
    _, lab = csgraph.connected_components(graph, directed=False)
    ref = top["vertex_root"] >= 0
    lowest = np.full(lab.max() + 1, len(v))
    np.minimum.at(lowest, lab[ref], np.nonzero(ref)[0])
    assert np.array_equal(top["vertex_root"][ref], lowest[lab[ref]])
    for name in ("sphere2", "sphere1", "sheet", "triple", "corner", "double"):                       # one component per part, the corner pair included
        assert set(top["vertex_root"][parts[name]].tolist()) == {int(parts[name][0])}, name
    assert (top["vertex_root"][parts["loose"]] == -1).all() and top["vertex_root"][parts["nan"][0]] == -1
    lab_size, lab_index = twin.labels(top["vertex_root"], top["face_root"]), twin.labels(top["vertex_root"], top["face_root"], "index")
    assert lab_size["face_sizes"].tolist() == [320, 128, 80, 3, 2, 2] and lab_size["vertex_sizes"].tolist()[:4] == [162, 81, 42, 5]
    assert sorted(lab_size["vertex_sizes"].tolist()[4:]) == [3, 5] and lab_size["roots"][4] < lab_size["roots"][5]        # equal counts: by root
    assert sorted(lab_index["roots"].tolist()) == lab_index["roots"].tolist() and set(lab_index["roots"]) == set(lab_size["roots"])


def test_closed_form_facts():
    for sub, nv, nf in ((2, 162, 320), (1, 42, 80)):
        v, f = twin.icosphere(sub)
        c = twin.topology(v, f)["counts"]
        assert (len(v), len(f)) == (nv, nf) and c[1] - c[2] + c[0] == 2 and c[3] == 0 and c[4] == 0 and twin.volume(v, f) > 0
    v, f = twin.grid_sheet(9, 9)
    c = twin.topology(v, f)["counts"]
    assert (len(v), len(f)) == (81, 128) and c[3] == 32 and c[5] == 32 and c[1] - c[2] + c[0] == 1
    z = twin.zoo(0)
    top = twin.topology(z["vertices"], z["faces"])
    assert top["counts"].tolist() == [535, 298, 480 + 120 + 208 + 7 + 6 + 3, 32 + 6 + 6, 1, 32 + 5 + 5, 2, 0]
    nm = np.nonzero(top["vertex_flags"] & twin.NONMANIFOLD)[0]
    assert set(nm) <= set(z["parts"]["triple"]) and len(nm) == 2                                     # the triple edge is the one non-manifold edge
    assert not (top["vertex_flags"][z["parts"]["double"]] & (twin.BOUNDARY | twin.NONMANIFOLD)).any()   # multiplicity 2 everywhere
    rv, rf = twin.ribbon(200)
    assert (twin.topology(rv, rf)["vertex_root"] == 0).all()
    qv, qf, quad = twin.quads(50)
    want = np.empty(200, np.int32)
    want[quad.reshape(-1)] = np.repeat(quad.min(axis=1), 4)
    assert np.array_equal(twin.topology(qv, qf)["vertex_root"], want)
    fv, ff = twin.fan(100)
    assert twin.topology(fv, ff)["counts"].tolist() == [100, 101, 200, 100, 0, 100, 0, 0]


def test_select_twin():
    z = twin.zoo(0)
    v, f = z["vertices"], z["faces"]
    top = twin.topology(v, f)
    big = int(z["parts"]["sphere2"][0])
    out = twin.select(v, f, face_keep=(top["face_root"] == big).astype(np.uint8))
    assert out["counts"].tolist() == [162, 320] and np.array_equal(out["source_index"], z["parts"]["sphere2"])
    assert np.array_equal(out["vertices"].view(np.uint32), v[out["source_index"]].view(np.uint32))
    assert np.array_equal(out["source_index"][out["faces"]], f[out["face_index"]])
    again = twin.topology(out["vertices"], out["faces"])["counts"]
    assert again[:5].tolist() == [320, 162, 480, 0, 0]
    none = twin.select(v, f)
    assert none["counts"].tolist() == [298, 535]
    stripes = twin.select(v, f, vertex_keep=(np.arange(len(v)) % 3 != 0).astype(np.uint8))
    assert 0 < stripes["counts"][1] < 535 and (stripes["source_index"] % 3 != 0).all()


# ---------------------------------------------------------------------------------------------
# smoothing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [2, 3])
def test_taubin_takes_the_noise_and_keeps_the_volume(sub):
    v, f = twin.noisy_icosphere(sub, noise=0.02, seed=1)
    lap = twin.smooth(v, f, 10, 0.5, 0.0)["vertices"]
    tau = twin.smooth(v, f, 10, 0.5, -0.53)["vertices"]
    s0, sl, st = twin.radius_spread(v), twin.radius_spread(lap), twin.radius_spread(tau)
    v0, vl, vt = twin.volume(v, f), twin.volume(lap, f), twin.volume(tau, f)
    print("subdivision %d: spread %.4f -> %.4f / %.4f, volume %+.2f %% / %+.2f %%" % (sub, s0, sl, st, 100 * (vl / v0 - 1), 100 * (vt / v0 - 1)))
    assert sl < s0 and st < s0
    assert abs(vt / v0 - 1) < abs(vl / v0 - 1)


def test_factor_zero_fixed_and_boundary_vertices_keep_their_bytes():
    v, f = twin.noisy_icosphere(2)
    assert not (np.signbit(v) & (v == 0)).any()
    still = twin.smooth(v, f, 3, 0.0, 0.0)["vertices"]                       # the twin takes any factor; the API refuses lam = 0
    assert np.array_equal(still.view(np.uint32), v.view(np.uint32))
    fixed = (np.arange(len(v)) % 5 == 0).astype(np.uint8)
    out = twin.smooth(v, f, 4, fixed=fixed)["vertices"]
    same = (out.view(np.uint32) == v.view(np.uint32)).all(axis=1)
    assert same[fixed != 0].all() and not same[fixed == 0].any()
    sv, sf = twin.grid_sheet(9, 9)
    sv[:, 2] = (0.01 * np.random.default_rng(3).standard_normal(81)).astype(F)
    rim = twin.sheet_rim(9, 9)
    out = twin.smooth(sv, sf, 5)["vertices"]
    same = (out.view(np.uint32) == sv.view(np.uint32)).all(axis=1)
    assert same[rim].all() and not same[~rim].any()
    free = twin.smooth(sv, sf, 5, fix_boundary=False)["vertices"]
    assert not (free.view(np.uint32) == sv.view(np.uint32)).all(axis=1)[rim].all()


def test_result_does_not_depend_on_the_order_of_faces_or_corners():
    z = twin.zoo(0)
    v, f = z["vertices"], z["faces"]
    base = twin.smooth(v, f, 4)
    rng = np.random.default_rng(9)
    shuffled = f[rng.permutation(len(f))]
    turned = np.stack([np.roll(row, k) for row, k in zip(f, rng.integers(0, 3, len(f)))])
    for name, g in (("faces permuted", shuffled), ("corners rotated", turned)):
        out = twin.smooth(v, np.ascontiguousarray(g), 4)
        _bytes_equal(base, out, name)
        t0, t1 = twin.topology(v, f), twin.topology(v, np.ascontiguousarray(g))
        for k in ("vertex_root", "vertex_flags", "counts"):
            assert np.array_equal(t0[k], t1[k]), (name, k)


def test_frame_follows_the_mesh_and_nonfinite_is_reported():
    v, f = twin.noisy_icosphere(2)
    box0 = (v.min(axis=0), v.max(axis=0))
    out = twin.smooth(v, f, 1, 0.5, -4.0)["vertices"]                         # one strong inflate step: the mesh leaves the input's box
    assert (out.min(axis=0) < box0[0]).all() and (out.max(axis=0) > box0[1]).all()
    big = (v.astype(np.float64) * 3e37).astype(F)
    with pytest.raises(twin.NonFinite):
        twin.smooth(big, f, 3, 1.0, -60.0)


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
STRUCTS = (("ovg_mesh_topology_params", "MeshTopologyParams"), ("ovg_mesh_select_params", "MeshSelectParams"),
           ("ovg_mesh_smooth_params", "MeshSmoothParams"))


def test_ctypes_struct_layouts_and_enums_match_c():
    enums = ["OVG_MT_REFERENCED", "OVG_MT_BOUNDARY", "OVG_MT_NONMANIFOLD", "OVG_MT_INTERNAL", "OVG_MSEL_COUNT", "OVG_MSEL_SCATTER",
             "OVG_MSM_NONFINITE", "OVG_ABI_VERSION"]
    got, _ = abi_layout.check({cname: getattr(L, pyname) for cname, pyname in STRUCTS}, enums, rename={"lam": "lambda"})
    assert got == [L.MT_REFERENCED, L.MT_BOUNDARY, L.MT_NONMANIFOLD, L.MT_INTERNAL, L.MSEL_COUNT, L.MSEL_SCATTER,
                   L.MSM_NONFINITE, L.ABI_VERSION] == [1, 2, 4, 1, 1, 2, 1, 13]
    assert (twin.REFERENCED, twin.BOUNDARY, twin.NONMANIFOLD) == (L.MT_REFERENCED, L.MT_BOUNDARY, L.MT_NONMANIFOLD)


def test_entries_are_declared_under_abi_13_and_built_exact():
    text = open(HEADER).read()
    for entry in ENTRIES:
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (entry, entry), text), entry
        assert re.search(r"int64_t\s+%s_workspace_bytes\s*\(\s*int64_t\s+vertices\s*,\s*int64_t\s+faces\s*\)\s*;" % entry, text), entry
        for name in (entry, entry + "_workspace_bytes"):
            assert name in L.SYMBOLS and text.index(entry) < text.index("#define OVG_ABI_VERSION")  # named in the ABI-13 list
    assert L.SYMBOLS["ovg_mesh_smooth"][1][0]._type_ is L.MeshSmoothParams
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text) and L.load().ovg_abi_version() == 13 == L.ABI_VERSION
    from omnivggt_official_amd import build as B
    assert "ovg_meshops.hip" in B.SOURCES and B.EXTRA_FLAGS["ovg_meshops.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(B.CSRC, "ovg_meshops.hip")).read()
    assert re.search(r'^\s*#\s*include\s+"ovg_geom.h"', src, re.M)
    for name in ("cl_ld", "cl_find", "cl_unite"):                                                    # the union-find lives in the shared header alone
        assert re.search(r"OVG_DEV\s+\w+\s+%s\s*\(" % name, open(os.path.join(B.CSRC, "ovg_geom.h")).read()), name
        for unit in ("ovg_radius.hip", "ovg_meshops.hip"):
            assert not re.search(r"OVG_DEV\s+\w+\s+%s\s*\(" % name, open(os.path.join(B.CSRC, unit)).read()), (unit, name)


def test_workspace_queries_and_refusals_without_gpu():
    lib = L.load()
    r256 = lambda b: (b + 255) // 256 * 256
    for m, f in ((1, 1), (304, 539), (5001, 5000), (70000, 69998), (64 * 518 * 518, 2 * 64 * 517 * 517)):
        E, tv, tf = max(1024, 6 * f), -(-m // 4096), -(-f // 4096)
        want = dict(topology=(256, 4 * m, 8 * E, 4 * E), select=(m, f, 4 * m, 8 * tv, 8 * tv, 8 * tf, 8 * tf),
                    smooth=(256, 4 * m, 8 * E, 4 * E, 4 * m, 8 * (m + 1), 8 * tv, 8 * tv, 24 * f, 16 * m, 24 * m))
        for name, parts in want.items():
            q = getattr(lib, "ovg_mesh_%s_workspace_bytes" % name)
            assert q(m, f) == sum(r256(b) for b in parts) == getattr(ops, "mesh_%s_workspace_bytes" % name)(m, f), (name, m, f)
    outside = ((0, 5), (5, 0), (0, 0), (-1, 5), (5, -3), (1 << 31, 5), (5, 1 << 31), (5, 1 << 40), (1 << 40, 5))
    for name in ("topology", "select", "smooth"):
        q = getattr(lib, "ovg_mesh_%s_workspace_bytes" % name)
        assert [q(*a) for a in outside] == [-1] * len(outside) and q((1 << 31) - 1, (1 << 31) - 1) > 0
        for bad in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31), (1 << 70, 5)):
            with pytest.raises(L.OvgError):
                getattr(ops, "mesh_%s_workspace_bytes" % name)(*bad)
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    M, Fc = 4096, 8000

    def run(entry, cls, base, **kw):
        p = cls(**{**base, **kw})
        return getattr(lib, entry)(ctypes.byref(p), None)

    common_bad = (dict(vertices=None), dict(faces=None), dict(ws=None), dict(ws=big + 8), dict(ws_bytes=0), dict(ws_bytes=-5), dict(num_vertices=0),
                  dict(num_vertices=-1), dict(num_faces=0), dict(num_vertices=1 << 31, ws_bytes=1 << 60), dict(num_faces=1 << 31, ws_bytes=1 << 60),
                  dict(num_vertices=2 * M), dict(num_faces=2 * Fc), dict(vertices=big + 2), dict(faces=big + 1))
    need = lib.ovg_mesh_topology_workspace_bytes(M, Fc)
    base = dict(vertices=big, faces=big, num_vertices=M, num_faces=Fc, vertex_root=big, face_root=big, vertex_flags=big + 1, out_count=big, ws=big,
                ws_bytes=need)
    assert lib.ovg_mesh_topology(None, None) == -1
    for bad in common_bad + (dict(ws_bytes=need - 1), dict(vertex_root=None), dict(face_root=None), dict(vertex_flags=None), dict(out_count=None),
                             dict(vertex_root=big + 2), dict(face_root=big + 1), dict(out_count=big + 4)):
        assert run("ovg_mesh_topology", L.MeshTopologyParams, base, **bad) == -1, bad
    need = lib.ovg_mesh_select_workspace_bytes(M, Fc)
    base = dict(vertices=big, faces=big, face_keep=big + 1, vertex_keep=big + 3, num_vertices=M, num_faces=Fc, stage=L.MSEL_COUNT | L.MSEL_SCATTER,
                vertex_capacity=10, face_capacity=10, out_vertices=big, out_source_index=big, out_faces=big, out_face_index=big, out_count=big, ws=big,
                ws_bytes=need)
    assert lib.ovg_mesh_select(None, None) == -1
    for bad in common_bad + (dict(ws_bytes=need - 1), dict(stage=0), dict(stage=4), dict(stage=-1), dict(out_count=None), dict(vertex_capacity=-1),
                             dict(face_capacity=-1), dict(out_vertices=None), dict(out_faces=None), dict(out_count=big + 4), dict(out_vertices=big + 2),
                             dict(out_source_index=big + 4), dict(out_faces=big + 2), dict(out_face_index=big + 4)):
        assert run("ovg_mesh_select", L.MeshSelectParams, base, **bad) == -1, bad
    need = lib.ovg_mesh_smooth_workspace_bytes(M, Fc)
    base = dict(vertices=big, faces=big, fixed=big + 1, num_vertices=M, num_faces=Fc, iterations=3, fix_boundary=1, lam=0.5, mu=-0.53,
                out_vertices=big + 4096 * 16, out_normals=big, out_status=big, ws=big, ws_bytes=need)
    assert lib.ovg_mesh_smooth(None, None) == -1
    for bad in common_bad + (dict(ws_bytes=need - 1), dict(iterations=-1), dict(iterations=65537), dict(fix_boundary=2), dict(fix_boundary=-1),
                             dict(lam=float("nan")), dict(lam=float("inf")), dict(mu=float("-inf")), dict(mu=float("nan")), dict(out_vertices=None),
                             dict(out_status=None), dict(out_vertices=big), dict(out_vertices=big + 2), dict(out_normals=big + 2), dict(out_status=big + 4)):
        assert run("ovg_mesh_smooth", L.MeshSmoothParams, base, **bad) == -1, bad


# ---------------------------------------------------------------------------------------------
# the Python layers
# ---------------------------------------------------------------------------------------------
def _cpu_mesh(cls=postprocess.Mesh):
    v, f = twin.icosphere(1)
    t = torch.from_numpy
    return cls(t(v), t(f), t(v.copy()), torch.zeros(len(v), 3, dtype=torch.uint8), np.eye(4), None, torch.tensor(1.0))


def test_postprocess_refusals_that_need_no_device():
    mesh = _cpu_mesh()
    P = postprocess
    bad_smooth = (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.0), dict(iterations=True), dict(lam=0.0), dict(lam=1.5), dict(lam=-0.5),
                  dict(lam=float("nan")), dict(lam="0.5"), dict(mu=0.1), dict(mu=float("-inf")), dict(mu=float("nan")), dict(mu=None),
                  dict(fix_boundary=1), dict(normals="smooth"), dict(normals=0), dict(fixed=torch.zeros(5, dtype=torch.uint8)),
                  dict(fixed=torch.zeros(42)), dict(fixed=[0] * 42))
    for kw in bad_smooth:
        with pytest.raises(ValueError):
            P.smooth_mesh(mesh, **kw)
    for kw in (dict(), dict(min_faces=3, keep_largest=True), dict(min_faces=3, rel_faces=0.5), dict(min_faces=0), dict(min_faces=2.5), dict(min_faces=True),
               dict(rel_faces=0.0), dict(rel_faces=1.5), dict(rel_faces=float("nan")), dict(keep_largest=1), dict(keep_largest=False)):
        with pytest.raises(ValueError):
            P.remove_small_components(mesh, **kw)
    for kw in (dict(face_mask=torch.zeros(3, dtype=torch.bool)), dict(vertex_mask=torch.zeros(42)), dict(face_mask=np.zeros(80, bool))):
        with pytest.raises(ValueError):
            P.select_faces(mesh, **kw)
    with pytest.raises(ValueError):
        P.mesh_topology(mesh, order="root")
    for fn, kw in ((P.mesh_topology, {}), (P.select_faces, {}), (P.remove_small_components, dict(keep_largest=True)), (P.smooth_mesh, {}),
                   (P.mesh_vertex_normals, {})):
        with pytest.raises(ValueError):
            fn("mesh", **kw)
        with pytest.raises(L.OvgError):
            fn(mesh, **kw)                                                  # CPU tensors: no fallback
        with pytest.raises(L.OvgError):
            fn(_cpu_mesh(postprocess.MapMesh), **kw)
    assert issubclass(P.MeshSubset, P.Mesh) and P.MESH_NORMALS == ("recompute", "keep", None)
    s = P.MeshSubset(1, 2, 3, 4, 5)
    assert s.source_index is None and s.face_index is None and s.pixel_index is None
    for name in ("hole filling", "edge-adjacency components", "pinch-vertex detection", "cotangent or area weights", "quadric simplification",
                 "self-intersections"):
        assert name in open(HEADER).read() and name in P.smooth_mesh.__doc__ and name in P.mesh_topology.__doc__, name


def test_ops_wrappers_check_their_arguments_before_any_device_call():
    v, f = (torch.from_numpy(a) for a in twin.icosphere(1))
    M, Fc = len(v), len(f)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    good = dict(vertices=v, faces=f, ws=ws, vertex_root=torch.zeros(M, dtype=i32), face_root=torch.zeros(Fc, dtype=i32),
                vertex_flags=torch.zeros(M, dtype=u8), out_count=torch.zeros(8, dtype=i64))
    for bad in (dict(vertices=v[:, :2]), dict(vertices=v.double()), dict(faces=f.long()), dict(faces=f[:, :2]), dict(vertices=v[:0]), dict(faces=f[:0]),
                dict(ws=ws.int()), dict(vertex_root=torch.zeros(M, dtype=i64)), dict(face_root=torch.zeros(M, dtype=i32)),
                dict(vertex_flags=torch.zeros(M, dtype=i32)), dict(out_count=torch.zeros(7, dtype=i64)), dict(out_count=None)):
        with pytest.raises(L.OvgError) as e:
            ops.mesh_topology(**{**good, **bad})
        assert "mesh_topology" in str(e.value), bad
    good_sel = dict(stage=L.MSEL_COUNT, vertices=v, faces=f, ws=ws, out_count=torch.zeros(2, dtype=i64))
    for bad in (dict(stage=0), dict(stage=4), dict(face_keep=torch.zeros(M, dtype=u8)), dict(vertex_keep=torch.zeros(M, dtype=torch.bool)),
                dict(out_count=None), dict(out_count=torch.zeros(1, dtype=i64)), dict(stage=L.MSEL_SCATTER, vertex_capacity=-1),
                dict(stage=L.MSEL_SCATTER, vertex_capacity=4), dict(stage=L.MSEL_SCATTER, face_capacity=4),
                dict(stage=L.MSEL_SCATTER, vertex_capacity=4, out_vertices=torch.zeros(3, 3)),
                dict(stage=L.MSEL_SCATTER, vertex_capacity=4, out_vertices=torch.zeros(4, 3), source_index=torch.zeros(4, dtype=i32))):
        with pytest.raises(L.OvgError) as e:
            ops.mesh_select(**{**good_sel, **bad})
        assert "mesh_select" in str(e.value), bad
    good_sm = dict(vertices=v, faces=f, ws=ws, iterations=2, lam=0.5, mu=-0.53, out_vertices=torch.zeros(M, 3), out_status=torch.zeros(1, dtype=i64))
    for bad in (dict(iterations=-1), dict(iterations=1 << 17), dict(iterations=1.0), dict(lam=float("nan")), dict(mu=float("inf")), dict(lam="x"),
                dict(fix_boundary=1), dict(fixed=torch.zeros(M)), dict(out_vertices=v), dict(out_vertices=torch.zeros(M, 3, dtype=torch.float64)),
                dict(out_normals=torch.zeros(M, 2)), dict(out_status=torch.zeros(1, dtype=i32)), dict(out_status=None)):
        with pytest.raises(L.OvgError) as e:
            ops.mesh_smooth(**{**good_sm, **bad})
        assert "mesh_smooth" in str(e.value), bad
    for fn, kw in ((ops.mesh_topology, good), (ops.mesh_select, good_sel), (ops.mesh_smooth, good_sm)):
        with pytest.raises(L.OvgError) as e:
            fn(**kw)                                                        # everything in order but the device
        assert "HIP device tensor" in str(e.value)
