"""What the geometry wrappers of ops.py (unproject .. mesh_smooth) write into their parameter structs, pinned without a device.

Every wrapper is called on CPU tensors of the smallest legal shapes, once with every optional argument None and once with all of
them given (staged wrappers once per stage), with ops._chk_dev a no-op, ops._stream -> 0 and L.call replaced by a recorder: no
entry of the library is invoked. A record holds the entry's name, every field of the struct (pointers as the name of the argument
or returned tensor they equal, "null", or "other" for a tensor the wrapper allocated and kept, e.g. a workspace), and the dtype and
shape of what the wrapper returns. The records must equal tests/golden/ops_marshalling.json, which was written by this module (run
as a script) on the commit BEFORE the wrappers were rebuilt on shared argument checks; it is never regenerated from later code.
The workspace queries are host-only functions of the library; their values at the corpus sizes are pinned alongside."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops

FIXTURE = os.path.join(ROOT, "tests", "golden", "ops_marshalling.json")
NQ, NR, K = 5, 7, 3
S, H, W = 2, 3, 4
M, F = 4, 2
G, N = 2, 6
INF = float("inf")


def f32(*s):
    return torch.zeros(*s, dtype=torch.float32)


def f64(*s):
    return torch.zeros(*s, dtype=torch.float64)


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64)


def ws(need=0):
    return u8(max(int(need), 16))


def corpus():
    """[(case id, wrapper name, kwargs)]: fresh tensors on every call."""
    c = []

    def add(case, fn, **kw):
        c.append((case, fn, kw))

    add("unproject", "unproject", depth=f32(S, H, W), cam=f32(S, 16))

    add("percentile/none", "percentile", x=f32(2 * N), n=N, stride=1, col_stride=N, ncols=2, qs=(5, 95))
    add("percentile/all", "percentile", x=f32(4 * N), n=N, stride=2, col_stride=2 * N, ncols=2, qs=(5, 95), mask=f32(N), norm=True,
        ws=ws(ops.percentile_workspace_bytes(N, 2)))

    pf = lambda: dict(conf=f32(N), images=f32(1, 3, N), points=f32(N, 3), hw=N, ws=ws())
    add("point_filter/count/none", "point_filter", stage=L.PF_COUNT, **pf())
    add("point_filter/scatter/all", "point_filter", stage=L.PF_SCATTER, threshold=f32(1), mask=f32(N), min_conf=1e-3, flags=1, index_base=10,
        out_count=i64(1), capacity=4, out_points=f32(4, 3), out_colors=u8(4, 3), out_index=i64(4), **pf())

    add("voxel_downsample/count/none", "voxel_downsample", stage=L.VG_COUNT, points=f32(NR, 3), voxel=f32(1), ws=ws())
    add("voxel_downsample/scatter/all", "voxel_downsample", stage=L.VG_SCATTER, points=f32(NR, 3), voxel=f32(1), ws=ws(), conf=f32(NR),
        colors=u8(NR, 3), out_count=i64(2), capacity=4, out_points=f32(4, 3), out_colors=u8(4, 3), out_index=i64(4))

    add("render_points/none", "render_points", points=f32(NR, 3), colors=u8(NR, 3), cams=f32(S, 16), H=H, W=W)
    add("render_points/all", "render_points", points=f32(NR, 3), colors=u8(NR, 3), cams=f32(S, 16), H=H, W=W, radius=2, near=0.5,
        background=(1, 2, 3), depth=True, index=True, ws=ws(ops.render_workspace_bytes(S, H, W)), flags=L.RENDER_NO_PREREAD)
    add("render_points/no_depth", "render_points", points=f32(NR, 3), colors=u8(NR, 3), cams=f32(S, 16), H=H, W=W, depth=False)

    mesh = lambda: dict(vertices=f32(M, 3), faces=i32(F, 3))
    add("render_mesh/none", "render_mesh", cams=f32(S, 16), H=H, W=W, **mesh())
    add("render_mesh/all", "render_mesh", cams=f32(S, 16), H=H, W=W, normals=f32(M, 3), colors=u8(M, 3), shading=L.MESH_SHADE_COLOR,
        cull=L.MESH_CULL_BACK, near=0.5, background=(1, 2, 3), depth=True, index=True, coop_threshold=5,
        ws=ws(ops.render_mesh_workspace_bytes(S, H, W)), out=(u8(S, H, W, 3), f32(S, H, W), i64(S, H, W)), flags=1, **mesh())

    add("multiview_consistency/none", "multiview_consistency", points=f32(S, H, W, 3), cams=f32(S, 16), tol=0.1)
    add("multiview_consistency/all", "multiview_consistency", points=f32(S, H, W, 3), cams=f32(S, 16), tol=0.1, near=0.5, valid=u8(S, H, W),
        src_first=1, src_count=1, occluded=True, ws=ws(ops.consistency_workspace_bytes(S, H, W)), tile=L.MVC_TILE_16x16,
        flags=L.MVC_ROTATE_TARGETS | L.MVC_KEEP_MAP)

    add("nearest_neighbours/none", "nearest_neighbours", query=f32(NQ, 3), reference=f32(NR, 3))
    add("nearest_neighbours/all", "nearest_neighbours", query=f32(NQ, 3), reference=f32(NQ, 3), query_valid=u8(NQ), reference_valid=u8(NQ),
        exclude_self=True, splits=2, ws=ws(ops.nn_workspace_bytes(NQ, NQ)), index=i32(NQ), sqdist=f32(NQ))

    add("farthest_point_sample/none", "farthest_point_sample", points=f32(2, NR, 3), npoint=K)
    add("farthest_point_sample/all", "farthest_point_sample", points=f32(2, NR, 3), npoint=K, valid=u8(2, NR), first=1, include_last=True,
        path=L.FPS_PATH_PER_STEP, ws=ws(ops.fps_workspace_bytes(2, NR, K)), index=i32(2, K), sqdist=f32(2, K), distance=f32(2, NR))
    add("farthest_point_sample/distance_true", "farthest_point_sample", points=f32(2, NR, 3), npoint=K, distance=True)

    grid = dict(radius_sq=0.25, cell=1.0)
    grid_all = lambda: dict(query=f32(NQ, 3), reference=f32(NQ, 3), ws=ws(), query_valid=u8(NQ), reference_valid=u8(NQ), origin=f32(3),
                            exclude_self=True, max_pairs=100, out_stats=i64(2, 2))
    add("radius_search/build/none", "radius_search", stage=L.RS_BUILD, query=f32(NQ, 3), reference=f32(NR, 3), ws=ws(), **grid)
    add("radius_search/search/none", "radius_search", stage=L.RS_SEARCH, query=f32(NQ, 3), reference=f32(NR, 3), ws=ws(), **grid)
    add("radius_search/build/all", "radius_search", stage=L.RS_BUILD, **grid, **grid_all())
    add("radius_search/search/all", "radius_search", stage=L.RS_SEARCH, count=i32(NQ), index=i32(NQ, 1), sqdist=f32(1, NQ), **grid, **grid_all())
    add("radius_search/both/none", "radius_search", stage=L.RS_BUILD | L.RS_SEARCH, query=f32(NQ, 3), reference=f32(NR, 3), ws=ws(), **grid)

    add("knn_search/none", "knn_search", query=f32(NQ, 3), reference=f32(NR, 3), ws=ws(), k=K, **grid)
    add("knn_search/all", "knn_search", k=K, count=i32(NQ), index=i32(NQ, K), sqdist=f32(NQ * K), **grid, **grid_all())

    add("cluster/none", "cluster", points=f32(NR, 3), ws=ws(), min_neighbours=0, **grid)
    add("cluster/all", "cluster", points=f32(NR, 3), ws=ws(), min_neighbours=2, valid=u8(NR), origin=f32(3), max_pairs=100, out_stats=i64(4),
        root=i32(NR), kind=u8(NR), degree=i32(NR), **grid)
    add("cluster/no_degree", "cluster", points=f32(NR, 3), ws=ws(), min_neighbours=2, degree=False, **grid)

    add("knn_normals/none", "knn_normals", query=f32(NQ, 3), reference=f32(NR, 3), index=i32(NQ, K))
    add("knn_normals/all", "knn_normals", query=f32(NQ, 3), reference=f32(NR, 3), index=i32(NQ, K), viewpoint=f32(NQ, 3), normal=f32(NQ, 3),
        curvature=f32(NQ), covariance=f64(NQ, 6), used=i32(NQ))
    add("knn_normals/allocate", "knn_normals", query=f32(NQ, 3), reference=f32(NR, 3), index=i32(NQ, K), viewpoint=f32(3), curvature=True,
        covariance=True, used=True)

    add("align_moments/none", "align_moments", source=f32(NQ, 3), target=f32(NQ, 3))
    add("align_moments/all", "align_moments", source=f32(NQ, 3), target=f32(NR, 3), index=i32(NQ), source_valid=u8(NQ), target_valid=u8(NR),
        sqdist=f32(NQ), max_sqdist=0.5, centre=f64(6), ws=ws(ops.align_workspace_bytes(NQ)), count=i64(1), sums=f64(L.ALIGN_SUMS))
    add("align_solve/none", "align_solve", count=i64(1), sums=f64(L.ALIGN_SUMS), transform=f64(4, 4))
    add("align_solve/all", "align_solve", count=i64(1), sums=f64(L.ALIGN_SUMS), transform=f64(4, 4), centre=f64(6), with_scale=False,
        compose=True, scale=f64(1), rms=f64(1), out_count=i64(1), status=i32(1))
    add("align_apply/none", "align_apply", points=f32(NQ, 3), transform=f64(4, 4))
    add("align_apply/all", "align_apply", points=f32(NQ, 3), transform=f64(4, 4), out=f32(NQ, 3))

    add("deptheval_median/none", "deptheval_median", pred=f32(G, N), gt=f32(G, N))
    add("deptheval_median/all", "deptheval_median", pred=f32(G, N + 2)[:, :N], gt=f32(G, N + 2)[:, :N], valid=u8(G, N + 2)[:, :N],
        min_depth=0.5, max_depth=80.0, ws=ws(ops.deptheval_median_workspace_bytes(G, N)), count=i64(G), median=f32(G, 2, 2))
    add("deptheval_sums/none", "deptheval_sums", pred=f32(G, N), gt=f32(G, N))
    add("deptheval_sums/all", "deptheval_sums", pred=f32(G, N + 2)[:, :N], gt=f32(G, N + 2)[:, :N], valid=u8(G, N + 2)[:, :N], min_depth=0.5,
        max_depth=80.0, coeff=f64(G, 2), clip_min=0.01, clip_max=100.0, ws=ws(ops.deptheval_sums_workspace_bytes(G, N)),
        counts=i64(G, L.DEPTHEVAL_COUNTS), sums=f64(G, L.DEPTHEVAL_SUMS))
    add("deptheval_solve/none", "deptheval_solve", mode=L.DEPTHEVAL_NONE, count=i64(G))
    add("deptheval_solve/median", "deptheval_solve", mode=L.DEPTHEVAL_MEDIAN, count=i64(G), median=f32(G, 2, 2))
    add("deptheval_solve/all", "deptheval_solve", mode=L.DEPTHEVAL_SCALE_SHIFT, count=i64(G, L.DEPTHEVAL_COUNTS), sums=f64(G, L.DEPTHEVAL_SUMS),
        median=f32(G, 2, 2), coeff=f64(G, 2), status=i32(G))

    add("plane_hypotheses/none", "plane_hypotheses", points=f32(NR, 3), hypotheses=K)
    add("plane_hypotheses/all", "plane_hypotheses", points=f32(NR, 3), hypotheses=K, seed=(1 << 63) + 12345, valid=u8(NR), candidates=i32(4),
        axis=f32(3), min_abs_cos=0.5, planes=f32(K, 4), index=i32(K, 3))
    add("plane_score/none", "plane_score", points=f32(NR, 3), planes=f32(K, 4), threshold=0.1)
    add("plane_score/all", "plane_score", points=f32(NR, 3), planes=f32(K, 4), threshold=0.1, valid=u8(NR), splits=2, count=i32(K))
    add("plane_select/none", "plane_select", count=i32(K), planes=f32(K, 4))
    add("plane_select/all", "plane_select", count=i32(K), planes=f32(K, 4), min_inliers=5, best=i32(1), plane=f32(4), best_count=i32(1),
        status=i32(1))
    add("plane_mask/none", "plane_mask", points=f32(NR, 3), plane=f32(4), threshold=0.1)
    add("plane_mask/all", "plane_mask", points=f32(NR, 3), plane=f32(4), threshold=0.1, valid=u8(NR), gate=i32(1), inlier=u8(NR),
        distance=f32(NR), out_count=i64(1))
    add("plane_mask/distance_true", "plane_mask", points=f32(NR, 3), plane=f32(4), threshold=0, distance=True)
    add("plane_fit/none", "plane_fit", count=i64(1), sums=f64(L.ALIGN_SUMS), plane=f32(4))
    add("plane_fit/all", "plane_fit", count=i64(1), sums=f64(L.ALIGN_SUMS), plane=f32(4), centre=f64(6), axis=f32(3), rms=f64(1), eigen=f64(3),
        status=i32(1))

    vol = lambda: dict(tsdf=f32(S, H, W), weight=f32(S, H, W), origin=(0.5, -1.0, 2.0), voxel=0.1)
    add("tsdf_integrate/none", "tsdf_integrate", depth=f32(S, H, W), cams=f32(S, 16), trunc=0.3, **vol())
    add("tsdf_integrate/all", "tsdf_integrate", depth=f32(S, H, W), cams=f32(S, 16), trunc=0.3, max_weight=32.0, near=0.01,
        color=f32(S, H, W, 4), valid=u8(S, H, W), obs_weight=f32(S, H, W), colors=u8(S, H, W, 3), view_first=1, view_count=1,
        tile=L.TSDF_TILE_8x8x4, **vol())
    add("tsdf_extract/count/none", "tsdf_extract", stage=L.TSDF_COUNT, ws=ws(), out_count=i64(2), **vol())
    add("tsdf_extract/scatter/all", "tsdf_extract", stage=L.TSDF_SCATTER, ws=ws(), min_weight=2.0, color=f32(S, H, W, 4), out_count=i64(2),
        vertex_capacity=5, quad_capacity=3, vertices=f32(5, 3), normals=f32(5, 3), colors=u8(5, 3), faces=i32(6, 3), **vol())

    add("map_depth/points", "map_depth", points=f32(S, H, W, 3), cams=f32(S, 16))
    add("map_depth/depth/all", "map_depth", depth=f32(S, H, W), valid=u8(S, H, W), near=0.5, out=f32(S, H, W))
    add("map_normals/none", "map_normals", points=f32(S, H, W, 3), z=f32(S, H, W))
    add("map_normals/all", "map_normals", points=f32(S, H, W, 3), z=f32(S, H, W), rel_tol=INF, out=f32(S, H, W, 3))
    add("map_edges/none", "map_edges", z=f32(S, H, W))
    add("map_edges/all", "map_edges", z=f32(S, H, W), normals=f32(S, H, W, 3), radius=2, rel_tol=0.05, min_cos=0.5, tile=L.MAP_TILE_16x16,
        out=u8(S, H, W))
    add("map_triangulate/count/none", "map_triangulate", stage=L.MAP_COUNT, z=f32(S, H, W), points=f32(S, H, W, 3), ws=ws(), out_count=i64(2))
    add("map_triangulate/scatter/all", "map_triangulate", stage=L.MAP_SCATTER, z=f32(S, H, W), points=f32(S, H, W, 3), ws=ws(), rel_tol=0.05,
        keep=u8(S, H, W), normals=f32(S, H, W, 3), colors=u8(S, H, W, 3), out_count=i64(2), vertex_capacity=5, face_capacity=3,
        vertices=f32(5, 3), out_normals=f32(5, 3), out_colors=u8(5, 3), pixel_index=i64(5), faces=i32(3, 3))

    add("mesh_simplify/count/none", "mesh_simplify", stage=L.MS_COUNT, voxel=f32(1), ws=ws(), out_count=i64(6), **mesh())
    add("mesh_simplify/scatter/all", "mesh_simplify", stage=L.MS_SCATTER, voxel=f32(1), ws=ws(), normals=f32(M, 3), colors=u8(M, 3),
        position=L.MS_POS_FIRST, out_count=i64(6), vertex_capacity=5, face_capacity=3, out_vertices=f32(5, 3), out_normals=f32(5, 3),
        out_colors=u8(5, 3), source_index=i64(5), vertex_count=i32(5), out_faces=i32(3, 3), **mesh())
    add("mesh_topology", "mesh_topology", ws=ws(), vertex_root=i32(M), face_root=i32(F), vertex_flags=u8(M), out_count=i64(8), **mesh())
    add("mesh_select/count/none", "mesh_select", stage=L.MSEL_COUNT, ws=ws(), out_count=i64(2), **mesh())
    add("mesh_select/scatter/all", "mesh_select", stage=L.MSEL_SCATTER, ws=ws(), face_keep=u8(F), vertex_keep=u8(M), out_count=i64(2),
        vertex_capacity=5, face_capacity=3, out_vertices=f32(5, 3), source_index=i64(5), out_faces=i32(3, 3), face_index=i64(3), **mesh())
    add("mesh_smooth/none", "mesh_smooth", ws=ws(), iterations=2, lam=0.5, mu=-0.53, out_vertices=f32(M, 3), out_status=i64(1), **mesh())
    add("mesh_smooth/all", "mesh_smooth", ws=ws(), iterations=2, lam=0.5, mu=0, out_vertices=f32(M, 3), out_status=i64(1), fixed=u8(M),
        fix_boundary=False, out_normals=f32(M, 3), **mesh())
    return c


def workspace_queries():
    q = ops
    return {"percentile": q.percentile_workspace_bytes(N, 2), "point_filter": q.point_filter_workspace_bytes(N),
            "voxel_downsample": q.voxel_downsample_workspace_bytes(NR), "render": q.render_workspace_bytes(S, H, W),
            "render_mesh": q.render_mesh_workspace_bytes(S, H, W), "consistency": q.consistency_workspace_bytes(S, H, W),
            "nn": q.nn_workspace_bytes(NQ, NR), "fps": q.fps_workspace_bytes(2, NR, K), "radius": q.radius_workspace_bytes(NQ, NR),
            "align": q.align_workspace_bytes(NQ), "deptheval_median": q.deptheval_median_workspace_bytes(G, N),
            "deptheval_sums": q.deptheval_sums_workspace_bytes(G, N), "tsdf_extract": q.tsdf_extract_workspace_bytes(W, H, S),
            "map_triangulate": q.map_triangulate_workspace_bytes(S, H, W), "mesh_simplify": q.mesh_simplify_workspace_bytes(M, F),
            "mesh_topology": q.mesh_topology_workspace_bytes(M, F), "mesh_select": q.mesh_select_workspace_bytes(M, F),
            "mesh_smooth": q.mesh_smooth_workspace_bytes(M, F)}


def _tensors(prefix, v):
    """(name, tensor) of a tensor, or of the tensors in a tuple / list."""
    if isinstance(v, torch.Tensor):
        return [(prefix, v)]
    if isinstance(v, (tuple, list)):
        return [(n, t) for i, e in enumerate(v) for n, t in _tensors("%s[%d]" % (prefix, i), e)]
    return []


def record(patch):
    """Run the corpus with the device checks, the stream and L.call replaced through patch(obj, name, value) -> the records."""
    calls = []

    def recorder(name, params, stream):
        fields = {}
        for fname, ftype in params._fields_:
            v = getattr(params, fname)
            if ftype is ctypes.c_void_p:
                v = ("ptr", v)
            elif isinstance(v, ctypes.Array):
                v = list(v)
            fields[fname] = v
        calls.append({"entry": name, "stream": stream, "fields": fields})

    patch(ops, "_chk_dev", lambda *ts: None)
    patch(ops, "_stream", lambda: 0)
    patch(L, "call", recorder)
    records = {}
    for case, fn, kw in corpus():
        del calls[:]
        ret = getattr(ops, fn)(**kw)
        names = {}
        for k, v in kw.items():
            for n, t in _tensors(k, v):
                names.setdefault(t.data_ptr(), n)
        for n, t in _tensors("ret", ret if isinstance(ret, tuple) else (ret,)):
            names.setdefault(t.data_ptr(), n)
        for c in calls:
            for fname, v in c["fields"].items():
                if isinstance(v, tuple):
                    c["fields"][fname] = "null" if not v[1] else names.get(v[1], "other")
        rets = [None if t is None else [str(t.dtype), list(t.shape)] for t in (ret if isinstance(ret, tuple) else (ret,))]
        records[case] = {"calls": [dict(c) for c in calls], "returns": rets}
    return {"records": records, "workspace_bytes": workspace_queries()}


def test_geometry_wrappers_fill_their_structs_as_recorded(monkeypatch):
    got = record(monkeypatch.setattr)
    want = json.load(open(FIXTURE))
    got = json.loads(json.dumps(got))                                        # tuples -> lists, as the fixture holds them
    assert sorted(got["records"]) == sorted(want["records"])
    for case in want["records"]:
        assert got["records"][case] == want["records"][case], case
    assert got["workspace_bytes"] == want["workspace_bytes"]
    every = {"unproject", "percentile", "point_filter", "voxel_downsample", "render_points", "render_mesh", "multiview_consistency",
             "nearest_neighbours", "farthest_point_sample", "radius_search", "knn_search", "cluster", "knn_normals", "align_moments",
             "align_solve", "align_apply", "deptheval_median", "deptheval_sums", "deptheval_solve", "plane_hypotheses", "plane_score",
             "plane_select", "plane_mask", "plane_fit", "tsdf_integrate", "tsdf_extract", "map_depth", "map_normals", "map_edges",
             "map_triangulate", "mesh_simplify", "mesh_topology", "mesh_select", "mesh_smooth"}
    assert {fn for _, fn, _ in corpus()} == every
    assert all(len(r["calls"]) == 1 and r["calls"][0]["stream"] == 0 for r in want["records"].values())


if __name__ == "__main__":
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    try:
        out = record(patch)
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (FIXTURE, len(out["records"])))
