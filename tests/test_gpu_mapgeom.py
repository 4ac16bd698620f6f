"""ovg_map_depth / ovg_map_normals / ovg_map_edges / ovg_map_triangulate and postprocess.camera_depth_maps, map_normals, map_edges,
edge_mask, triangulate_maps, predictions_to_mesh on the device against tests/mapgeom_twin.py: every output byte for byte in exact-size
guarded buffers (a scene that tests/test_mapgeom_host.py shows to be non-trivial; every window radius, every tile, the tests on and
off, both depth inputs, with and without normals / colours / keep), views and rows that must never be stitched, the second level of
the scan, capacities, winding, the glue down to the writers and the rasteriser, every refusal, and the gated cases of the four
entries for the stream contract's coverage test. Every case runs twice."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mapgeom_scenes as scenes
import mapgeom_twin as twin
import stream_contract as sc
import test_gpu_stream_contract as tsc
from kernel_guards import GUARD_BYTE, guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
TILES = (L.MAP_TILE_DEFAULT, L.MAP_TILE_256x1, L.MAP_TILE_16x16, L.MAP_TILE_32x8, L.MAP_TILE_64x4)
MIN_COS = float(twin.min_cos(30.0))


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


def _depth(points=None, cams=None, depth=None, valid=None, near=scenes.NEAR):
    shape = (points if points is not None else depth).shape[:3]
    z, chk = _g(shape, torch.float32)
    assert ops.map_depth(points=points, cams=cams, depth=depth, valid=valid, near=near, out=z) is z
    torch.cuda.synchronize()
    chk("map_depth")
    return z


def _normals(points, z, rel_tol):
    n, chk = _g(tuple(z.shape) + (3,), torch.float32)
    ops.map_normals(points, z, rel_tol=rel_tol, out=n)
    torch.cuda.synchronize()
    chk("map_normals")
    return n


def _edges(z, normals, radius, rel_tol, min_cos, tile):
    f, chk = _g(tuple(z.shape), torch.uint8)
    ops.map_edges(z, normals, radius=radius, rel_tol=rel_tol, min_cos=min_cos, tile=tile, out=f)
    torch.cuda.synchronize()
    chk("map_edges tile %d" % tile)
    return f


def _mesh(z, points, rel_tol, keep=None, normals=None, colors=None, short=(0, 0)):
    """COUNT, the counts, SCATTER into guarded buffers of exactly (M - short[0], F - short[1]) entries -> (M, F, dict of tensors)."""
    S, H, W = z.shape
    (ws, c0), (count, c1) = _g((ops.map_triangulate_workspace_bytes(S, H, W),), torch.uint8), _g((2,), torch.int64)
    args = dict(z=z, points=points, ws=ws, rel_tol=rel_tol, keep=keep, normals=normals, colors=colors, out_count=count)
    ops.map_triangulate(L.MAP_COUNT, **args)
    M, Fc = (int(v) for v in count.cpu())
    cm, cf = max(M - short[0], 0), max(Fc - short[1], 0)
    (v, c2), (n, c3), (c, c4) = _g((max(cm, 1), 3), torch.float32), _g((max(cm, 1), 3), torch.float32), _g((max(cm, 1), 3), torch.uint8)
    (idx, c5), (f, c6) = _g((max(cm, 1),), torch.int64), _g((max(cf, 1), 3), torch.int32)
    if not cm:                                                                # nothing may be written at all: one guarded element each
        v, n, c, idx = v[:0], n[:0], c[:0], idx[:0]
    if not cf:
        f = f[:0]
    ops.map_triangulate(L.MAP_SCATTER, vertex_capacity=cm, face_capacity=cf, vertices=v, out_normals=n, out_colors=c, pixel_index=idx, faces=f, **args)
    torch.cuda.synchronize()
    for chk in (c0, c1, c2, c3, c4, c5, c6):
        chk("map_triangulate")
    if not cm:
        for t in (c2, c3, c4, c5):
            assert bool((t.buffer == GUARD_BYTE).all())
    if not cf:
        assert bool((c6.buffer == GUARD_BYTE).all())
    return M, Fc, dict(vertices=v, normals=n, colors=c, pixel_index=idx, faces=f)


def _same_mesh(got, want, name, vertices=None, faces=None):
    for k in ("vertices", "normals", "colors", "pixel_index"):
        _same(got[k], want[k][:vertices], "%s %s" % (name, k))
    _same(got["faces"], want["faces"][:faces], "%s faces" % name)


# ---------------------------------------------------------------------------------------------
# every output equals the twin
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _box():
    s = scenes.box_scene()
    s["z"] = twin.map_depth(points=s["points"], cams=s["cams"], valid=s["valid"], near=scenes.NEAR)
    return s


@functools.lru_cache(maxsize=None)
def _box_normals(rel_tol):
    s = _box()
    return twin.map_normals(s["points"], s["z"], rel_tol)


@pytest.mark.parametrize("rel_tol", [0.03, INF])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_every_output_equals_the_twin(radius, rel_tol):
    s = _box()
    pts, cams, valid, keep, colors = (_dev(s[k]) for k in ("points", "cams", "valid", "keep", "colors"))
    want_n = _box_normals(rel_tol)
    want_plain = twin.map_edges(s["z"], None, radius, rel_tol)
    want_flags = twin.map_edges(s["z"], want_n, radius, rel_tol, MIN_COS)
    want_mesh = {(k, n, c): twin.triangulate(s["z"], s["points"], s["keep"] if k else None, want_n if n else None, s["colors"] if c else None, rel_tol)
                 for k in (0, 1) for n, c in ((0, 0), (1, 1), (1, 0))}
    for rep in range(2):
        z = _depth(points=pts, cams=cams, valid=valid)
        _same(z, s["z"], "z from points")
        _same(_depth(depth=_dev(s["depth"]), valid=valid), s["z"], "z from depth")
        _same(_depth(depth=_dev(s["depth"])), twin.map_depth(depth=s["depth"], near=scenes.NEAR), "z from depth, no valid")
        normals = _normals(pts, z, rel_tol)
        _same(normals, want_n, "normals")
        for tile in TILES:
            _same(_edges(z, None, radius, rel_tol, MIN_COS, tile), want_plain, "flags without normals, tile %d" % tile)
            _same(_edges(z, normals, radius, rel_tol, MIN_COS, tile), want_flags, "flags, tile %d" % tile)
        for (k, n, c), want in want_mesh.items():
            M, Fc, got = _mesh(z, pts, rel_tol, keep if k else None, normals if n else None, colors if c else None)
            assert (M, Fc) == (len(want["vertices"]), len(want["faces"])) and M > 100 and Fc > 100
            _same_mesh(got, want, "mesh keep=%d normals=%d colors=%d" % (k, n, c))


# ---------------------------------------------------------------------------------------------
# views and rows are never stitched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(2, 2), (1, 5), (5, 1), (2, 3)])
def test_views_and_rows_are_never_stitched(H, W):
    pts_h, cams_h = scenes.stacked_views(H, W)
    S = pts_h.shape[0]
    pts, cams = _dev(pts_h), _dev(cams_h)
    want_z = twin.map_depth(points=pts_h, cams=cams_h)
    want_n = twin.map_normals(pts_h, want_z, 0.03)
    want_mesh = twin.triangulate(want_z, pts_h, None, want_n, None, 0.03)
    z = _depth(points=pts, cams=cams)
    normals = _normals(pts, z, 0.03)
    _same(z, want_z, "z")
    _same(normals, want_n, "normals")
    for radius in (1, 2, 3):
        want_f = twin.map_edges(want_z, want_n, radius, 0.03, MIN_COS)
        assert not (want_f & twin.DEPTH_EDGE).any()                           # a neighbouring view, a factor of ten away, would flag every pixel
        for tile in TILES:
            _same(_edges(z, normals, radius, 0.03, MIN_COS, tile), want_f, "flags r %d tile %d" % (radius, tile))
    M, Fc, got = _mesh(z, pts, 0.03, normals=normals)
    assert (M, Fc) == (len(want_mesh["vertices"]), len(want_mesh["faces"])) == ((S * H * W, S * 2 * (H - 1) * (W - 1)) if H > 1 and W > 1 else (0, 0))
    _same_mesh(got, want_mesh, "mesh")
    # each view alone gives the bytes it has in the batch
    for s in range(S):
        zs = _depth(points=pts[s:s + 1].contiguous(), cams=cams[s:s + 1].contiguous())
        ns = _normals(pts[s:s + 1].contiguous(), zs, 0.03)
        assert torch.equal(ns, normals[s:s + 1]) and torch.equal(_edges(zs, ns, 3, 0.03, MIN_COS, L.MAP_TILE_16x16), _edges(z, normals, 3, 0.03, MIN_COS, L.MAP_TILE_16x16)[s:s + 1])
    # directly: the three pixels of every face lie in one view and are a, c, b or b, c, d of one quad
    if Fc:
        pix = got["pixel_index"].cpu().numpy()[got["faces"].cpu().numpy()]
        assert ((pix // (H * W)) == (pix[:, :1] // (H * W))).all()
        first = pix[:, 0]
        x, y = first % W, (first // W) % H
        is_acb = (pix == np.stack([first, first + W, first + 1], 1)).all(axis=1)              # a = first: c below it, b to its right
        is_bcd = (pix == np.stack([first, first + W - 1, first + W], 1)).all(axis=1)          # b = first: c below left, d below
        assert (is_acb ^ is_bcd).all() and is_acb.sum() == is_bcd.sum() == Fc // 2
        assert (y < H - 1).all() and (x[is_acb] < W - 1).all() and (x[is_bcd] >= 1).all()


# ---------------------------------------------------------------------------------------------
# the scan's second level, empty maps, capacities
# ---------------------------------------------------------------------------------------------
def test_scan_second_level_empty_maps_and_capacities():
    pts_h, keep_h = scenes.random_keep_scene()
    S, H, W = keep_h.shape
    assert -(-S * H * W // L.MAP_BLOCK) > 256
    want_z = twin.map_depth(depth=pts_h[..., 2])
    want = twin.triangulate(want_z, pts_h, keep_h, None, None, 0.03)
    pts, keep = _dev(pts_h), _dev(keep_h)
    z = _depth(depth=_dev(np.ascontiguousarray(pts_h[..., 2])))
    for rep in range(2):
        M, Fc, got = _mesh(z, pts, 0.03, keep)
        assert (M, Fc) == (len(want["vertices"]), len(want["faces"])) and M > 20000 and Fc > 20000
        _same_mesh(got, want, "second level")
    M2, F2, short = _mesh(z, pts, 0.03, keep, short=(3, 5))                    # capacities M - 3 and F - 5: exactly the prefix, nothing beyond
    assert (M2, F2) == (M, Fc)
    _same_mesh(short, want, "short capacities", vertices=M - 3, faces=Fc - 5)
    for dead in (torch.full_like(z, float("nan")), None):
        zz = dead if dead is not None else z
        kk = keep if dead is not None else torch.zeros_like(keep)
        M0, F0, empty = _mesh(zz, pts, 0.03, kk)
        assert (M0, F0) == (0, 0) and empty["vertices"].shape[0] == 0
    flags = _edges(torch.full_like(z, float("nan")), None, 2, 0.03, MIN_COS, L.MAP_TILE_32x8)
    assert bool((flags == L.MAP_UNUSABLE).all())


def test_scan_carries_past_1024_workgroups():
    """The count scan is one workgroup of 1024 threads: from 1025 counts on it loops and carries the running total. The smallest such
    map: one view of two rows, 1024 * MAP_BLOCK + 2 pixels, so the last workgroup holds the last two pixels and its offsets are the carry."""
    W = 1024 * L.MAP_BLOCK // 2 + 1
    pts_h, keep_h = scenes.random_keep_scene(S=1, H=2, W=W, seed=11)
    n = keep_h.size
    assert -(-n // L.MAP_BLOCK) == 1025
    keep_h[:, :, -2:] = 1                                                      # the last quad is emitted: vertices in the last workgroup
    want_z = twin.map_depth(depth=pts_h[..., 2])
    want = twin.triangulate(want_z, pts_h, keep_h, None, None, 0.03)
    assert want["pixel_index"][-1] == n - 1 and want["pixel_index"][-2] == n - 2
    pts, keep = _dev(pts_h), _dev(keep_h)
    z = _depth(depth=_dev(np.ascontiguousarray(pts_h[..., 2])))
    _same(z, want_z, "z")
    for rep in range(2):
        M, Fc, got = _mesh(z, pts, 0.03, keep)
        assert (M, Fc) == (len(want["vertices"]), len(want["faces"])) and M > 100000 and Fc > 50000
        _same_mesh(got, want, "carry")


# ---------------------------------------------------------------------------------------------
# winding and orientation
# ---------------------------------------------------------------------------------------------
def test_winding_faces_the_camera_and_agrees_with_the_normals():
    pts_h, _, cams_h, centre = scenes.sphere_patch(H=24, W=31, radius=2.0, focal=90.0)
    pts = _dev(pts_h.astype(F))
    z = _depth(points=pts, cams=_dev(cams_h))
    normals = _normals(pts, z, INF)
    M, Fc, got = _mesh(z, pts, INF, normals=normals)
    assert M == 24 * 31 and Fc == 2 * 23 * 30
    v, n, f = (got[k].cpu().numpy().astype(np.float64) for k in ("vertices", "normals", "faces"))
    f = f.astype(np.int64)
    tri = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.linalg.norm(tri, axis=1) > 0).all()
    assert ((tri * (centre - v[f].mean(axis=1))).sum(1) > 0).all()            # towards the camera centre
    for k in range(3):
        assert ((tri * n[f[:, k]]).sum(1) > 0).all()                          # and along its vertices' map normals
    assert (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-6).all()


# ---------------------------------------------------------------------------------------------
# the glue
# ---------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(head.split(b"element vertex ")[1].split()[0])
    nf = int(head.split(b"element face ")[1].split()[0])
    vert = np.frombuffer(body[:27 * nv], dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    face = np.frombuffer(body[27 * nv:], dtype=[("k", "u1"), ("v", "<i4", (3,))])
    assert len(face) == nf and (face["k"] == 3).all()
    return vert, face["v"]


@pytest.mark.parametrize("with_world_points", [True, False])
def test_predictions_to_mesh_is_the_glue(with_world_points, tmp_path):
    import json
    import struct
    import raster_twin
    s = scenes.prediction_scene()
    S, H, W = s["conf"].shape
    pts, conf, images = _dev(s["points"])[None], _dev(s["conf"])[None], _dev(s["images"])[None]
    ext, intr = _dev(s["extrinsic"]).float()[None], _dev(s["intrinsic"]).float()[None]
    pred = {"images": images, "extrinsic": ext, "intrinsic": intr}
    if with_world_points:
        pred.update(world_points=pts, world_points_conf=conf)
    else:
        pred.update(world_points_from_depth=pts, depth_conf=conf)
    # the twin's route: z, the percentile rule, the depth edges, the normals, the mesh
    cams_h = postprocess._pack_cams(ext[0], intr[0], S, "cuda").cpu().numpy()
    z_h = twin.map_depth(points=s["points"], cams=cams_h, near=1e-3)
    thr = F(np.percentile(s["conf"].reshape(-1), 50.0))
    keep_h = (s["conf"] >= thr) & (s["conf"] > F(1e-5)) & ((twin.map_edges(z_h, None, 1, 0.03) & twin.DEPTH_EDGE) == 0)
    n_h = twin.map_normals(s["points"], z_h, 0.03)
    col_h = np.clip(np.trunc(s["images"] * F(255.0)), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    want = twin.triangulate(z_h, s["points"], keep_h, n_h, col_h, 0.03)
    assert 200 < len(want["vertices"]) < keep_h.size and len(want["faces"]) > 200
    mesh = postprocess.predictions_to_mesh(pred, prediction_mode="Predicted Pointmap" if with_world_points else "Depthmap and Camera Branch")
    assert isinstance(mesh, postprocess.Mesh)
    _same_mesh(dict(vertices=mesh.vertices, normals=mesh.normals, colors=mesh.colors, pixel_index=mesh.pixel_index, faces=mesh.faces), want, "glue")
    cloud = postprocess.predictions_to_point_cloud(pred, prediction_mode="Predicted Pointmap" if with_world_points else "Depthmap and Camera Branch",
                                                   return_indices=True)
    assert torch.equal(mesh.conf_threshold.view(torch.int32), cloud.conf_threshold.view(torch.int32)) and float(mesh.conf_threshold) == float(thr)
    assert np.array_equal(mesh.transform, cloud.transform) and torch.equal(mesh.extrinsic, cloud.extrinsic) and float(mesh.scene_scale) > 0
    # the writers round-trip
    postprocess.write_mesh_ply(str(tmp_path / "m.ply"), mesh, apply_transform=False)
    vert, faces = _read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(vert["p"], want["vertices"]) and np.array_equal(vert["n"], want["normals"]) and np.array_equal(vert["c"], want["colors"])
    assert np.array_equal(faces, want["faces"])
    postprocess.write_mesh_glb(str(tmp_path / "m.glb"), mesh, cameras=True)
    raw = open(str(tmp_path / "m.glb"), "rb").read()
    assert raw[:4] == b"glTF" and struct.unpack("<I", raw[8:12])[0] == len(raw)
    jlen = struct.unpack("<I", raw[12:16])[0]
    gltf = json.loads(raw[20:20 + jlen])
    binary = raw[20 + jlen + 8:]
    acc, views = gltf["accessors"], gltf["bufferViews"]
    assert acc[0]["count"] == len(want["vertices"]) and acc[3]["count"] == 3 * len(want["faces"]) and len(gltf["meshes"][0]["primitives"]) >= 1
    pos = np.frombuffer(binary[views[0]["byteOffset"]:views[0]["byteOffset"] + views[0]["byteLength"]], "<f4").reshape(-1, 3)
    ind = np.frombuffer(binary[views[3]["byteOffset"]:views[3]["byteOffset"] + views[3]["byteLength"]], "<u4").reshape(-1, 3)
    assert np.array_equal(pos, want["vertices"]) and np.array_equal(ind, want["faces"].astype(np.uint32))
    assert len(postprocess.mesh_to_point_cloud(mesh)) == len(want["vertices"])
    # the rasteriser from camera 0: the visible-face map of the twin's mesh, and on the pixels it covers the input depth again
    res = postprocess.render_mesh(mesh, ext[0, :1], intr[0, :1], (H, W), cull="back", return_index=True)
    _, want_depth, want_index = raster_twin.render(want["vertices"], want["faces"], want["normals"], want["colors"], cams_h[:1], H, W,
                                                   cull=raster_twin.CULL_BACK)
    _same(res.index, want_index, "visible faces")
    covered = want_index[0] >= 0
    own = np.zeros((H, W), bool)
    own.reshape(-1)[want["pixel_index"][want["pixel_index"] < H * W]] = True
    assert covered.sum() > 300 and (covered & own).sum() > 300
    dev = np.abs(res.depth.cpu().numpy()[0] - z_h[0])[covered & own]
    print("render_mesh depth against the input z on %d covered vertex pixels: max |diff| %.3g" % (dev.size, dev.max()))
    # edge_mask as keep_mask of the cloud: exactly the flagged pixels go
    edges = postprocess.prediction_edges(pred, prediction_mode="Predicted Pointmap" if with_world_points else "Depthmap and Camera Branch")
    _same(edges.flags, twin.map_edges(z_h, None, 1, 0.03), "prediction_edges")
    mask = postprocess.edge_mask(edges)
    assert 0 < int((~mask).sum()) < mask.numel() // 2
    kw = dict(conf_thres=0.0, return_indices=True, prediction_mode="Predicted Pointmap" if with_world_points else "Depthmap and Camera Branch")
    full = postprocess.predictions_to_point_cloud(pred, **kw)
    kept = postprocess.predictions_to_point_cloud(pred, keep_mask=mask, **kw)
    assert len(full) == S * H * W and torch.equal(kept.indices, full.indices[mask.reshape(-1)[full.indices]])
    normals, z = postprocess.prediction_normals(pred, prediction_mode=kw["prediction_mode"])
    _same(normals, n_h, "prediction_normals")
    _same(z, z_h, "prediction z")
    one = postprocess.predictions_to_mesh(pred, filter_by_frames="1: x", prediction_mode=kw["prediction_mode"], conf_thres=0.0, edge_radius=0, with_normals=False)
    w1 = twin.triangulate(z_h[1:], s["points"][1:], None, None, col_h[1:], 0.03)
    _same_mesh(dict(vertices=one.vertices, normals=one.normals, colors=one.colors, pixel_index=one.pixel_index, faces=one.faces), w1, "frame 1")


def test_predictions_to_mesh_reads_back_once():
    s = scenes.prediction_scene()
    pred = {"images": _dev(s["images"])[None], "extrinsic": _dev(s["extrinsic"]).float()[None], "world_points": _dev(s["points"])[None],
            "world_points_conf": _dev(s["conf"])[None]}
    reads = []
    names = ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__")
    orig = {n: getattr(torch.Tensor, n) for n in names}

    def spy(name):
        def fn(self, *a, **k):
            if self.is_cuda:
                reads.append((name, tuple(self.shape)))
            return orig[name](self, *a, **k)
        return fn
    for n in names:
        setattr(torch.Tensor, n, spy(n))
    try:
        mesh = postprocess.predictions_to_mesh(pred)
    finally:
        for n in names:
            setattr(torch.Tensor, n, orig[n])
    assert reads == [("cpu", (14,))] and mesh.faces.shape[0] > 0              # the two counts and the first camera, in one copy


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing():
    lib = L.load()
    s = _box()
    S, H, W = s["z"].shape
    pts, cams, valid, keep, colors, zin, nin = (_dev(a) for a in (s["points"], s["cams"], s["valid"], s["keep"], s["colors"], s["z"], _box_normals(0.03)))
    (z, _), (nrm, _), (flags, _) = _g((S, H, W), torch.float32), _g((S, H, W, 3), torch.float32), _g((S, H, W), torch.uint8)
    need = ops.map_triangulate_workspace_bytes(S, H, W)
    (ws, _), (count, _), (v, _), (vn, _), (vc, _), (idx, _), (faces, _) = (_g((need,), torch.uint8), _g((2,), torch.int64), _g((64, 3), torch.float32),
                                                                          _g((64, 3), torch.float32), _g((64, 3), torch.uint8), _g((64,), torch.int64),
                                                                          _g((64, 3), torch.int32))
    outs = (z, nrm, flags, ws, count, v, vn, vc, idx, faces)
    nan = float("nan")
    st = torch.cuda.current_stream().cuda_stream
    shape = (dict(S=0), dict(H=-1), dict(W=0), dict(S=8192, H=512, W=512))

    def run(fn, struct, base, **kw):
        q = struct(**base)
        for k, x in kw.items():
            setattr(q, k, x)
        return fn(ctypes.byref(q), st)

    depth = functools.partial(run, lib.ovg_map_depth, L.MapDepthParams, dict(points=pts.data_ptr(), cams=cams.data_ptr(), depth=None, valid=valid.data_ptr(),
                                                                              S=S, H=H, W=W, near=1e-3, z=z.data_ptr()))
    normals = functools.partial(run, lib.ovg_map_normals, L.MapNormalsParams, dict(points=pts.data_ptr(), z=zin.data_ptr(), S=S, H=H, W=W, rel_tol=0.03,
                                                                                   normals=nrm.data_ptr()))
    edges = functools.partial(run, lib.ovg_map_edges, L.MapEdgesParams, dict(z=zin.data_ptr(), normals=nin.data_ptr(), S=S, H=H, W=W, radius=2, rel_tol=0.03,
                                                                             min_cos=0.5, tile=L.MAP_TILE_16x16, pad=0, flags=flags.data_ptr()))
    tri = functools.partial(run, lib.ovg_map_triangulate, L.MapTriangulateParams,
                            dict(z=zin.data_ptr(), points=pts.data_ptr(), keep=keep.data_ptr(), normals=nin.data_ptr(), colors=colors.data_ptr(), S=S, H=H, W=W,
                                 rel_tol=0.03, stage=L.MAP_COUNT | L.MAP_SCATTER, pad=0, vertex_capacity=64, face_capacity=64, out_vertices=v.data_ptr(),
                                 out_normals=vn.data_ptr(), out_colors=vc.data_ptr(), out_pixel_index=idx.data_ptr(), out_faces=faces.data_ptr(),
                                 out_count=count.data_ptr(), ws=ws.data_ptr(), ws_bytes=need))
    for bad in shape + (dict(points=None), dict(depth=zin.data_ptr()), dict(cams=None), dict(z=None), dict(near=0.0), dict(near=-1.0), dict(near=nan),
                        dict(near=INF), dict(z=z.data_ptr() + 2), dict(points=pts.data_ptr() + 1)):
        assert depth(**bad) == -1, bad
    for bad in shape + (dict(points=None), dict(z=None), dict(normals=None), dict(rel_tol=-0.5), dict(rel_tol=nan), dict(normals=nrm.data_ptr() + 2)):
        assert normals(**bad) == -1, bad
    for bad in shape + (dict(z=None), dict(flags=None), dict(radius=0), dict(radius=4), dict(rel_tol=-1.0), dict(rel_tol=nan), dict(min_cos=nan),
                        dict(tile=5), dict(tile=-1), dict(z=zin.data_ptr() + 2)):
        assert edges(**bad) == -1, bad
    for bad in shape + (dict(z=None), dict(points=None), dict(ws=None), dict(out_count=None), dict(rel_tol=-1.0), dict(rel_tol=nan), dict(stage=0),
                        dict(stage=4), dict(vertex_capacity=-1), dict(face_capacity=-1), dict(out_vertices=None), dict(out_normals=None),
                        dict(out_colors=None), dict(out_pixel_index=None), dict(out_faces=None), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1),
                        dict(ws_bytes=0), dict(out_count=count.data_ptr() + 4), dict(out_pixel_index=idx.data_ptr() + 4), dict(out_faces=faces.data_ptr() + 2)):
        assert tri(**bad) == -1, bad
    assert lib.ovg_map_triangulate_workspace_bytes(8192, 512, 512) == -1 and lib.ovg_map_triangulate_workspace_bytes(1, 1 << 16, 1 << 15) == -1
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.contiguous().view(torch.uint8) == GUARD_BYTE).all())
    assert depth() == 0 and normals() == 0 and edges() == 0 and tri() == 0    # the same structs without the fault are accepted
    torch.cuda.synchronize()
    assert count.tolist()[0] > 64 and not bool((faces.contiguous().view(torch.uint8) == GUARD_BYTE).all())


# ---------------------------------------------------------------------------------------------
# the stream and no-sync contract of the four entries (recorded for test_gpu_stream_contract's coverage test)
# ---------------------------------------------------------------------------------------------
def test_map_geometry_entries_are_gated():
    s = _box()
    S, H, W = s["z"].shape
    t = torch.from_numpy
    z_h, n_h = s["z"], _box_normals(0.03)

    def depth_case():
        c = sc.Case("map_depth from points, 3 x 37 x 53, valid")
        pts, valid = c.inp(t(s["points"])), c.inp(t(s["valid"]))
        cams = c.const(t(s["cams"]))
        z = c.out((S, H, W), torch.float32)
        c.call = lambda: ops.map_depth(points=pts, cams=cams, valid=valid, near=scenes.NEAR, out=z)
        return c

    def normals_case():
        c = sc.Case("map_normals 3 x 37 x 53")
        pts, z = c.inp(t(s["points"])), c.inp(t(z_h))
        out = c.out((S, H, W, 3), torch.float32)
        c.call = lambda: ops.map_normals(pts, z, rel_tol=0.03, out=out)
        return c

    def edges_case(tile, name):
        def build():
            c = sc.Case("map_edges %s, radius 3, with normals" % name)
            z, n = c.inp(t(z_h)), c.inp(t(n_h))
            out = c.out((S, H, W), torch.uint8)
            c.call = lambda: ops.map_edges(z, n, radius=3, rel_tol=0.03, min_cos=MIN_COS, tile=tile, out=out)
            return c
        return build

    def triangulate_case():
        c = sc.Case("map_triangulate COUNT then SCATTER, keep + normals + colors")
        z, pts, keep = c.inp(t(z_h)), c.inp(t(s["points"])), c.inp(t(s["keep"]))
        n, col = c.inp(t(n_h)), c.inp(t(s["colors"]))
        ws, count = c.ws(ops.map_triangulate_workspace_bytes(S, H, W)), c.out((2,), torch.int64)
        want = twin.triangulate(z_h, s["points"], s["keep"], n_h, s["colors"], 0.03)
        M, Fc = len(want["vertices"]), len(want["faces"])
        v, vn, vc, idx, f = (c.out((M, 3), torch.float32), c.out((M, 3), torch.float32), c.out((M, 3), torch.uint8), c.out((M,), torch.int64),
                             c.out((Fc, 3), torch.int32))

        def call():
            args = dict(z=z, points=pts, ws=ws, rel_tol=0.03, keep=keep, normals=n, colors=col, out_count=count)
            ops.map_triangulate(L.MAP_COUNT, **args)
            ops.map_triangulate(L.MAP_SCATTER, vertex_capacity=M, face_capacity=Fc, vertices=v, out_normals=vn, out_colors=vc, pixel_index=idx, faces=f, **args)
        c.call = call
        return c

    cases = tsc.family([depth_case, normals_case, edges_case(L.MAP_TILE_256x1, "plain"), edges_case(L.MAP_TILE_16x16, "16x16 in LDS"), triangulate_case],
                       "map geometry")
    assert {e for c in cases for e in c.entries} == {"ovg_map_depth", "ovg_map_normals", "ovg_map_edges", "ovg_map_triangulate"}
