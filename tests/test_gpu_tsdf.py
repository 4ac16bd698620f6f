"""ovg_tsdf_integrate / ovg_tsdf_extract and postprocess.tsdf_* / fuse_predictions on the device against tests/tsdf_twin.py, byte for
byte: volumes whose dims leave partial bricks on every axis for every tile, cameras behind, inside and half across the volume, depth
maps with 0, NaN, infinities, negatives and values at the near plane, every optional input, view ranges and populated volumes; the
mesh of analytic volumes and of a random-sign volume with holes; capacities below the counts; the Python layer on the sphere scene,
a hand-made prediction dict and the real infinigen depth views. Every output sits in an exact-size guarded buffer, every case runs
twice."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import kernel_guards as kg
import pointcloud_twin as pctwin
import tsdf_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
REAL = os.path.join(common.ROOT, "tests", "golden", "real")
TILES = (L.TSDF_TILE_DEFAULT, L.TSDF_TILE_256x1x1, L.TSDF_TILE_8x8x4, L.TSDF_TILE_16x4x4, L.TSDF_TILE_32x8x1)
H, W = 37, 53


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded_like(a):
    """A guarded device copy of the host array a (at least 2-D). -> (view, check)."""
    view, check = kg.guarded(a.shape, torch.from_numpy(a[:0].copy()).dtype, "cuda")
    view.copy_(_dev(a))
    return view, check


# ---------------------------------------------------------------------------------------------------------------------------------
# integrate
# ---------------------------------------------------------------------------------------------------------------------------------

def _scene(dims, S, seed=0):
    """A lattice of `dims` points over about [-0.5, 0.5]^3 with a sphere of radius 0.3 in it, and five views in this order: one whose
    narrow frame covers only part of the volume, one inside the volume, one behind it looking away, two ordinary ones. Their depth
    maps (sphere in front of a backdrop) are spoiled with 0, NaN, +-inf, negatives and values at and below the near plane; the
    weights with 0, negatives and non-finite values; valid has holes."""
    rng = np.random.default_rng(seed)
    voxel = F(1.0 / max(max(dims) - 1, 1))
    origin = np.array([-0.5 * float(voxel) * (d - 1) for d in dims], F)
    ext = np.stack([twin.look_at((1.4, 0.3, -0.2), (0.0, 0.25, 0.2)), twin.look_at((0.05, -0.1, 0.1), (1.0, 0.2, 0.3)),
                    twin.look_at((0.0, 0.0, -1.5), (0.0, 0.0, -3.0)), twin.look_at((-0.9, -0.8, 1.0), (0.0, 0.0, 0.0)),
                    twin.look_at((0.3, 1.2, 0.9), (0.05, 0.0, -0.05))])[:S]
    fov = np.array([25.0, 100.0, 70.0, 60.0, 75.0])[:S]
    intr = np.stack([twin.pinhole(H, W, f) for f in fov])
    intr[:, 1, 1] *= 0.9                                                    # non-square pixels
    depth = np.concatenate([twin.sphere_depth(ext[s:s + 1], intr[s], H, W, (0.0, 0.0, 0.0), 0.3, miss=2.5) for s in range(S)])
    r = rng.random((S, H, W))
    bad = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -1.0, 1e-3, 5e-4], F)
    depth = np.where(r < 0.12, bad[rng.integers(0, len(bad), r.shape)], depth).astype(F)
    wbad = np.array([0.0, -2.0, np.nan, np.inf, -np.inf], F)
    obs = np.where(rng.random((S, H, W)) < 0.1, wbad[rng.integers(0, len(wbad), r.shape)], rng.choice(np.array([0.5, 1.0, 2.0, 0.3], F), r.shape)).astype(F)
    valid = (rng.random((S, H, W)) >= 0.1).astype(np.uint8) * rng.choice(np.array([1, 7, 255], np.uint8), r.shape)
    colors = rng.integers(0, 256, (S, H, W, 3)).astype(np.uint8)
    return dict(dims=dims, origin=origin, voxel=voxel, trunc=F(0.11), depth=depth, cams=twin.pack_cams(ext, intr), valid=valid, obs_weight=obs,
                colors=colors, S=S)


def _device_integrate(sc, state, opts, tile=L.TSDF_TILE_DEFAULT, views=None, max_weight=64.0, near=1e-3):
    """One or more device calls on guarded copies of `state` = (tsdf, weight, color or None). views: a list of (first, count), all
    views in one call by default. -> the three host arrays (color None without a colour volume)."""
    T, ct = _guarded_like(state[0])
    Wt, cw = _guarded_like(state[1])
    C, cc = _guarded_like(state[2]) if state[2] is not None else (None, None)
    kw = {k: _dev(sc[k]) for k in opts}
    for first, count in (views or [(0, sc["S"])]):
        ops.tsdf_integrate(T, Wt, _dev(sc["depth"]), _dev(sc["cams"]), [float(v) for v in sc["origin"]], float(sc["voxel"]), float(sc["trunc"]),
                           max_weight=max_weight, near=near, color=C, view_first=first, view_count=count, tile=tile, **kw)
    torch.cuda.synchronize()
    for c, name in ((ct, "tsdf"), (cw, "weight"), (cc, "color")):
        if c is not None:
            c(name)
    return T.cpu().numpy(), Wt.cpu().numpy(), None if C is None else C.cpu().numpy()


def _twin_integrate(sc, state, opts, views=None, max_weight=64.0, near=1e-3):
    T, Wt, C = (None if a is None else a.copy() for a in state)
    twin.integrate(T, Wt, C, sc["origin"], sc["voxel"], sc["trunc"], max_weight, near, sc["depth"], sc["cams"], views=views,
                   **{k: sc[k] for k in opts})
    return T, Wt, C


def _same(got, want, name):
    for g, w, what in zip(got, want, ("tsdf", "weight", "color")):
        assert (g is None) == (w is None), (name, what)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (name, what, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


OPTS = ((), ("valid",), ("obs_weight",), ("colors",), ("valid", "obs_weight", "colors"))


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (9, 5, 3), (65, 7, 5), (63, 9, 4), (33, 33, 33)])
@pytest.mark.parametrize("S", [1, 2, 5])
def test_integrate_matches_twin_bit_exactly(dims, S):
    L.require_gpu()
    sc = _scene(dims, S, seed=S)
    fresh = twin.fresh(dims)
    for opts in OPTS:
        state = fresh if "colors" in opts else (fresh[0], fresh[1], None)
        want = _twin_integrate(sc, state, opts)
        got = _device_integrate(sc, state, opts)
        _same(got, want, (dims, S, opts))
        _same(_device_integrate(sc, state, opts), got, (dims, S, opts, "again"))            # two runs: identical bytes
    if S == 5 and dims == (33, 33, 33):
        assert 0.2 < (want[1] > 0).mean() < 0.95 and (want[0] < 0).sum() > 100 and (want[2][..., 3] > 0).sum() > 100   # the case is not empty
    # every tile gives the same bytes (with every optional input)
    opts = OPTS[-1]
    for tile in TILES:
        _same(_device_integrate(sc, fresh, opts, tile=tile), want, (dims, S, "tile", tile))
    # a colour volume that no colours are given for is left alone
    got = _device_integrate(sc, fresh, ("valid",))
    assert got[2].tobytes() == fresh[2].tobytes()
    _same(got[:2], _twin_integrate(sc, fresh, ("valid",))[:2], (dims, S, "colour volume without colours"))
    # a near plane that cuts into the scene, a clamp that is reached
    _same(_device_integrate(sc, fresh, opts, max_weight=1.5, near=0.9), _twin_integrate(sc, fresh, opts, max_weight=1.5, near=0.9), (dims, S, "near / clamp"))
    if S > 1:
        # a view range, then the rest, equals all at once; so does one call per view
        for k in {1, S - 1}:
            _same(_device_integrate(sc, fresh, opts, views=[(0, k), (k, S - k)]), want, (dims, S, "split", k))
        _same(_device_integrate(sc, fresh, opts, views=[(s, 1) for s in range(S)], tile=L.TSDF_TILE_256x1x1), want, (dims, S, "per view"))
        # a range alone is the twin's range
        _same(_device_integrate(sc, fresh, opts, views=[(1, S - 1)]), _twin_integrate(sc, fresh, opts, views=range(1, S)), (dims, S, "range"))
    # integration into an already populated volume (a second pass over the same views, then with other options)
    _same(_device_integrate(sc, want, opts), _twin_integrate(sc, want, opts), (dims, S, "populated"))
    _same(_device_integrate(sc, want, ("obs_weight",)), _twin_integrate(sc, want, ("obs_weight",)), (dims, S, "populated, other inputs"))


# ---------------------------------------------------------------------------------------------------------------------------------
# extract
# ---------------------------------------------------------------------------------------------------------------------------------

def _device_extract(tsdf, weight, color, origin, voxel, min_weight=1.0, capacity=None):
    """COUNT, then SCATTER into exact-size guarded buffers (capacity: (vertices, quads) below the counts to drop the tail).
    -> (vertices, normals, colors, faces, (M, Q)) as host arrays."""
    nz, ny, nx = tsdf.shape
    need = ops.tsdf_extract_workspace_bytes(nx, ny, nz)
    ws, cws = kg.guarded((1, need), torch.uint8, "cuda")
    cnt, ccnt = kg.guarded((1, 2), torch.int64, "cuda")
    dt, dw, dc = _dev(tsdf), _dev(weight), None if color is None else _dev(color)
    args = dict(tsdf=dt, weight=dw, origin=[float(v) for v in origin], voxel=float(voxel), ws=ws.view(-1), min_weight=min_weight, color=dc,
                out_count=cnt.view(-1))
    ops.tsdf_extract(L.TSDF_COUNT, **args)
    M, Q = (int(v) for v in cnt.cpu().numpy().reshape(-1))
    cv, cq = (M, Q) if capacity is None else (min(capacity[0], M), min(capacity[1], Q))
    empty = {"vertices": np.zeros((0, 3), F), "normals": np.zeros((0, 3), F), "colors": np.zeros((0, 3), np.uint8), "faces": np.zeros((0, 3), np.int32)}
    outs = {}
    if cv:
        outs.update(vertices=kg.guarded((cv, 3), torch.float32, "cuda"), normals=kg.guarded((cv, 3), torch.float32, "cuda"),
                    colors=kg.guarded((cv, 3), torch.uint8, "cuda"))
    if cq:
        outs.update(faces=kg.guarded((2 * cq, 3), torch.int32, "cuda"))
    ops.tsdf_extract(L.TSDF_SCATTER, vertex_capacity=cv, quad_capacity=cq, **{k: v[0] for k, v in outs.items()}, **args)
    torch.cuda.synchronize()
    for name, (view, check) in outs.items():
        check(name)
    cws("ws"), ccnt("count")
    assert tuple(int(v) for v in cnt.cpu().numpy().reshape(-1)) == (M, Q)
    return tuple(outs[k][0].cpu().numpy() if k in outs else empty[k] for k in ("vertices", "normals", "colors", "faces")) + ((M, Q),)


def _same_mesh(got, want, name, capacity=None):
    M, Q = len(want[0]), len(want[3]) // 2
    assert got[4] == (M, Q), (name, got[4], (M, Q))
    cv, cq = (M, Q) if capacity is None else (min(capacity[0], M), min(capacity[1], Q))
    for g, w, what, n in zip(got[:4], want, ("vertices", "normals", "colors", "faces"), (cv, cv, cv, 2 * cq)):
        assert g.dtype == w.dtype and g.shape == (n, 3), (name, what, g.dtype, g.shape, n)
        assert g.tobytes() == w[:n].tobytes(), (name, what, int((g != w[:n]).sum()))


def _colour_volume(shape, seed):
    rng = np.random.default_rng(seed)
    c = (rng.random(shape + (4,)) * 255).astype(F)
    c[..., 3] = np.where(rng.random(shape) < 0.3, 0, rng.random(shape) * 3).astype(F)
    return c


@pytest.mark.parametrize("kind", ["sphere", "torus", "slab", "two_spheres"])
def test_extract_analytic_volumes_matches_twin_bit_exactly(kind):
    L.require_gpu()
    for n in (9, 17, 33):
        tsdf, weight, origin, voxel, _ = twin.sdf_volume(kind, n)
        for color in (None, _colour_volume(tsdf.shape, n)):
            want = twin.extract(tsdf, weight, color, origin, voxel)
            assert len(want[0]) > 50 and len(want[3]) > 50
            got = _device_extract(tsdf, weight, color, origin, voxel)
            _same_mesh(got, want, (kind, n))
            _same_mesh(_device_extract(tsdf, weight, color, origin, voxel), want, (kind, n, "again"))
        # capacities below the counts drop the tail and write nothing past it (the guards of the exact-size buffers)
        M, Q = got[4]
        for cap in ((M // 2, Q // 3), (1, 1), (M, Q - 1), (M - 1, Q), (M + 5, Q + 5)):
            _same_mesh(_device_extract(tsdf, weight, color, origin, voxel, capacity=cap), want, (kind, n, cap), capacity=cap)
    # a box that is no cube: the slab in (19, 12, 7) lattice points
    tsdf, weight, origin, voxel, _ = twin.sdf_volume(kind, 0, dims=(19, 12, 7))
    _same_mesh(_device_extract(tsdf, weight, None, origin, voxel), twin.extract(tsdf, weight, None, origin, voxel), (kind, "box"))


def test_extract_random_signs_with_holes_and_the_empty_cases():
    L.require_gpu()
    for seed in range(4):
        rng = np.random.default_rng(seed)
        shape = (5, 6, 7)                                                   # (nz, ny, nx): the (7, 6, 5) volume
        tsdf = (rng.random(shape) * 2 - 1).astype(F)
        tsdf[rng.random(shape) < 0.05] = F(-0.0)                            # outside
        tsdf[rng.random(shape) < 0.05] = F(0.0)
        weight = np.where(rng.random(shape) < 0.12, F(0.5), rng.choice(np.array([1.0, 2.5, 64.0], F), shape)).astype(F)
        color = _colour_volume(shape, seed)
        origin, voxel = np.array([0.3, -7.0, 100.0], F), F(0.0173)
        for mw in (1.0, 0.5, 2.5):
            want = twin.extract(tsdf, weight, color, origin, voxel, mw)
            st = twin.mesh_stats(want[0], want[3])
            if mw == 0.5:
                assert len(want[0]) > 60 and st["bad_edges"] > 0            # ambiguous cells: no manifold, and none is promised
            _same_mesh(_device_extract(tsdf, weight, color, origin, voxel, mw), want, ("random", seed, mw))
        # the default min_weight leaves holes: fewer cells than with every point observed, and quads with a missing cell are dropped
        assert 0 < len(twin.extract(tsdf, weight, color, origin, voxel, 1.0)[0]) < len(twin.extract(tsdf, weight, color, origin, voxel, 0.5)[0])
    # the empty cases return zeros
    one, o, v = np.ones((4, 5, 6), F), np.zeros(3, F), F(0.1)
    for tsdf, weight in ((one, one), (-one, one), (np.where(np.arange(120).reshape(4, 5, 6) % 2 == 0, F(-1), F(1)).astype(F), 0.5 * one)):
        got = _device_extract(tsdf, weight, None, o, v)
        assert got[4] == (0, 0) and all(len(a) == 0 for a in got[:4])
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1), (1, 1, 300)):
        tsdf = np.where(np.arange(int(np.prod(shape))).reshape(shape) % 2 == 0, F(-1), F(1)).astype(F)
        assert _device_extract(tsdf, np.ones(shape, F), None, o, v)[4] == (0, 0), shape
    # two layers: one layer of cells, the quads of the inner z edges only; a single row of cells has vertices and no face
    tsdf = np.stack([-np.ones((5, 5), F), np.ones((5, 5), F)])
    got = _device_extract(tsdf, np.ones(tsdf.shape, F), None, o, v)
    assert got[4] == (16, 9)
    _same_mesh(got, twin.extract(tsdf, np.ones(tsdf.shape, F), None, o, v), "two layers")
    got = _device_extract(tsdf[:, :2], np.ones((2, 2, 5), F), None, o, v)
    assert got[4] == (4, 0) and twin.extract(tsdf[:, :2], np.ones((2, 2, 5), F), None, o, v)[0].shape == (4, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------------------

def _twin_of(volume, depth, cams, valid=None, colors=None, **kw):
    """The twin on the volume parameters the Python layer chose. -> (state, mesh)."""
    T, Wt, C = twin.fresh(volume.dims, color=volume.color is not None)
    origin, voxel = np.array(volume.origin, F), F(volume.voxel_size)
    assert tuple(float(v) for v in origin) == tuple(volume.origin) and float(voxel) == volume.voxel_size
    twin.integrate(T, Wt, C, origin, voxel, F(volume.trunc), kw.get("max_weight", 64.0), kw.get("near", 1e-3), depth, cams, valid=valid, colors=colors)
    return (T, Wt, C), twin.extract(T, Wt, C, origin, voxel, kw.get("min_weight", 1.0))


def _same_volume(volume, state, name):
    _same((volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy(), None if volume.color is None else volume.color.cpu().numpy()), state, name)


def _same_py_mesh(mesh, want, name):
    for g, w, what in zip((mesh.vertices, mesh.normals, mesh.colors, mesh.faces), want, ("vertices", "normals", "colors", "faces")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, what, g.shape, w.shape)


def test_python_layer_on_the_sphere_scene(tmp_path):
    L.require_gpu()
    sc = twin.sphere_scene(24, 64)
    depth, ext, intr, r = sc["depth"], sc["ext"], sc["intr"], sc["radius"]
    S, Hs, Ws = depth.shape
    hit = depth < 100 * r
    pts = _dev(ctwin.unproject64(depth, ext, intr))
    vol = postprocess.tsdf_volume_for(pts, resolution=40, valid=_dev(hit))
    # the bounds of the sphere's visible points, 4 voxels of margin: the longest side spans 40 lattice points
    assert max(vol.dims) == 40 and min(vol.dims) >= 38 and vol.trunc == float(F(4.0 * vol.voxel_size)) and vol.color is not None
    assert abs(vol.voxel_size - 2 * r / 31) < 0.02 * r / 31 and all(abs(o + r + 4 * vol.voxel_size) < 0.05 * r for o in vol.origin)
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and bool((vol.color == 0).all())
    rng = np.random.default_rng(0)
    images = rng.random((S, 3, Hs, Ws)).astype(F)
    images[0, :, :4] = np.array([np.nan, -0.5, 1.5, np.inf], F)[None, :, None]
    out = postprocess.tsdf_integrate(vol, _dev(depth), ext, intr, images=_dev(images))
    assert out is vol
    cams = twin.pack_cams(ext, intr)
    colors = pctwin.colors_u8(images).reshape(S, Hs, Ws, 3)
    state, want = _twin_of(vol, depth, cams, colors=colors)
    _same_volume(vol, state, "sphere scene")
    mesh = postprocess.tsdf_extract(vol)
    _same_py_mesh(mesh, want, "sphere scene")
    st = twin.mesh_stats(want[0], want[3])
    dist = np.abs(np.linalg.norm(want[0].astype(np.float64), axis=1) - r) / vol.voxel_size
    assert st["chi"] == 2 and abs(st["volume"] / (4.0 / 3.0 * np.pi * r ** 3) - 1) <= 0.03 and dist.mean() <= 0.2 and dist.max() <= 1.5
    assert (mesh.transform == np.eye(4)).all() and mesh.extrinsic is None
    # the incremental form through the Python layer, with u8 images, (S,H,W,1) depth, device cameras and a bool mask
    vol2 = postprocess.tsdf_volume(vol.origin, vol.voxel_size, vol.dims, trunc=vol.trunc)
    for views in ((0, 5), range(5, S)):
        postprocess.tsdf_integrate(vol2, _dev(depth)[..., None], _dev(ext), _dev(intr), images=_dev(colors), views=views,
                                   valid=torch.ones(S, Hs, Ws, dtype=torch.bool, device="cuda"), weight=torch.ones(S, Hs, Ws, device="cuda"))
    _same_volume(vol2, state, "sphere scene, two calls")
    # the mesh as a cloud: every cloud function takes it
    cloud = postprocess.mesh_to_point_cloud(mesh)
    assert torch.equal(cloud.points, mesh.vertices) and torch.equal(cloud.colors, mesh.colors) and len(cloud) == len(want[0])
    assert np.asarray(cloud.scene_scale.cpu().numpy(), F).tobytes() == np.asarray(pctwin.scene_scale(want[0]), F).tobytes()
    small = postprocess.voxel_downsample(cloud, voxel_size=4 * vol.voxel_size)
    assert 0 < len(small) < len(cloud)
    nrm = postprocess.estimate_normals(cloud, k=8, radius=4 * vol.voxel_size)
    assert nrm.shape == (len(cloud), 3)
    for writer, path in ((postprocess.write_mesh_ply, "m.ply"), (postprocess.write_mesh_glb, "m.glb"), (postprocess.write_ply, "c.ply")):
        writer(str(tmp_path / path), cloud if path == "c.ply" else mesh)
        assert os.path.getsize(str(tmp_path / path)) > 15 * len(cloud)
    # a volume without colours, a min_weight that thins the mesh, an empty volume
    vol3 = postprocess.tsdf_volume(vol.origin, vol.voxel_size, vol.dims, trunc=vol.trunc, color=False)
    postprocess.tsdf_integrate(vol3, _dev(depth), ext, intr)
    _same_volume(vol3, (state[0], state[1], None), "no colours")
    m3 = postprocess.tsdf_extract(vol3, min_weight=3.0)
    _same_py_mesh(m3, twin.extract(state[0], state[1], None, np.array(vol.origin, F), F(vol.voxel_size), 3.0), "min_weight 3")
    assert bool((m3.colors == 128).all()) and 0 < len(m3.vertices) <= len(mesh.vertices)
    empty = postprocess.tsdf_extract(postprocess.tsdf_volume((0, 0, 0), 0.1, (5, 4, 3)))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.faces.dtype == torch.int32
    assert len(postprocess.mesh_to_point_cloud(empty)) == 0
    # errors on the device path
    with pytest.raises(ValueError, match="exceed max_voxels"):
        postprocess.tsdf_volume_for(pts, voxel_size=1e-4, valid=_dev(hit))
    with pytest.raises(ValueError, match="no finite point"):
        postprocess.tsdf_volume_for(torch.full((4, 3), float("nan"), device="cuda"))
    with pytest.raises(L.OvgError):
        postprocess.tsdf_integrate(vol, torch.from_numpy(depth), ext, intr)
    with pytest.raises(ValueError):
        postprocess.tsdf_integrate(vol, _dev(depth), ext[:3], intr)


def test_fuse_predictions_on_a_hand_made_dict():
    L.require_gpu()
    sc = twin.sphere_scene(24, 48)
    depth, ext, intr, r = sc["depth"], sc["ext"].astype(F), np.broadcast_to(sc["intr"].astype(F), (14, 3, 3)).copy(), sc["radius"]
    depth = np.where(depth > 100 * r, F(4 * r), depth).astype(F)              # a backdrop 4 r away: outside the volume's reach
    S, Hs, Ws = depth.shape
    rng = np.random.default_rng(1)
    images = rng.random((S, 3, Hs, Ws)).astype(F)
    conf = (1.0 + 4.0 * rng.random((S, Hs, Ws))).astype(F)
    conf[depth > 2 * r] = F(1e-6)                                            # the backdrop carries no confidence: below min_conf
    pred = {"images": _dev(images)[None], "depth": _dev(depth)[None, ..., None], "depth_conf": _dev(conf)[None], "extrinsic": _dev(ext)[None],
            "intrinsic": _dev(intr)[None], "world_points_from_depth": _dev(ctwin.unproject64(depth, ext, intr))[None]}
    keep = rng.random((S, Hs, Ws)) < 0.9
    volume, mesh = postprocess.fuse_predictions(pred, resolution=36, conf_thres=20.0, keep_mask=_dev(keep))
    thr = pctwin.percentile(conf.reshape(-1), [20.0])[0]
    valid = np.isfinite(depth) & (depth > F(1e-3)) & (conf >= thr) & (conf > F(1e-5)) & keep
    assert 0.2 < valid.mean() < 0.8 and max(volume.dims) == 36
    # the same volume by hand
    by_hand = postprocess.tsdf_volume_for(pred["world_points_from_depth"][0], resolution=36, valid=_dev(valid))
    assert by_hand.dims == volume.dims and by_hand.origin == volume.origin and by_hand.voxel_size == volume.voxel_size
    state, want = _twin_of(volume, depth, twin.pack_cams(ext, intr), valid=valid.astype(np.uint8), colors=pctwin.colors_u8(images).reshape(S, Hs, Ws, 3))
    _same_volume(volume, state, "fused")
    _same_py_mesh(mesh, want, "fused")
    assert len(want[0]) > 500 and len(want[3]) > 500                          # the masked-out backdrop leaves holes at the limb: no closed mesh is asked for
    assert np.abs(mesh.transform - pctwin.alignment(ext[0])).max() < 1e-12 and torch.equal(mesh.extrinsic, pred["extrinsic"][0])
    assert np.asarray(mesh.scene_scale.cpu().numpy(), F).tobytes() == np.asarray(pctwin.scene_scale(want[0]), F).tobytes()
    # without confidences and masks every finite depth counts; without colours the mesh is grey; the cameras decoded from pose_enc
    # are the dict's own when it carries them
    bare = {k: v for k, v in pred.items() if k != "depth_conf"}
    v2, m2 = postprocess.fuse_predictions(bare, voxel_size=volume.voxel_size, color=False, conf_thres=0)
    assert v2.color is None and bool((m2.colors == 128).all()) and len(m2.vertices) > 0
    v3, m3 = postprocess.fuse_predictions(pred, voxel_size=volume.voxel_size, conf_thres=0, min_conf=0.5)
    state3, want3 = _twin_of(v3, depth, twin.pack_cams(ext, intr), valid=(conf > F(0.5)).astype(np.uint8), colors=pctwin.colors_u8(images).reshape(S, Hs, Ws, 3))
    _same_volume(v3, state3, "fused, min_conf")
    _same_py_mesh(m3, want3, "fused, min_conf")
    with pytest.raises(ValueError):
        postprocess.fuse_predictions(pred, keep_mask=_dev(keep)[:2])
    with pytest.raises(L.OvgError):
        postprocess.fuse_predictions(pred, keep_mask=torch.from_numpy(keep))


def test_real_depth_views_fuse_like_the_twin():
    L.require_gpu()
    g = np.load(os.path.join(REAL, "infinigen_294_aux_inputs.npz"))
    ext, intr, depth = g["extrinsics"][0], g["intrinsics"][0], g["depth"].astype(F)
    valid = depth > 0                                                       # pixels with depth 0 are invalid
    S, Hs, Ws = depth.shape
    assert (S, Hs, Ws) == (4, 294, 518)
    pts = ctwin.unproject64(depth, ext, intr)
    lo, hi = pts[valid].min(0).astype(np.float64), pts[valid].max(0).astype(np.float64)
    dims = (96, 64, 96)
    voxel = float(F(((hi - lo) / (np.array(dims) - 1)).max()))               # the 96 x 64 x 96 volume over the cloud's bounds
    vol = postprocess.tsdf_volume([float(v) for v in lo], voxel, dims)
    rng = np.random.default_rng(2)
    colors = rng.integers(0, 256, (S, Hs, Ws, 3)).astype(np.uint8)
    postprocess.tsdf_integrate(vol, _dev(depth), ext, intr, images=_dev(colors), valid=_dev(valid))
    state, want = _twin_of(vol, depth, twin.pack_cams(ext, intr), valid=valid.astype(np.uint8), colors=colors)
    _same_volume(vol, state, "infinigen")
    mesh = postprocess.tsdf_extract(vol)
    _same_py_mesh(mesh, want, "infinigen")
    assert len(want[0]) > 1000 and len(want[3]) > 1000 and (state[1] > 0).mean() > 0.05
    assert torch.equal(postprocess.tsdf_extract(vol).faces, mesh.faces)
