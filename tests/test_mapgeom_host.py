"""Image-space map geometry (ovg_map_depth / ovg_map_normals / ovg_map_edges / ovg_map_triangulate), host side: the numpy twin
(tests/mapgeom_twin.py) against the recorded faces of the reference's pts3d_to_trimesh, against formulations that share no code with
it (scipy's rank filters, analytic normals of a plane and a sphere), crafted boundary cases in powers of two, the C ABI without a
device (struct layouts, enums, every argument check that returns before a launch), the Python layers' argument checks, and the
conditions under which the GPU comparison of tests/test_gpu_mapgeom.py cannot pass on empty output."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import mapgeom_scenes as scenes
import mapgeom_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
GOLDEN = os.path.join(common.ROOT, "tests", "golden", "mapgeom_reference.npz")
F = np.float32
INF = float("inf")


# ---------------------------------------------------------------------------------------------
# the twin against the reference and against independent formulations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, shape", [("small", (5, 7)), ("large", (12, 9))])
def test_twin_emits_the_reference_faces(name, shape):
    g = np.load(GOLDEN)
    pts, valid, want = g[name + "_pts"], g[name + "_valid"], g[name + "_triples"].astype(np.int64)
    assert pts.shape == shape + (3,) and valid.shape == shape and 0 < len(want) < 2 * (shape[0] - 1) * (shape[1] - 1)
    z = twin.map_depth(depth=pts[None, ..., 2])
    pix, emitted = twin.quad_faces(z, pts[None], keep=valid[None], rel_tol=np.inf)
    assert np.array_equal(twin.pixel_triples(pix[emitted]), want)
    mesh = twin.triangulate(z, pts[None], keep=valid[None], rel_tol=np.inf)
    assert np.array_equal(twin.pixel_triples(mesh["pixel_index"][mesh["faces"]]), want)
    assert np.array_equal(mesh["pixel_index"], np.unique(want)) and np.array_equal(mesh["vertices"], pts.reshape(-1, 3)[mesh["pixel_index"]])
    # the other diagonal (a-d) is not what the reference builds
    H, W = shape
    idx = np.arange(H * W).reshape(H, W)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    other = np.concatenate([np.c_[a, c, d], np.c_[a, d, b]])
    other = other[valid.ravel()[other].all(axis=1)]
    assert not np.array_equal(twin.pixel_triples(other), want)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_twin_depth_edge_is_a_rank_filter_difference(radius):
    ndimage = pytest.importorskip("scipy.ndimage")
    sc = scenes.box_scene()
    z = twin.map_depth(points=sc["points"], cams=sc["cams"], valid=sc["valid"], near=scenes.NEAR)
    usable = ~np.isnan(z)
    size = (1, 2 * radius + 1, 2 * radius + 1)
    zmax = ndimage.maximum_filter(np.where(usable, z, -np.inf), size=size, mode="constant", cval=-np.inf)
    zmin = ndimage.minimum_filter(np.where(usable, z, np.inf), size=size, mode="constant", cval=np.inf)
    for tol in (0.03, 0.0, INF):
        with np.errstate(all="ignore"):
            want = usable & ((zmax - zmin).astype(F) > F(tol) * z)
        flags = twin.map_edges(z, radius=radius, rel_tol=tol)
        assert np.array_equal((flags & twin.DEPTH_EDGE) != 0, want)
        assert np.array_equal(flags == twin.UNUSABLE, ~usable) and not (flags & (twin.NORMAL_EDGE | twin.NO_NORMAL)).any()


def test_twin_normals_of_a_tilted_plane_and_a_sphere_face_the_camera():
    rng = np.random.default_rng(2)
    # a plane n . X = d through a random camera
    n = np.array([0.3, -0.2, -1.0])
    n /= np.linalg.norm(n)
    R, t = scenes.rotation(rng.normal(size=3), 25.0), rng.normal(size=3)
    v, u = np.mgrid[0:9, 0:11].astype(np.float64)
    rays = np.stack([(u - 5) / 20, (v - 4) / 20, np.ones_like(u)], -1)
    cam_pts = rays * (3.0 / (rays @ -n))[..., None]                           # camera coordinates on the plane n . X = -3
    world = (cam_pts - t) @ R                                                 # X_w = R^T (X_c - t)
    cams = scenes.pack_cam(R, t, 20, 20, 5, 4)[None]
    z = twin.map_depth(points=world[None].astype(F), cams=cams)
    got = twin.map_normals(world[None].astype(F), z, rel_tol=INF)[0]
    want = n @ R                                                              # the plane's normal in world coordinates, towards the camera
    assert np.abs(got - want).max() <= 1e-6
    centre = -R.T @ t
    assert ((centre - world) @ want > 0).all()
    # a sphere patch, large against the pixel pitch (mapgeom_scenes.sphere_patch says why the stencil is exact to far below 1e-6 there)
    pts, normals, cams, centre = scenes.sphere_patch()
    assert np.abs(normals[0, 0, 0] - normals[0, -1, -1]).max() > 2e-4        # the normal turns across the patch by far more than the bound
    z = twin.map_depth(points=pts.astype(F), cams=cams)
    assert np.abs(z[0] - 5.0).max() < 0.01
    got = twin.map_normals(pts.astype(F), z, rel_tol=INF).astype(np.float64)
    print("sphere patch: interior %.3g, frame %.3g" % (np.abs(got - normals)[0, 1:-1, 1:-1].max(), np.abs(got - normals).max()))
    assert np.abs(got - normals)[0, 1:-1, 1:-1].max() <= 1e-6                 # central differences; the frame's one-sided ones are first order
    assert np.abs(got - normals).max() <= 1e-4
    assert ((got * (centre - pts)).sum(-1) > 0).all()


def test_twin_boundary_cases_in_powers_of_two():
    z = np.array([[[2.0, 2.5]]], F)
    below = float(np.nextafter(F(0.25), F(0)))
    assert twin.map_edges(z, radius=1, rel_tol=0.25).tolist() == [[[0, 0]]]                    # 0.5 > 0.25 * 2 fails: the test is strict
    assert twin.map_edges(z, radius=1, rel_tol=below).tolist() == [[[twin.DEPTH_EDGE, 0]]]     # 0.5 > 0.24999999 * 2; 0.5 > 0.625 still fails
    # the neighbour test |z_q - z_p| <= rel_tol * z_p is inclusive: at equality the neighbour is used, one ulp below it is not
    pts = np.zeros((1, 3, 3, 3), F)
    pts[0, ..., 0], pts[0, ..., 1] = np.mgrid[0:3, 0:3][1], np.mgrid[0:3, 0:3][0]
    zz = np.full((1, 3, 3), 2.0, F)
    zz[0, 1, 2] = 2.5
    pts[0, ..., 2] = zz[0]
    n_incl, one_h, _ = twin.map_normals(pts, zz, rel_tol=0.25, return_one_sided=True)
    n_excl, one_h2, _ = twin.map_normals(pts, zz, rel_tol=below, return_one_sided=True)
    assert not one_h[0, 1, 1] and one_h2[0, 1, 1]                              # centre pixel: central difference at equality, one-sided below it
    assert not np.array_equal(n_incl[0, 1, 1], n_excl[0, 1, 1]) and np.array_equal(n_excl[0, 1, 1], [0, 0, -1])
    # the tear test (max - min) > rel_tol * min is strict: at equality the face is kept
    pix, emitted = twin.quad_faces(zz, pts, rel_tol=0.25)
    assert emitted[0, 0, 1].all() and emitted[0, 1, 1].all()
    pix, emitted = twin.quad_faces(zz, pts, rel_tol=below)
    # pixel (1, 2) is d of the quad above it (face 1 only) and b of its own row's quad (both faces)
    assert emitted[0, 0, 1].tolist() == [True, False] and emitted[0, 1, 1].tolist() == [False, False] and emitted[0, :, 0].all()
    assert twin.quad_faces(zz, pts, rel_tol=INF)[1].all()


def test_twin_stencils_never_leave_their_view():
    for H, W in ((2, 2), (1, 5), (5, 1), (2, 3)):
        pts, cams = scenes.stacked_views(H, W)
        z = twin.map_depth(points=pts, cams=cams)
        normals = twin.map_normals(pts, z, rel_tol=0.03)
        flags = twin.map_edges(z, normals, radius=3, rel_tol=0.03, min_cos=twin.min_cos(30))
        mesh = twin.triangulate(z, pts, rel_tol=0.03)
        for s in range(3):
            zs = twin.map_depth(points=pts[s:s + 1], cams=cams[s:s + 1])
            ns = twin.map_normals(pts[s:s + 1], zs, rel_tol=0.03)
            assert np.array_equal(normals[s:s + 1], ns)
            assert np.array_equal(flags[s:s + 1], twin.map_edges(zs, ns, radius=3, rel_tol=0.03, min_cos=twin.min_cos(30)))
        assert not (flags & twin.DEPTH_EDGE).any()                            # 1 % of relief inside a view, factors of ten between views
        nfaces = 3 * 2 * (H - 1) * (W - 1)
        assert len(mesh["faces"]) == nfaces and len(mesh["vertices"]) == (3 * H * W if nfaces else 0)


# ---------------------------------------------------------------------------------------------
# the scenes of the GPU test are not trivial
# ---------------------------------------------------------------------------------------------
def test_the_gpu_scene_exercises_every_branch():
    sc = scenes.box_scene()
    pts, cams, valid, keep = sc["points"], sc["cams"], sc["valid"], sc["keep"]
    assert pts.shape == (3, 37, 53, 3) and -(-pts[..., 0].size // 256) == 23
    z = twin.map_depth(points=pts, cams=cams, valid=valid, near=scenes.NEAR)
    usable = ~np.isnan(z)
    assert usable[:2].mean() > 0.8 and not usable[2].any()                    # the third view lies behind its camera
    assert np.array_equal(np.nan_to_num(z), np.nan_to_num(twin.map_depth(depth=sc["depth"], valid=valid, near=scenes.NEAR)))
    assert (~np.isfinite(pts)).any(axis=-1).sum() >= 6
    normals, one_h, one_v = twin.map_normals(pts, z, rel_tol=0.03, return_one_sided=True)
    assert one_h.any() and one_v.any()
    for radius in (1, 2, 3):
        flags = twin.map_edges(z, normals, radius=radius, rel_tol=0.03, min_cos=twin.min_cos(30.0))
        share = ((flags & twin.DEPTH_EDGE) != 0).sum() / usable.sum()
        assert 0.05 <= share <= 0.5, (radius, share)
        assert (flags & twin.NORMAL_EDGE).any() and (flags & twin.NO_NORMAL).any() and (flags == twin.UNUSABLE).any()
        assert (flags == 0).sum() > 0.3 * usable.sum()
    assert (normals[0, 8, 41] == 0).all() and usable[0, 8, 41]
    lens = np.linalg.norm(normals.astype(np.float64), axis=-1)
    assert (np.abs(lens[lens > 0] - 1) < 1e-6).all() and (lens > 0).sum() > 0.9 * usable.sum()
    for k in (None, keep):
        pix, emitted, all_corners, is_torn = twin.quad_faces(z, pts, k, 0.03, return_causes=True)
        assert emitted.any() and (~all_corners).any() and (all_corners & is_torn).any()
        assert (emitted[..., 0] != emitted[..., 1]).any()                     # a quad that emits exactly one face
        mesh = twin.triangulate(z, pts, k, normals, sc["colors"], 0.03)
        cor = twin.corners(z, pts, k).reshape(-1)
        assert cor.sum() > len(mesh["pixel_index"]) > 0 and cor[mesh["pixel_index"]].all()          # an unreferenced corner
        assert cor[22 * 53 + 12] and 22 * 53 + 12 not in mesh["pixel_index"]
    without = twin.quad_faces(z, pts, None, 0.03)[1]
    with_keep = twin.quad_faces(z, pts, keep, 0.03)[1]
    assert (without & ~with_keep).any() and not (with_keep & ~without).any()  # faces dropped by keep alone
    assert twin.quad_faces(z, pts, None, INF)[1].sum() > without.sum()        # faces dropped by the tear test alone
    # the scan's second level: more than 256 workgroups, both counts far from empty
    pts2, keep2 = scenes.random_keep_scene()
    assert -(-keep2.size // 256) > 256 and 0.65 < keep2.mean() < 0.75
    mesh = twin.triangulate(twin.map_depth(depth=pts2[..., 2]), pts2, keep2, rel_tol=0.03)
    assert len(mesh["faces"]) > 20000 and len(mesh["vertices"]) > 20000


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def _layout(struct, cname, extra):
    return abi_layout.check({cname: struct}, extra)[0]


def test_ctypes_struct_layouts_and_enums_match_c_mapgeom():
    bits = ["OVG_MAP_UNUSABLE", "OVG_MAP_DEPTH_EDGE", "OVG_MAP_NORMAL_EDGE", "OVG_MAP_NO_NORMAL"]
    assert _layout(L.MapDepthParams, "ovg_map_depth_params", bits) == [L.MAP_UNUSABLE, L.MAP_DEPTH_EDGE, L.MAP_NORMAL_EDGE, L.MAP_NO_NORMAL] == \
        [twin.UNUSABLE, twin.DEPTH_EDGE, twin.NORMAL_EDGE, twin.NO_NORMAL] == [1, 2, 4, 8]
    assert _layout(L.MapNormalsParams, "ovg_map_normals_params", ["OVG_ABI_VERSION", "OVG_TSDF_GREY"]) == [L.ABI_VERSION, twin.GREY] == [13, L.TSDF_GREY]
    tiles = ["OVG_MAP_TILE_DEFAULT", "OVG_MAP_TILE_256x1", "OVG_MAP_TILE_16x16", "OVG_MAP_TILE_32x8", "OVG_MAP_TILE_64x4", "OVG_MAP_MAX_RADIUS"]
    assert _layout(L.MapEdgesParams, "ovg_map_edges_params", tiles) == \
        [L.MAP_TILE_DEFAULT, L.MAP_TILE_256x1, L.MAP_TILE_16x16, L.MAP_TILE_32x8, L.MAP_TILE_64x4, L.MAP_MAX_RADIUS] == [0, 1, 2, 3, 4, 3]
    assert _layout(L.MapTriangulateParams, "ovg_map_triangulate_params", ["OVG_MAP_COUNT", "OVG_MAP_SCATTER", "OVG_MAP_BLOCK"]) == \
        [L.MAP_COUNT, L.MAP_SCATTER, L.MAP_BLOCK] == [1, 2, 256]
    text = open(HEADER).read()
    for entry in ("ovg_map_depth", "ovg_map_normals", "ovg_map_edges", "ovg_map_triangulate"):
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (entry, entry), text)
        assert entry in L.SYMBOLS and text.index(entry) < text.index("#define OVG_ABI_VERSION")      # named in the ABI-13 list
    q = "ovg_map_triangulate_workspace_bytes"
    assert re.search(r"int64_t\s+%s\s*\(\s*int32_t\s+S\s*,\s*int32_t\s+H\s*,\s*int32_t\s+W\s*\)\s*;" % q, text) and q in L.SYMBOLS
    assert text.index(q) < text.index("#define OVG_ABI_VERSION") and L.load().ovg_abi_version() == 13
    build_py = open(os.path.join(common.ROOT, "omnivggt-official_amd", "build.py")).read()
    from omnivggt_official_amd import build as B
    assert "ovg_mapgeom.hip" in B.SOURCES and B.EXTRA_FLAGS["ovg_mapgeom.hip"] == ["-ffp-contract=off"] and "ovg_mapgeom.hip" in build_py


def test_argument_validation_of_the_four_entries_without_gpu():
    lib = L.load()
    wsb = lib.ovg_map_triangulate_workspace_bytes
    r256 = lambda b: (b + 255) // 256 * 256
    for S, H, W in ((1, 1, 1), (3, 37, 53), (2, 190, 180), (64, 518, 518)):
        n = S * H * W
        assert wsb(S, H, W) == r256(4 * n) + r256(n) + 2 * r256(8 * (-(-n // 256)))
    assert [wsb(*a) for a in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 11, 1 << 10, 1 << 10), (1, 1 << 16, 1 << 15), (8192, 512, 512),
                              (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))] == [-1] * 8
    assert wsb(8191, 512, 512) > 0 and ops.map_triangulate_workspace_bytes(3, 37, 53) == wsb(3, 37, 53)
    for bad in ((0, 1, 1), (8192, 512, 512), (1, 1, 1 << 40)):
        with pytest.raises(L.OvgError):
            ops.map_triangulate_workspace_bytes(*bad)
    big = 1 << 40                                                             # fake, never dereferenced: every call below fails its checks
    nan = float("nan")
    shape = (dict(S=0), dict(H=0), dict(W=-1), dict(S=8192, H=512, W=512), dict(S=1, H=1 << 16, W=1 << 15))

    def depth(**kw):
        p = L.MapDepthParams(points=big, cams=big, depth=None, valid=big + 1, S=3, H=37, W=53, near=1e-3, z=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_map_depth(ctypes.byref(p), None)

    assert lib.ovg_map_depth(None, None) == -1
    for bad in shape + (dict(points=None), dict(depth=big), dict(cams=None), dict(z=None), dict(near=0.0), dict(near=-1.0), dict(near=nan),
                        dict(near=INF), dict(points=big + 2), dict(cams=big + 1), dict(z=big + 2), dict(points=None, depth=big + 2)):
        assert depth(**bad) == -1, bad

    def normals(**kw):
        p = L.MapNormalsParams(points=big, z=big, S=3, H=37, W=53, rel_tol=0.03, normals=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_map_normals(ctypes.byref(p), None)

    assert lib.ovg_map_normals(None, None) == -1
    for bad in shape + (dict(points=None), dict(z=None), dict(normals=None), dict(rel_tol=-0.5), dict(rel_tol=nan), dict(rel_tol=-INF),
                        dict(points=big + 2), dict(z=big + 1), dict(normals=big + 3)):
        assert normals(**bad) == -1, bad

    def edges(**kw):
        p = L.MapEdgesParams(z=big, normals=big, S=3, H=37, W=53, radius=1, rel_tol=0.03, min_cos=0.5, tile=0, pad=0, flags=big + 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_map_edges(ctypes.byref(p), None)

    assert lib.ovg_map_edges(None, None) == -1
    for bad in shape + (dict(z=None), dict(flags=None), dict(radius=0), dict(radius=4), dict(radius=-1), dict(rel_tol=-1.0), dict(rel_tol=nan),
                        dict(min_cos=nan), dict(tile=5), dict(tile=-1), dict(z=big + 2), dict(normals=big + 2)):
        assert edges(**bad) == -1, bad

    def tri(**kw):
        p = L.MapTriangulateParams(z=big, points=big, keep=big + 1, normals=big, colors=big + 1, S=3, H=37, W=53, rel_tol=0.03,
                                   stage=L.MAP_COUNT | L.MAP_SCATTER, pad=0, vertex_capacity=10, face_capacity=10, out_vertices=big,
                                   out_normals=big, out_colors=big + 1, out_pixel_index=big, out_faces=big, out_count=big, ws=big,
                                   ws_bytes=wsb(3, 37, 53))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_map_triangulate(ctypes.byref(p), None)

    assert lib.ovg_map_triangulate(None, None) == -1
    for bad in shape + (dict(z=None), dict(points=None), dict(ws=None), dict(out_count=None), dict(rel_tol=-1.0), dict(rel_tol=nan), dict(stage=0),
                        dict(stage=4), dict(stage=-1), dict(vertex_capacity=-1), dict(face_capacity=-1), dict(out_vertices=None),
                        dict(out_normals=None), dict(out_colors=None), dict(out_pixel_index=None), dict(out_faces=None), dict(ws=big + 8),
                        dict(ws_bytes=wsb(3, 37, 53) - 1), dict(ws_bytes=0), dict(ws_bytes=-5), dict(z=big + 2), dict(points=big + 1),
                        dict(normals=big + 2), dict(out_count=big + 4), dict(out_pixel_index=big + 4), dict(out_faces=big + 2),
                        dict(out_vertices=big + 2), dict(out_normals=big + 1)):
        assert tri(**bad) == -1, bad


# ---------------------------------------------------------------------------------------------
# the Python layers
# ---------------------------------------------------------------------------------------------
def test_ops_wrappers_check_their_arguments_before_any_device_call():
    pts, z = torch.ones(2, 4, 5, 3), torch.ones(2, 4, 5)
    cams, u8 = torch.ones(2, 16), torch.ones(2, 4, 5, dtype=torch.uint8)
    for kw in (dict(), dict(points=pts, cams=cams, depth=z), dict(points=pts), dict(points=pts.double(), cams=cams), dict(points=pts[..., :2], cams=cams),
               dict(points=pts, cams=cams[:1]), dict(depth=z[0]), dict(depth=torch.ones(2, 4, 10)[..., ::2]), dict(depth=z, valid=u8.bool()),
               dict(depth=z, valid=u8[:1]), dict(depth=z, near=0.0), dict(depth=z, near=float("nan")), dict(depth=z, out=torch.ones(2, 4, 4)),
               dict(depth=torch.ones(0, 4, 5))):
        with pytest.raises(L.OvgError):
            ops.map_depth(**kw)
    for kw in (dict(points=pts.double()), dict(z=z[:1]), dict(z=z.double()), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(rel_tol="1"),
               dict(out=torch.ones(2, 4, 5))):
        with pytest.raises(L.OvgError):
            ops.map_normals(**dict(dict(points=pts, z=z), **kw))
    for kw in (dict(z=z.double()), dict(normals=pts.double()), dict(normals=pts[:1]), dict(radius=0), dict(radius=4), dict(radius=1.0), dict(radius=True),
               dict(rel_tol=-1.0), dict(min_cos=float("nan")), dict(tile=5), dict(tile=-1), dict(out=torch.ones(2, 4, 5))):
        with pytest.raises(L.OvgError):
            ops.map_edges(**dict(dict(z=z), **kw))
    ws, count = torch.zeros(4096, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    ok = dict(stage=L.MAP_COUNT, z=z, points=pts, ws=ws, out_count=count)
    for kw in (dict(stage=0), dict(stage=4), dict(z=z.double()), dict(points=pts[:1]), dict(keep=u8.bool()), dict(normals=pts[..., :2]),
               dict(colors=pts), dict(rel_tol=-1.0), dict(ws=torch.zeros(4096)), dict(out_count=count[:1]), dict(out_count=count.int()),
               dict(stage=L.MAP_SCATTER, vertex_capacity=-1), dict(stage=L.MAP_SCATTER, vertex_capacity=4), dict(stage=L.MAP_SCATTER, face_capacity=2),
               dict(stage=L.MAP_SCATTER, face_capacity=2, faces=torch.zeros(1, 3, dtype=torch.int32))):
        with pytest.raises(L.OvgError):
            ops.map_triangulate(**dict(ok, **kw))
    for call in (lambda: ops.map_depth(depth=z), lambda: ops.map_depth(points=pts, cams=cams, valid=u8), lambda: ops.map_normals(pts, z),
                 lambda: ops.map_edges(z, pts, radius=3, min_cos=0.5), lambda: ops.map_triangulate(**ok)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            call()


def test_public_entries_check_their_arguments_and_refuse_cpu_tensors():
    pts, z = torch.ones(2, 4, 5, 3), torch.ones(2, 4, 5)
    ext = torch.eye(4)[None, :3].repeat(2, 1, 1)
    keep = torch.ones(2, 4, 5, dtype=torch.bool)
    for kw in (dict(), dict(points=pts), dict(points=pts, depth=z, extrinsic=ext), dict(points=pts[0], extrinsic=ext), dict(points=pts, extrinsic=ext[:1]),
               dict(depth=z[0]), dict(depth=z.long()), dict(depth=z, valid=z), dict(depth=z, valid=keep[:1]), dict(depth=z, near=0.0),
               dict(depth=z, near=float("inf")), dict(depth=z, near="x")):
        with pytest.raises(ValueError):
            postprocess.camera_depth_maps(**kw)
    for kw in (dict(points=pts[0]), dict(z=z[:1]), dict(z=z.long()), dict(rel_tol=-0.1), dict(rel_tol=float("nan")), dict(rel_tol=True)):
        with pytest.raises(ValueError):
            postprocess.map_normals(**dict(dict(points=pts, z=z), **kw))
    for kw in (dict(z=z[0]), dict(normals=pts[:1]), dict(radius=0), dict(radius=4), dict(radius=1.5), dict(rel_tol=-1.0), dict(max_angle_deg=30.0),
               dict(normals=pts, max_angle_deg=181.0), dict(normals=pts, max_angle_deg=-1.0), dict(normals=pts, max_angle_deg="30")):
        with pytest.raises(ValueError):
            postprocess.map_edges(**dict(dict(z=z), **kw))
    for kw in (dict(points=pts[0]), dict(z=z[:1]), dict(keep=z), dict(keep=keep[:1]), dict(normals=pts[:1]), dict(images=torch.ones(2, 4, 5, 3)),
               dict(rel_tol=-1.0), dict(extrinsic=ext[:1])):
        with pytest.raises(ValueError):
            postprocess.triangulate_maps(**dict(dict(points=pts, z=z), **kw))
    with pytest.raises(ValueError):
        postprocess.edge_mask(z)
    for call in (lambda: postprocess.camera_depth_maps(depth=z), lambda: postprocess.camera_depth_maps(points=pts, extrinsic=ext, valid=keep),
                 lambda: postprocess.map_normals(pts, z, rel_tol=None), lambda: postprocess.map_edges(z, pts, radius=2, max_angle_deg=30),
                 lambda: postprocess.triangulate_maps(pts, z, keep=keep, images=torch.ones(2, 3, 4, 5), normals=pts, extrinsic=ext)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            call()
    pred = {"images": torch.ones(1, 2, 3, 4, 5), "world_points": pts[None], "world_points_conf": z[None], "extrinsic": ext[None]}
    for kw in (dict(conf_thres=101.0), dict(conf_thres="50"), dict(edge_radius=4), dict(edge_radius=-1), dict(rel_tol=-1.0), dict(batch_index=1),
               dict(keep_mask=keep[:1]), dict(keep_mask=z)):
        with pytest.raises(ValueError):
            postprocess.predictions_to_mesh(pred, **kw)
    for fn in (postprocess.predictions_to_mesh, postprocess.prediction_normals, postprocess.prediction_edges):
        with pytest.raises(ValueError):
            fn([])
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            fn(pred)
    res = postprocess.MapEdges(torch.tensor([[[0, 1, 2, 4, 8, 6, 10]]], dtype=torch.uint8))
    assert postprocess.edge_mask(res).tolist() == [[[True, False, False, True, True, False, False]]]
    assert postprocess.edge_mask(res, normal=True).tolist() == [[[True, False, False, False, True, False, False]]]
    assert postprocess.edge_mask(res, depth=False).tolist() == [[[True, False, True, True, True, True, True]]]
    assert issubclass(postprocess.MapMesh, postprocess.Mesh)
