"""ovg_render_mesh / postprocess.render_mesh on the device against tests/raster_twin.py: images, depth maps and face-index maps byte
for byte -- the analytic sphere and torus meshes of tsdf_twin from 1 / 3 / 14 cameras with every shading, cull mode, optional input
and both drawing paths; frame-filling, frame-crossing, interpenetrating and tiny triangles at 70 x 50; spoiled vertices, faces and
normals; the edge sizes; 3 views of 518 x 518; the Python layer on a mesh fused on the device. Outputs and workspace sit in exact-size
guarded buffers and every case runs twice."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_guards as kg
import raster_twin as twin
import tsdf_twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
BG = (12, 200, 77)
E_ARG = -1
HUGE = 1 << 30                          # a coop_threshold no box reaches: every face is walked by its own lane
_MESHES, _ZBUF = {}, {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(kind, n):
    """(vertices, normals, faces, random colours) of an analytic tsdf_twin volume, extracted once."""
    if (kind, n) not in _MESHES:
        tsdf, weight, origin, voxel, _ = tsdf_twin.sdf_volume(kind, n)
        vert, nrm, _, faces = tsdf_twin.extract(tsdf, weight, None, origin, voxel)
        col = np.random.default_rng(n).integers(0, 256, (len(vert), 3)).astype(np.uint8)
        _MESHES[(kind, n)] = (vert, nrm, faces, col)
    return _MESHES[(kind, n)]


def _zbuffer(tag, vert, faces, cams, H, W, cull, near):
    """The twin's key buffer and its statistics, shared by the cases that differ only in shading, attributes or coop_threshold."""
    key = (tag, cams.tobytes(), H, W, cull, near)
    if key not in _ZBUF:
        stats = {}
        _ZBUF[key] = (twin.zbuffer(vert, faces, cams, H, W, cull, near, stats), stats)
    return _ZBUF[key]


def _device(vert, faces, nrm, col, cams, H, W, shading, cull, coop, near, bg, name):
    """Two runs of the raw entry into guarded exact-size buffers (outputs and workspace). -> (rgb, depth, index) host arrays."""
    V = len(cams)
    need = ops.render_mesh_workspace_bytes(V, H, W)
    assert need == (8 * V * H * W + 15) // 16 * 16
    args = [None if a is None else _dev(a) for a in (vert, faces, nrm, col)]
    runs = []
    for _ in range(2):
        ws, cws = kg.guarded((1, need), torch.uint8, "cuda")
        rgb, crgb = kg.guarded((V, H, W, 3), torch.uint8, "cuda")
        dep, cdep = kg.guarded((V, H, W), torch.float32, "cuda")
        idx, cidx = kg.guarded((V, H, W), torch.int64, "cuda")
        out = ops.render_mesh(args[0], args[1], _dev(cams), H, W, normals=args[2], colors=args[3], shading=shading, cull=cull, near=near,
                              background=bg, coop_threshold=coop, ws=ws.reshape(-1), out=(rgb, dep, idx))
        assert out[0] is rgb and out[1] is dep and out[2] is idx
        torch.cuda.synchronize()
        for c, what in ((cws, "workspace"), (crgb, "rgb"), (cdep, "depth"), (cidx, "index")):
            c("%s %s" % (name, what))
        runs.append((rgb.cpu().numpy(), dep.cpu().numpy(), idx.cpu().numpy()))
    for a, b, what in zip(runs[0], runs[1], ("rgb", "depth", "index")):
        assert a.tobytes() == b.tobytes(), (name, what, "two runs differ")
    return runs[0]


def _check(tag, vert, faces, nrm, col, cams, H, W, shading=twin.SHADE_HEADLIGHT, cull=twin.CULL_NONE, coop=0, near=1e-3, bg=BG):
    """Device against twin, byte for byte. -> (twin rgb, depth, index, stats)."""
    name = (tag, H, W, len(cams), "shading %d cull %d coop %d" % (shading, cull, coop), nrm is not None, col is not None)
    zbuf, stats = _zbuffer(tag, vert, faces, cams, H, W, cull, near)
    want = twin.resolve(zbuf, vert, faces, nrm, col, cams, H, W, shading, near, bg)
    got = _device(vert, faces, nrm, col, cams, H, W, shading, cull, coop, near, bg, str(name))
    for g, w, what in zip(got, want, ("rgb", "depth", "index")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%r %s: %d values differ, first at %s: got %s want %s"
                                 % (name, what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
    return want + (stats,)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the twin meshes
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n", [("sphere", 17), ("torus", 17), ("sphere", 33), ("torus", 33)])
def test_twin_meshes_match_bit_exactly(kind, n):
    L.require_gpu()
    vert, nrm, faces, col = _mesh(kind, n)
    all_cams = tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 1.2)
    # the sphere of radius 0.6 at distance 1.2 under 60 degrees covers >= 60 % of the frame (tests/test_raster_host.py); the torus seen
    # edge-on shows at least its 1.1 x 0.5 core rectangle of the 1.39 x 1.39 the frame spans at the centre's depth: >= 25 %
    floor = 0.6 if kind == "sphere" else 0.25
    for views, (H, W) in (([0], (48, 48)), ([1, 6, 13], (37, 53)), (list(range(14)), (48, 48)), (list(range(14)), (37, 53))):
        cams = twin.pack_cams(all_cams[views], tsdf_twin.pinhole(H, W, 60.0))
        tag = (kind, n)
        many = len(views) == 14
        # every value of one argument against the defaults of the others, then mixed rows
        rows = [dict(), dict(shading=twin.SHADE_COLOR), dict(shading=twin.SHADE_NORMAL), dict(nrm=None), dict(col=None),
                dict(nrm=None, col=None, shading=twin.SHADE_NORMAL), dict(cull=twin.CULL_BACK), dict(cull=twin.CULL_FRONT),
                dict(coop=1), dict(coop=HUGE), dict(coop=1, cull=twin.CULL_FRONT, nrm=None, shading=twin.SHADE_COLOR),
                dict(coop=HUGE, cull=twin.CULL_BACK, col=None)]
        for row in (rows if not many or (H, W) == (37, 53) else rows[:1] + rows[8:10]):
            kw = dict(nrm=nrm, col=col)
            kw.update(row)
            rgb, depth, index, stats = _check(tag, vert, faces, kw.pop("nrm"), kw.pop("col"), cams, H, W, **kw)
            for v in range(len(views)):
                hit, covered = int((index[v] >= 0).sum()), stats["covered"][v]
                assert hit >= floor * H * W, (kind, n, v, hit)
                # a closed mesh: both sides of it cover every hit pixel; with one side culled only shared edges are covered twice
                assert covered >= 1.5 * hit if row.get("cull", 0) == twin.CULL_NONE else covered > hit, (kind, n, v, hit, covered)
        print("%s %d at %d x %d, %d views: largest box %d pixels" % (kind, n, H, W, len(views), stats["boxes"]))
        assert stats["boxes"] > 1                                           # coop_threshold = 1 sends faces down the cooperative path


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. large and edge shapes at 70 x 50
# ---------------------------------------------------------------------------------------------------------------------------------

FH, FW = 50, 70
FRAME_K = np.array([[32.0, 0.0, 32.0], [0.0, 32.0, 24.0], [0.0, 0.0, 1.0]])


def _at(u, w, z):
    """The camera-space point that the identity camera with FRAME_K sees at pixel (u, w) and depth z (exact for u, w in 1/8 pixel and
    z a power of two)."""
    return [(u - 32.0) / 32.0 * z, (w - 24.0) / 32.0 * z, z]


def _shapes_mesh(coop):
    """-> (vertices, faces, colours). In face order: two triangles over the whole frame (tilted in depth), triangles over each frame
    edge and corner, one outside, two interpenetrating ones, boxes of exactly coop and coop + 1 pixels, then a fan of 260 small
    random ones."""
    rng = np.random.default_rng(5)
    tris = []
    a, b, c, d = _at(-6, -6, 4.0), _at(76, -6, 6.0), _at(76, 56, 8.0), _at(-6, 56, 5.0)
    tris += [(a, c, b), (a, d, c)]
    for u, w in ((0, 25), (69, 25), (35, 0), (35, 49), (0, 0), (69, 0), (0, 49), (69, 49)):
        tris.append((_at(u - 4.5, w - 3.25, 2.0), _at(u + 1.25, w + 5.5, 2.5), _at(u + 5.75, w - 2.5, 3.0)))
    tris.append((_at(80, 10, 2.0), _at(90, 30, 2.0), _at(100, 12, 2.0)))
    tris += [(_at(10, 5, 1.5), _at(20, 45, 3.5), _at(60, 20, 3.5)), (_at(10, 40, 3.5), _at(60, 30, 1.5), _at(25, 5, 3.5))]
    # vertices on pixel centres: the boxes are exact. w x 1 pixels: a sliver half a pixel high on one row
    for n, u0 in ((coop, 2), (coop + 1, 3)):
        bw, bh = (n, 1) if n <= 64 else (13, n // 13)
        assert bw * bh == n
        tris.append((_at(u0, 30, 1.0), _at(u0 + bw - 1, 30, 1.0), _at(u0, 30 + bh - 0.5, 1.0)))
    for _ in range(260):
        u, w, z = rng.uniform(-2, 72), rng.uniform(-2, 52), rng.uniform(1.0, 3.0)
        p = [_at(u + rng.uniform(-2.5, 2.5), w + rng.uniform(-2.5, 2.5), z + rng.uniform(-0.2, 0.2)) for _ in range(3)]
        tris.append(tuple(p))
    vert = np.asarray(tris, F).reshape(-1, 3)
    faces = np.arange(len(vert), dtype=np.int32).reshape(-1, 3)
    col = rng.integers(0, 256, (len(vert), 3)).astype(np.uint8)
    return vert, faces, col


def test_large_and_edge_shapes():
    L.require_gpu()
    E = np.eye(4)[:3][None]
    ext = np.concatenate([E, tsdf_twin.look_at((0.4, -0.3, -0.5), (0.0, 0.1, 3.0))[None]])      # the frame camera and an oblique one
    cams = twin.pack_cams(ext, FRAME_K)
    for coop, settings in ((12, (12, 1, HUGE)), (64, (0, 64, 5))):
        vert, faces, col = _shapes_mesh(coop)
        assert len(faces) >= 257
        # the two boxes round the threshold, as the twin's setup sees them in the frame camera
        ok, X, Y, _ = twin.project_vertices(vert, cams[0], 1e-3)
        drawn, _, x0, x1, y0, y1 = twin.face_setup(X[faces[13:15]], Y[faces[13:15]], ok[faces[13:15]], 0, FH, FW)
        assert drawn.all() and ((x1 - x0 + 1) * (y1 - y0 + 1)).tolist() == [coop, coop + 1]
        for nf in (1, 63, 64, 65, 257):
            for k, c in enumerate(settings):
                if nf not in (65, 257) and k:
                    continue
                _, depth, index, stats = _check(("shapes", coop, nf), vert, faces[:nf], None, col, cams, FH, FW, coop=c)
                hit, covered = int((index[0] >= 0).sum()), stats["covered"][0]
                print("F = %d, coop_threshold %d: %d pixels hit, %d covered" % (nf, c, hit, covered))
                assert stats["boxes"] == FH * FW                            # a box of the whole frame
                if nf == 1:
                    assert 0.4 * FH * FW <= hit < 0.6 * FH * FW             # one half of the frame
                else:
                    # the two big triangles fill the frame camera's picture; everything else lies in front of them
                    assert hit == FH * FW and covered > hit and (nf < 257 or covered >= 1.25 * hit)
                assert (index[1] >= 0).any()
        for cull in (twin.CULL_FRONT, twin.CULL_BACK):
            _, _, culled, _ = _check(("shapes", coop, "culled"), vert, faces, None, col, cams, FH, FW, cull=cull, coop=settings[0])
            assert (culled[0] >= 0).any()
        shown = set(np.unique(index[0]).tolist())                           # of the last case above: all faces, both sides
        assert 10 not in shown and {11, 12} <= shown                        # the one outside the frame; both interpenetrating ones show


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. spoiled input
# ---------------------------------------------------------------------------------------------------------------------------------

def test_spoiled_vertices_faces_and_normals():
    L.require_gpu()
    near = 0.5
    rng = np.random.default_rng(9)
    good = [_at(5, 5, 2.0), _at(60, 8, 2.0), _at(30, 44, 4.0), _at(12, 40, 2.0)]
    bad = [[np.nan, 0.0, 2.0], [0.0, np.inf, 2.0], [0.0, 0.0, -np.inf],
           [1e30, 1e30, 1e30], [3e38, -3e38, 3e38],                         # finite: usable in the frame camera, at pixel (64, 56) / (64, -8)
           _at(30, 20, -2.0),                                               # behind the camera
           _at(30, 20, 0.25),                                               # in front, nearer than the near plane
           [0.0, 0.0, 0.5],                                                 # exactly on the near plane: zc > near fails
           [1022.0, 0.0, 2.0],                                              # sx = 16384 exactly: the last usable position
           [1022.001, 0.0, 2.0],                                            # sx just beyond the band
           [0.0, -1023.5, 2.0],                                             # sy = -16352: inside
           [0.0, -1026.0, 2.0]]                                             # sy = -16392: beyond
    line = [_at(10, 10, 2.0), _at(20, 20, 2.0), _at(30, 30, 2.0)]           # collinear but distinct: zero area
    vert = np.asarray(good + bad + line, F)
    M = len(vert)
    faces = [[0, 2, 1], [0, 3, 2]]
    faces += [[0, 1, 4 + k] for k in range(len(bad))] + [[4 + k, 2, 3] for k in range(len(bad))]
    faces += [[0, 0, 1], [1, 2, 2], [3, 3, 3], [0, 2, 1], [0, 2, 1], [0, 3, 2]]      # repeated vertices; exact duplicates of faces 0 and 1
    faces += [[-1, 1, 2], [0, M, 2], [0, 1, M + 5], [-7, -1, M], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1]]
    faces += [[M - 3, M - 2, M - 1]]
    faces = np.asarray(faces, np.int64).astype(np.int32)
    nrm = rng.standard_normal((len(vert), 3)).astype(F)
    nrm[0] = 0.0
    nrm[1] = np.nan
    nrm[3] = [np.inf, 0.0, 0.0]
    col = rng.integers(0, 256, (len(vert), 3)).astype(np.uint8)
    ext = np.stack([np.eye(4)[:3], tsdf_twin.look_at((0.5, 0.2, -1.0), (0.0, 0.0, 3.0)), tsdf_twin.look_at((0.0, 0.0, 6.0), (0.0, 0.0, 0.0))])
    cams = twin.pack_cams(ext, FRAME_K)
    ok, _, _, _ = twin.project_vertices(vert, cams[0], near)
    assert ok[:4].all() and ok[4:4 + len(bad)].tolist() == [False] * 3 + [True, True] + [False] * 3 + [True, False, True, False]
    for shading in (twin.SHADE_HEADLIGHT, twin.SHADE_COLOR, twin.SHADE_NORMAL):
        for coop in (0, 1, HUGE):
            for n in (nrm, None):
                rgb, _, index, stats = _check("spoiled", vert, faces, n, col, cams, FH, FW, shading=shading, coop=coop, near=near)
    shown = set(np.unique(index[0]).tolist())
    print("faces shown by the frame camera:", sorted(shown))
    # the good quad, the sliver out to sx = 16384 and the one up to sy = -16352; never a face with an unusable vertex, a bad index or
    # no area
    usable = (3, 4, 8, 10)
    assert {0, 1, 2 + 8, 2 + 10} <= shown and shown <= {-1, 0, 1} | {2 + k for k in usable} | {14 + k for k in usable}
    quad = (index[0] == 0) | (index[0] == 1)
    assert quad.sum() >= 100 and stats["covered"][0] >= 2 * int(quad.sum())      # the duplicates lose on the index alone
    # zero and non-finite normals under the normal map: 128 where the interpolated length is bad
    rgb, _, index, _ = _check("spoiled", vert, faces, nrm, col, cams, FH, FW, shading=twin.SHADE_NORMAL, near=near)
    # face 0 mixes in the NaN normal of vertex 1 and face 1 the infinite one of vertex 3 (0 x inf is NaN as well): no length, 128
    assert (rgb[0][quad] == 128).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. sizes
# ---------------------------------------------------------------------------------------------------------------------------------

def test_edge_sizes_and_empty_meshes():
    L.require_gpu()
    vert, nrm, faces, col = _mesh("sphere", 17)
    ext = tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 1.2)[[0, 9]]
    for H, W in ((1, 1), (1, 53), (37, 1), (3, 5)):
        K = tsdf_twin.pinhole(max(H, W, 8), max(H, W, 8), 60.0)
        K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
        cams = twin.pack_cams(ext, K)
        for coop in (0, 1):
            _, _, index, _ = _check(("sizes", H, W), vert, faces, nrm, col, cams, H, W, coop=coop)
            assert (index >= 0).mean() > 0.9                                # the sphere fills these narrow frames but for a limb pixel
    cams = twin.pack_cams(ext, tsdf_twin.pinhole(12, 16, 60.0))
    for v, f, n, c, what in ((vert, faces[:0], nrm, col, "F = 0"), (vert[:0], faces[:0], None, None, "M = 0, F = 0"),
                             (vert[:0], faces, nrm[:0], col[:0], "M = 0: every face index is out of range")):
        rgb, depth, index, _ = _check(what, v, f, n, c, cams, 12, 16)
        assert (index == -1).all() and (depth == 0).all() and (rgb == np.asarray(BG, np.uint8)).all(), what


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. 3 views of 518 x 518
# ---------------------------------------------------------------------------------------------------------------------------------

def test_three_views_of_518_squared():
    """The 33^3 torus from distance 2: a lattice cell spans about 16 pixels, so most faces have boxes of a few hundred pixels (the
    cooperative path at the default threshold) and the slivers at the limb stay below it (the lane path): both in one launch."""
    L.require_gpu()
    vert, nrm, faces, col = _mesh("torus", 33)
    H = W = 518
    cams = twin.pack_cams(tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 2.0)[[0, 4, 10]], tsdf_twin.pinhole(H, W, 60.0))
    assert ops.render_mesh_workspace_bytes(3, H, W) == 8 * 3 * H * W
    _, _, index, stats = _check("518", vert, faces, nrm, col, cams, H, W)
    ok, X, Y, _ = twin.project_vertices(vert, cams[0], 1e-3)
    f64 = faces.astype(np.int64)
    drawn, _, x0, x1, y0, y1 = twin.face_setup(X[f64], Y[f64], ok[f64], 0, H, W)
    boxes = ((x1 - x0 + 1) * (y1 - y0 + 1))[drawn]
    print("boxes: %d faces, %d of at most 64 pixels, largest %d" % (len(boxes), int((boxes <= 64).sum()), int(boxes.max())))
    assert (boxes <= 64).sum() >= 20 and (boxes > 64).sum() >= 1000
    for v in range(3):
        hit = int((index[v] >= 0).sum())
        assert hit >= 0.1 * H * W and stats["covered"][v] >= 1.5 * hit


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Python layer
# ---------------------------------------------------------------------------------------------------------------------------------

def _host(t):
    return None if t is None else t.cpu().numpy()


def test_python_layer_on_a_mesh_fused_on_the_device():
    L.require_gpu()
    sc = tsdf_twin.sphere_scene(24, 32)
    vol = postprocess.tsdf_volume([float(v) for v in sc["origin"]], float(sc["voxel"]), sc["dims"], trunc=float(sc["trunc"]))
    rng = np.random.default_rng(2)
    images = rng.integers(0, 256, sc["depth"].shape + (3,)).astype(np.uint8)
    postprocess.tsdf_integrate(vol, _dev(sc["depth"]), sc["ext"], sc["intr"], images=_dev(images))
    mesh = postprocess.tsdf_extract(vol)
    assert len(mesh.faces) > 1000 and mesh.faces.dtype == torch.int32
    centre = postprocess.cloud_centre(postprocess.mesh_to_point_cloud(mesh))
    assert float(centre.abs().max()) < 0.05
    ring = postprocess.orbit_cameras(sc["ext"][4], centre.cpu(), 6, axis=(0.2, 1.0, 0.1))
    H, W = 40, 56
    K = tsdf_twin.pinhole(H, W, 60.0)
    v, f, n, c = _host(mesh.vertices), _host(mesh.faces), _host(mesh.normals), _host(mesh.colors)

    def same(res, want, name):
        for g, w, what in zip((res.rgb, res.depth, res.index), want, ("rgb", "depth", "index")):
            assert g is not None and g.is_cuda and g.cpu().numpy().tobytes() == w.tobytes(), (name, what)

    cams = twin.pack_cams(ring, K)
    nearest = {}
    for shading, code in postprocess.MESH_SHADINGS.items():
        for cull, ccode in postprocess.MESH_CULLS.items():
            for smooth in (True, False):
                res = postprocess.render_mesh(mesh, ring, K, (H, W), shading=shading, cull=cull, smooth=smooth, background=BG, return_index=True)
                want = twin.render(v, f, n if smooth else None, c, cams, H, W, shading=code, cull=ccode, background=BG)
                same(res, want, (shading, cull, smooth))
                hit = want[2] >= 0
                assert hit.mean() > 0.3 and hit.mean() < 1.0
                if cull != "front":
                    # the sphere of radius 0.5 from distance 1: every depth lies between the near pole (0.5) and beyond the limb (0.75)
                    assert want[1][hit].min() > 0.45 and want[1][hit].max() < 1.0
                    nearest[smooth] = want[1]
                else:
                    # back faces alone: never nearer than what both sides show, and farther on most pixels
                    both = hit & (nearest[smooth] > 0)
                    assert (want[1][both] >= nearest[smooth][both]).all() and (want[1][both] > nearest[smooth][both]).mean() > 0.9
    # device-resident float32 cameras, float64 cameras (rounded to f32 first), one (3, 4) extrinsic with a (1, 3, 3) intrinsic
    want = twin.render(v, f, n, c, cams, H, W)
    same(postprocess.render_mesh(mesh, _dev(ring.astype(F)), _dev(K.astype(F)), (H, W), return_index=True), want, "device cameras")
    same(postprocess.render_mesh(mesh, _dev(ring), K, (H, W), return_index=True), want, "float64 device extrinsics")
    same(postprocess.render_mesh(mesh, ring + 1e-10, np.tile(K, (6, 1, 1)) + 1e-10, (H, W), return_index=True), want, "float64 cameras are rounded to f32")
    one = postprocess.render_mesh(mesh, ring[2], K[None], (H, W), return_index=True)
    same(one, tuple(a[2:3] for a in want), "one camera")
    plain = postprocess.render_mesh(mesh, ring, K, (H, W), return_depth=False)
    assert plain.depth is None and plain.index is None and plain.rgb.cpu().numpy().tobytes() == want[0].tobytes()
    only_depth = postprocess.render_mesh(mesh, ring, K, (H, W))
    assert only_depth.index is None and only_depth.depth.cpu().numpy().tobytes() == want[1].tobytes()
    # a mesh without colours or normals: 128 grey, face normals; the default background is white
    bare = postprocess.Mesh(mesh.vertices, mesh.faces, None, None, mesh.transform)
    res = postprocess.render_mesh(bare, ring, K, (H, W), return_index=True)
    same(res, twin.render(v, f, None, None, cams, H, W), "bare mesh")
    assert bool((res.rgb[res.index < 0] == 255).all())
    empty = postprocess.tsdf_extract(postprocess.tsdf_volume((0, 0, 0), 0.1, (5, 4, 3)))
    res = postprocess.render_mesh(empty, ring, K, (H, W), return_index=True)
    assert bool((res.rgb == 255).all()) and bool((res.depth == 0).all()) and bool((res.index == -1).all())
    with pytest.raises(L.OvgError):
        postprocess.render_mesh(postprocess.Mesh(mesh.vertices.cpu(), mesh.faces, None, None, mesh.transform), ring, K, (H, W))


def test_every_entry_level_argument_error():
    L.require_gpu()
    lib = L.load()
    vert, nrm, faces, col = (_dev(a) for a in _mesh("sphere", 17))
    V, H, W = 2, 12, 16
    cams = _dev(twin.pack_cams(tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 1.2)[:V], tsdf_twin.pinhole(H, W, 60.0)))
    need = ops.render_mesh_workspace_bytes(V, H, W)
    ws = torch.empty(need + 16, device="cuda", dtype=torch.uint8)
    rgb = torch.full((V, H, W, 3), 7, device="cuda", dtype=torch.uint8)

    def params(**kw):
        p = L.RenderMeshParams()
        p.vertices, p.faces, p.normals, p.colors, p.M, p.F = vert.data_ptr(), faces.data_ptr(), nrm.data_ptr(), col.data_ptr(), len(vert), len(faces)
        p.cams, p.V, p.H, p.W, p.shading, p.cull, p.coop_threshold, p.near, p.flags = cams.data_ptr(), V, H, W, 1, 0, 0, 1e-3, 0
        p.ws, p.ws_bytes, p.out_rgb = ws.data_ptr(), need, rgb.data_ptr()
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    assert lib.ovg_render_mesh(ctypes.byref(params()), None) == 0
    assert lib.ovg_render_mesh(ctypes.byref(params(normals=None, colors=None, M=0, vertices=None)), None) == 0
    assert lib.ovg_render_mesh(ctypes.byref(params(F=0, faces=None)), None) == 0
    torch.cuda.synchronize()
    rgb.fill_(7)
    bad = [dict(cams=None), dict(ws=None), dict(out_rgb=None), dict(vertices=None), dict(faces=None), dict(M=-1), dict(F=-1), dict(M=1 << 31),
           dict(F=1 << 31), dict(V=0), dict(H=0), dict(W=-3), dict(V=1 << 20, H=1 << 10, W=1 << 10), dict(near=0.0), dict(near=-1.0),
           dict(near=float("nan")), dict(near=float("inf")), dict(shading=3), dict(shading=-1), dict(cull=3), dict(cull=-1), dict(flags=1),
           dict(flags=-1), dict(coop_threshold=-1), dict(ws=ws.data_ptr() + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert lib.ovg_render_mesh(ctypes.byref(params(**kw)), None) == E_ARG, kw
    assert lib.ovg_render_mesh(None, None) == E_ARG
    torch.cuda.synchronize()
    assert bool((rgb == 7).all())                                           # nothing is written when the entry refuses
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 15), (1 << 11, 1 << 10, 1 << 10)):
        assert lib.ovg_render_mesh_workspace_bytes(*shape) == -1, shape
        with pytest.raises(L.OvgError):
            ops.render_mesh_workspace_bytes(*shape)
    assert lib.ovg_render_mesh_workspace_bytes(5, 3, 5) == 608              # 600 rounded up to 16
    with pytest.raises(L.OvgError):
        ops.render_mesh(vert.cpu(), faces, cams, H, W)
    with pytest.raises(L.OvgError):
        ops.render_mesh(vert, faces.long(), cams, H, W)
    with pytest.raises(L.OvgError):
        ops.render_mesh(vert, faces, cams, H, W, normals=nrm[:-1])
