"""Mesh rasterisation without a device: the C layout of ovg_render_mesh_params against the ctypes mirror, every ValueError of
postprocess.render_mesh, and self-checks of tests/raster_twin.py (the oracle of tests/test_gpu_raster.py) on the analytic sphere
meshes of tsdf_twin and on hand-made quads."""

import numpy as np
import pytest
import torch

import abi_layout
import raster_twin as twin
import tsdf_twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

F = np.float32


def test_params_layout_matches_c():
    """sizeof and every field offset of ovg_render_mesh_params as gcc sees the header == the ctypes mirror; the enums too."""
    enums, _ = abi_layout.check({"ovg_render_mesh_params": L.RenderMeshParams},
                                ["OVG_MESH_SHADE_COLOR", "OVG_MESH_SHADE_HEADLIGHT", "OVG_MESH_SHADE_NORMAL", "OVG_MESH_CULL_NONE",
                                 "OVG_MESH_CULL_BACK", "OVG_MESH_CULL_FRONT"])
    assert enums[:3] == [L.MESH_SHADE_COLOR, L.MESH_SHADE_HEADLIGHT, L.MESH_SHADE_NORMAL] == [twin.SHADE_COLOR, twin.SHADE_HEADLIGHT, twin.SHADE_NORMAL]
    assert enums[3:] == [L.MESH_CULL_NONE, L.MESH_CULL_BACK, L.MESH_CULL_FRONT] == [twin.CULL_NONE, twin.CULL_BACK, twin.CULL_FRONT]
    assert postprocess.MESH_SHADINGS == {"color": L.MESH_SHADE_COLOR, "headlight": L.MESH_SHADE_HEADLIGHT, "normal": L.MESH_SHADE_NORMAL}
    assert postprocess.MESH_CULLS == {None: L.MESH_CULL_NONE, "back": L.MESH_CULL_BACK, "front": L.MESH_CULL_FRONT}
    for name in ("ovg_render_mesh", "ovg_render_mesh_workspace_bytes"):
        assert name in L.SYMBOLS


def _cpu_mesh():
    v = torch.tensor([[0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0]])
    return postprocess.Mesh(v, torch.tensor([[0, 2, 1]], dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.uint8), np.eye(4))


def test_every_value_error_of_render_mesh():
    mesh, E, K = _cpu_mesh(), np.eye(4)[:3], np.eye(3)
    good = dict(extrinsic=E, intrinsic=K, size=(4, 5))
    bad = [dict(size=(4,)), dict(size=(0, 5)), dict(size=(4, -1)), dict(size=(4.5, 5)), dict(size=5), dict(size=("a", "b")),
           dict(shading="phong"), dict(shading=1), dict(shading=None),
           dict(cull="both"), dict(cull=1), dict(cull=["back"]),
           dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(near=1e-60), dict(near="x"), dict(near=True),
           dict(background=(1, 2)), dict(background=(0, 0, 256)), dict(background=(-1, 0, 0)), dict(background=(0.5, 0, 0)), dict(background=7),
           dict(extrinsic=np.eye(4)), dict(extrinsic=np.zeros((0, 3, 4))), dict(extrinsic=np.zeros((2, 2, 3, 4))),
           dict(intrinsic=np.eye(4)), dict(intrinsic=np.zeros((2, 3, 3))), dict(extrinsic=np.tile(E, (3, 1, 1)), intrinsic=np.zeros((2, 3, 3))),
           dict(size=(1 << 16, 1 << 15))]
    for kw in bad:
        with pytest.raises(ValueError):
            postprocess.render_mesh(mesh, **{**good, **kw})
    with pytest.raises(ValueError):
        postprocess.render_mesh("not a mesh", **good)
    with pytest.raises(ValueError):
        postprocess.render_mesh(postprocess.Mesh(None, None, None, None, np.eye(4)), **good)
    # good arguments and a mesh on the host: there is no CPU fallback
    with pytest.raises(L.OvgError):
        postprocess.render_mesh(mesh, **good)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin on the analytic sphere meshes
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[(17, 48), (33, 96)])
def sphere(request):
    n, size = request.param
    tsdf, weight, origin, voxel, _ = tsdf_twin.sdf_volume("sphere", n)
    vert, nrm, col, faces = tsdf_twin.extract(tsdf, weight, None, origin, voxel)
    ext, intr = tsdf_twin.sphere_cameras((0.0, 0.0, 0.0), 1.2), tsdf_twin.pinhole(size, size, 60.0)
    cams = twin.pack_cams(ext, intr)
    stats = {}
    zbuf = twin.zbuffer(vert, faces, cams, size, size, twin.CULL_NONE, 1e-3, stats)
    return dict(vert=vert, nrm=nrm, faces=faces, cams=cams, size=size, voxel=float(voxel), zbuf=zbuf, stats=stats,
                analytic=tsdf_twin.sphere_depth(ext, intr, size, size, (0.0, 0.0, 0.0), 0.6, miss=0.0))


def test_twin_sphere_coverage_silhouette_and_depth(sphere):
    S, zbuf = sphere["size"], sphere["zbuf"]
    _, depth, index = twin.resolve(zbuf, sphere["vert"], sphere["faces"], sphere["nrm"], None, sphere["cams"], S, S)
    for v in range(len(zbuf)):
        hit = index[v] >= 0
        n_hit, covered = int(hit.sum()), sphere["stats"]["covered"][v]
        inside = sphere["analytic"][v] > 0
        d = np.abs(depth[v][hit & inside].astype(np.float64) - sphere["analytic"][v][hit & inside]) / sphere["voxel"]
        print("view %d: %d of %d pixels hit, %d covered, %d outside the silhouette, |depth - analytic| median %.3f max %.3f voxel"
              % (v, n_hit, S * S, covered, int((hit & ~inside).sum()), np.median(d), d.max()))
        assert n_hit >= 0.6 * S * S
        assert covered >= 1.5 * n_hit                                       # the depth test decides pixels
        assert int((hit & ~inside).sum()) <= 0.01 * n_hit
        assert np.median(d) <= 0.2 and d.max() <= 1.5
        assert (depth[v][~hit] == 0).all() and (depth[v][hit] > 0).all()


def test_twin_cull_modes_on_a_closed_mesh(sphere):
    S, zbuf = sphere["size"], sphere["zbuf"]
    args = (sphere["vert"], sphere["faces"], sphere["cams"], S, S)
    back = twin.zbuffer(*args, twin.CULL_BACK)
    assert back.tobytes() == zbuf.tobytes()                                 # outward-wound, seen from outside: nothing visible is dropped
    front = twin.zbuffer(*args, twin.CULL_FRONT)
    both = (front != twin.EMPTY) & (zbuf != twin.EMPTY)
    assert both.sum() >= 0.9 * (zbuf != twin.EMPTY).sum()
    near_z = (zbuf[both] >> np.uint64(32)).astype(np.uint32).view(F)
    far_z = (front[both] >> np.uint64(32)).astype(np.uint32).view(F)
    assert (far_z > near_z).all()
    # every winning face is front-facing: area < 0 with x to the right and y down
    faces = np.asarray(sphere["faces"], np.int64)
    for v in (0, 7):
        ok, X, Y, _ = twin.project_vertices(sphere["vert"], sphere["cams"][v], 1e-3)
        win = np.unique((zbuf[v][zbuf[v] != twin.EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64))
        Xf, Yf = X[faces[win]], Y[faces[win]]
        area = (Xf[:, 1] - Xf[:, 0]) * (Yf[:, 2] - Yf[:, 0]) - (Yf[:, 1] - Yf[:, 0]) * (Xf[:, 2] - Xf[:, 0])
        assert ok.all() and (area < 0).all()


def test_twin_edge_functions_sum_to_the_area(sphere):
    S = sphere["size"]
    seen = 0
    for cull in (twin.CULL_NONE, twin.CULL_FRONT):
        for _, px, py, X, Y, area, _, w in twin.candidates(sphere["vert"], sphere["faces"], sphere["cams"][3], S, S, cull, 1e-3):
            assert (w[0] + w[1] + w[2] == np.abs(area)).all() and (area != 0).all()
            assert (px >= 0).all() and (px < S).all() and (py >= 0).all() and (py < S).all()
            seen += len(px)
    assert seen > 1000


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-made quads
# ---------------------------------------------------------------------------------------------------------------------------------

def _quad(tilt_deg=0.0, z=2.0, half=0.6):
    """A square of side 2 half centred on the optical axis at depth z, rotated by tilt_deg about the camera's y axis; wound so that
    its normal looks at the camera (area < 0)."""
    t = np.deg2rad(tilt_deg)
    corners = np.array([[-half, -half, 0.0], [half, -half, 0.0], [half, half, 0.0], [-half, half, 0.0]])
    rot = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    vert = (corners @ rot.T + [0.0, 0.0, z]).astype(F)
    return vert, np.array([[0, 2, 1], [0, 3, 2]], np.int32)


def test_twin_duplicate_triangles_resolve_to_the_lower_index():
    vert, faces = _quad()
    faces = np.concatenate([faces, faces, faces[::-1]])                     # 0 = 2 = 5, 1 = 3 = 4
    cams = twin.pack_cams(np.eye(4)[:3][None], tsdf_twin.pinhole(32, 32, 60.0))
    _, depth, index = twin.render(vert, faces, None, None, cams, 32, 32)
    hit = index[0] >= 0
    assert hit.sum() >= 100 and set(np.unique(index[0][hit])) == {0, 1}
    assert (depth[0][hit] == F(2.0)).all()                                  # a plane of constant camera depth interpolates exactly


def test_twin_headlight_of_a_facing_and_of_a_tilted_quad():
    cams = twin.pack_cams(np.eye(4)[:3][None], tsdf_twin.pinhole(32, 32, 60.0))
    colour = np.array([[200, 100, 50]] * 4, np.uint8)
    for normals in (None, "vertex"):
        for tilt, factor in ((0.0, 1.0), (60.0, 0.25 + 0.75 * 0.5)):
            vert, faces = _quad(tilt)
            t = np.deg2rad(tilt)
            nrm = None if normals is None else np.tile(np.array([-np.sin(t), 0.0, -np.cos(t)], F), (4, 1))
            rgb, _, index = twin.render(vert, faces, nrm, colour, cams, 32, 32, shading=twin.SHADE_HEADLIGHT)
            hit = index[0] >= 0
            assert hit.sum() >= 50
            want = np.floor(factor * colour[0].astype(np.float64) + 0.5)
            got = rgb[0][hit].astype(np.float64)
            if tilt == 0.0:
                assert (got == colour[0]).all()                             # the colour itself
            assert np.abs(got - want).max() <= 1, (normals, tilt, got.min(0), got.max(0), want)
            flat, _, _ = twin.render(vert, faces, nrm, colour, cams, 32, 32, shading=twin.SHADE_COLOR)
            assert (flat[0][hit] == colour[0]).all() and (flat[0][~hit] == 255).all()
            nmap, _, _ = twin.render(vert, faces, nrm, colour, cams, 32, 32, shading=twin.SHADE_NORMAL)
            n_unit = np.array([-np.sin(t), 0.0, -np.cos(t)])
            assert np.abs(nmap[0][hit].astype(np.float64) - np.floor((0.5 * n_unit + 0.5) * 255 + 0.5)).max() <= 1
