"""Volumetric fusion (ovg_tsdf_integrate / ovg_tsdf_extract, postprocess.tsdf_* / fuse_predictions / write_mesh_*), host side: the
numpy twin (tests/tsdf_twin.py) on analytic volumes and analytic sphere depth, the properties of the two rules, the C ABI without a
device (exported symbols, struct layout, enums, argument checks that return before any HIP call), the Python API's argument checks
and the two mesh writers parsed back."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

import abi_layout
import common
import tsdf_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
ENTRIES = ("ovg_tsdf_integrate", "ovg_tsdf_extract")


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------

def _layout(struct_type, cname, extra):
    return abi_layout.check({cname: struct_type}, extra)[0]


def test_library_exports_the_entries_and_ctypes_layout_matches_c():
    lib = L.load()
    assert lib.ovg_abi_version() == 13 == L.ABI_VERSION
    for name in ENTRIES + ("ovg_tsdf_extract_workspace_bytes",):
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    enums = ["OVG_TSDF_TILE_DEFAULT", "OVG_TSDF_TILE_256x1x1", "OVG_TSDF_TILE_8x8x4", "OVG_TSDF_TILE_16x4x4", "OVG_TSDF_TILE_32x8x1",
             "OVG_TSDF_COUNT", "OVG_TSDF_SCATTER", "OVG_TSDF_GREY", "OVG_TSDF_EXTRACT_BLOCK", "OVG_ABI_VERSION"]
    want = [L.TSDF_TILE_DEFAULT, L.TSDF_TILE_256x1x1, L.TSDF_TILE_8x8x4, L.TSDF_TILE_16x4x4, L.TSDF_TILE_32x8x1, L.TSDF_COUNT, L.TSDF_SCATTER,
            L.TSDF_GREY, L.TSDF_EXTRACT_BLOCK, 13]
    assert want[:5] == [0, 1, 2, 3, 4] and L.TSDF_GREY == twin.GREY
    for struct_type, cname in ((L.TsdfIntegrateParams, "ovg_tsdf_integrate_params"), (L.TsdfExtractParams, "ovg_tsdf_extract_params")):
        assert _layout(struct_type, cname, enums) == want, cname
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (name, name), text), name
    assert re.search(r"int64_t\s+ovg_tsdf_extract_workspace_bytes\s*\(\s*int32_t\s+nx\s*,\s*int32_t\s+ny\s*,\s*int32_t\s+nz\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    # the workspace: an int32 vertex-index volume, one byte and two int64 per 256 lattice points, each part rounded up to 256
    r256 = lambda b: (b + 255) // 256 * 256
    for nx, ny, nz in ((1, 1, 1), (9, 5, 3), (33, 33, 33), (256, 256, 256), (2047, 1024, 1024)):
        n = nx * ny * nz
        assert lib.ovg_tsdf_extract_workspace_bytes(nx, ny, nz) == r256(4 * n) + r256(n) + 2 * r256(8 * ((n + 255) // 256))
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (2048, 1024, 1024), (1 << 16, 1 << 16, 1), (1 << 30, 1 << 30, 1 << 30)):
        assert lib.ovg_tsdf_extract_workspace_bytes(*bad) == -1, bad
        with pytest.raises(L.OvgError):
            ops.tsdf_extract_workspace_bytes(*bad)


def test_argument_validation_of_the_entries_without_gpu():
    lib = L.load()
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    nan, inf = float("nan"), float("inf")

    def run(name, struct_type, base, **kw):
        p = struct_type()
        for k, v in dict(base, **kw).items():
            if k == "origin":
                for q in range(3):
                    p.origin[q] = v[q]
            else:
                setattr(p, k, v)
        return getattr(lib, name)(ctypes.byref(p), None)

    for name in ENTRIES:
        assert getattr(lib, name)(None, None) == -1
    base = dict(tsdf=big, weight=big, color=big, nx=8, ny=8, nz=8, origin=(0.0, 0.0, 0.0), voxel=0.1, trunc=0.3, max_weight=64.0, near=1e-3,
                depth=big, cams=big, valid=big + 1, obs_weight=big, colors=big + 1, S=4, H=37, W=53, view_first=0, view_count=4, tile=0)
    bads = [dict(tsdf=None), dict(weight=None), dict(depth=None), dict(cams=None), dict(color=None), dict(nx=0), dict(ny=-1), dict(nz=0),
            dict(nx=2048, ny=1024, nz=1024), dict(nx=1 << 16, ny=1 << 16, nz=1), dict(S=0), dict(H=0), dict(W=-3), dict(S=1 << 11, H=1 << 10, W=1 << 10),
            dict(H=1 << 16, W=1 << 16, S=1), dict(view_first=-1), dict(view_first=4), dict(view_count=0), dict(view_count=5),
            dict(view_first=2, view_count=3), dict(tile=-1), dict(tile=5), dict(origin=(nan, 0.0, 0.0)), dict(origin=(0.0, inf, 0.0)),
            dict(origin=(0.0, 0.0, -inf)), dict(tsdf=big + 2), dict(weight=big + 1), dict(color=big + 4), dict(color=big + 8), dict(depth=big + 2),
            dict(cams=big + 2), dict(obs_weight=big + 2)]
    for name in ("voxel", "trunc", "max_weight", "near"):
        bads += [{name: v} for v in (0.0, -0.0, -1.0, nan, inf, -inf)]
    for bad in bads:
        assert run("ovg_tsdf_integrate", L.TsdfIntegrateParams, base, **bad) == -1, bad
    base = dict(tsdf=big, weight=big, color=big, nx=8, ny=8, nz=8, origin=(0.0, 0.0, 0.0), voxel=0.1, min_weight=1.0, stage=L.TSDF_SCATTER,
                vertex_capacity=10, quad_capacity=10, vertices=big, normals=big, colors=big + 1, faces=big, out_count=big, ws=big,
                ws_bytes=lib.ovg_tsdf_extract_workspace_bytes(8, 8, 8))
    bads = [dict(tsdf=None), dict(weight=None), dict(ws=None), dict(out_count=None), dict(nx=0), dict(ny=-1), dict(nz=0),
            dict(nx=2048, ny=1024, nz=1024), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(min_weight=0.0),
            dict(min_weight=-1.0), dict(min_weight=nan), dict(min_weight=inf), dict(origin=(nan, 0.0, 0.0)), dict(origin=(0.0, 0.0, inf)),
            dict(stage=0), dict(stage=4), dict(stage=-1), dict(vertex_capacity=-1), dict(quad_capacity=-1), dict(vertices=None), dict(normals=None),
            dict(colors=None), dict(faces=None), dict(tsdf=big + 2), dict(weight=big + 1), dict(color=big + 8), dict(out_count=big + 4),
            dict(ws=big + 8), dict(ws_bytes=base["ws_bytes"] - 1), dict(ws_bytes=0), dict(vertices=big + 2), dict(normals=big + 1), dict(faces=big + 2)]
    for bad in bads:
        assert run("ovg_tsdf_extract", L.TsdfExtractParams, base, **bad) == -1, bad
    for bad in (dict(stage=L.TSDF_COUNT, ws_bytes=8), dict(stage=L.TSDF_COUNT | L.TSDF_SCATTER, vertices=None)):
        assert run("ovg_tsdf_extract", L.TsdfExtractParams, base, **bad) == -1, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# extraction on analytic volumes
# ---------------------------------------------------------------------------------------------------------------------------------

def _closed(vert, faces, chi):
    st = twin.mesh_stats(vert, faces)
    assert st["bad_edges"] == 0 and st["dup_directed"] == 0 and st["degenerate"] == 0, st   # a closed, consistently oriented 2-manifold
    assert st["V"] == len(vert) and st["chi"] == chi and st["volume"] > 0, st
    return st


# what the twin gives (V, E, F, signed volume / true volume): recorded, and gated below
ANALYTIC = {("sphere", 33): (1760, 5274, 3516, 0.9877), ("torus", 33): (1864, 5592, 3728, 0.9750), ("two_spheres", 33): (832, 2484, 1656, 0.9507),
            ("sphere", 17): (416, 1242, 828, 0.9507), ("torus", 17): (432, 1296, 864, 0.8930), ("two_spheres", 17): (256, 756, 504, 0.8236),
            ("sphere", 9): (128, 378, 252, 0.8236), ("torus", 9): (104, 312, 208, 0.5094), ("two_spheres", 9): (64, 180, 120, 0.3547)}


@pytest.mark.parametrize("kind,chi", [("sphere", 2), ("torus", 0), ("two_spheres", 4)])
def test_extraction_of_analytic_volumes_is_a_closed_oriented_manifold(kind, chi):
    for n in (9, 17, 33):
        tsdf, weight, origin, voxel, true = twin.sdf_volume(kind, n)
        vert, nrm, col, faces = twin.extract(tsdf, weight, None, origin, voxel)
        assert vert.dtype == F and nrm.dtype == F and col.dtype == np.uint8 and faces.dtype == np.int32
        st = _closed(vert, faces, chi)
        ratio = st["volume"] / true
        print("%s %d^3: V %d E %d F %d volume %.4f of the true volume" % (kind, n, st["V"], st["E"], st["F"], ratio))
        assert (st["V"], st["E"], st["F"]) == ANALYTIC[kind, n][:3] and abs(ratio - ANALYTIC[kind, n][3]) < 1e-4
        if n == 33 and kind != "two_spheres":                                # each of the two spheres is as coarse as the 17^3 sphere
            assert 0.95 <= ratio <= 1.0
        assert (col == twin.GREY).all()
        # unit normals along the gradient: outwards, within 30 degrees of the triangle normals of the faces round the vertex
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
        tri = np.cross(vert[faces[:, 1]] - vert[faces[:, 0]], vert[faces[:, 2]] - vert[faces[:, 0]]).astype(np.float64)
        acc = np.zeros((len(vert), 3))
        for k in range(3):
            np.add.at(acc, faces[:, k], tri)
        cos = (acc * nrm).sum(1) / np.linalg.norm(acc, axis=1)
        assert cos.min() > np.cos(np.deg2rad(30.0 if n > 9 else 60.0)), (kind, n, cos.min())
    # the torus with minor radius 0.2 at 9^3: barely two voxels thick, still a closed torus
    tsdf, weight, origin, voxel, _ = twin.sdf_volume("torus", 9, minor=0.2)
    st = _closed(*twin.extract(tsdf, weight, None, origin, voxel)[::3], 0)
    assert (st["V"], st["E"], st["F"]) == (88, 264, 176)


def test_extraction_rules_on_small_volumes():
    # one inside point in a 3^3 volume: 8 active cells, 6 crossing edges, each with its four cells -> a closed octahedron-like cube
    tsdf, weight = np.ones((3, 3, 3), F), np.ones((3, 3, 3), F)
    tsdf[1, 1, 1] = F(-1)
    origin, voxel = np.array([10.0, 20.0, 30.0], F), F(0.5)
    vert, nrm, col, faces = twin.extract(tsdf, weight, None, origin, voxel)
    assert len(vert) == 8 and len(faces) == 12
    st = _closed(vert, faces, 2)
    # every crossing sits half-way, three per cell: the mean is (5/6, 5/6, 5/6) from the cell's far corner, so the vertices are the
    # corners of a cube of a third of a voxel round the inside lattice point
    centre = origin.astype(np.float64) + float(voxel)
    assert np.allclose(np.abs(vert - centre), float(voxel) / 6.0, rtol=0, atol=4e-6)
    assert abs(st["volume"] - (float(voxel) / 3.0) ** 3) < 1e-6
    assert ((vert - centre) * nrm > 0).all()                                # inside to outside
    # -0 counts as outside, a NaN as outside; min_weight is inclusive
    t2 = tsdf.copy()
    t2[1, 1, 1] = F(-0.0)
    assert len(twin.extract(t2, weight, None, origin, voxel)[0]) == 0
    w2 = weight.copy()
    w2[0, 0, 0] = F(0.5)
    assert len(twin.extract(tsdf, w2, None, origin, voxel, 0.5)[0]) == 8 and len(twin.extract(tsdf, w2, None, origin, voxel, 0.75)[0]) == 7
    # a missing cell removes the three quads that need it, never adds one; the vertices keep their order
    v7, _, _, f7 = twin.extract(tsdf, w2, None, origin, voxel, 0.75)
    assert len(f7) == 6 and (v7 == vert[1:]).all()
    # no crossing, and every axis of length 1
    assert all(len(a) == 0 for a in twin.extract(np.ones((4, 4, 4), F), np.ones((4, 4, 4), F), None, origin, voxel))
    assert all(len(a) == 0 for a in twin.extract(-np.ones((4, 4, 4), F), np.ones((4, 4, 4), F), None, origin, voxel))
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)):
        t = np.where(np.arange(np.prod(shape)).reshape(shape) % 2 == 0, F(-1), F(1)).astype(F)
        out = twin.extract(t, np.ones(shape, F), None, origin, voxel)
        assert [a.shape for a in out] == [(0, 3)] * 4 and out[3].dtype == np.int32
    # colours: the mean of the coloured corners, rounded half up; grey without any
    color = np.zeros((3, 3, 3, 4), F)
    color[1, 1, 1] = (10, 20, 30, 2)
    color[0, 0, 0] = (11, 21, 33, 1)
    color[2, 2, 2] = (255, 300, -5, 0.5)
    col = twin.extract(tsdf, weight, color, origin, voxel)[2]
    assert col[0].tolist() == [11, 21, 32] and col[1].tolist() == [10, 20, 30] and col[7].tolist() == [133, 160, 13]
    color[1, 1, 1, 3] = 0
    assert twin.extract(tsdf, weight, color, origin, voxel)[2][1].tolist() == [twin.GREY] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# integration of analytic sphere depth
# ---------------------------------------------------------------------------------------------------------------------------------

def _fuse(sc, **kw):
    T, W, C = twin.fresh(sc["dims"], color=kw.get("colors") is not None)
    twin.integrate(T, W, C, sc["origin"], sc["voxel"], sc["trunc"], kw.pop("max_weight", 64.0), 1e-3, sc["depth"], sc["cams"], **kw)
    return T, W, C


@pytest.mark.parametrize("n,size", [(24, 64), (24, 128), (32, 64), (32, 128), (48, 64), (48, 128)])
def test_integration_of_analytic_sphere_depth(n, size):
    """What the twin gives (signed volume / true, mean and max vertex distance in voxels, edges not shared by two triangles):
    24/64 0.978 0.092 0.353 0; 24/128 0.981 0.091 0.358 0; 32/64 0.987 0.083 0.368 0; 32/128 0.991 0.080 0.365 0;
    48/64 0.986 0.111 0.359 0; 48/128 0.987 0.092 0.361 0."""
    sc = twin.sphere_scene(n, size)
    assert sc["depth"].shape == (14, size, size) and sc["trunc"] == F(3) * sc["voxel"]
    T, W, _ = _fuse(sc)
    vert, nrm, col, faces = twin.extract(T, W, None, sc["origin"], sc["voxel"])
    st = twin.mesh_stats(vert, faces)
    r = sc["radius"]
    dist = np.abs(np.linalg.norm(vert.astype(np.float64), axis=1) - r) / float(sc["voxel"])
    ratio = st["volume"] / (4.0 / 3.0 * np.pi * r ** 3)
    print("%d^3, %d^2: chi %d volume %.4f distance mean %.3f max %.3f bad edges %d of %d" % (n, size, st["chi"], ratio, dist.mean(), dist.max(),
                                                                                              st["bad_edges"], st["E"]))
    assert st["chi"] == 2 and abs(ratio - 1.0) <= 0.03
    assert dist.mean() <= 0.2 and dist.max() <= 1.5
    assert st["bad_edges"] <= 0.002 * st["E"] and st["degenerate"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# properties of the integration rule
# ---------------------------------------------------------------------------------------------------------------------------------

def _bytes(*arrays):
    return [None if a is None else a.tobytes() for a in arrays]


def test_split_integration_weights_valid_and_clamp():
    sc = twin.sphere_scene(20, 48)
    S, H, Wd = sc["depth"].shape
    rng = np.random.default_rng(0)
    colors = rng.integers(0, 256, (S, H, Wd, 3)).astype(np.uint8)
    full = _fuse(sc, colors=colors)
    assert (full[1] > 0).mean() > 0.5 and (full[0] < 0).any() and (full[2][..., 3] > 0).any()
    # a view range and then the rest: the bytes of one call, for every split point
    for k in (1, 5, 13):
        T, W, C = twin.fresh(sc["dims"])
        args = (sc["origin"], sc["voxel"], sc["trunc"], 64.0, 1e-3, sc["depth"], sc["cams"])
        twin.integrate(T, W, C, *args, colors=colors, views=range(0, k))
        twin.integrate(T, W, C, *args, colors=colors, views=range(k, S))
        assert _bytes(T, W, C) == _bytes(*full), k
    # the order of the views matters (a running mean in float32), which is why it is fixed
    T, W, C = twin.fresh(sc["dims"])
    twin.integrate(T, W, C, *args, colors=colors, views=range(S - 1, -1, -1))
    assert W.tobytes() == full[1].tobytes() and T.tobytes() != full[0].tobytes() and np.abs(T - full[0]).max() < 1e-5
    # obs_weight of all ones is no weight; valid of all ones is no mask
    assert _bytes(*_fuse(sc, colors=colors, obs_weight=np.ones((S, H, Wd), F), valid=np.ones((S, H, Wd), np.uint8))) == _bytes(*full)
    # the clamp: the weight never exceeds max_weight, and reaches it where more views than that agree
    T, W, C = _fuse(sc, colors=colors, max_weight=3.0)
    assert W.max() == 3 and (W == 3).sum() > 100 and C[..., 3].max() == 3 and full[1].max() > 3
    assert (np.abs(T[W > 0]) <= 1).all()
    # valid = 0, depths that are 0 / negative / <= near / not finite and weights that are 0 / negative / not finite are all skipped:
    # spoiling half of every map that way equals masking that half
    spoil = rng.random((S, H, Wd)) < 0.5
    keep = (~spoil).astype(np.uint8)
    want = _fuse(sc, colors=colors, valid=keep)
    assert _bytes(*want) != _bytes(*full)
    bad_depth = np.array([0.0, -1.0, 1e-3, 5e-4, np.nan, np.inf, -np.inf], F)
    d2 = np.where(spoil, bad_depth[rng.integers(0, len(bad_depth), spoil.shape)], sc["depth"]).astype(F)
    assert _bytes(*_fuse(dict(sc, depth=d2), colors=colors)) == _bytes(*want)
    bad_weight = np.array([0.0, -0.0, -2.0, np.nan, np.inf, -np.inf], F)
    w2 = np.where(spoil, bad_weight[rng.integers(0, len(bad_weight), spoil.shape)], F(1)).astype(F)
    assert _bytes(*_fuse(sc, colors=colors, obs_weight=w2)) == _bytes(*want)
    # a weight scales an observation: doubling every weight doubles the accumulated weight and keeps the mean (powers of two are exact)
    T2, W2, C2 = _fuse(sc, colors=colors, obs_weight=np.full((S, H, Wd), 2, F), max_weight=128.0)
    assert (W2 == 2 * full[1]).all() and T2.tobytes() == full[0].tobytes() and (C2[..., :3] == full[2][..., :3]).all()
    # integration into a populated volume goes on from its state
    T, W, C = (a.copy() for a in full)
    twin.integrate(T, W, C, *args, colors=colors, views=[3])
    touched = W != full[1]
    assert touched.any() and (T[~touched] == full[0][~touched]).all() and (W[touched] == full[1][touched] + 1).all()


def test_free_space_carves_a_floater_and_does_not_colour_it():
    # two cameras look along +z at a wall z = 2. The first also sees a blob at z = 1 in the middle of its frame; the second one,
    # moved sideways, sees the wall behind the blob's place: free space
    H = W = 48
    intr = twin.pinhole(H, W, 60.0)
    ext = np.stack([twin.look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), twin.look_at((0.3, 0.0, 0.0), (0.3, 0.0, 1.0))])
    depth = twin.plane_depth(ext, intr, H, W, (0.0, 0.0, 1.0), -2.0)
    assert np.allclose(depth, 2.0)
    depth[0, 20:28, 20:28] = F(1.0)
    colors = np.zeros((2, H, W, 3), np.uint8)
    colors[0, ..., 0], colors[1, ..., 1] = 200, 200                          # view 0 paints red, view 1 green
    cams = twin.pack_cams(ext, intr)
    n = 40
    origin, voxel = np.array([-0.5, -0.5, 0.5], F), F(2.0 / (n - 1))
    trunc = F(3) * voxel

    def run(views):
        T, Wt, C = twin.fresh((n, n, n))
        twin.integrate(T, Wt, C, origin, voxel, trunc, 64.0, 1e-3, depth, cams, colors=colors, views=views)
        return T, Wt, C

    X, Y, Z = twin.lattice(origin, voxel, (n, n, n))
    blob = (np.abs(X) < 0.08) & (np.abs(Y) < 0.08) & (np.abs(Z - 1.0) < 0.5 * float(voxel))      # lattice points on the blob's surface
    assert blob.sum() >= 4
    T0, W0, C0 = run([0])
    assert (np.abs(T0[blob]) < 0.2).all() and (W0[blob] == 1).all()
    m0 = twin.extract(T0, W0, C0, origin, voxel)
    near_blob = (np.abs(m0[0][:, 2] - 1.0) < 2 * float(voxel)).sum()
    assert near_blob >= 4                                                   # view 0 alone: the floater is part of the mesh
    T, Wt, C = run([0, 1])
    assert (Wt[blob] == 2).all() and (T[blob] > 0.4).all()                   # (about 0 + 1) / 2: carved towards free space
    m = twin.extract(T, Wt, C, origin, voxel)
    assert (np.abs(m[0][:, 2] - 1.0) < 2 * float(voxel)).sum() == 0          # no zero crossing is left at the blob
    assert (np.abs(m[0][:, 2] - 2.0) < float(voxel)).mean() > 0.9            # the wall stays
    # the free-space observation of view 1 did not colour the blob: still view 0's red, colour weight 1
    assert (C[blob][:, 3] == 1).all() and (C[blob][:, 0] == 200).all() and (C[blob][:, 1] == 0).all()
    # on the wall both views colour: the mean of red and green
    wall = (np.abs(Z - 2.0) < 0.5 * float(voxel)) & (Wt == 2) & (np.abs(X) > 0.2)
    assert wall.sum() > 50 and (C[wall][:, 3] == 2).all() and (C[wall][:, 0] == 100).all() and (C[wall][:, 1] == 100).all()
    # lattice points behind the wall by more than trunc are never touched
    behind = Z > 2.0 + float(trunc) + float(voxel)
    assert (Wt[behind] == 0).all() and (T[behind] == 1).all()
    # the two-wall corner: both walls are found
    ext2 = np.stack([twin.look_at((1.5, 0.2, 1.5), (0.0, 0.0, 0.0)), twin.look_at((1.0, -0.3, 2.0), (0.2, 0.0, 0.0)), twin.look_at((2.0, 0.3, 1.0), (0.0, 0.0, 0.2))])
    d2 = twin.corner_depth(ext2, intr, H, W)
    T, Wt, C = twin.fresh((n, n, n), color=False)
    o2, v2 = np.array([-0.2, -0.5, -0.2], F), F(1.2 / (n - 1))
    twin.integrate(T, Wt, None, o2, v2, F(3) * v2, 64.0, 1e-3, d2, twin.pack_cams(ext2, intr))
    vert = twin.extract(T, Wt, None, o2, v2)[0]
    on_wall = np.minimum(np.abs(vert[:, 0]), np.abs(vert[:, 2])) < 0.5 * float(v2)
    assert len(vert) > 500 and on_wall.mean() > 0.95 and (np.abs(vert[:, 0]) < 0.5 * float(v2)).sum() > 100 and (np.abs(vert[:, 2]) < 0.5 * float(v2)).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python layer without a device, and the writers
# ---------------------------------------------------------------------------------------------------------------------------------

def _cpu_volume(n=4, color=True):
    return postprocess.TSDFVolume(torch.ones(n, n, n), torch.zeros(n, n, n), torch.zeros(n, n, n, 4) if color else None, (0.0, 0.0, 0.0), 0.1, 0.4,
                                  (n, n, n))


def test_python_argument_checks_and_cpu_tensors():
    for kw in (dict(origin=(0, 0)), dict(origin=(0, 0, float("nan"))), dict(origin="abc"), dict(voxel_size=0), dict(voxel_size=-1.0),
               dict(voxel_size=float("inf")), dict(voxel_size=True), dict(dims=(4, 4)), dict(dims=(4, 4, 0)), dict(dims=(4, 4, 2.0)), dict(dims=8),
               dict(trunc=0.0), dict(trunc=float("nan")), dict(max_voxels=0), dict(max_voxels=1.5)):
        with pytest.raises(ValueError):
            postprocess.tsdf_volume(**dict(dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4)), **kw))
    with pytest.raises(ValueError, match=r"2048 x 2048 x 2048 = 8589934592 lattice points exceed max_voxels"):
        postprocess.tsdf_volume((0, 0, 0), 0.1, (2048, 2048, 2048))
    with pytest.raises(ValueError, match=r"65 x 64 x 64 = 266240 lattice points exceed max_voxels = 262144"):
        postprocess.tsdf_volume((0, 0, 0), 0.1, (65, 64, 64), max_voxels=1 << 18)
    assert postprocess.TSDF_MAX_VOXELS == 1 << 28 and postprocess.TSDF_TRUNC_VOXELS == 4.0
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.tsdf_volume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    pts = torch.rand(2, 5, 6, 3)
    for kw in (dict(points_or_cloud=pts.double()), dict(points_or_cloud=pts[..., :2]), dict(points_or_cloud=None), dict(voxel_size=0.0),
               dict(voxel_size=float("nan")), dict(resolution=9), dict(resolution=2.5), dict(resolution=True), dict(margin=-1), dict(margin="x"),
               dict(valid=torch.ones(2, 5, 6)), dict(valid=torch.ones(2, 5, dtype=torch.bool))):
        with pytest.raises(ValueError):
            postprocess.tsdf_volume_for(**dict(dict(points_or_cloud=pts), **kw))
    for kw in (dict(), dict(voxel_size=0.1), dict(resolution=10), dict(valid=torch.ones(2, 5, 6, dtype=torch.bool)), dict(margin=0, resolution=2)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.tsdf_volume_for(pts, **kw)
    vol = _cpu_volume()
    S, H, W = 2, 5, 6
    depth, ext, intr = torch.ones(S, H, W), np.zeros((S, 3, 4)), np.eye(3)
    good = dict(volume=vol, depth=depth, extrinsic=ext, intrinsic=intr)
    for kw in (dict(volume=None), dict(depth=depth[0]), dict(depth=depth.long()), dict(depth=[1.0]), dict(extrinsic=ext[:1]), dict(intrinsic=np.eye(4)),
               dict(intrinsic=np.zeros((3, 3, 3))), dict(valid=torch.ones(S, H, W)), dict(valid=torch.ones(S, H, dtype=torch.bool)),
               dict(weight=torch.ones(S, H)), dict(weight=torch.ones(S, H, W, dtype=torch.int32)), dict(images=torch.zeros(S, H, W, 3)),
               dict(images=torch.zeros(S, 3, H, W, dtype=torch.uint8)), dict(images=torch.zeros(S, 3, H, W), volume=_cpu_volume(color=False)),
               dict(near=0.0), dict(near=float("nan")), dict(max_weight=0.0), dict(max_weight=float("inf")), dict(views=(0, 3)), dict(views=(2, 1)),
               dict(views=(-1, 1)), dict(views=(0, 0)), dict(views=1), dict(views=range(0, 2, 2)), dict(views=(0.0, 1))):
        with pytest.raises(ValueError):
            postprocess.tsdf_integrate(**dict(good, **kw))
    for kw in (dict(), dict(depth=depth[..., None]), dict(images=torch.zeros(S, 3, H, W)), dict(images=torch.zeros(S, H, W, 3, dtype=torch.uint8)),
               dict(valid=torch.ones(S, H, W, dtype=torch.bool), weight=torch.ones(S, H, W)), dict(views=(1, 1)), dict(views=range(0, 2)),
               dict(intrinsic=np.stack([np.eye(3)] * S))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.tsdf_integrate(**dict(good, **kw))
    for bad in (None, depth):
        with pytest.raises(ValueError):
            postprocess.tsdf_extract(bad)
    for mw in (0.0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            postprocess.tsdf_extract(vol, min_weight=mw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.tsdf_extract(vol)
    with pytest.raises(ValueError):
        postprocess.mesh_to_point_cloud(vol)
    mesh = postprocess.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.uint8), np.eye(4))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.mesh_to_point_cloud(mesh)
    pred = {"images": torch.zeros(1, S, 3, H, W), "depth": torch.ones(1, S, H, W, 1)}
    for kw in (dict(predictions=[pred]), dict(batch_index=1), dict(keep_mask=torch.ones(S, H, W)), dict(keep_mask=torch.ones(S, H, dtype=torch.bool)),
               dict(conf_thres=101.0), dict(conf_thres=-1.0), dict(conf_thres="x"), dict(predictions={"images": pred["images"]})):
        with pytest.raises(ValueError):
            postprocess.fuse_predictions(**dict(dict(predictions=pred), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.fuse_predictions(pred)
    # the thin wrappers
    t, w, c = torch.ones(4, 4, 4), torch.zeros(4, 4, 4), torch.zeros(4, 4, 4, 4)
    cams, ws, cnt = torch.zeros(S, 16), torch.zeros(4096, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    o = (0.0, 0.0, 0.0)
    for call in (lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3), lambda: ops.tsdf_integrate(t, w[:2], depth, cams, o, 0.1, 0.3),
                 lambda: ops.tsdf_integrate(t.double(), w, depth, cams, o, 0.1, 0.3), lambda: ops.tsdf_integrate(t, w, depth, cams[:1], o, 0.1, 0.3),
                 lambda: ops.tsdf_integrate(t, w, depth, cams, (0.0, 0.0), 0.1, 0.3), lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.0, 0.3),
                 lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, float("nan")), lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3, tile=9),
                 lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3, view_first=2), lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3, view_count=3),
                 lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3, colors=torch.zeros(S, H, W, 3, dtype=torch.uint8)),
                 lambda: ops.tsdf_integrate(t, w, depth, cams, o, 0.1, 0.3, color=c[..., :3]),
                 lambda: ops.tsdf_extract(L.TSDF_COUNT, t, w, o, 0.1, ws, out_count=cnt), lambda: ops.tsdf_extract(0, t, w, o, 0.1, ws, out_count=cnt),
                 lambda: ops.tsdf_extract(L.TSDF_COUNT, t, w, o, 0.1, ws, out_count=cnt[:1]), lambda: ops.tsdf_extract(L.TSDF_COUNT, t, w, o, 0.1, ws),
                 lambda: ops.tsdf_extract(L.TSDF_COUNT, t, w, o, 0.1, ws, out_count=cnt, min_weight=0.0),
                 lambda: ops.tsdf_extract(L.TSDF_SCATTER, t, w, o, 0.1, ws, out_count=cnt, vertex_capacity=4),
                 lambda: ops.tsdf_extract(L.TSDF_SCATTER, t, w, o, 0.1, ws, out_count=cnt, quad_capacity=-1)):
        with pytest.raises(L.OvgError):
            call()


def _mesh_of(kind="sphere", n=17):
    tsdf, weight, origin, voxel, _ = twin.sdf_volume(kind, n)
    color = np.zeros(tsdf.shape + (4,), F)
    color[..., 0], color[..., 1], color[..., 2], color[..., 3] = 250, np.arange(n, dtype=F)[None, None, :] * 10, 7, 1
    vert, nrm, col, faces = twin.extract(tsdf, weight, color, origin, voxel)
    ext = np.stack([twin.look_at((2.0, 0.0, 0.0), (0, 0, 0)), twin.look_at((0.0, 0.5, -2.0), (0, 0, 0)), twin.look_at((0.0, 2.0, 0.1), (0, 0, 0))])
    transform = postprocess.scene_alignment(ext[0])
    mesh = postprocess.Mesh(torch.from_numpy(vert), torch.from_numpy(faces), torch.from_numpy(nrm), torch.from_numpy(col), transform,
                            torch.from_numpy(ext), torch.tensor(1.5))
    return mesh, vert, nrm, col, faces


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l]
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert "property list uchar int vertex_indices" in lines
    v = np.frombuffer(body[:27 * nv], dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    f = np.frombuffer(body[27 * nv:], dtype=[("k", "u1"), ("v", "<i4", (3,))])
    assert len(body) == 27 * nv + 13 * nf and len(f) == nf
    return v, f


def test_write_mesh_ply_parses_back(tmp_path):
    mesh, vert, nrm, col, faces = _mesh_of()
    path = str(tmp_path / "m.ply")
    postprocess.write_mesh_ply(path, mesh, apply_transform=False)
    v, f = _read_ply(path)
    assert len(v) == len(vert) and len(f) == len(faces) and (f["k"] == 3).all()
    assert v["p"].tobytes() == vert.tobytes() and v["n"].tobytes() == nrm.tobytes() and v["c"].tobytes() == col.tobytes()
    assert f["v"].tobytes() == faces.tobytes() and f["v"].min() == 0 and f["v"].max() == len(vert) - 1
    assert len(np.unique(col[:, 1])) > 5 and (col[:, 0] == 250).all() and (col[:, 2] == 7).all()
    postprocess.write_mesh_ply(path, mesh)                                   # the aligned scene: a rigid motion of vertices and normals
    v2, f2 = _read_ply(path)
    T = np.asarray(mesh.transform)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12 and f2["v"].tobytes() == faces.tobytes()
    assert np.abs(v2["p"] - (vert.astype(np.float64) @ T[:3, :3].T + T[:3, 3])).max() < 1e-6
    assert np.abs(v2["n"] - nrm.astype(np.float64) @ T[:3, :3].T).max() < 1e-6
    st = twin.mesh_stats(v2["p"], f2["v"])
    assert st["chi"] == 2 and st["volume"] > 0 and st["bad_edges"] == 0
    # a mirroring transform turns the winding round, so the solid stays positively oriented
    mesh.transform = np.diag([1.0, -1.0, 1.0, 1.0])
    postprocess.write_mesh_ply(path, mesh)
    v3, f3 = _read_ply(path)
    assert twin.mesh_stats(v3["p"], f3["v"])["volume"] > 0 and f3["v"].tobytes() == faces[:, ::-1].tobytes()
    empty = postprocess.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.uint8), np.eye(4))
    postprocess.write_mesh_ply(path, empty)
    v0, f0 = _read_ply(path)
    assert len(v0) == 0 and len(f0) == 0
    with pytest.raises(ValueError):
        postprocess.write_mesh_ply(path, None)


def _read_glb(path):
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack("<III", raw[:12])
    assert magic == 0x46546C67 and version == 2 and total == len(raw)
    n, kind = struct.unpack("<II", raw[12:20])
    assert kind == 0x4E4F534A and n % 4 == 0
    gltf = json.loads(raw[20:20 + n].decode("utf-8"))
    binary = b""
    if 20 + n < len(raw):
        m, kind = struct.unpack("<II", raw[20 + n:28 + n])
        assert kind == 0x004E4942 and m % 4 == 0 and 28 + n + m == len(raw)
        binary = raw[28 + n:]
        assert gltf["buffers"] == [{"byteLength": m}] or gltf["buffers"][0]["byteLength"] <= m
    return gltf, binary


def _accessor(gltf, binary, k):
    a = gltf["accessors"][k]
    bv = gltf["bufferViews"][a["bufferView"]]
    dt, width = {5126: ("<f4", 4), 5121: ("u1", 1), 5123: ("<u2", 2), 5125: ("<u4", 4)}[a["componentType"]]
    comps = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}[a["type"]]
    off = bv["byteOffset"] + a.get("byteOffset", 0)
    assert off % width == 0 and off + a["count"] * comps * width <= bv["byteOffset"] + bv["byteLength"] <= len(binary)
    return np.frombuffer(binary, dtype=dt, count=a["count"] * comps, offset=off).reshape(a["count"], comps), a, bv


def test_write_mesh_glb_parses_back(tmp_path):
    mesh, vert, nrm, col, faces = _mesh_of("torus")
    path = str(tmp_path / "m.glb")
    postprocess.write_mesh_glb(path, mesh)
    gltf, binary = _read_glb(path)
    assert gltf["nodes"] == [{"matrix": [float(v) for v in np.asarray(mesh.transform).T.reshape(-1)], "mesh": 0}]
    prims = gltf["meshes"][0]["primitives"]
    assert prims == [{"attributes": {"POSITION": 0, "NORMAL": 1, "COLOR_0": 2}, "indices": 3, "mode": 4}] and "materials" not in gltf
    pos, a, bv = _accessor(gltf, binary, 0)
    assert pos.tobytes() == vert.tobytes() and a["count"] == len(vert) and bv["target"] == 34962
    assert a["min"] == [float(v) for v in vert.min(0)] and a["max"] == [float(v) for v in vert.max(0)]
    assert _accessor(gltf, binary, 1)[0].tobytes() == nrm.tobytes()
    rgba, a, _ = _accessor(gltf, binary, 2)
    assert a["normalized"] is True and (rgba[:, :3] == col).all() and (rgba[:, 3] == 255).all()
    idx, a, bv = _accessor(gltf, binary, 3)
    assert a["count"] == 3 * len(faces) and bv["target"] == 34963 and idx.reshape(-1, 3).tolist() == faces.tolist()
    assert idx.min() == 0 and idx.max() == len(vert) - 1
    # with the cameras: the same mesh primitive first, then write_glb's pyramids under the same node
    postprocess.write_mesh_glb(path, mesh, cameras=True, camera_scale=0.1)
    g2, b2 = _read_glb(path)
    assert g2["nodes"] == gltf["nodes"] and g2["meshes"][0]["primitives"][0] == prims[0] and len(g2["meshes"][0]["primitives"]) == 1 + 3
    assert b2[:len(binary)] == binary and g2["materials"] == [{"doubleSided": True}]
    want = postprocess.camera_frusta(mesh.extrinsic.numpy(), 0.1 * 1.5).astype(np.float32)
    for i, prim in enumerate(g2["meshes"][0]["primitives"][1:]):
        assert prim["mode"] == 4 and prim["material"] == 0
        p, a, _ = _accessor(g2, b2, prim["attributes"]["POSITION"])
        assert p.tobytes() == want[i].tobytes() and a["min"] == [float(v) for v in want[i].min(0)]
        c = _accessor(g2, b2, prim["attributes"]["COLOR_0"])[0]
        assert (c == np.array(postprocess.CAMERA_COLORS[i] + (255,), np.uint8)).all()
        assert _accessor(g2, b2, prim["indices"])[0].reshape(-1).tolist() == list(postprocess._FRUSTUM_FACES)
    # the same cameras as write_glb writes for a cloud with this transform, extrinsic and scale
    cloud = postprocess.PointCloud(mesh.vertices, mesh.colors, None, mesh.scene_scale, mesh.transform, mesh.extrinsic)
    cpath = str(tmp_path / "c.glb")
    postprocess.write_glb(cpath, cloud, cameras=True, camera_scale=0.1)
    g3, b3 = _read_glb(cpath)
    assert g3["nodes"] == g2["nodes"]
    p3 = _accessor(g3, b3, g3["meshes"][0]["primitives"][1]["attributes"]["POSITION"])[0]
    assert p3.tobytes() == want[0].tobytes()
    no_cam = postprocess.Mesh(mesh.vertices, mesh.faces, mesh.normals, mesh.colors, mesh.transform)
    with pytest.raises(ValueError):
        postprocess.write_mesh_glb(path, no_cam, cameras=True)
    empty = postprocess.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.uint8), np.eye(4))
    postprocess.write_mesh_glb(path, empty)
    g0, b0 = _read_glb(path)
    assert "meshes" not in g0 and b0 == b"" and g0["nodes"] == [{"matrix": [float(v) for v in np.eye(4).reshape(-1)]}]
