"""Voxel-grid decimation on the MI355X (ovg_voxel_downsample through postprocess.voxel_downsample) against the numpy twin
(tests/voxelgrid_twin.py), bit for bit: the kept indices in order and the copied point / colour bytes; on real selections of the golden
point-cloud cases; the grid's properties; determinism, the overflow flag and the 64 x 518^2 size inside the queried workspace."""
import json
import os

import numpy as np
import pytest
import torch

import common
import voxelgrid_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
FULL = 64 * 518 * 518


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cloud(pts, col=None, scale=1.0, indices=None):
    pts = np.asarray(pts, F).reshape(-1, 3)
    if col is None:
        col = (np.arange(3 * len(pts), dtype=np.int64).reshape(-1, 3) * 7 % 256).astype(np.uint8)
    return postprocess.PointCloud(_dev(pts), _dev(col), torch.zeros((), device="cuda"), torch.tensor(scale, device="cuda", dtype=torch.float32),
                                  np.eye(4), torch.eye(4, device="cuda")[:3][None], None if indices is None else _dev(indices))


def _check(cloud, out, want, name):
    """out is exactly the rows `want` of cloud: indices in order, point and colour bytes."""
    got = out.indices.cpu().numpy() if cloud.indices is None else None
    pts, col = cloud.points.cpu().numpy(), cloud.colors.cpu().numpy()
    if got is not None:
        assert got.dtype == np.int64 and np.array_equal(got, want), name
    assert len(out) == len(want), name
    assert out.points.cpu().numpy().tobytes() == np.ascontiguousarray(pts[want]).tobytes(), name
    assert out.colors.cpu().numpy().tobytes() == np.ascontiguousarray(col[want]).tobytes(), name


def _random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    pts = (rng.standard_normal((n, 3)) * F(1.5)).astype(F)
    conf = (F(1.0) + np.floor(rng.random(n, dtype=F) * F(16.0)) / F(4.0)).astype(F)      # quantised: many ties inside a cell
    return pts, conf


def test_random_cloud_matches_twin_bit_exactly():
    L.require_gpu()
    n = 300_000
    pts, conf = _random_cloud(n, 1)
    conf[::97] = np.nan
    conf[5::101] = -conf[5::101]
    cloud = _cloud(pts, scale=3.25)
    scale = cloud.scene_scale.cpu().numpy()
    for v in (0.05, 0.2, 0.8):
        for c in (None, conf):
            want = twin.downsample(pts, F(v), c)
            assert 0 < len(want) < n                                      # many cells hold several points
            out = postprocess.voxel_downsample(cloud, voxel_size=v, conf=None if c is None else _dev(c))
            _check(cloud, out, want, ("voxel_size", v, c is not None))
            out = postprocess.voxel_downsample(cloud, voxel_size=torch.tensor(v, device="cuda"), conf=None if c is None else _dev(c))
            _check(cloud, out, want, ("voxel_size tensor", v, c is not None))
            if c is not None:
                assert out.conf.cpu().numpy().tobytes() == c[want].tobytes()
    for rel in (0.01, 0.037, 0.2):
        want = twin.downsample(pts, twin.voxel_from_rel(rel, scale), conf)
        out = postprocess.voxel_downsample(cloud, rel_size=rel, conf=_dev(conf))
        _check(cloud, out, want, ("rel_size", rel))
        assert out.scene_scale is cloud.scene_scale and out.transform is cloud.transform and out.extrinsic is cloud.extrinsic


def test_face_hits_duplicates_and_non_finite_entries():
    L.require_gpu()
    rng = np.random.default_rng(2)
    n = 50_000
    # coordinates on a lattice of step 1/8 with voxel edges 1/8, 1/4, 3/8: every quotient is an exact integer (all face hits) or not
    pts = (rng.integers(-64, 64, (n, 3)).astype(F) / F(8.0)).astype(F)
    pts[1000:2000] = pts[:1000]                                           # exact duplicates
    pts[rng.integers(0, n, 500), rng.integers(0, 3, 500)] = np.nan
    pts[rng.integers(0, n, 500), rng.integers(0, 3, 500)] = np.inf
    pts[rng.integers(0, n, 500), rng.integers(0, 3, 500)] = -np.inf
    pts[0] = np.nan                                                       # the first point is invalid
    conf = np.floor(rng.random(n) * 4).astype(F)
    conf[rng.integers(0, n, 2000)] = np.nan
    conf[rng.integers(0, n, 500)] = -0.0
    conf[rng.integers(0, n, 500)] = np.inf
    cloud = _cloud(pts)
    for v in (0.125, 0.25, 0.375, 0.1, 1.0 / 3.0, 100.0):
        for c in (None, conf):
            want = twin.downsample(pts, F(v), c)
            out = postprocess.voxel_downsample(cloud, voxel_size=v, conf=None if c is None else _dev(c))
            _check(cloud, out, want, (v, c is not None))
            assert np.isfinite(out.points.cpu().numpy()).all()
    for bad in (np.full((10, 3), np.nan, F), np.array([[np.inf, 0, 0]], F)):
        out = postprocess.voxel_downsample(_cloud(bad), voxel_size=1.0)
        assert len(out) == 0 and out.indices.numel() == 0
    one = postprocess.voxel_downsample(_cloud([[1e30, -1e30, 0.5]]), voxel_size=1e-3)
    assert one.indices.tolist() == [0]
    empty = postprocess.voxel_downsample(_cloud(np.zeros((0, 3), F)), rel_size=0.5)
    assert len(empty) == 0


def test_on_real_selections_of_the_golden_cases():
    L.require_gpu()
    g = dict(np.load(os.path.join(common.GOLD, "pointcloud.npz")))
    cases = json.loads(str(g["cases"]))
    used = 0
    for i, case in enumerate(cases):
        if case["mode"] == "Predicted Depth" or case["empty"]:
            continue
        p, m = "c%d_" % i, case["map"]
        world = g[m + "_world_points"]
        pred = {"world_points": _dev(world)[None], "world_points_conf": _dev(g[m + "_world_points_conf"])[None],
                "images": _dev(g[m + "_images"])[None], "extrinsic": _dev(g[m + "_extrinsic"])[None]}
        sky = g.get(p + "sky")
        kw = dict(conf_thres=case["conf_thres"], filter_by_frames=case["filter_by_frames"], mask_black_bg=case["mask_black_bg"],
                  mask_white_bg=case["mask_white_bg"], prediction_mode=case["mode"], sky_mask=None if sky is None else _dev(sky))
        cloud = postprocess.predictions_to_point_cloud(pred, return_conf=True, return_indices=True, **kw)
        plain = postprocess.predictions_to_point_cloud(pred, return_indices=True, **kw)
        assert plain.conf is None and torch.equal(plain.points, cloud.points) and torch.equal(plain.indices, cloud.indices)
        idx = cloud.indices.cpu().numpy()
        assert np.array_equal(idx, g[p + "indices"].astype(np.int64)), case["name"]
        cf = g[m + "_world_points_conf"].reshape(-1).astype(F)
        if sky is not None:
            with np.errstate(invalid="ignore"):
                cf = cf * (sky.reshape(-1) > 0.1).astype(F)
        conf_h = cloud.conf.cpu().numpy()
        assert conf_h.dtype == F and np.array_equal(conf_h, cf[idx], equal_nan=True), case["name"]
        pts_h = cloud.points.cpu().numpy()
        scale = cloud.scene_scale.cpu().numpy()
        for rel in (0.02, 0.1):
            if not scale > 0:                                             # a selection of one point (or of equal points) has no scale:
                with pytest.raises(ValueError, match="positive"):         # rel_size gives no usable edge, an absolute one works
                    postprocess.voxel_downsample(cloud, rel_size=rel, conf=cloud.conf)
                want = twin.downsample(pts_h, F(rel), conf_h)
                out = postprocess.voxel_downsample(cloud, voxel_size=rel, conf=cloud.conf)
            else:
                want = twin.downsample(pts_h, twin.voxel_from_rel(rel, scale), conf_h)
                out = postprocess.voxel_downsample(cloud, rel_size=rel, conf=cloud.conf)
            _check(cloud, out, want, (case["name"], rel))
            comp = out.indices.cpu().numpy()
            assert np.array_equal(comp, idx[want]), case["name"]           # composed with the selection's pixel indices
            assert world.reshape(-1, 3)[comp].tobytes() == out.points.cpu().numpy().tobytes(), case["name"]
            assert np.array_equal(out.conf.cpu().numpy(), conf_h[want], equal_nan=True)
            assert len(want) <= len(idx)
        used += 1
    assert used >= 10


def test_grid_properties():
    L.require_gpu()
    pts, conf = _random_cloud(200_000, 3)
    cloud = _cloud(pts)
    v = F(0.3)
    out = postprocess.voxel_downsample(cloud, voxel_size=float(v), conf=_dev(conf))
    keep = out.indices.cpu().numpy()
    _, _, c = twin.cells(pts, v)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    assert np.all(np.diff(keep) > 0) and keep.min() >= 0 and keep.max() < len(pts)      # a subsequence of the input
    assert len(np.unique(key[keep])) == len(keep)                         # no two outputs share a cell
    assert np.array_equal(np.unique(key[keep]), np.unique(key))           # every occupied cell appears once
    assert out.points.cpu().numpy().tobytes() == pts[keep].tobytes()
    # a voxel below the smallest spacing returns the input unchanged: a lattice of step 1/4 sampled without repetition, edge 1/8
    rng = np.random.default_rng(4)
    cells = rng.choice(64 ** 3, 100_000, replace=False)
    lat = (np.stack([cells % 64, cells // 64 % 64, cells // 4096], 1).astype(F) / F(4.0) - F(8.0)).astype(F)
    lc = _cloud(lat)
    same = postprocess.voxel_downsample(lc, voxel_size=0.125, conf=_dev(rng.random(len(lat), dtype=F)))
    assert np.array_equal(same.indices.cpu().numpy(), np.arange(len(lat))) and torch.equal(same.points, lc.points)
    assert torch.equal(same.colors, lc.colors)


def test_overflow_raises_value_error_and_bad_device_voxel():
    L.require_gpu()
    pts, _ = _random_cloud(10_000, 5)
    cloud = _cloud(pts)
    with pytest.raises(ValueError, match="2\\^21"):
        postprocess.voxel_downsample(cloud, voxel_size=1e-7)              # ~1e8 cells along an axis
    with pytest.raises(twin.Overflow):
        twin.downsample(pts, F(1e-7))
    with pytest.raises(ValueError, match="positive"):
        postprocess.voxel_downsample(cloud, voxel_size=torch.tensor(0.0, device="cuda"))
    flat = _cloud(np.ones((100, 3), F), scale=0.0)                        # a degenerate scene: rel_size * 0 is not a usable edge
    with pytest.raises(ValueError, match="positive"):
        postprocess.voxel_downsample(flat, rel_size=0.1)
    out = postprocess.voxel_downsample(cloud, voxel_size=0.5)             # the same cloud still works afterwards
    assert np.array_equal(out.indices.cpu().numpy(), twin.downsample(pts, F(0.5)))


def test_full_size_within_queried_workspace_deterministic_and_exact():
    """64 x 518^2 points through the raw entry with a workspace of exactly the queried size between two guard regions; two runs give
    equal bytes; the kept set equals the twin's."""
    L.require_gpu()
    n = FULL
    gen = torch.Generator(device="cuda").manual_seed(9)
    pts = torch.randn(n, 3, device="cuda", generator=gen) * 2.0
    conf = torch.floor(torch.rand(n, device="cuda", generator=gen) * 32.0) / 4.0
    col = torch.randint(0, 256, (n, 3), device="cuda", generator=gen, dtype=torch.uint8)
    need = ops.voxel_downsample_workspace_bytes(n)
    guard = 1 << 20
    buf = torch.full((need + 2 * guard,), 0xA5, device="cuda", dtype=torch.uint8)
    ws = buf[guard:guard + need]
    voxel = torch.tensor(0.08, device="cuda")
    runs = []
    for _ in range(2):
        count = torch.empty(2, device="cuda", dtype=torch.int64)
        args = dict(points=pts, voxel=voxel, ws=ws, conf=conf, colors=col)
        ops.voxel_downsample(L.VG_COUNT, out_count=count, **args)
        kept, flags = count.cpu().tolist()
        assert flags == 0 and 0 < kept < n
        op, oc, oi = (torch.empty(kept, 3, device="cuda"), torch.empty(kept, 3, device="cuda", dtype=torch.uint8),
                      torch.empty(kept, device="cuda", dtype=torch.int64))
        ops.voxel_downsample(L.VG_SCATTER, capacity=kept, out_points=op, out_colors=oc, out_index=oi, **args)
        runs.append((op, oc, oi))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())     # nothing outside the queried bytes
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    op, oc, oi = runs[0]
    assert torch.equal(op, pts[oi]) and torch.equal(oc, col[oi])
    want = twin.downsample(pts.cpu().numpy(), F(0.08), conf.cpu().numpy())
    assert np.array_equal(oi.cpu().numpy(), want)
