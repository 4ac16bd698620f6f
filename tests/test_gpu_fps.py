"""ovg_farthest_point_sample / postprocess.farthest_point_sample and farthest_point_downsample on the device against tests/fps_twin.py:
index, sqdist and distance byte for byte -- shapes around the constants of both forms, every path on the same input, crafted inputs
(ties, duplicates, nothing usable, forced samples on unusable points, saturated and overflowing distances), the cross-check of
distance with the nearest-neighbour kernel, guard bytes behind the workspace and the outputs, the indices recorded from the
reference, a medium case on the per-step form and the down-sampling of a real cloud."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import fps_twin as twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
FAR = F(1e10)
SMALL, TILE = L.FPS_SMALL_MAX, L.FPS_TILE
AUTO, ONE, STEP = L.FPS_PATH_AUTO, L.FPS_PATH_ONE_WORKGROUP, L.FPS_PATH_PER_STEP
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
GOLDEN = os.path.join(common.ROOT, "tests", "golden", "fps_reference.npz")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("index", "sqdist", "distance")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


def _check(pts, npoint, val=None, first=0, include_last=False, paths=(AUTO,), name="", want=None):
    """pts [B, N, 3]: the device result of every path against the twin (or `want`), all three outputs."""
    if want is None:
        want = twin.sample(pts, npoint, val, first=first, include_last=include_last)
    dp, dv = _dev(pts), _dev(val)
    for path in paths:
        got = ops.farthest_point_sample(dp, npoint, dv, first=first, include_last=include_last, path=path, distance=True)
        _same(got, want, "%s path=%d" % (name, path))
    return want


def test_shapes_around_the_constants_match_twin_bit_exactly():
    L.require_gpu()
    assert SMALL >= 2048 and TILE >= 256
    sizes = (1, 2, 63, 65, 1023, 1025, SMALL - 1, SMALL, SMALL + 1, 2 * TILE + 1)
    pts, val = twin.scene(3, max(sizes), seed=0)
    for N in sizes:
        for npoint in sorted({1, min(2, N), min(N, 257)} | ({N} if N <= 1025 else set())):
            for masks in (True, False):
                p, v = np.ascontiguousarray(pts[:, :N]), (np.ascontiguousarray(val[:, :N]) if masks else None)
                want = _check(p, npoint, v, name="B=3 N=%d npoint=%d masks=%d" % (N, npoint, masks))
                _check(p[:1], npoint, None if v is None else v[:1], name="B=1 N=%d npoint=%d masks=%d" % (N, npoint, masks),
                       want=tuple(w[:1] for w in want))
                if N >= 1023 and npoint >= 257:
                    assert (want[1][:, 1:] < FAR).any() and np.isposinf(want[2]).any() and (want[0] >= 0).all()


def test_every_path_gives_identical_bytes():
    L.require_gpu()
    for N, npoint, first, ends, seed in ((SMALL, 300, 0, False, 1), (SMALL - 77, 64, 11, True, 2), (3 * TILE + 5, 200, 7, True, 3), (65, 65, 64, False, 4),
                                         (2, 2, 1, True, 5)):
        pts, val = twin.scene(2, N, seed=seed)
        _check(pts, npoint, val, first=first, include_last=ends, paths=(AUTO, ONE, STEP), name="N=%d" % N)
    # beyond the one-workgroup form: auto is the per-step form
    pts, val = twin.scene(2, SMALL + 1, seed=6)
    _check(pts, 50, val, include_last=True, paths=(AUTO, STEP), name="N=SMALL+1")
    with pytest.raises(L.OvgError, match="OVG_E_ARG"):
        ops.farthest_point_sample(_dev(pts), 50, path=ONE)


def test_crafted_inputs_match_twin():
    L.require_gpu()
    rng = np.random.default_rng(1)
    both = (AUTO, STEP)
    lattice = (rng.integers(-8, 9, (2, 3000, 3)) / 4.0).astype(F)
    want = _check(lattice, 600, paths=both, name="lattice ties")
    assert (np.diff(want[1][:, 1:].astype(np.float64)) == 0).mean() > 0.5   # runs of equal distances: ties decided by index
    want = _check(np.ones((1, 500, 3), F), 20, paths=both, name="all duplicates")
    assert (want[0] == 0).all() and want[1][0].tolist() == [1e10] + [0.0] * 19
    bad = np.full((2, 300, 3), np.nan, F)
    bad[1, :, 1] = np.inf
    want = _check(bad, 5, paths=both, name="nothing usable")
    assert want[0][0].tolist() == [0, -1, -1, -1, -1] and np.isposinf(want[1][:, 1:]).all() and np.isposinf(want[2]).all()
    want = _check(np.zeros((1, 300, 3), F), 5, np.zeros((1, 300), np.uint8), include_last=True, paths=both, name="nothing valid")
    assert want[0][0].tolist() == [0, 299, -1, -1, -1] and want[1][0, :2].tolist() == [1e10, 1e10]
    one = rng.normal(size=(1, 300, 3)).astype(F)
    mask = np.zeros((1, 300), np.uint8)
    mask[0, 123] = 1
    want = _check(one, 4, mask, paths=both, name="one usable point")
    assert want[0][0].tolist() == [0, 123, 123, 123] and want[1][0].tolist() == [1e10, 1e10, 0, 0]
    p = np.array([[[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -3], [2e5, 0, 0], [1e20, 0, 0]]], F)
    want = _check(p, 9, paths=both, name="saturation and overflow")
    assert want[0][0].tolist() == [0, 7, 8, 6, 3, 1, 0, 0, 0] and want[1][0].tolist() == [1e10, 1e10, 1e10, 9, 4, 1, 0, 0, 0]
    _check(p, 3, first=4, paths=both, name="forced first on a NaN point")
    _check(p[:, :6], 4, include_last=True, paths=both, name="forced last on an inf point")
    _check(p, 5, np.array([[0, 1, 1, 1, 1, 1, 1, 1, 0]], np.uint8), include_last=True, paths=both, name="forced samples on masked points")
    _check(p, 6, first=6, paths=both, name="first != 0")
    _check(p[:, :1], 2, include_last=True, paths=both, name="N = 1")
    pts, val = twin.scene(2, 1500, seed=7)
    for first, ends in ((0, True), (1499, False), (700, True)):
        want = _check(pts, 400, val, first=first, include_last=ends, paths=both, name="scene first=%d ends=%d" % (first, ends))
        assert (want[0][:, 0] == first).all() and (not ends or (want[0][:, 1] == 1499).all())
        assert (np.diff(want[1][:, 2:].astype(np.float64), axis=1) <= 0).all()
    # the public entry: one cloud, a batch, bool masks, PointClouds, empty results, no distance unless asked for
    res = postprocess.farthest_point_sample(_dev(pts), 100, valid=_dev(val.astype(bool)), include_ends=True, return_distance=True)
    assert res.index.shape == (2, 100) and res.sqdist.shape == (2, 100) and res.distance.shape == (2, 1500) and res.index.dtype == torch.int32
    _same((res.index, res.sqdist, res.distance), twin.sample(pts, 100, val, include_last=True), "batch")
    res = postprocess.farthest_point_sample(_dev(pts[1]), 100, first=3)
    assert res.index.shape == (100,) and res.distance is None
    _same((res.index, res.sqdist), twin.sample(pts[1], 100, first=3)[:2], "one cloud")
    cloud = postprocess.PointCloud(_dev(pts[0]), None, None, None, None, None)
    _same((postprocess.farthest_point_sample(cloud, 1500).index,), twin.sample(pts[0], 1500)[:1], "PointCloud, npoint = N")
    res = postprocess.farthest_point_sample(_dev(pts), 0, return_distance=True)
    assert res.index.shape == (2, 0) and res.sqdist.shape == (2, 0) and torch.isposinf(res.distance).all() and res.distance.shape == (2, 1500)
    assert postprocess.farthest_point_sample(_dev(pts[0][:0]), 0).index.shape == (0,)


def test_distance_agrees_with_the_nearest_neighbour_kernel():
    L.require_gpu()
    pts, val = twin.scene(2, 5000, seed=8)
    # 5 samples leave points farther than 1e5 from every sample: the clamp at 1e10 is part of the comparison
    for first, ends, path, npoint in ((0, False, ONE, 333), (9, True, STEP, 333), (0, False, AUTO, 5)):
        index, sqdist, distance = ops.farthest_point_sample(_dev(pts), npoint, _dev(val), first=first, include_last=ends, path=path, distance=True)
        for b in range(2):
            p, v, idx = _dev(pts[b]), _dev(val[b]), index[b].long()
            assert bool((idx >= 0).all())
            nn_idx, nn_sq = ops.nearest_neighbours(p, p[idx].contiguous(), v, v[idx].contiguous())
            ok = torch.from_numpy(twin.usable(pts[b], val[b])).cuda()
            want = torch.minimum(nn_sq, torch.full_like(nn_sq, 1e10))
            assert bool(ok.any()) and bool((nn_idx[ok] >= 0).all()) and (npoint > 5 or bool((nn_sq[ok] > 1e10).any()))
            assert torch.equal(distance[b][ok].view(torch.int32), want[ok].view(torch.int32))
            assert bool(torch.isposinf(distance[b][~ok]).all())


def test_nothing_is_written_behind_the_workspace_or_the_outputs():
    L.require_gpu()
    B, N, npoint = 2, 2 * TILE + 3, 101
    pts, val = twin.scene(B, N, seed=9)
    want = twin.sample(pts, npoint, val, include_last=True)
    need = ops.fps_workspace_bytes(B, N, npoint)
    assert need == B * ((4 * N + 8 * (npoint + 1) + 15) // 16 * 16)
    for path in (ONE, STEP, AUTO):
        ws = torch.full((need + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
        index, check_i = guarded((B, npoint), torch.int32, "cuda")
        sqdist, check_s = guarded((B, npoint), torch.float32, "cuda")
        distance, check_d = guarded((B, N), torch.float32, "cuda")
        got = ops.farthest_point_sample(_dev(pts), npoint, _dev(val), include_last=True, path=path, ws=ws[:need], index=index, sqdist=sqdist,
                                        distance=distance)
        torch.cuda.synchronize()
        check_i("index path=%d" % path)
        check_s("sqdist path=%d" % path)
        check_d("distance path=%d" % path)
        assert bool((ws[need:] == 0xA5).all()), path
        _same(got, want, "guarded path=%d" % path)


def test_device_reproduces_the_reference_indices():
    L.require_gpu()
    g = np.load(GOLDEN)
    for name in ("small", "large"):
        xyz, npoint = g[name + "_xyz"], int(g[name + "_npoint"])
        for key, ends in (("_index", False), ("_index_ends", True)):
            want = g[name + key].astype(np.int32)
            for path in (ONE, STEP):
                got = ops.farthest_point_sample(_dev(xyz), npoint, include_last=ends, path=path)[0].cpu().numpy()
                assert got.tobytes() == want.tobytes(), (name, key, path, int((got != want).sum()))
            res = postprocess.farthest_point_sample(_dev(xyz), npoint, include_ends=ends)
            assert res.index.cpu().numpy().tobytes() == want.tobytes()


def test_medium_case_on_the_per_step_form():
    L.require_gpu()
    N, npoint = 200001, 512
    pts, val = twin.scene(1, N, seed=10)
    want = _check(pts, npoint, val, name="medium")                           # auto: the per-step form
    assert N > SMALL and (np.diff(want[1][0, 1:].astype(np.float64)) <= 0).all() and len(np.unique(want[0])) == npoint


def test_downsample_of_a_real_cloud():
    L.require_gpu()
    g = np.load(REAL)
    depth = g["depth"].astype(F)
    pts = ctwin.unproject64(depth, g["extrinsics"][0], g["intrinsics"][0])[0][::4, ::4].reshape(-1, 3).astype(F)
    keep = depth[0][::4, ::4].reshape(-1) > 0
    pts[~keep] = np.nan                                                      # pixels without depth: unusable, never sampled
    M = len(pts)
    rng = np.random.default_rng(11)
    col, conf = rng.integers(0, 256, (M, 3)).astype(np.uint8), rng.random(M).astype(F)
    pix = (np.arange(M) * 16).astype(np.int64)
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0)
    cloud = postprocess.PointCloud(_dev(pts), _dev(col), torch.zeros((), device="cuda"), torch.ones((), device="cuda"), T, _dev(g["extrinsics"][0].astype(F)),
                                   _dev(pix), _dev(conf))
    n = 777
    want = twin.sample(pts, n, first=int(np.nonzero(keep)[0][0]))[0]
    out = postprocess.farthest_point_downsample(cloud, n, first=int(np.nonzero(keep)[0][0]))
    assert len(out) == n and keep[want].all() and len(np.unique(want)) == n
    assert out.points.cpu().numpy().tobytes() == pts[want].tobytes() and out.colors.cpu().numpy().tobytes() == col[want].tobytes()
    assert out.indices.cpu().numpy().tobytes() == pix[want].tobytes() and out.conf.cpu().numpy().tobytes() == conf[want].tobytes()
    assert out.transform is T and out.extrinsic is cloud.extrinsic and out.scene_scale is cloud.scene_scale
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fps.ply")
        postprocess.write_ply(path, out)
        raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex %d\n" % n in head and len(body) == n * 15
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert np.array_equal(rec["xyz"], (pts[want].astype(np.float64) + T[:3, 3]).astype(F)) and np.array_equal(rec["rgb"], col[want])
    # without indices the positions in the input cloud are reported; samples of -1 are dropped
    plain = postprocess.PointCloud(_dev(pts), _dev(col), None, None, T, None)
    out = postprocess.farthest_point_downsample(plain, 5, first=int(np.nonzero(keep)[0][0]))
    assert out.indices.cpu().numpy().tolist() == want[:5].tolist() and out.conf is None
    dead = postprocess.PointCloud(_dev(np.full((10, 3), np.nan, F)), _dev(col[:10]), None, None, T, None)
    out = postprocess.farthest_point_downsample(dead, 4)
    assert len(out) == 1 and out.indices.tolist() == [0] and out.colors.shape == (1, 3)
