"""Farthest-point sampling, host side: the numpy twin (tests/fps_twin.py) against the indices recorded from the reference's
farthest_point_sample (tests/golden/fps_reference.npz, written by tools/gen_fps_golden.py) and on crafted inputs that pin every clause
of the rule, the C ABI without a device (struct layout, the workspace query, argument checks that return before any HIP call) and the
Python API's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import fps_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
GOLDEN = os.path.join(common.ROOT, "tests", "golden", "fps_reference.npz")
F = np.float32
FAR = F(1e10)


def test_twin_reproduces_the_reference_indices():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    for name in ("small", "large"):
        xyz, npoint = g[name + "_xyz"], int(g[name + "_npoint"])
        assert xyz.dtype == F and xyz.shape[0] == 3 and npoint <= xyz.shape[1]
        for key, ends in (("_index", False), ("_index_ends", True)):
            want = g[name + key].astype(np.int32)
            idx, sq, dist = twin.sample(xyz, npoint, include_last=ends)
            assert idx.dtype == np.int32 and idx.tobytes() == want.tobytes(), (name, key, int((idx != want).sum()))
            assert (idx[:, 0] == 0).all() and (not ends or (idx[:, 1] == xyz.shape[1] - 1).all())
    # the cases are not empty: the lattice cloud has exact ties, the duplicate cloud runs out of distinct points and repeats index 0
    small = g["small_index"].astype(np.int32)
    assert len(np.unique(small[0])) == 300 and len(np.unique(small[2])) == 100 and (small[2][100:] == 0).all()
    lat = g["small_xyz"][1]
    assert len(np.unique(lat, axis=0)) < 300 and (small[1][len(np.unique(lat, axis=0)):] == 0).all()


def test_twin_invariants_on_the_scene():
    """sqdist never increases after the forced samples, nothing repeats while distinct usable points remain, unusable points are never
    chosen and keep a distance of +inf, and with npoint = N every usable point ends at distance 0."""
    B, N, npoint = 3, 700, 700
    pts, val = twin.scene(B, N, seed=2)
    ok = twin.usable(pts, val)
    assert (~ok).any() and ok.any() and (val == 0).any() and not np.isfinite(pts).all()
    for ends, first in ((False, 0), (True, 0), (False, 5), (True, 17)):
        idx, sq, dist = twin.sample(pts, npoint, val, first=first, include_last=ends)
        forced = 2 if ends else 1
        assert (idx[:, 0] == first).all() and (not ends or (idx[:, 1] == N - 1).all()) and (sq[:, 0] == FAR).all()
        for b in range(B):
            free = idx[b, forced:]
            assert ok[b, free].all() and (np.diff(sq[b, forced:].astype(np.float64)) <= 0).all()
            distinct = len(np.unique(pts[b][ok[b]], axis=0))
            head = idx[b, :min(npoint, distinct - forced)]                   # forced samples may be unusable or duplicates of each other
            assert len(np.unique(head[forced:])) == len(head[forced:])
            assert (sq[b, forced:forced + 8] > 0).all()
            assert np.isposinf(dist[b][~ok[b]]).all() and (dist[b][ok[b]] <= FAR).all()
            assert (dist[b][ok[b]] == 0).all()                               # npoint = N: every distinct usable point was sampled
    # a saturated scene point exists: farther than 1e5 from everything, its first sqdist is exactly 1e10
    idx, sq, dist = twin.sample(pts, 40, val)
    assert (sq[:, 1] == FAR).any()


def test_twin_crafted_inputs():
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -3], [2e5, 0, 0], [1e20, 0, 0]], F)
    idx, sq, dist = twin.sample(p, 9)
    # 2e5 and 1e20 both saturate at 1e10 and tie: the lower index first; then (0,0,-3) d=9, (0,2,0) d=4, (1,0,0) d=1, then repeats of 0
    assert idx.tolist() == [0, 7, 8, 6, 3, 1, 0, 0, 0]
    assert sq.tolist() == [1e10, 1e10, 1e10, 9, 4, 1, 0, 0, 0] and sq.dtype == F
    assert np.isposinf(dist[[4, 5]]).all() and (dist[[0, 1, 2, 3, 6, 7, 8]] == 0).all()
    idx, sq, dist = twin.sample(p, 3, first=4)                               # a forced unusable first sample updates nothing
    assert idx.tolist() == [4, 0, 7] and sq.tolist() == [1e10, 1e10, 1e10] and dist[1] == 1
    idx, sq, dist = twin.sample(p[:6], 4, include_last=True)                 # a forced unusable last sample
    assert idx.tolist() == [0, 5, 3, 1] and sq.tolist() == [1e10, 1e10, 4, 1]
    idx, sq, dist = twin.sample(p[:4], 3, include_last=True)
    assert idx.tolist() == [0, 3, 1] and sq.tolist() == [1e10, 4, 1]          # the second sample's sqdist is its distance to the first
    idx, sq, dist = twin.sample(p[4:6], 3)                                   # nothing usable: the forced first, then -1 / +inf
    assert idx.tolist() == [0, -1, -1] and sq[0] == FAR and np.isposinf(sq[1:]).all() and np.isposinf(dist).all()
    idx, sq, dist = twin.sample(p, 4, valid=np.array([0, 0, 1, 0, 1, 1, 0, 0, 0], np.uint8))    # one usable point
    assert idx.tolist() == [0, 2, 2, 2] and sq.tolist() == [1e10, 1e10, 0, 0] and dist[2] == 0 and np.isposinf(np.delete(dist, 2)).all()
    idx, sq, dist = twin.sample(np.ones((5, 3), F), 4)                       # all duplicates: the lowest index repeats
    assert idx.tolist() == [0, 0, 0, 0] and sq.tolist() == [1e10, 0, 0, 0]
    idx, sq, dist = twin.sample(p[:1], 2, include_last=True)                 # N = 1: both forced samples are point 0
    assert idx.tolist() == [0, 0] and sq.tolist() == [1e10, 0]
    # batch = a loop over the clouds
    pts, val = twin.scene(2, 90, seed=3)
    both = twin.sample(pts, 30, val, first=3, include_last=True)
    for b in range(2):
        one = twin.sample(pts[b], 30, val[b], first=3, include_last=True)
        assert all(x[b].tobytes() == y.tobytes() for x, y in zip(both, one))


def test_ctypes_struct_layout_matches_c_fps():
    enums, _ = abi_layout.check({"ovg_fps_params": L.FpsParams},
                                ["OVG_FPS_SMALL_MAX", "OVG_FPS_TILE", "OVG_FPS_INCLUDE_LAST", "OVG_FPS_PATH_AUTO", "OVG_FPS_PATH_ONE_WORKGROUP",
                                 "OVG_FPS_PATH_PER_STEP", "OVG_ABI_VERSION"])
    assert enums == [L.FPS_SMALL_MAX, L.FPS_TILE, L.FPS_INCLUDE_LAST, L.FPS_PATH_AUTO, L.FPS_PATH_ONE_WORKGROUP, L.FPS_PATH_PER_STEP, L.ABI_VERSION]
    assert (L.FPS_INCLUDE_LAST, L.FPS_PATH_AUTO, L.FPS_PATH_ONE_WORKGROUP, L.FPS_PATH_PER_STEP) == (1, 0, 1, 2)
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+ovg_fps_workspace_bytes\s*\(\s*int64_t\s+batch,\s*int64_t\s+n,\s*int64_t\s+npoint\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_farthest_point_sample\s*\(\s*const\s+ovg_fps_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_farthest_point_sample" in L.SYMBOLS and "ovg_fps_workspace_bytes" in L.SYMBOLS


def test_fps_workspace_query_and_argument_validation_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    q = lib.ovg_fps_workspace_bytes
    top = (1 << 31) - 1
    for b, n, m in ((1, 1, 1), (1, 2, 1), (3, 7, 5), (8, 8192, 1024), (1, 268324, 2048), (1, 1 << 20, 4096), (65535, top, top), (2, 1, top)):
        assert q(b, n, m) == b * ((4 * n + 8 * (m + 1) + 15) // 16 * 16), (b, n, m)
    assert q(1, 1, 1) == 32 and q(1, 3, 1) == 32 and q(1, 5, 1) == 48 and q(3, 5, 1) == 144
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4), (4, -1, 4), (4, 4, -1), (65536, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 31),
                (1 << 40, 1 << 40, 1 << 40), (-(1 << 62), 1, 1), ((1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1)):
        assert q(*bad) == -1, bad
    assert ops.fps_workspace_bytes(8, 8192, 1024) == 8 * (4 * 8192 + 8 * 1025 + 8)
    for bad in ((0, 1, 1), (1, 1 << 31, 1), (1 << 70, 1, 1)):
        with pytest.raises(L.OvgError):
            ops.fps_workspace_bytes(*bad)

    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks

    def run(**kw):
        p = L.FpsParams(points=big, valid=big, batch=2, n=1000, npoint=100, first=0, flags=0, path=0, ws=big, ws_bytes=q(2, 1000, 100),
                        index=big, sqdist=big, distance=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_farthest_point_sample(ctypes.byref(p), None)

    assert lib.ovg_farthest_point_sample(None, None) == -1
    for bad in (dict(points=None), dict(ws=None), dict(index=None), dict(sqdist=None),
                dict(batch=0), dict(batch=-1), dict(batch=65536, ws_bytes=1 << 50), dict(n=0), dict(n=-7), dict(n=1 << 31, ws_bytes=1 << 50),
                dict(n=1 << 62, ws_bytes=1 << 62), dict(n=-(1 << 63)), dict(npoint=0), dict(npoint=-1), dict(npoint=1 << 31, ws_bytes=1 << 50),
                dict(first=-1), dict(first=1000), dict(first=1 << 40), dict(first=-(1 << 63)),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(path=3), dict(path=-1), dict(path=1 << 30),
                dict(path=L.FPS_PATH_ONE_WORKGROUP, n=L.FPS_SMALL_MAX + 1, ws_bytes=1 << 30),
                dict(ws_bytes=q(2, 1000, 100) - 1), dict(ws_bytes=q(1, 1000, 100)), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8),
                dict(ws=big + 4), dict(points=big + 2), dict(index=big + 2), dict(sqdist=big + 3), dict(distance=big + 1)):
        assert run(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    x = torch.zeros(2, 5, 3)
    for kw in (dict(xyz=torch.zeros(5, 4)), dict(xyz=torch.zeros(5, 3, dtype=torch.float64)), dict(xyz=np.zeros((5, 3), F)),
               dict(xyz=torch.zeros(3)), dict(xyz=torch.zeros(1, 2, 5, 3)), dict(npoint=6), dict(npoint=-1), dict(npoint=2.0), dict(npoint=True),
               dict(valid=torch.ones(5, dtype=torch.bool)), dict(valid=torch.ones(2, 5)), dict(valid=np.ones((2, 5), bool)),
               dict(first=5), dict(first=-1), dict(first=1.0),
               dict(xyz=torch.zeros(1, 3), npoint=1, include_ends=True), dict(xyz=torch.zeros(0, 3), npoint=0, include_ends=True)):
        with pytest.raises(ValueError):
            postprocess.farthest_point_sample(**dict(dict(xyz=x, npoint=3), **kw))
    for kw in (dict(), dict(valid=torch.ones(2, 5, dtype=torch.bool)), dict(xyz=torch.zeros(5, 3), include_ends=True), dict(npoint=0),
               dict(xyz=torch.zeros(0, 3), npoint=0), dict(return_distance=True, first=4)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.farthest_point_sample(**dict(dict(xyz=x, npoint=3), **kw))
    with pytest.raises(L.OvgError):
        ops.farthest_point_sample(x, 3)                                     # CPU tensors at the thin wrapper as well
    cloud = postprocess.PointCloud(torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8), None, None, None, None)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.farthest_point_sample(cloud, 2)                         # a PointCloud is taken by its points
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.farthest_point_downsample(cloud, 2)
    with pytest.raises(ValueError):
        postprocess.farthest_point_downsample(cloud, 6)
    r = postprocess.FPSResult(torch.tensor([1, -1], dtype=torch.int32), torch.tensor([0.5, float("inf")]))
    assert r.index.tolist() == [1, -1] and r.sqdist[0] == 0.5 and r.distance is None
