"""Nearest-neighbour search, host side: the numpy twin (tests/nn_twin.py) against scipy's k-d tree (the library the reference's
find_reciprocal_matches calls) and on crafted inputs that pin every clause of the rule, the C ABI without a device (struct layout,
the workspace query, argument checks that return before any HIP call) and the Python API's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import nn_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def _d64(a, b):
    return np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1))


def test_twin_agrees_with_ckdtree_on_the_reference_contract():
    """P1 5000 and P2 4097 uniform points in [-2, 2)^3. An index may differ from the tree's only where the two candidates are within
    1e-6 relative in float64, at most 0.1 % of the queries may, and the reciprocal flags agree wherever the indices do. The
    reciprocity rule is written here on its own (the tree's indices through the reference's expression)."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    P1 = rng.random((5000, 3)).astype(F) * 4 - 2
    P2 = rng.random((4097, 3)).astype(F) * 4 - 2
    d12, nn1_in_P2 = cKDTree(P2).query(P1)
    d21, nn2_in_P1 = cKDTree(P1).query(P2)
    rec_tree = nn1_in_P2[nn2_in_P1] == np.arange(len(nn2_in_P1))
    assert (nn2_in_P1[nn1_in_P2] == np.arange(len(nn1_in_P2))).sum() == rec_tree.sum()

    rec, got21, count = twin.reciprocal(P1, P2)
    got12, sq12 = twin.nearest(P1, P2)
    assert got21.dtype == np.int32 and rec.dtype == bool and count == int(rec.sum()) and 0 < count < len(P2)
    mismatches = 0
    for got, want, q, r in ((got12, nn1_in_P2, P1, P2), (got21, nn2_in_P1, P2, P1)):
        diff = np.nonzero(got != want)[0]
        mismatches += len(diff)
        a, b = _d64(q[diff], r[got[diff]]), _d64(q[diff], r[want[diff]])
        assert (np.abs(a - b) <= 1e-6 * np.maximum(a, b)).all()
        assert len(diff) <= 1e-3 * len(q)
    same = (got21 == nn2_in_P1) & (got12[np.maximum(got21, 0)] == nn1_in_P2[nn2_in_P1])
    assert (rec[same] == rec_tree[same]).all()
    rel = np.abs(np.sqrt(sq12.astype(np.float64)) - d12) / d12
    print("index mismatches %d, flag mismatches %d, count %d / %d, max relative distance error %.2e"
          % (mismatches, int((rec != rec_tree).sum()), count, int(rec_tree.sum()), rel.max()))
    assert rel.max() <= 1e-6                                                 # a float32 sum of three squares against float64
    if mismatches == 0:
        assert (rec == rec_tree).all() and count == int(rec_tree.sum())


def test_twin_ties_on_a_lattice_go_to_the_lowest_index():
    """Coordinates k / 4, |k| <= 8: every difference, square and sum is exact in float32, so equal distances are exact ties. The
    tree breaks them its own way: its DISTANCES must equal the twin's exactly, its indices need not."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(1)
    q = (rng.integers(-8, 9, (5000, 3)) / 4.0).astype(F)
    r = (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    idx, sq = twin.nearest(q, r)
    d_tree, _ = cKDTree(r).query(q)
    assert (np.sqrt(sq.astype(np.float64)) == d_tree).all()
    all_d = ((q[:, None, :].astype(np.float64) - r[None].astype(np.float64)) ** 2).sum(-1)
    ties = (all_d == all_d.min(1, keepdims=True)).sum(1)
    assert (ties > 1).mean() > 0.2                                           # the case is not empty
    assert (idx == (all_d == all_d.min(1, keepdims=True)).argmax(1)).all()   # the first of the equal ones


def test_twin_duplicates_non_finite_masks_overflow_and_exclude_self():
    r = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e20, 0, 0]], F)
    q = np.array([[0.9, 0, 0], [0, 0, 0], [np.nan, 1, 1], [0, -np.inf, 0], [-3e38, 0, 0], [0, 1.0, 0], [1e20, 1e20, 0], [1e20, 1e10, 0]], F)
    idx, sq = twin.nearest(q, r)
    assert idx.tolist() == [1, 0, -1, -1, 0, 0, 0, 7]                        # duplicates 1 / 2 -> 1; (0,1,0) ties 0 and 3 -> 0
    assert sq[0] == F(F(0.9) - F(1)) * F(F(0.9) - F(1)) and sq[1] == 0 and np.isposinf(sq[[2, 3]]).all() and sq[5] == 1
    # every d overflows to +inf and the query is still matched, to the lowest usable index
    assert np.isposinf(sq[[4, 6]]).all() and idx[4] == 0 and idx[6] == 0
    assert sq[7] == F(1e10) * F(1e10) and np.isfinite(sq[7])                 # the one reference at 1e20 is the only finite distance
    # masks: a masked reference is no candidate, a masked query has no result
    rv = np.array([0, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    qv = np.array([1, 1, 1, 1, 1, 0, 1, 1], np.uint8)
    idx, sq = twin.nearest(q, r, qv, rv)
    assert idx.tolist() == [2, 2, -1, -1, 2, -1, 2, 7] and sq[1] == 1 and np.isposinf(sq[5])
    # all references unusable
    idx, sq = twin.nearest(q, r[4:7])
    assert (idx == -1).all() and np.isposinf(sq).all()
    idx, sq = twin.nearest(q, r, None, np.zeros(8, np.uint8))
    assert (idx == -1).all() and np.isposinf(sq).all()
    # inside one cloud: without exclude_self every usable point finds itself (or an earlier duplicate), with it the nearest other
    idx, sq = twin.nearest(r, r)
    assert idx.tolist() == [0, 1, 1, 3, -1, -1, -1, 7] and (sq[[0, 1, 2, 3, 7]] == 0).all()
    idx, sq = twin.nearest(r, r, exclude_self=True)
    assert idx.tolist() == [1, 2, 1, 0, -1, -1, -1, 0] and sq.tolist()[:4] == [1, 0, 0, 4] and np.isposinf(sq[7])
    idx, sq = twin.nearest(r[:1], r[:1], exclude_self=True)
    assert idx.tolist() == [-1] and np.isposinf(sq[0])
    # rows= evaluates a subset with the original indices (exclude_self included)
    idx2, sq2 = twin.nearest(r, r, exclude_self=True, rows=[3, 1], budget=8)
    assert idx2.tolist() == [0, 2] and sq2.tolist() == [4, 0]
    # the chunk size never changes a result
    q, r, qv, rv = twin.scene(300, 211, seed=3)
    a = twin.nearest(q, r, qv, rv)
    b = twin.nearest(q, r, qv, rv, budget=211 * 7)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (a[0] == -1).any() and (a[0] >= 0).any() and np.isposinf(a[1][a[0] >= 0]).any()


def test_twin_reciprocal_never_matches_a_missing_neighbour():
    P1 = np.array([[0, 0, 0], [5, 0, 0], [np.nan, 0, 0]], F)
    P2 = np.array([[0.1, 0, 0], [4, 0, 0], [0.2, 0, 0], [0, np.inf, 0]], F)
    rec, nn2, count = twin.reciprocal(P1, P2)
    assert nn2.tolist() == [0, 1, 0, -1] and rec.tolist() == [True, True, False, False] and count == 2
    rec, nn2, count = twin.reciprocal(P1[2:], P2)
    assert nn2.tolist() == [-1] * 4 and not rec.any() and count == 0
    rec, nn2, count = twin.reciprocal(P1, P2, np.array([0, 1, 1], np.uint8), None)
    assert nn2.tolist() == [1, 1, 1, -1] and rec.tolist() == [False, True, False, False] and count == 1


def test_ctypes_struct_layout_matches_c_nn():
    enums, _ = abi_layout.check({"ovg_nn_params": L.NnParams},
                                ["OVG_NN_QUERY_TILE", "OVG_NN_REFERENCE_TILE", "OVG_NN_EXCLUDE_SAME_INDEX", "OVG_ABI_VERSION"])
    assert enums == [L.NN_QUERY_TILE, L.NN_REFERENCE_TILE, L.NN_EXCLUDE_SAME_INDEX, L.ABI_VERSION]
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+ovg_nn_workspace_bytes\s*\(\s*int64_t\s+nq,\s*int64_t\s+nr\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_nearest_neighbours\s*\(\s*const\s+ovg_nn_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_nearest_neighbours" in L.SYMBOLS and "ovg_nn_workspace_bytes" in L.SYMBOLS


def test_nn_workspace_query_and_argument_validation_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    q = lib.ovg_nn_workspace_bytes
    top = (1 << 31) - 1
    for nq, nr in ((1, 1), (2, 1), (3, 7), (512, 1), (9500, 9500), (1 << 20, 1 << 20), (top, 1), (1, top), (top, top)):
        assert q(nq, nr) == (8 * nq + 15) // 16 * 16, (nq, nr)
    assert q(1, 1) == 16 and q(2, 5) == 16 and q(3, 5) == 32
    for bad in ((0, 1), (1, 0), (-1, 4), (4, -1), (1 << 31, 1), (1, 1 << 31), (1 << 40, 1 << 40), (-(1 << 62), 1), ((1 << 63) - 1, (1 << 63) - 1)):
        assert q(*bad) == -1, bad
    assert ops.nn_workspace_bytes(9500, 4097) == 76000
    for bad in ((0, 1), (1, 1 << 31), (1 << 70, 1)):
        with pytest.raises(L.OvgError):
            ops.nn_workspace_bytes(*bad)

    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks

    def run(**kw):
        p = L.NnParams(query=big, reference=big, query_valid=big, reference_valid=big, nq=1000, nr=1000, flags=0, splits=0,
                       ws=big, ws_bytes=q(1000, 1000), index=big, sqdist=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_nearest_neighbours(ctypes.byref(p), None)

    assert lib.ovg_nearest_neighbours(None, None) == -1
    for bad in (dict(query=None), dict(reference=None), dict(ws=None), dict(index=None), dict(sqdist=None),
                dict(nq=0), dict(nr=0), dict(nq=-1), dict(nr=-7), dict(nq=1 << 31, ws_bytes=1 << 50), dict(nr=1 << 31),
                dict(nq=1 << 62, ws_bytes=1 << 62), dict(nq=-(1 << 63)),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=L.NN_EXCLUDE_SAME_INDEX, nr=999),
                dict(flags=L.NN_EXCLUDE_SAME_INDEX, nq=999), dict(splits=-1), dict(splits=-(1 << 31)),
                dict(ws_bytes=q(1000, 1000) - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8), dict(ws=big + 4),
                dict(query=big + 2), dict(reference=big + 1), dict(index=big + 2), dict(sqdist=big + 3)):
        assert run(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    q, r = torch.zeros(5, 3), torch.zeros(2, 4, 3)
    for kw in (dict(query=torch.zeros(5, 4)), dict(query=torch.zeros(5, 3, dtype=torch.float64)), dict(query=np.zeros((5, 3), F)),
               dict(query=torch.zeros(())), dict(reference=torch.zeros(8, 2)), dict(reference=[[0.0, 0.0, 0.0]]),
               dict(query_valid=torch.ones(4, dtype=torch.bool)), dict(query_valid=torch.ones(5)), dict(query_valid=np.ones(5, bool)),
               dict(reference_valid=torch.ones(8, dtype=torch.bool)), dict(reference_valid=torch.ones(2, 4, dtype=torch.int32)),
               dict(exclude_self=True)):
        with pytest.raises(ValueError):
            postprocess.nearest_neighbours(**dict(dict(query=q, reference=r), **kw))
    for kw in (dict(), dict(query_valid=torch.ones(5, dtype=torch.bool)), dict(reference_valid=torch.ones(2, 4, dtype=torch.uint8)),
               dict(reference=torch.zeros(5, 3), exclude_self=True), dict(query=torch.zeros(0, 3)), dict(reference=torch.zeros(0, 3))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.nearest_neighbours(**dict(dict(query=q, reference=r), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.reciprocal_matches(q, r)
    with pytest.raises(ValueError):
        postprocess.reciprocal_matches(q, torch.zeros(3, 2))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.cloud_distance(q, r)
    for t in (0, -1.0, float("nan"), "x", True):
        with pytest.raises(ValueError):
            postprocess.cloud_distance(q, r, threshold=t)
    with pytest.raises(L.OvgError):
        ops.nearest_neighbours(q, r.reshape(-1, 3))                         # CPU tensors at the thin wrapper as well
    cloud = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, None, None, None)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.nearest_neighbours(cloud, cloud, exclude_self=True)     # a PointCloud is taken by its points
    r = postprocess.NNResult(torch.tensor([1, -1], dtype=torch.int32), torch.tensor([0.5, float("inf")]))
    assert r.index.tolist() == [1, -1] and r.sqdist[0] == 0.5
    d = postprocess.CloudDistance(accuracy=1.0, n_pred=3)
    assert d.accuracy == 1.0 and d.n_pred == 3 and d.fscore is None and "accuracy=1.0" in repr(d)
