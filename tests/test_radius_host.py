"""Radius neighbour search, host side: the brute-force twin (tests/radius_twin.py) on crafted inputs that pin every clause of the
rule, the covering argument as a test (a dictionary grid in numpy built from the restated cell function must equal the brute force),
the C ABI without a device (struct layout, the workspace query, argument checks that return before any HIP call) and the Python
API's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import nn_twin
import radius_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def _same(a, b, name=""):
    for x, y, what in zip(a, b, ("count", "index", "sqdist")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, what, int((x.view(np.int32) != y.view(np.int32)).sum()))


def test_twin_inclusive_boundary_on_the_quarter_lattice():
    """Coordinates k / 4: every difference, square and sum is exact in float32, and radius 0.25 squares to exactly 1 / 16, the
    squared distance of a lattice neighbour. d == radius_sq counts."""
    rng = np.random.default_rng(1)
    q = (rng.integers(-8, 9, (400, 3)) / 4.0).astype(F)
    r = (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    r2 = twin.radius_sq(0.25)
    assert r2 == F(0.0625)
    count, index, sqdist = twin.search(q, r, r2)
    d = ((q[:, None, :].astype(np.float64) - r[None].astype(np.float64)) ** 2).sum(-1)       # exact
    assert (count == (d <= 0.0625).sum(1)).all()
    assert ((sqdist == r2) & (count > 0)).sum() > 20                           # nearest exactly ON the boundary: the case is not empty
    assert (count == (d < 0.0625).sum(1)).mean() < 0.9                         # and a strict bound would give other counts
    hit = count > 0
    assert (index[hit] == (d[hit] == d[hit].min(1, keepdims=True)).argmax(1)).all()          # ties to the lowest index
    assert (index[~hit] == -1).all() and np.isposinf(sqdist[~hit]).all()
    # just below: the boundary neighbours leave
    below = twin.search(q, r, np.nextafter(r2, F(0)))
    assert (below[0] == (d < 0.0625).sum(1)).all()


def test_twin_ties_duplicates_non_finite_masks_overflow_and_exclude_self():
    r = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e20, 0, 0]], F)
    q = np.array([[0.9, 0, 0], [0, 0, 0], [np.nan, 1, 1], [0, -np.inf, 0], [-3e38, 0, 0], [0, 1.0, 0], [1e20, 1e20, 0], [1e20, 1e10, 0]], F)
    count, index, sqdist = twin.search(q, r, F(1.0))
    # (0.9,0,0): 0 (0.81), 1 and 2 (0.01 each: duplicates -> the lower index); (0,1,0) ties 0 and 3 at exactly 1 -> 0
    assert count.tolist() == [3, 3, 0, 0, 0, 2, 0, 0] and index.tolist() == [1, 0, -1, -1, -1, 0, -1, -1]
    assert sqdist[0] == F(F(0.9) - F(1)) * F(F(0.9) - F(1)) and sqdist[1] == 0 and sqdist[5] == 1 and np.isposinf(sqdist[[2, 3, 4, 6, 7]]).all()
    # an overflowing d is never a candidate, whatever the radius: the unbounded search matches these queries (nn_twin), this one does not
    huge = F(3e38)
    count, index, sqdist = twin.search(q, r, huge)
    assert nn_twin.nearest(q, r)[0].tolist() == [1, 0, -1, -1, 0, 0, 0, 7]
    assert index.tolist() == [1, 0, -1, -1, -1, 0, -1, 7] and count.tolist() == [4, 4, 0, 0, 0, 4, 0, 1]
    assert sqdist[7] == F(1e10) * F(1e10)
    # masks: a masked reference is no candidate, a masked query has no result
    rv = np.array([0, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    qv = np.array([1, 1, 1, 1, 1, 0, 1, 1], np.uint8)
    count, index, sqdist = twin.search(q, r, F(1.0), qv, rv)
    assert count.tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and index.tolist() == [2, 2, -1, -1, -1, -1, -1, -1] and sqdist[1] == 1
    # all references unusable
    for got in (twin.search(q, r[4:7], F(1.0)), twin.search(q, r, F(1.0), None, np.zeros(8, np.uint8))):
        assert (got[0] == 0).all() and (got[1] == -1).all() and np.isposinf(got[2]).all()
    # inside one cloud: without exclude_self every usable point counts itself, with it only the others
    count, index, sqdist = twin.search(r, r, F(1.0))
    assert count.tolist() == [3, 3, 3, 1, 0, 0, 0, 1] and index.tolist() == [0, 1, 1, 3, -1, -1, -1, 7]
    count, index, sqdist = twin.search(r, r, F(1.0), exclude_self=True)
    assert count.tolist() == [2, 2, 2, 0, 0, 0, 0, 0] and index.tolist() == [1, 2, 1, -1, -1, -1, -1, -1] and sqdist.tolist()[:3] == [1, 0, 0]
    got = twin.search(r[:1], r[:1], F(1.0), exclude_self=True)
    assert got[0].tolist() == [0] and got[1].tolist() == [-1] and np.isposinf(got[2][0])
    # rows= evaluates a subset with the original indices; the chunk size never changes a result
    sub = twin.search(r, r, F(1.0), exclude_self=True, rows=[2, 0], budget=8)
    assert sub[0].tolist() == [2, 2] and sub[1].tolist() == [1, 1]
    q, r, qv, rv = nn_twin.scene(300, 211, seed=3)
    _same(twin.search(q, r, F(0.25), qv, rv), twin.search(q, r, F(0.25), qv, rv, budget=211 * 7), "chunks")
    # where the unbounded search finds something within the radius, both agree
    count, index, sqdist = twin.search(q, r, F(0.25), qv, rv)
    ni, ns = nn_twin.nearest(q, r, qv, rv)
    inside = (ni >= 0) & (ns <= F(0.25))
    assert inside.any() and (~inside).any() and (index[inside] == ni[inside]).all() and (sqdist[inside] == ns[inside]).all()
    assert (count[~inside] == 0).all() and (index[~inside] == -1).all()


def test_reach_and_cell_function():
    for r2 in (F(0.0625), F(0.25), F(1.0), F(2.0 ** -100), F(3e38), F(0.01), twin.radius_sq(0.05)):
        R = twin.reach(r2)
        v = np.sqrt(np.float64(r2)) * (1 + 2.0 ** -20)
        assert R.dtype == F and np.float64(R) > v and np.float64(np.nextafter(R, F(0))) <= v
        assert ops.radius_reach(float(r2)) == float(R)
    assert twin.reach(F(0.0625)) > F(0.25) and twin.reach(F(0.0625)) < F(0.2500004)
    c = twin.cells(np.array([[0, -0.0, 0.25], [-1e-30, 0.2499, -0.25], [1e20, -1e20, np.inf], [-np.inf, 262143.9, 262144.0]], F), (0, 0, 0), 0.25)
    assert c.tolist() == [[0, 0, 1], [-1, 0, -1], [2 ** 20 - 1, -2 ** 20, 2 ** 20 - 1], [-2 ** 20, 2 ** 20 - 1, 2 ** 20 - 1]]
    assert twin.cells(np.array([[1000.5, 16384.25, -3.0]], F), (1000, 16384, -3), 0.25).tolist() == [[2, 1, 0]]
    x = np.sort(np.random.default_rng(0).normal(0, 50, 4000).astype(F))
    cx = twin.cells(np.stack([x, x, x], 1), (0.3, -7, 1e3), 0.37)
    assert (np.diff(cx, axis=0) >= 0).all()                                    # monotone
    k = twin.pack(np.array([[-2 ** 20, -2 ** 20, -2 ** 20], [2 ** 20 - 1, 2 ** 20 - 1, 2 ** 20 - 1], [0, 0, 1]]))
    assert k.tolist() == [0, 2 ** 63 - 1, (1 << 62) | (1 << 41) | ((1 << 20) + 1)]


def _grid_search(q, r, r2, cell, origin, qv=None, rv=None, exclude_self=False):
    """The search THROUGH a grid, in numpy and dictionaries: bin the usable references by the restated cell function, and give every
    query only the references in the cells of its box. -> (count, index, sqdist, largest box)."""
    q_ok, r_ok = nn_twin.usable(q, qv), nn_twin.usable(r, rv)
    grid = {}
    for j in np.nonzero(r_ok)[0]:
        grid.setdefault(tuple(twin.cells(r[j], origin, cell).tolist()), []).append(j)
    count, index, sqdist = np.zeros(len(q), np.int32), np.full(len(q), -1, np.int32), np.full(len(q), np.inf, F)
    largest = 0
    for i in np.nonzero(q_ok)[0]:
        lo, hi = twin.boxes(q[i], r2, cell, origin)
        lo, hi = lo[0], hi[0]
        largest = max(largest, int((hi - lo + 1).prod()))
        cand = []
        for cx in range(lo[0], hi[0] + 1):
            for cy in range(lo[1], hi[1] + 1):
                for cz in range(lo[2], hi[2] + 1):
                    cand += grid.get((cx, cy, cz), [])
        cand = np.array(sorted(j for j in cand if not (exclude_self and j == i)), np.int64)
        if len(cand):
            c, k, s = twin.search(q[i:i + 1], r[cand], r2)
            count[i], sqdist[i] = c[0], s[0]
            index[i] = cand[k[0]] if k[0] >= 0 else -1                          # cand ascends: the lowest index survives the mapping
    return count, index, sqdist, largest


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_dictionary_grid_equals_brute_force(seed):
    """The covering argument as a test: scanning exactly the box [C(fl(q - REACH)), C(fl(q + REACH))] gives the exhaustive result, byte
    for byte, for cell = REACH and 2 REACH, with the +-1e20 coordinates of the scene (the clamped cells) and a non-zero origin."""
    q, r, qv, rv = nn_twin.scene(260, 300, seed=seed)
    boxes = []
    for radius in (0.25, 0.5):
        r2 = twin.radius_sq(radius)
        want = twin.search(q, r, r2, qv, rv)
        assert (want[0] > 0).any() and (want[0] == 0).any()
        for cell, origin in ((twin.reach(r2), (0, 0, 0)), (F(2) * twin.reach(r2), (0, 0, 0)), (twin.reach(r2), (0.37, -5.0, 1e3))):
            got = _grid_search(q, r, r2, cell, origin, qv, rv)
            _same(got[:3], want, "seed %d radius %g cell %g" % (seed, radius, cell))
            boxes.append(got[3])
    assert max(boxes) <= 64
    c, _, cv, _ = nn_twin.scene(260, 0, seed=seed, same=True)
    r2 = twin.radius_sq(0.25)
    _same(_grid_search(c, c, r2, twin.reach(r2), (0, 0, 0), cv, cv, exclude_self=True)[:3], twin.search(c, c, r2, cv, cv, exclude_self=True), "exclude-self")


@pytest.mark.parametrize("offset", [1000.0, 16384.0])
def test_dictionary_grid_on_offset_clouds(offset):
    """Clouds far from the origin (spacing of the floats 6e-5 and 1e-3) at radius 0.05: the rounding of q +- REACH and of the cell
    function is where the covering argument has to hold."""
    rng = np.random.default_rng(int(offset))
    r = (rng.random((400, 3)) * 0.6 + offset).astype(F)
    q = (rng.random((300, 3)) * 0.6 + offset).astype(F)
    r2 = twin.radius_sq(0.05)
    want = twin.search(q, r, r2)
    assert (want[0] > 0).mean() > 0.3
    for origin in ((0, 0, 0), (offset, offset, offset)):
        _same(_grid_search(q, r, r2, twin.reach(r2), origin)[:3], want, "offset %g origin %r" % (offset, origin))
    stats = twin.box_stats(q, r, r2, twin.reach(r2))
    assert stats[2] >= int(want[0].sum()) and stats[0] <= 400 and stats[3] <= 64


def test_ctypes_struct_layout_matches_c_radius():
    enums, _ = abi_layout.check({"ovg_radius_params": L.RadiusParams},
                                ["OVG_RS_BUILD", "OVG_RS_SEARCH", "OVG_RS_EXCLUDE_SAME_INDEX", "OVG_RS_BAD_ORIGIN", "OVG_RS_OVER_BUDGET",
                                 "OVG_RS_NOT_BUILT", "OVG_RS_MIN_SLOTS", "OVG_RS_QUERY_BLOCK", "OVG_ABI_VERSION"])
    assert enums == [L.RS_BUILD, L.RS_SEARCH, L.RS_EXCLUDE_SAME_INDEX, L.RS_BAD_ORIGIN, L.RS_OVER_BUDGET,
                     L.RS_NOT_BUILT, L.RS_MIN_SLOTS, L.RS_QUERY_BLOCK, L.ABI_VERSION]
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+ovg_radius_workspace_bytes\s*\(\s*int64_t\s+nq,\s*int64_t\s+nr\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_radius_search\s*\(\s*const\s+ovg_radius_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_radius_search" in L.SYMBOLS and "ovg_radius_workspace_bytes" in L.SYMBOLS


def _ws_bytes(nr):
    r256 = lambda b: (b + 255) // 256 * 256
    slots = max(L.RS_MIN_SLOTS, 2 * nr)
    return 256 + r256(16 * slots) + r256(16 * nr) + r256(4 * ((slots + 4095) // 4096))


def test_radius_workspace_query_and_argument_validation_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    w = lib.ovg_radius_workspace_bytes
    top = (1 << 31) - 1
    for nq, nr in ((1, 1), (7, 511), (7, 512), (1, 513), (9500, 4097), (1 << 20, 1 << 20), (top, 1), (1, top), (top, top)):
        assert w(nq, nr) == _ws_bytes(nr), (nq, nr)
    assert w(1, 1) == 256 + 16384 + 256 + 256 and w(5, 512) == w(1, 1) + 8192 - 256 and w(1, 513) > w(1, 512)
    for bad in ((0, 1), (1, 0), (-1, 4), (4, -1), (1 << 31, 1), (1, 1 << 31), (1 << 40, 1 << 40), (-(1 << 62), 1), ((1 << 63) - 1, (1 << 63) - 1)):
        assert w(*bad) == -1, bad
    assert ops.radius_workspace_bytes(9500, 4097) == _ws_bytes(4097)
    for bad in ((0, 1), (1, 1 << 31), (1 << 70, 1)):
        with pytest.raises(L.OvgError):
            ops.radius_workspace_bytes(*bad)

    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    reach = ops.radius_reach(0.0625)

    def run(**kw):
        p = L.RadiusParams(query=big, reference=big, query_valid=big, reference_valid=big, origin=big, nq=1000, nr=1000, radius_sq=0.0625,
                           cell=reach, flags=0, stage=L.RS_BUILD | L.RS_SEARCH, max_pairs=1 << 40, ws=big, ws_bytes=w(1000, 1000),
                           out_stats=big, count=big, index=big, sqdist=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_radius_search(ctypes.byref(p), None)

    below = float(np.nextafter(F(reach), F(0)))
    assert lib.ovg_radius_search(None, None) == -1
    for bad in (dict(query=None), dict(reference=None), dict(ws=None), dict(out_stats=None), dict(count=None), dict(index=None), dict(sqdist=None),
                dict(stage=L.RS_BUILD, out_stats=None), dict(stage=L.RS_SEARCH, count=None), dict(stage=L.RS_SEARCH, index=None),
                dict(stage=L.RS_SEARCH, sqdist=None),
                dict(nq=0), dict(nr=0), dict(nq=-1), dict(nr=-7), dict(nq=1 << 31), dict(nr=1 << 31, ws_bytes=1 << 50),
                dict(nr=1 << 62, ws_bytes=1 << 62), dict(nq=-(1 << 63)),
                dict(radius_sq=0.0), dict(radius_sq=-1.0), dict(radius_sq=2.0 ** -101), dict(radius_sq=1e-45), dict(radius_sq=float("inf")),
                dict(radius_sq=float("nan")), dict(radius_sq=-float("inf")),
                dict(cell=below), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(radius_sq=0.25),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(stage=0), dict(stage=4), dict(stage=-1), dict(stage=7),
                dict(flags=L.RS_EXCLUDE_SAME_INDEX, nr=999), dict(flags=L.RS_EXCLUDE_SAME_INDEX, nq=999),
                dict(max_pairs=-1), dict(stage=L.RS_SEARCH, max_pairs=-(1 << 63)),
                dict(ws_bytes=w(1000, 1000) - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8), dict(ws=big + 4),
                dict(query=big + 2), dict(reference=big + 1), dict(origin=big + 2), dict(count=big + 1), dict(index=big + 2),
                dict(sqdist=big + 3), dict(out_stats=big + 4)):
        assert run(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    q, r = torch.zeros(5, 3), torch.zeros(2, 4, 3)
    for kw in (dict(query=torch.zeros(5, 4)), dict(query=torch.zeros(5, 3, dtype=torch.float64)), dict(query=np.zeros((5, 3), F)),
               dict(reference=torch.zeros(8, 2)), dict(reference=[[0.0, 0.0, 0.0]]),
               dict(query_valid=torch.ones(4, dtype=torch.bool)), dict(query_valid=torch.ones(5)),
               dict(reference_valid=torch.ones(8, dtype=torch.bool)), dict(exclude_self=True),
               dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="x"), dict(radius=True),
               dict(radius=1e-16), dict(radius=1e20), dict(radius=torch.tensor(0.5)),
               dict(cell_size=0.4), dict(cell_size=0.5), dict(cell_size=float("inf")), dict(cell_size="x"),
               dict(origin=(0, 0)), dict(origin=(0, 0, float("nan"))), dict(origin=1.0), dict(origin=torch.zeros(2)),
               dict(origin=torch.zeros(3, dtype=torch.float64)), dict(max_pairs=-1), dict(max_pairs=1.5)):
        with pytest.raises(ValueError):
            postprocess.radius_neighbours(**dict(dict(query=q, reference=r, radius=0.5), **kw))
    for kw in (dict(), dict(query_valid=torch.ones(5, dtype=torch.bool)), dict(reference=torch.zeros(5, 3), exclude_self=True),
               dict(cell_size=1.0, origin=(1.0, 2.0, 3.0)), dict(origin=torch.zeros(3)), dict(max_pairs=10),
               dict(query=torch.zeros(0, 3)), dict(reference=torch.zeros(0, 3))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.radius_neighbours(**dict(dict(query=q, reference=r, radius=0.5), **kw))
    cloud = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, torch.tensor(2.0), None, None)
    for kw in (dict(), dict(radius=0.5, rel_radius=0.1), dict(radius=-1.0), dict(rel_radius=0.0), dict(rel_radius=float("nan")),
               dict(radius=0.5, min_neighbours=0), dict(radius=0.5, min_neighbours=1.5), dict(radius=0.5, min_neighbours=True)):
        with pytest.raises(ValueError):
            postprocess.radius_outlier_mask(cloud, **kw)
        with pytest.raises(ValueError):
            postprocess.remove_radius_outliers(cloud, **kw)
    for bad in (dict(cloud_or_points=q, rel_radius=0.1), dict(cloud_or_points=q, radius=0.5, valid=torch.ones(4, dtype=torch.bool)),
                dict(cloud_or_points=torch.zeros(5, 2), radius=0.5)):
        with pytest.raises(ValueError):
            postprocess.radius_outlier_mask(**bad)
    with pytest.raises(ValueError):
        postprocess.remove_radius_outliers(q, radius=0.5)                   # a PointCloud, not a tensor
    for kw in (dict(radius=0.5), dict(rel_radius=0.1), dict(radius=0.5, min_neighbours=3)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.radius_outlier_mask(cloud, **kw)
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.remove_radius_outliers(cloud, **kw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.radius_outlier_mask(q, radius=0.5, valid=torch.ones(5, dtype=torch.bool))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.cloud_fscore(q, r, 0.1)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.cloud_fscore(cloud, cloud, 0.1, max_pairs=100)
    for t in (0, -1.0, float("nan"), "x", True, None):
        with pytest.raises(ValueError):
            postprocess.cloud_fscore(q, r, t)
    with pytest.raises(ValueError):
        postprocess.cloud_fscore(q, torch.zeros(3, 2), 0.1)
    with pytest.raises(L.OvgError):
        ops.radius_search(L.RS_BUILD, q, r.reshape(-1, 3), 0.25, 0.6, torch.zeros(1 << 16, dtype=torch.uint8))   # CPU tensors at the thin wrapper
    res = postprocess.RadiusResult(torch.tensor([2, 0], dtype=torch.int32), torch.tensor([1, -1], dtype=torch.int32), torch.tensor([0.5, float("inf")]))
    assert res.count.tolist() == [2, 0] and res.index.tolist() == [1, -1] and res.sqdist[0] == 0.5
    assert postprocess.RADIUS_MAX_PAIRS > 0 and postprocess.RADIUS_MAX_PAIRS & (postprocess.RADIUS_MAX_PAIRS - 1) == 0
