"""Clustering (ovg_cluster, postprocess.cluster_points), host side: the brute-force twin (tests/cluster_twin.py) checked for the
properties the rule promises and against the radius twin and a k-d tree, the C ABI without a device (struct layout, enums, argument
checks that return before any HIP call) and the Python API's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import cluster_twin as twin
import common
import nn_twin
import radius_twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def _partition(root):
    """The partition a root array describes, without the names: a sorted list of sorted member tuples."""
    groups = {}
    for i, r in enumerate(root.tolist()):
        if r >= 0:
            groups.setdefault(r, []).append(i)
    return sorted(tuple(g) for g in groups.values())


def test_twin_roots_are_lowest_indices_and_degree_is_the_radius_twins_count():
    c, _, cv, _ = nn_twin.scene(700, 0, seed=2, same=True)
    for radius in (0.25, 0.5):
        r2 = radius_twin.radius_sq(radius)
        for valid in (None, cv):
            I, J, bits = twin.edges(c, valid, r2)
            assert (I != J).all() and len(I) % 2 == 0
            back = np.lexsort((I, J))
            assert (I[back] == J).all() and (J[back] == I).all() and (bits[back] == bits).all()       # symmetric bit for bit
            count = radius_twin.search(c, c, r2, valid, valid, exclude_self=True)[0]
            ok = twin.usable(c, valid)
            for mn in (0, 1, 3, 6):
                degree, kind, root = twin.cluster(len(c), ok, I, J, bits, mn)
                assert degree.dtype == np.int32 and kind.dtype == np.uint8 and root.dtype == np.int32
                assert degree.tobytes() == count.tobytes()
                member = root >= 0
                core = kind == twin.CORE
                assert (root[core] <= np.nonzero(core)[0]).all()                 # root[i] <= i for a core point (a border point may lie below its cluster's cores)
                assert mn > 0 or (core == member).all()
                assert (root[root[member]] == root[member]).all()                # root[root] == root
                assert (kind[root[member]] == twin.CORE).all()                   # a cluster is named by a core point
                assert ((kind == twin.UNUSABLE) == ~ok).all() and (member == (kind >= twin.BORDER)).all()
                assert ((kind == twin.CORE) == (ok & (degree >= mn))).all()
                lone = (kind == twin.NOISE)
                assert mn > 0 or not lone.any()
                # a noise point has no core neighbour, a border point has one in its own cluster
                core_nb = np.zeros(len(c), bool)
                core_nb[I[kind[J] == twin.CORE]] = True
                assert not core_nb[lone].any() and core_nb[kind == twin.BORDER].all()
                # every edge between core points stays inside one cluster
                cc = (kind[I] == twin.CORE) & (kind[J] == twin.CORE)
                assert (root[I[cc]] == root[J[cc]]).all()
            assert (twin.cluster(len(c), ok, I, J, bits, 3)[1] == twin.BORDER).any()


def test_twin_partition_is_invariant_under_a_permutation_of_the_input():
    c, _, cv, _ = nn_twin.scene(600, 0, seed=5, same=True)
    r2 = radius_twin.radius_sq(0.25)
    perm = np.random.default_rng(3).permutation(len(c))
    for mn in (0, 3):
        _, kind, root = twin.run(c, cv, r2, mn)
        _, kind_p, root_p = twin.run(c[perm], cv[perm], r2, mn)
        assert (kind_p == kind[perm]).all()
        core = kind == twin.CORE
        # the core partition does not depend on the order; a border point's choice between equidistant cores may (lowest INDEX)
        back = {tuple(sorted(perm[list(g)].tolist())) for g in _partition(np.where(kind_p == twin.CORE, root_p, -1))}
        assert back == set(_partition(np.where(core, root, -1)))
        if mn == 0:
            assert back == set(_partition(root))


def test_twin_crafted_border_between_two_clusters_and_labels():
    def scene(order, bx):
        a = [[-0.25, 0, 0]] + [[-0.5, 0, 0]] * 4
        b = [[bx, 0, 0]] + [[bx + 0.25, 0, 0]] * 4
        parts = {"a": a, "b": b, "x": [[0, 0, 0]]}
        pts, names = [], []
        for name in order:
            pts += parts[name]
            names += [name] * len(parts[name])
        return np.array(pts, F), names
    for order, bx, joins in (("axb", 0.25, "a"), ("bxa", 0.25, "b"), ("xba", 0.25, "b"), ("axb", 0.125, "b"), ("bxa", 0.125, "b")):
        pts, names = scene(order, bx)
        degree, kind, root = twin.run(pts, None, F(0.0625), 4)
        x = names.index("x")
        assert degree[x] == 2 and kind[x] == twin.BORDER and root[x] == names.index(joins), (order, bx)
        assert (kind[np.arange(11) != x] == twin.CORE).all() and len(set(root.tolist())) == 2
    root = np.array([4, -1, 2, 2, 4, 5, 2, -1, 8, 8], np.int32)
    lab, roots, sizes = twin.labels(root, "index")
    assert lab.tolist() == [1, -1, 0, 0, 1, 2, 0, -1, 3, 3] and roots.tolist() == [2, 4, 5, 8] and sizes.tolist() == [3, 2, 1, 2]
    lab, roots, sizes = twin.labels(root, "size")
    assert lab.tolist() == [1, -1, 0, 0, 1, 3, 0, -1, 2, 2] and roots.tolist() == [2, 4, 8, 5] and sizes.tolist() == [3, 2, 2, 1]
    assert sizes.dtype == np.int64 and roots.dtype == np.int32 and lab.dtype == np.int32
    lab, roots, sizes = twin.labels(np.full(3, -1, np.int32))
    assert lab.tolist() == [-1] * 3 and len(roots) == 0 and len(sizes) == 0


def test_brute_force_and_kd_tree_edges_agree_on_the_lattice():
    pts, radius = twin.lattice_scene()
    pts = pts[:20000]
    r2 = radius_twin.radius_sq(radius)
    assert F(6.0 / 4096) < r2 < F(7.0 / 4096)
    I, J, bits = twin.edges(pts, None, r2, budget=1 << 24)
    Ik, Jk, bk = twin.kdtree_edges(pts, radius)
    assert len(I) > 1000 and (I == Ik).all() and (J == Jk).all() and bits.tobytes() == bk.tobytes()
    units = bits.view(F).astype(np.float64) * 4096
    assert (units == np.round(units)).all() and units.max() == 6 and (units == 6).any()               # exact multiples of 2^-12


def _layout(struct, cname, extra):
    return abi_layout.check({cname: struct}, extra)[0]


def test_ctypes_struct_layout_and_enums_match_c_cluster():
    enums = ["OVG_CL_UNUSABLE", "OVG_CL_NOISE", "OVG_CL_BORDER", "OVG_CL_CORE", "OVG_CL_INTERNAL", "OVG_ABI_VERSION"]
    assert _layout(L.ClusterParams, "ovg_cluster_params", enums) == [L.CL_UNUSABLE, L.CL_NOISE, L.CL_BORDER, L.CL_CORE, L.CL_INTERNAL, L.ABI_VERSION]
    assert (L.CL_UNUSABLE, L.CL_NOISE, L.CL_BORDER, L.CL_CORE) == (0, 1, 2, 3) == (twin.UNUSABLE, twin.NOISE, twin.BORDER, twin.CORE)
    assert L.CL_INTERNAL & (L.RS_BAD_ORIGIN | L.RS_OVER_BUDGET | L.RS_NOT_BUILT) == 0 and L.ABI_VERSION == 13
    assert (postprocess.CL_UNUSABLE, postprocess.CL_NOISE, postprocess.CL_BORDER, postprocess.CL_CORE) == (0, 1, 2, 3)
    text = open(HEADER).read()
    assert re.search(r"int\s+ovg_cluster\s*\(\s*const\s+ovg_cluster_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert re.search(r"\(ovg_cluster\): added the same way", text)
    assert "ovg_cluster" in L.SYMBOLS


def test_argument_validation_of_the_entry_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    reach = ops.radius_reach(0.0625)
    need = lib.ovg_radius_workspace_bytes(1000, 1000)

    def run(**kw):
        p = L.ClusterParams(points=big, valid=big, origin=big, n=1000, radius_sq=0.0625, cell=reach, min_neighbours=3, flags=0,
                            max_pairs=1 << 40, ws=big, ws_bytes=need, out_stats=big, root=big, kind=big + 1, degree=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_cluster(ctypes.byref(p), None)

    below = float(np.nextafter(F(reach), F(0)))
    assert lib.ovg_cluster(None, None) == -1
    for bad in (dict(points=None), dict(ws=None), dict(root=None), dict(kind=None),
                dict(n=0), dict(n=-1), dict(n=1 << 31, ws_bytes=1 << 50), dict(n=-(1 << 63)),
                dict(radius_sq=0.0), dict(radius_sq=-1.0), dict(radius_sq=2.0 ** -101), dict(radius_sq=float("inf")), dict(radius_sq=float("nan")),
                dict(cell=below), dict(cell=0.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(radius_sq=0.25),
                dict(flags=1), dict(flags=2), dict(flags=-1), dict(min_neighbours=-1), dict(min_neighbours=-(1 << 31)),
                dict(max_pairs=-1), dict(max_pairs=-(1 << 63)),
                dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8), dict(ws=big + 4),
                dict(points=big + 2), dict(origin=big + 2), dict(root=big + 1), dict(root=big + 2), dict(degree=big + 2), dict(degree=big + 3),
                dict(out_stats=big + 4)):
        assert run(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    q = torch.zeros(5, 3)
    cloud = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, torch.tensor(2.0), None, None)
    for kw in (dict(), dict(radius=0.5, rel_radius=0.1), dict(radius=0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=True),
               dict(radius=1e20), dict(rel_radius=0.0), dict(rel_radius=float("nan")),
               dict(radius=0.5, min_neighbours=-1), dict(radius=0.5, min_neighbours=1.0), dict(radius=0.5, min_neighbours=True),
               dict(radius=0.5, min_neighbours=None), dict(radius=0.5, min_neighbours=1 << 31),
               dict(radius=0.5, order="root"), dict(radius=0.5, order=None), dict(radius=0.5, valid=torch.ones(4, dtype=torch.bool)),
               dict(radius=0.5, cell_size=0.4), dict(radius=0.5, cell_size="x"), dict(radius=0.5, origin=(0, 0)),
               dict(radius=0.5, origin=torch.zeros(2)), dict(radius=0.5, max_pairs=-1), dict(radius=0.5, max_pairs=1.5)):
        with pytest.raises(ValueError):
            postprocess.cluster_points(cloud, **kw)
    for bad in (torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.float64), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            postprocess.cluster_points(bad, radius=0.5)
    with pytest.raises(ValueError):
        postprocess.cluster_points(q, rel_radius=0.1)                       # rel_radius needs a PointCloud
    for kw in (dict(radius=0.5), dict(rel_radius=0.1), dict(radius=0.5, min_neighbours=3, order="index"),
               dict(radius=0.5, valid=torch.ones(5, dtype=torch.bool)), dict(radius=0.5, cell_size=1.0, origin=(1.0, 2.0, 3.0), max_pairs=10)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.cluster_points(cloud, **kw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.cluster_points(torch.zeros(0, 3), radius=0.5)
    for kw in (dict(radius=0.5), dict(radius=0.5, min_size=2, keep_largest=True), dict(min_size=2), dict(radius=0.5, rel_radius=0.5, min_size=2),
               dict(radius=0.5, min_size=0), dict(radius=0.5, min_size=2.0), dict(radius=0.5, min_size=True), dict(radius=0.5, keep_largest=1),
               dict(radius=0.5, keep_largest=False), dict(radius=0.5, min_size=2, min_neighbours=-1)):
        with pytest.raises(ValueError):
            postprocess.remove_small_clusters(cloud, **kw)
    with pytest.raises(ValueError):
        postprocess.remove_small_clusters(q, radius=0.5, min_size=2)        # a PointCloud, not a tensor
    for kw in (dict(radius=0.5, min_size=2), dict(rel_radius=0.1, keep_largest=True), dict(radius=0.5, min_size=2, keep_largest=False)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.remove_small_clusters(cloud, **kw)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    with pytest.raises(L.OvgError):
        ops.cluster(q, 0.25, 0.6, ws, 0)                                    # CPU tensors at the thin wrapper
    for bad in (None, "x", 3):
        with pytest.raises(ValueError):
            postprocess.largest_cluster_mask(bad)
        with pytest.raises(ValueError):
            postprocess.cluster_size_mask(bad, 2)


def test_masks_and_colours_on_a_result_built_by_hand():
    root = np.array([4, -1, 2, 2, 4, 5, 2, -1, 8, 8], np.int32)
    kind = torch.full((10,), 3, dtype=torch.uint8)
    for order in ("size", "index"):
        lab, roots, sizes = twin.labels(root, order)
        res = postprocess.ClusterResult(torch.from_numpy(lab), kind, torch.from_numpy(root), torch.zeros(10, dtype=torch.int32),
                                        torch.from_numpy(roots), torch.from_numpy(sizes), len(roots))
        assert postprocess.largest_cluster_mask(res).tolist() == (root == 2).tolist()
        assert postprocess.cluster_size_mask(res, 2).tolist() == np.isin(root, (2, 4, 8)).tolist()
        assert postprocess.cluster_size_mask(res, 3).tolist() == (root == 2).tolist() and not postprocess.cluster_size_mask(res, 4).any()
        assert postprocess.cluster_size_mask(res, 1).tolist() == (root >= 0).tolist()
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError):
                postprocess.cluster_size_mask(res, bad)
    # equal sizes: the lowest root is the largest cluster
    tie = np.array([3, 1, 1, 3, -1], np.int32)
    lab, roots, sizes = twin.labels(tie, "index")
    res = postprocess.ClusterResult(torch.from_numpy(lab), kind[:5], torch.from_numpy(tie), None, torch.from_numpy(roots), torch.from_numpy(sizes), 2)
    assert postprocess.largest_cluster_mask(res).tolist() == [False, True, True, False, False]
    none = postprocess.ClusterResult(torch.full((2, 3), -1, dtype=torch.int32), None, torch.full((2, 3), -1, dtype=torch.int32), None,
                                     torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), 0)
    assert postprocess.largest_cluster_mask(none).shape == (2, 3) and not postprocess.largest_cluster_mask(none).any()
    assert not postprocess.cluster_size_mask(none, 1).any()
    labels = torch.tensor([[0, 1, 2, -1], [1, 0, 1000000, -1]], dtype=torch.int32)
    col = postprocess.cluster_colors(labels)
    assert col.dtype == torch.uint8 and col.shape == (2, 4, 3)
    assert col[0, 3].tolist() == [128, 128, 128] == col[1, 3].tolist()
    assert col[0, 0].tolist() == col[1, 1].tolist() and col[0, 1].tolist() == col[1, 0].tolist()
    assert torch.equal(col, postprocess.cluster_colors(labels.long())) and int(col[labels >= 0].min()) >= 56
    many = postprocess.cluster_colors(torch.arange(64, dtype=torch.int32))
    assert len({tuple(c) for c in many.tolist()}) == 64                      # the first labels get distinct colours
    for bad in (labels.float(), [0, 1], None):
        with pytest.raises(ValueError):
            postprocess.cluster_colors(bad)
