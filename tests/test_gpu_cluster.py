"""ovg_cluster and postprocess.cluster_points, largest_cluster_mask, cluster_size_mask, remove_small_clusters on the device against
the brute force of tests/cluster_twin.py: root, kind and degree byte for byte, every case into exact-size guarded outputs over an
exact-size workspace and run twice with identical bytes -- shapes around the block and the hash table's minimum at two radii, as
connected components and as DBSCAN, with and without a valid mask, another cell edge and origin; crafted inputs (a chain in three
index orders at d == radius_sq exactly, a lattice where many threads hook one root, one cell, duplicates, a border point between two
clusters, no usable point); a 262 144-point lattice over every XCD against a k-d tree; the work guard; composition with
ovg_radius_search; the Python layer; a cloud un-projected from real views."""
import os

import numpy as np
import pytest
import torch

import cluster_twin as twin
import common
import consistency_twin as ctwin
import nn_twin
import radius_twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
QB = L.RS_QUERY_BLOCK
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
FILL32 = -0x5A5A5A5B                             # kernel_guards' fill byte 0xA5 four times, as int32
UNUSABLE, NOISE, BORDER, CORE = twin.UNUSABLE, twin.NOISE, twin.BORDER, twin.CORE


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(pts, r2, valid=None, cell=None, origin=None):
    """BUILD inside one cloud in an exact-size workspace. -> (the arguments of ops.cluster, [flags, cells, largest, pairs])"""
    cell = radius_twin.reach(r2) if cell is None else cell
    n = len(pts)
    ws = torch.empty(ops.radius_workspace_bytes(n, n), device="cuda", dtype=torch.uint8)
    p, v = _dev(pts), _dev(valid)
    org = None if origin is None else _dev(np.asarray(origin, F))
    stats = ops.radius_search(L.RS_BUILD, p, p, float(r2), float(cell), ws, query_valid=v, reference_valid=v, origin=org, exclude_self=True)[0]
    return dict(points=p, radius_sq=float(r2), cell=float(cell), ws=ws, valid=v, origin=org), stats.cpu().tolist()


def _once(args, mn, max_pairs, out_stats):
    n = args["points"].shape[0]
    root, check_r = guarded((1, n), torch.int32, "cuda", guard_bytes=4096)
    kind, check_k = guarded((1, n), torch.uint8, "cuda", guard_bytes=4096)
    degree, check_d = guarded((1, n), torch.int32, "cuda", guard_bytes=4096)
    out = ops.cluster(min_neighbours=mn, max_pairs=max_pairs, out_stats=out_stats, root=root[0], kind=kind[0], degree=degree[0], **args)
    torch.cuda.synchronize()
    check_r("root"), check_k("kind"), check_d("degree")
    assert out[0] is out_stats
    return degree[0], kind[0], root[0]


def _cluster(args, mn, max_pairs=1 << 40, out_stats=None):
    """ovg_cluster into exact-size guarded outputs, twice: nothing may be written outside them, and the two runs give identical
    bytes. -> (degree, kind, root) like the twin"""
    own = torch.zeros(4, device="cuda", dtype=torch.int64) if out_stats is None else out_stats
    first = _once(args, mn, max_pairs, own)
    assert (int(own[0]) & L.CL_INTERNAL) == 0
    second = _once(args, mn, max_pairs, own)
    for a, b, what in zip(first, second, ("degree", "kind", "root")):
        assert torch.equal(a, b), ("two runs differ", what)
    return first


def _same(got, want, name):
    for g, w, what in zip(got, want, ("degree", "kind", "root")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, int((g != w).sum()), np.nonzero(g != w)[0][:8].tolist())


def _check(pts, radius, mns, valid=None, cell=None, origin=None, name="", r2=None):
    """-> {min_neighbours: the twin's (degree, kind, root)}; the twin's edges are listed once per cloud"""
    r2 = radius_twin.radius_sq(radius) if r2 is None else r2
    I, J, bits = twin.edges(pts, valid, r2)
    args, stats = _grid(pts, r2, valid, cell, origin)
    assert stats[0] == 0
    out = {}
    for mn in mns:
        out[mn] = twin.cluster(len(pts), twin.usable(pts, valid), I, J, bits, mn)
        _same(_cluster(args, mn), out[mn], "%s min_neighbours %d" % (name, mn))
    return out


def _summary(kind, root):
    sizes = twin.labels(root)[2]
    return len(sizes), int((kind == CORE).sum()), int((kind == BORDER).sum()), int(sizes[0]) if len(sizes) else 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 529, 3000])
def test_shapes_radii_and_masks_match_twin_bit_exactly(n):
    """n around the block of 256 threads; 513 is the first n whose 2 n slots exceed the 1024-slot minimum table, 529 the same with
    an odd tail, 3000 takes several blocks. The scene holds blobs, a quarter lattice (exact ties), duplicates, NaN / inf / 1e20
    coordinates and a mask with holes."""
    L.require_gpu()
    assert QB == 256
    c, _, cv, _ = nn_twin.scene(n, 0, seed=2, same=True)
    seen = {}
    for radius in (0.25, 0.5):
        for valid in (None, cv):
            name = "%d radius %g%s" % (n, radius, "" if valid is None else " mask")
            want = _check(c, radius, (0, 3), valid, name=name)
            for mn in (0, 3):
                seen[(radius, mn, valid is not None)] = _summary(want[mn][1], want[mn][2])
                assert mn > 0 or not (want[mn][1] == NOISE).any()
    if n >= 513:
        r2 = radius_twin.radius_sq(0.5)
        _check(c, 0.5, (0, 3), cv, cell=F(2) * radius_twin.reach(r2), name="%d doubled cell" % n)
        _check(c, 0.5, (3,), cv, origin=(0.37, -5.0, 1e3), name="%d moved origin" % n)
    # what a CPU run of the twin gave: every kind occurs
    if n == 3000:
        assert seen[(0.25, 3, True)] == (21, 2108, 151, 836) and seen[(0.5, 0, True)][0] == 84 and seen[(0.5, 0, True)][3] == 2315
    if n == 513:
        assert seen[(0.25, 3, True)][:3] == (13, 185, 58)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_at_exactly_the_radius(order):
    """2048 points x = 0.25 k: d == radius_sq exactly between successive points (inclusive). The shuffled chain is the union-find's
    deep-path case: neighbours in space are far apart in index."""
    L.require_gpu()
    n = 2048
    k = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(4).permutation(n)}[order]
    pts = np.zeros((n, 3), F)
    pts[:, 0] = (k * 0.25).astype(F)
    ends = [int(np.nonzero(k == 0)[0][0]), int(np.nonzero(k == n - 1)[0][0])]
    want = _check(pts, 0.25, (0, 2, 3), name="chain " + order)
    for mn in (0, 2):
        degree, kind, root = want[mn]
        assert (root == np.nonzero(kind == CORE)[0][0]).all() and sorted(np.nonzero(degree == 1)[0].tolist()) == sorted(ends) and (np.delete(degree, ends) == 2).all()
        assert (np.delete(kind, ends) == CORE).all() and (kind[ends] == (CORE if mn == 0 else BORDER)).all()
    assert (want[3][1] == NOISE).all() and (want[3][2] == -1).all()
    want = _check(pts, 0.2499, (0, 1), name="chain below the spacing " + order)
    assert (want[0][2] == np.arange(n)).all() and (want[0][1] == CORE).all() and (want[0][0] == 0).all()
    assert (want[1][2] == -1).all() and (want[1][1] == NOISE).all()


def test_crafted_inputs_match_twin():
    L.require_gpu()
    rng = np.random.default_rng(1)
    lattice = (rng.integers(-8, 9, (2500, 3)) / 4.0).astype(F)               # the quarter lattice of test_gpu_knn: many threads hook one root
    want = _check(lattice, 0.25, (0, 3, 5), name="quarter lattice")
    sizes = twin.labels(want[0][2])[2]
    assert sizes[0] > 1500 and (want[3][1] == BORDER).any() and (want[5][1] == NOISE).any()
    ball = (rng.random((700, 3)) * 0.2).astype(F)
    r2 = radius_twin.radius_sq(0.05)
    args, stats = _grid(ball, r2, cell=F(1e6))
    assert stats[:3] == [0, 1, 700] and stats[3] == 700 * 700               # every point in ONE cell, every point scans it
    I, J, bits = twin.edges(ball, None, r2)
    for mn in (0, 12, 34):                                                  # the mean degree is 34
        w = twin.cluster(700, np.ones(700, bool), I, J, bits, mn)
        _same(_cluster(args, mn), w, "one cell min_neighbours %d" % mn)
    assert (w[1] == BORDER).any() and (w[1] == CORE).any()
    dup = np.repeat((rng.random((90, 3)) * 3).astype(F), 5, axis=0)[rng.permutation(450)]             # five coincident copies: d = 0
    want = _check(dup, 0.25, (0, 4, 5), name="duplicates")
    assert (want[4][0] >= 4).all() and (want[4][1] == CORE).all() and (want[5][1] != CORE).any()
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1.0, 2.0, 3.0]], F)
    want = _check(bad, 0.25, (0, 1), valid=np.array([1, 1, 1, 0], np.uint8), name="no usable point")
    for mn in (0, 1):
        assert (want[mn][0] == 0).all() and (want[mn][1] == UNUSABLE).all() and (want[mn][2] == -1).all()
    far = (rng.random((900, 3)) * 0.6 + 16384.0).astype(F)
    want = _check(far, 0.05, (0, 2), name="offset 16384")
    assert (want[2][1] == BORDER).any()


def test_border_point_between_two_clusters():
    """Core a0 at -0.25 with four coincident satellites at -0.5, its mirror image b0, X at the origin with degree 2 at radius 0.25
    and min_neighbours 4: X is equidistant from a0 and b0 and joins the one with the LOWER index; with b0 moved to 0.125 it joins
    B whatever the indices."""
    L.require_gpu()

    def scene(order, bx):
        parts = {"a": [[-0.25, 0, 0]] + [[-0.5, 0, 0]] * 4, "b": [[bx, 0, 0]] + [[bx + 0.25, 0, 0]] * 4, "x": [[0, 0, 0]]}
        pts, names = [], []
        for name in order:
            pts += parts[name]
            names += [name] * len(parts[name])
        return np.array(pts, F), names

    for order, bx, joins in (("axb", 0.25, "a"), ("bxa", 0.25, "b"), ("xab", 0.25, "a"), ("xba", 0.25, "b"), ("axb", 0.125, "b"),
                             ("bxa", 0.125, "b"), ("xab", 0.125, "b")):
        pts, names = scene(order, bx)
        degree, kind, root = _check(pts, 0.25, (4,), name="border %s %g" % (order, bx))[4]
        x = names.index("x")
        assert degree[x] == 2 and kind[x] == BORDER and root[x] == names.index(joins), (order, bx)
        assert (np.delete(kind, x) == CORE).all() and len(set(root.tolist())) == 2


_SCALE = {}


def _scale_scene():
    if not _SCALE:
        pts, radius = twin.lattice_scene()
        _SCALE["pts"], _SCALE["radius"] = pts, radius
        _SCALE["edges"] = twin.kdtree_edges(pts, radius)                      # exact on this lattice: tests/test_cluster_host.py
    return _SCALE["pts"], _SCALE["radius"], _SCALE["edges"]


def test_lattice_of_262144_points_spans_every_xcd():
    """1024 workgroups. Every near d is an exact multiple of 2^-12 in float32 and float64 and no pair lies between 6 and 7 units at
    radius sqrt(6.5) / 64, so the float64 k-d tree lists the rule's pairs. This recipe gave, on the CPU: 569 438 neighbour pairs,
    62 010 clusters, the largest of 130 818 points, 35 697 singletons, 1 013 clusters of 10 to 999 points, mean degree 4.3."""
    L.require_gpu()
    pts, radius, (I, J, bits) = _scale_scene()
    n = len(pts)
    assert n == 262144 and (n + QB - 1) // QB == 1024
    r2 = radius_twin.radius_sq(radius)
    args, stats = _grid(pts, r2)
    assert stats[0] == 0
    ok = np.ones(n, bool)
    for mn in (0, 3):
        want = twin.cluster(n, ok, I, J, bits, mn)
        _same(_cluster(args, mn), want, "lattice min_neighbours %d" % mn)
        sizes = twin.labels(want[2])[2]
        print("min_neighbours %d: %d pairs, %d clusters, largest %d, %d singletons, %d of 10..999, mean degree %.2f, %d border, %d noise"
              % (mn, len(I) // 2, len(sizes), sizes[0], (sizes == 1).sum(), ((sizes >= 10) & (sizes <= 999)).sum(), want[0].mean(),
                 (want[1] == BORDER).sum(), (want[1] == NOISE).sum()))
        assert sizes[0] > 100000
        if mn == 0:
            assert ((sizes >= 10) & (sizes <= 999)).sum() > 500 and len(I) // 2 > 500000
        else:
            assert (want[1] == BORDER).sum() > 10000 and (want[1] == NOISE).sum() > 10000


def test_guards_refuse_without_writing_and_degree_is_the_radius_searchs_count():
    L.require_gpu()
    n = 5 * 512 + 1
    c, _, cv, _ = nn_twin.scene(n, 0, seed=4, same=True)
    r2 = radius_twin.radius_sq(0.5)
    cell = radius_twin.reach(r2)
    need = ops.radius_workspace_bytes(n, n)
    ws = torch.full((need + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    ws[:need] = 0                                                            # a cleared workspace: no BUILD
    stats, check_t = guarded((1, 4), torch.int64, "cuda")
    p, v = _dev(c), _dev(cv)
    args = dict(points=p, radius_sq=float(r2), cell=float(cell), ws=ws[:need], valid=v, origin=None)
    got = _cluster(args, 3, out_stats=stats[0])
    assert stats[0].tolist() == [L.RS_NOT_BUILT, 0, 0, 0]
    assert bool((got[0] == FILL32).all()) and bool((got[1] == 0xA5).all()) and bool((got[2] == FILL32).all())
    built = ops.radius_search(L.RS_BUILD, p, p, float(r2), float(cell), ws[:need], query_valid=v, reference_valid=v, exclude_self=True)[0].tolist()
    occupied, largest, pairs, _ = radius_twin.box_stats(c, c, r2, cell, (0.0, 0.0, 0.0), cv, cv)
    assert built == [0, occupied, largest, pairs] and pairs > 1000
    got = _cluster(args, 3, max_pairs=pairs - 1, out_stats=stats[0])       # one pair over the budget
    assert stats[0].tolist() == [L.RS_OVER_BUDGET, occupied, largest, pairs]
    assert bool((got[0] == FILL32).all()) and bool((got[1] == 0xA5).all()) and bool((got[2] == FILL32).all())
    got = _cluster(args, 3, max_pairs=pairs, out_stats=stats[0])           # exactly the budget
    assert stats[0].tolist() == [0, occupied, largest, pairs]
    check_t("out_stats")
    assert bool((ws[need:] == 0xA5).all())
    _same(got, twin.run(c, cv, r2, 3), "guarded")
    count = ops.radius_search(L.RS_SEARCH, p, p, float(r2), float(cell), ws[:need], query_valid=v, reference_valid=v, exclude_self=True,
                              max_pairs=pairs)[1]
    assert torch.equal(got[0], count)                                       # degree: the count of the radius search, byte for byte
    # the grid is only read: a search after the clustering still finds it, and degree may be left out
    _, root, kind, degree = ops.cluster(min_neighbours=3, max_pairs=pairs, degree=False, **args)
    assert degree is None and torch.equal(root, got[2]) and torch.equal(kind, got[1])
    with pytest.raises(ValueError, match="candidate pairs"):
        postprocess.cluster_points(p, radius=0.5, max_pairs=1000)
    with pytest.raises(L.OvgError):
        ops.cluster(min_neighbours=-1, **args)


def test_python_layer_labels_masks_and_removal():
    L.require_gpu()
    n = 3000
    c, _, cv, _ = nn_twin.scene(n, 0, seed=2, same=True)
    r2 = radius_twin.radius_sq(0.25)
    degree, kind, root = twin.run(c, cv, r2, 3)
    for order in ("size", "index"):
        lab, roots, sizes = twin.labels(root, order)
        res = postprocess.cluster_points(_dev(c.reshape(3, 1000, 3)), radius=0.25, min_neighbours=3, valid=_dev(cv.reshape(3, 1000).astype(bool)), order=order)
        assert res.labels.shape == res.kind.shape == res.root.shape == res.degree.shape == (3, 1000) and res.num_clusters == len(roots) == 21
        assert res.labels.dtype == res.root.dtype == res.degree.dtype == res.roots.dtype == torch.int32
        assert res.kind.dtype == torch.uint8 and res.sizes.dtype == torch.int64
        for g, w in ((res.labels, lab), (res.kind, kind), (res.root, root), (res.degree, degree), (res.roots, roots), (res.sizes, sizes)):
            assert g.cpu().numpy().reshape(-1).tobytes() == w.tobytes(), order
        assert postprocess.largest_cluster_mask(res).cpu().numpy().reshape(-1).tolist() == (root == roots[np.argmax(sizes)]).tolist()
        big = np.isin(root, roots[sizes >= 40])
        assert big.any() and not big[root >= 0].all()
        assert postprocess.cluster_size_mask(res, 40).cpu().numpy().reshape(-1).tolist() == big.tolist()
    assert int(postprocess.cluster_points(_dev(c), radius=0.25, min_neighbours=3, valid=_dev(cv)).sizes[0]) == 836
    other = postprocess.cluster_points(_dev(c), radius=0.25, min_neighbours=3, valid=_dev(cv), cell_size=0.9, origin=(0.1, -3.0, 77.0), order="index")
    assert torch.equal(other.root.reshape(-1), res.root.reshape(-1)) and torch.equal(other.labels.reshape(-1), res.labels.reshape(-1))
    empty = postprocess.cluster_points(_dev(c[:0]), radius=0.25)
    assert empty.num_clusters == 0 and empty.labels.shape == (0,) and empty.roots.shape == (0,) and empty.sizes.dtype == torch.int64
    assert postprocess.largest_cluster_mask(empty).shape == (0,) and postprocess.cluster_size_mask(empty, 2).shape == (0,)
    # a PointCloud: the gather of remove_radius_outliers, and rel_radius = f32(rel) * scene_scale
    ok = np.isfinite(c).all(1)
    cloud, colors, conf = c[ok], np.random.default_rng(0).integers(0, 256, (int(ok.sum()), 3)).astype(np.uint8), np.random.default_rng(1).random(int(ok.sum())).astype(F)
    scale = torch.tensor(2.0, device="cuda")
    pc = postprocess.PointCloud(_dev(cloud), _dev(colors), torch.tensor(0.5, device="cuda"), scale, np.eye(4), torch.zeros(2, 3, 4, device="cuda"),
                                _dev(np.arange(len(cloud), dtype=np.int64) * 3 + 1), _dev(conf))
    _, _, root = twin.run(cloud, None, r2, 0)
    _, roots, sizes = twin.labels(root)
    for kw, keep in ((dict(radius=0.25, min_size=30), np.nonzero(np.isin(root, roots[sizes >= 30]))[0]),
                     (dict(radius=0.25, keep_largest=True), np.nonzero(root == roots[0])[0])):
        out = postprocess.remove_small_clusters(pc, **kw)
        assert 0 < len(keep) < len(cloud) and len(out) == len(keep) and out.points.cpu().numpy().tobytes() == cloud[keep].tobytes()
        assert out.colors.cpu().numpy().tobytes() == colors[keep].tobytes() and out.conf.cpu().numpy().tobytes() == conf[keep].tobytes()
        assert out.indices.cpu().numpy().tolist() == (keep * 3 + 1).tolist()
        assert out.scene_scale is scale and out.extrinsic is pc.extrinsic and out.transform is pc.transform and out.conf_threshold is pc.conf_threshold
    rel_r2 = radius_twin.radius_sq(float(F(0.1) * F(2.0)))
    want = twin.run(cloud, None, rel_r2, 2)
    res = postprocess.cluster_points(pc, rel_radius=0.1, min_neighbours=2)
    assert res.root.cpu().numpy().tobytes() == want[2].tobytes() and res.kind.cpu().numpy().tobytes() == want[1].tobytes()
    out = postprocess.remove_small_clusters(pc, rel_radius=0.1, min_size=5, min_neighbours=2)
    _, roots, sizes = twin.labels(want[2])
    assert out.indices.cpu().numpy().tolist() == (np.nonzero(np.isin(want[2], roots[sizes >= 5]))[0] * 3 + 1).tolist()
    col = postprocess.cluster_colors(res.labels)
    assert col.is_cuda and col.shape == (len(cloud), 3) and torch.equal(col.cpu(), postprocess.cluster_colors(res.labels.cpu()))
    assert bool((col[res.labels < 0] == 128).all())


def test_cloud_of_real_views_matches_twin():
    L.require_gpu()
    g = np.load(REAL)
    depth, ext = g["depth"].astype(F), g["extrinsics"][0]
    S, H, W = depth.shape
    pts = ctwin.unproject64(depth, ext, g["intrinsics"][0])
    sub = np.zeros((S, H, W), bool)
    sub[:, ::6, ::6] = True
    sub &= depth > 0
    P = np.ascontiguousarray(pts.reshape(-1, 3)[np.nonzero(sub.reshape(-1))[0]]).astype(F)
    assert 10000 < len(P) < 25000
    radius, mn = 0.15, 4
    want = twin.run(P, None, radius_twin.radius_sq(radius), mn, budget=1 << 24)
    res = postprocess.cluster_points(_dev(P), radius=radius, min_neighbours=mn)
    for g_, w in ((res.degree, want[0]), (res.kind, want[1]), (res.root, want[2])):
        assert g_.cpu().numpy().tobytes() == w.tobytes()
    lab, roots, sizes = twin.labels(want[2])
    assert res.labels.cpu().numpy().tobytes() == lab.tobytes() and res.sizes.cpu().numpy().tobytes() == sizes.tobytes()
    print("real views: %d points, %d clusters, largest %d, %d border, %d noise" % (len(P), len(sizes), sizes[0], (want[1] == BORDER).sum(), (want[1] == NOISE).sum()))
    assert len(sizes) > 1 and (want[1] == BORDER).any() and (want[1] == NOISE).any() and sizes[0] > len(P) // 10
