"""ovg_knn_search / ovg_knn_normals and postprocess.knn_neighbours, estimate_normals, statistical_outlier_mask and
remove_statistical_outliers on the device against the brute force of tests/knn_twin.py: count, index and sqdist byte for byte in
exact-size guarded buffers -- shapes around the query block and the hash table's minimum, every k around the four kernel instances,
both radii, both cell edges, a moved origin, crafted inputs (exact ties, duplicates, k above the cloud, one cell, far offsets, no
usable reference, unusable queries), composition with ovg_radius_search, the work guard, a medium case, the covariance byte for byte
and the normals against numpy's eigh, orientation on real views, and the statistical filter against numpy."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import knn_twin as twin
import nn_twin
import radius_twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
QB = L.RS_QUERY_BLOCK
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)              # every instance (4, 8, 16, 32) and the sizes just above each
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
FILL32 = -0x5A5A5A5B                             # kernel_guards' fill byte 0xA5 four times, as int32


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("count", "index", "sqdist")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, int((g.view(np.int32) != w.view(np.int32)).sum()))


def _prefix(want, k):
    """The twin's result for k from its result for a larger k (tests/test_knn_host.py proves the prefix property of the twin)."""
    return want[0], np.ascontiguousarray(want[1][:, :k]), np.ascontiguousarray(want[2][:, :k])


def _grid(q, r, r2, cell=None, origin=None, qv=None, rv=None, exclude_self=False):
    """BUILD in an exact-size workspace. -> (the search arguments, [flags, cells, largest, pairs])"""
    cell = radius_twin.reach(r2) if cell is None else cell
    ws = torch.empty(ops.radius_workspace_bytes(len(q), len(r)), device="cuda", dtype=torch.uint8)
    args = dict(query=_dev(q), reference=_dev(r), radius_sq=float(r2), cell=float(cell), ws=ws, query_valid=_dev(qv), reference_valid=_dev(rv),
                origin=None if origin is None else _dev(np.asarray(origin, F)), exclude_self=exclude_self)
    return args, ops.radius_search(L.RS_BUILD, **args)[0].cpu().tolist()


def _knn(args, k, max_pairs=1 << 40, out_stats=None):
    """ovg_knn_search into exact-size guarded outputs: nothing may be written outside them. -> (count [nq], index [nq, k], sqdist [nq, k])"""
    nq = args["query"].shape[0]
    count, check_c = guarded((1, nq), torch.int32, "cuda", guard_bytes=4096)
    index, check_i = guarded((nq, k), torch.int32, "cuda", guard_bytes=4096)
    sqdist, check_s = guarded((nq, k), torch.float32, "cuda", guard_bytes=4096)
    out = ops.knn_search(k=k, max_pairs=max_pairs, out_stats=out_stats, count=count[0], index=index, sqdist=sqdist, **args)
    torch.cuda.synchronize()
    check_c("count"), check_i("index"), check_s("sqdist")
    assert out[0] is out_stats
    return count[0], index, sqdist


def _check(q, r, r2, ks, cell=None, origin=None, qv=None, rv=None, exclude_self=False, name=""):
    want = twin.search(q, r, r2, max(ks), qv, rv, exclude_self=exclude_self)
    args, stats = _grid(q, r, r2, cell, origin, qv, rv, exclude_self)
    assert stats[0] == 0
    for k in ks:
        _same(_knn(args, k), _prefix(want, k), "%s k %d" % (name, k))
    return want


@pytest.mark.parametrize("nr", [1, 65, 513, 1025])
def test_shapes_around_the_block_and_every_k_match_twin_bit_exactly(nr):
    """nq around the query block of 256 threads; nr = 1 and 65 stay in the 1024-slot minimum table, 513 is the first nr whose 2 nr
    slots exceed it, 1025 takes a second tile of the scan; k walks through all four instances. At radius 0.25 most rows are
    partial (the padding path); rows with more than 8 candidates overflow the two smaller instances."""
    L.require_gpu()
    assert QB == 256 and L.KNN_MAX_K == 32
    nqs = (1, 63, QB - 1, QB, QB + 1, 2 * QB + 1)
    q, r, qv, rv = nn_twin.scene(max(nqs), 1025, seed=0)
    partial, full = 0, 0
    for nq in nqs:
        for radius in (0.25, 0.5):
            r2 = radius_twin.radius_sq(radius)
            name = "%d x %d radius %g" % (nq, nr, radius)
            want = _check(q[:nq], r[:nr], r2, KS, None, None, qv[:nq], rv[:nr], name=name + " masks")
            _check(q[:nq], r[:nr], r2, KS, name=name)
            partial += int(((want[0] > 0) & (want[0] < 16)).sum())
            full += int((want[0] > 8).sum())
    for cell, origin in ((F(2) * radius_twin.reach(radius_twin.radius_sq(0.5)), None), (None, (0.37, -5.0, 1e3))):
        _check(q[:QB + 1], r[:nr], radius_twin.radius_sq(0.5), (5, 16), cell, origin, qv[:QB + 1], rv[:nr], name="%d cell %r origin %r" % (nr, cell, origin))
    assert nr < 1025 or (partial > 1000 and full > 50)


def test_crafted_inputs_match_twin():
    L.require_gpu()
    rng = np.random.default_rng(1)
    ql, rl = (rng.integers(-8, 9, (1500, 3)) / 4.0).astype(F), (rng.integers(-8, 9, (2500, 3)) / 4.0).astype(F)
    want = _check(ql, rl, radius_twin.radius_sq(0.25), (4, 7, 16), name="quarter lattice")
    ties = (want[2][:, 1:] == want[2][:, :-1]) & (want[1][:, 1:] >= 0)
    assert ties.sum() > 300 and (want[1][:, 1:][ties] > want[1][:, :-1][ties]).all()       # runs of exact ties: ordered by index
    assert ((want[2] == F(0.0625)) & (want[1] >= 0)).sum() > 100                           # neighbours exactly at d == radius_sq
    c, _, cv, _ = nn_twin.scene(3 * QB + 17, 0, seed=2, same=True)
    assert len(np.unique(c[np.isfinite(c).all(1)], axis=0)) < np.isfinite(c).all(1).sum()
    want = _check(c, c, radius_twin.radius_sq(0.25), (1, 6, 32), None, None, cv, cv, exclude_self=True, name="exclude-self with duplicates")
    ok = want[1] >= 0
    assert (want[1][ok] != np.nonzero(ok)[0]).all() and (want[2][ok] == 0).any()
    plain = _check(c, c, radius_twin.radius_sq(0.25), (6,), None, None, cv, cv, name="same cloud")
    use = nn_twin.usable(c, cv)
    assert (plain[1][use, 0] <= np.nonzero(use)[0]).all() and (plain[2][use, 0] == 0).all()     # rank 0: the point itself, or a lower-index duplicate
    want = _check(ql[:300], rl[:5], radius_twin.radius_sq(3.0), (8, 32), name="k above nr")
    assert (want[1][:, 5:] == -1).all() and (want[0] <= 5).all() and (want[0] == 5).any()
    ball = (rng.random((700, 3)) * 0.2).astype(F)
    args, stats = _grid(ball[:300], ball[300:], radius_twin.radius_sq(0.25), F(1e6))
    assert stats == [0, 1, 400, 300 * 400]                                   # every reference in ONE cell, every query scans it
    for k in (3, 32):
        _same(_knn(args, k), twin.search(ball[:300], ball[300:], radius_twin.radius_sq(0.25), k), "one cell k %d" % k)
    far = (rng.random((900, 3)) * 0.6 + 16384.0).astype(F)
    want = _check(far[:400], far[400:], radius_twin.radius_sq(0.05), (4, 12), name="offset 16384")
    assert (want[0] > 1).mean() > 0.2
    _check(far[:400], far[400:], radius_twin.radius_sq(0.05), (12,), None, (16384.0, 16384.0, 16384.0), name="offset 16384, origin there")
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    want = _check(ball[:5], bad, radius_twin.radius_sq(0.25), (2,), name="no usable reference")
    assert (want[0] == 0).all() and (want[1] == -1).all()
    qs = np.concatenate([bad, ball[:4]])
    want = _check(qs, ball[300:], radius_twin.radius_sq(0.25), (5, 20), None, None, np.array([1, 1, 1, 0, 1, 1, 1], np.uint8), name="unusable queries")
    assert want[0][:4].tolist() == [0, 0, 0, 0] and (want[1][:4] == -1).all() and np.isposinf(want[2][:4]).all() and (want[0][4:] == 400).all()


def test_composition_with_the_radius_search_and_between_k():
    L.require_gpu()
    q, r, qv, rv = nn_twin.scene(700, 900, seed=1)
    r2 = radius_twin.radius_sq(0.5)
    args, _ = _grid(q, r, r2, None, None, qv, rv)
    _, count, index, sqdist = ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, **args)
    wide = _knn(args, 32)
    for k in KS:
        got = _knn(args, k)
        assert torch.equal(got[0], count), k                                # the count of the radius search
        assert torch.equal(got[1][:, 0], index) and torch.equal(got[2][:, 0].view(torch.int32), sqdist.view(torch.int32)), k    # rank 0: its nearest
        assert torch.equal(got[1], wide[1][:, :k]) and torch.equal(got[2].view(torch.int32), wide[2][:, :k].view(torch.int32)), k
        again = _knn(args, k)
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    # another cell edge and origin: another grid, the same bytes
    other, _ = _grid(q, r, r2, F(3.0), (1.0, 2.0, 3.0), qv, rv)
    for a, b in zip(_knn(other, 32), wide):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(_knn(args, 5)[1], wide[1][:, :5])


def test_guards_refuse_without_writing_and_nothing_is_written_behind_the_buffers():
    L.require_gpu()
    nq, nr, k = QB + 3, 5 * 512 + 1, 7
    q, r, qv, rv = nn_twin.scene(nq, nr, seed=4)
    r2 = radius_twin.radius_sq(0.5)
    need = ops.radius_workspace_bytes(nq, nr)
    ws = torch.full((need + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    stats, check_t = guarded((1, 4), torch.int64, "cuda")
    args = dict(query=_dev(q), reference=_dev(r), radius_sq=float(r2), cell=float(radius_twin.reach(r2)), ws=ws[:need], query_valid=_dev(qv),
                reference_valid=_dev(rv))
    # a workspace no BUILD has filled: refused, the outputs keep their fill pattern, and out_stats says so
    got = _knn(args, k, out_stats=stats[0])
    assert stats[0].tolist() == [L.RS_NOT_BUILT, 0, 0, 0]
    for t in got:
        assert bool((t.view(torch.int32) == FILL32).all())
    built = ops.radius_search(L.RS_BUILD, **args)[0].tolist()
    occupied, largest, pairs, _ = radius_twin.box_stats(q, r, r2, radius_twin.reach(r2), (0.0, 0.0, 0.0), qv, rv)
    assert built == [0, occupied, largest, pairs] and pairs > 1000
    got = _knn(args, k, max_pairs=pairs - 1, out_stats=stats[0])            # one pair over the budget
    assert stats[0].tolist() == [L.RS_OVER_BUDGET, occupied, largest, pairs]
    for t in got:
        assert bool((t.view(torch.int32) == FILL32).all())
    got = _knn(args, k, max_pairs=pairs, out_stats=stats[0])                # exactly the budget
    assert stats[0].tolist() == [0, occupied, largest, pairs]
    check_t("out_stats")
    assert bool((ws[need:] == 0xA5).all())
    _same(got, twin.search(q, r, r2, k, qv, rv), "guarded")
    with pytest.raises(ValueError, match="candidate pairs"):
        postprocess.knn_neighbours(_dev(q), _dev(r), k, 0.5, max_pairs=1000)
    with pytest.raises(L.OvgError):
        ops.knn_search(k=33, **args)


def test_public_entry_shapes_masks_and_empty_sides():
    L.require_gpu()
    rng = np.random.default_rng(1)
    ql, rl = (rng.integers(-8, 9, (1200, 3)) / 4.0).astype(F), (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    want = twin.search(ql, rl, radius_twin.radius_sq(0.25), 6)
    res = postprocess.knn_neighbours(_dev(ql.reshape(12, 100, 3)), _dev(rl.reshape(7, 100, 3)), 6, 0.25, reference_valid=_dev(np.ones((7, 100), bool)))
    assert res.count.shape == (12, 100) and res.index.shape == res.sqdist.shape == (12, 100, 6)
    _same((res.count.reshape(-1), res.index.reshape(-1, 6), res.sqdist.reshape(-1, 6)), want, "leading shapes")
    res = postprocess.knn_neighbours(_dev(ql), _dev(rl), 6, 0.25, cell_size=0.9, origin=(0.1, -3.0, 77.0), max_pairs=int(1200 * 700))
    _same((res.count, res.index, res.sqdist), want, "cell_size, origin, max_pairs")
    qv = rng.random(1200) < 0.7
    res = postprocess.knn_neighbours(_dev(ql), _dev(rl), 6, 0.25, query_valid=_dev(qv))
    _same((res.count, res.index, res.sqdist), twin.search(ql, rl, radius_twin.radius_sq(0.25), 6, qv), "bool mask")
    cloud = postprocess.PointCloud(_dev(rl), None, None, None, None, None)
    res = postprocess.knn_neighbours(cloud, cloud, 9, 0.5, exclude_self=True)
    _same((res.count, res.index, res.sqdist), twin.search(rl, rl, radius_twin.radius_sq(0.5), 9, exclude_self=True), "PointCloud")
    res = postprocess.knn_neighbours(_dev(ql[:8]), _dev(rl[:0]), 3, 0.25)
    assert (res.count == 0).all() and (res.index == -1).all() and torch.isposinf(res.sqdist).all()
    assert res.count.dtype == res.index.dtype == torch.int32 and res.sqdist.dtype == torch.float32 and res.index.shape == (8, 3) and res.count.shape == (8,)
    assert postprocess.knn_neighbours(_dev(ql[:0]), _dev(rl), 3, 0.25).index.shape == (0, 3)


def test_medium_case_against_twin_on_a_sample():
    L.require_gpu()
    n, k = 20000, 16
    q, r, qv, rv = nn_twin.scene(n, n, seed=5)
    r2 = radius_twin.radius_sq(0.2)
    args, stats = _grid(q, r, r2, None, None, qv, rv)
    count, index, sqdist = (t.cpu().numpy() for t in _knn(args, k))
    rows = np.random.default_rng(6).choice(n, 512, replace=False)
    want = twin.search(q, r, r2, k, qv, rv, rows=rows)
    assert count[rows].tobytes() == want[0].tobytes() and index[rows].tobytes() == want[1].tobytes() and sqdist[rows].tobytes() == want[2].tobytes()
    assert (want[0] > k).any() and ((want[0] > 0) & (want[0] < k)).any() and (want[0] == 0).any()
    found = np.minimum(count, k)[:, None]
    pad = np.arange(k)[None, :] >= found
    assert (index[pad] == -1).all() and np.isposinf(sqdist[pad]).all() and ((index[~pad] >= 0) & (index[~pad] < n)).all()
    assert nn_twin.usable(r, rv)[index[~pad]].all() and (sqdist[~pad] <= r2).all()
    assert (sqdist[:, 1:][~pad[:, 1:]] >= sqdist[:, :-1][~pad[:, 1:]]).all()
    assert stats[3] >= int(count.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------------------------------------------

_TABLES = {}


def _table(seed, n):
    """A cloud of nn_twin.scene, its k = 16 neighbour table at radius 0.5 by the twin (computed once, left unchanged) and the twin's
    covariance and eigh normals."""
    if seed not in _TABLES:
        c, _, cv, _ = nn_twin.scene(n, 0, seed=seed, same=True)
        index = twin.search(c, c, radius_twin.radius_sq(0.5), 16, cv, cv)[1]
        cov, used = twin.covariance(c, c, index)
        _TABLES[seed] = (c, cv, index, cov, used)
    return _TABLES[seed]


def _well_separated(lam, used):
    """Rows whose normal is determined: m >= 3 and lambda1 - lambda0 >= 1e-6 lambda2. The condition may leave out at most 3 % of
    the rows with m >= 3."""
    have = used >= 3
    good = have & (lam[:, 1] - lam[:, 0] >= 1e-6 * lam[:, 2])
    assert have.sum() > 1000 and good.sum() >= 0.97 * have.sum(), (have.sum(), good.sum())
    return have, good


@pytest.mark.parametrize("seed,n", [(0, 1500), (3, 2000)])
def test_covariance_is_the_twins_bytes_and_normals_agree_with_eigh(seed, n):
    """float64 solvers differ by about 1e-14 lambda2 in the matrix; by Davis-Kahan the eigenvector then turns by at most about
    1e-14 lambda2 / (lambda1 - lambda0) <= 1e-8 where the gap is at least 1e-6 lambda2, and 1 - cos of that is far below the float32
    rounding of the stored normal (each component within 2^-24: 1 - |dot| <= about 1e-7). Bound: 1e-6."""
    L.require_gpu()
    c, cv, index, cov, used = _table(seed, n)
    dindex = _dev(index)
    got_index = _knn(_grid(c, c, radius_twin.radius_sq(0.5), None, None, cv, cv)[0], 16)[1]
    assert torch.equal(got_index, dindex)                                   # the table the device search writes is the twin's
    normal, check_n = guarded((n, 3), torch.float32, "cuda")
    curv, check_c = guarded((1, n), torch.float32, "cuda")
    dcov, check_v = guarded((n, 6), torch.float64, "cuda")
    dused, check_u = guarded((1, n), torch.int32, "cuda")
    ops.knn_normals(_dev(c), _dev(c), dindex, normal=normal, curvature=curv[0], covariance=dcov, used=dused[0])
    torch.cuda.synchronize()
    check_n("normal"), check_c("curvature"), check_v("covariance"), check_u("used")
    assert dused[0].cpu().numpy().tobytes() == used.tobytes()
    assert dcov.cpu().numpy().tobytes() == cov.tobytes()
    want, lam, solved = twin.normals(c, c, index)
    have, good = _well_separated(lam, used)
    assert (solved == have).all()
    g = normal.cpu().numpy().astype(np.float64)
    worst = (1 - np.abs((g[good] * want[good]).sum(1))).max()
    print("seed %d: %d rows with m >= 3, %d compared, worst 1 - |dot| = %.3g" % (seed, have.sum(), good.sum(), worst))
    assert worst <= 1e-6
    assert np.abs(np.linalg.norm(g[have], axis=1) - 1).max() <= 2.0 ** -22
    assert (g[~have] == 0).all() and (~have).sum() > 10 and (curv[0].cpu().numpy()[~have] == 0).all()       # rows with m < 3: zeros
    cu = curv[0].cpu().numpy().astype(np.float64)[have]
    total = lam[have].sum(1)
    ref = np.where(total > 0, lam[have, 0].clip(0) / np.where(total > 0, total, 1.0), 0.0)    # coincident neighbours: trace 0, curvature 0
    assert (cu >= 0).all() and (cu <= 1 / 3 + 1e-6).all() and np.abs(cu - ref).max() <= 1e-6
    # without a viewpoint: the component of largest magnitude is positive. The device decides on the float64 components, which the
    # float32 rounding can make equal (normals like (-1, 1, 0) / sqrt 2 on the lattice): a largest component within one float32
    # spacing of the maximum must be positive
    top = np.abs(g) >= np.abs(g).max(1, keepdims=True) - 2.0 ** -23
    assert ((g > 0) & top).any(1)[have].all()


def _orientation_agrees(normal, want, q, v, good):
    """Signs agree with the twin wherever |dot(n, v - q)| > 1e-6 |v - q| (the twin's normal and the device's differ by far less)."""
    d = np.asarray(v, np.float64).reshape(-1, 3) - q.astype(np.float64)
    with np.errstate(all="ignore"):
        dot = (want * d).sum(1)
        clear = good & (np.abs(dot) > 1e-6 * np.linalg.norm(d, axis=1))
    assert clear.sum() >= 0.95 * good.sum()
    g = normal.cpu().numpy().astype(np.float64)
    assert ((g[clear] * want[clear]).sum(1) > 0).all() and ((g[clear] * d[clear]).sum(1) > 0).all()
    return clear


def test_orientation_towards_shared_and_per_point_viewpoints():
    L.require_gpu()
    c, cv, index, cov, used = _table(3, 2000)
    _, lam, _ = twin.normals(c, c, index)
    _, good = _well_separated(lam, used)
    shared = np.array([0.5, -7.0, 3.0], F)
    want = twin.normals(c, c, index, viewpoint=shared)[0]
    got = ops.knn_normals(_dev(c), _dev(c), _dev(index), viewpoint=_dev(shared))[0]
    _orientation_agrees(got, want, c, shared, good)
    per = np.random.default_rng(9).normal(0.0, 5.0, (2000, 3)).astype(F)
    want = twin.normals(c, c, index, viewpoint=per)[0]
    got = ops.knn_normals(_dev(c), _dev(c), _dev(index), viewpoint=_dev(per))[0]
    clear = _orientation_agrees(got, want, c, per, good)
    flipped = ops.knn_normals(_dev(c), _dev(c), _dev(index), viewpoint=_dev((2 * c - per).astype(F)))[0].cpu().numpy()
    far = clear & (np.abs(c).max(1) < 100)                                  # 2 c - v mirrors the viewpoint through the point: the other side
    assert ((flipped[far].astype(np.float64) * want[far]).sum(1) < 0).all()
    # through the public entry: the same table, the same normals
    pub = postprocess.estimate_normals(_dev(c.reshape(4, 500, 3)), k=16, radius=0.5, viewpoint=(0.5, -7.0, 3.0), valid=_dev(cv.reshape(4, 500)))
    ref = ops.knn_normals(_dev(c), _dev(c), _dev(index), viewpoint=_dev(shared))[0]
    assert pub.shape == (4, 500, 3) and torch.equal(pub.reshape(-1, 3).view(torch.int32), ref.view(torch.int32))
    pub, curv = postprocess.estimate_normals(_dev(c), k=16, radius=0.5, viewpoint=_dev(per), valid=_dev(cv), return_curvature=True)
    assert torch.equal(pub.view(torch.int32), got.view(torch.int32)) and curv.shape == (2000,) and curv.dtype == torch.float32
    empty = postprocess.estimate_normals(_dev(c[:0]), radius=0.5, return_curvature=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


def test_cameras_orient_the_normals_of_real_views():
    L.require_gpu()
    g = np.load(REAL)
    depth, ext = g["depth"].astype(F), g["extrinsics"][0]
    S, H, W = depth.shape
    pts = ctwin.unproject64(depth, ext, g["intrinsics"][0])
    step = 10
    sub = np.zeros((S, H, W), bool)
    sub[:, ::step, ::step] = True
    sub &= depth > 0
    flat = np.nonzero(sub.reshape(-1))[0]
    P = pts.reshape(-1, 3)[flat]
    radius = 0.5
    index = twin.search(P, P, radius_twin.radius_sq(radius), 12, budget=1 << 24)[1]
    centres = np.stack([-(ext[s, :, :3].astype(np.float64).T @ ext[s, :, 3].astype(np.float64)) for s in range(S)]).astype(F)
    view = flat // (H * W)
    assert len(np.unique(view)) == S
    want, lam, solved = twin.normals(P, P, index, viewpoint=centres[view])
    used = (index >= 0).sum(1).astype(np.int32)
    have = used >= 3
    good = have & (lam[:, 1] - lam[:, 0] >= 1e-6 * lam[:, 2])
    assert have.mean() > 0.8 and good.sum() >= 0.97 * have.sum()
    cloud = postprocess.PointCloud(_dev(P), None, None, torch.tensor(1.0, device="cuda"), np.eye(4), _dev(ext), _dev(flat.astype(np.int64)), None)
    got = postprocess.estimate_normals(cloud, k=12, radius=radius, viewpoint="cameras", image_hw=(H, W))
    assert got.shape == (len(P), 3) and got.dtype == torch.float32
    clear = _orientation_agrees(got, want, P, centres[view], good)
    gn = got.cpu().numpy().astype(np.float64)
    assert (1 - np.abs((gn[good] * want[good]).sum(1))).max() <= 1e-6
    # a surface a camera sees faces it: the oriented normal and the viewing ray make an acute angle by construction, and on
    # these views most surfaces are seen at more than a grazing angle
    ray = centres[view].astype(np.float64) - P.astype(np.float64)
    cosine = (gn[clear] * ray[clear]).sum(1) / np.linalg.norm(ray[clear], axis=1)
    assert (cosine > 0).all() and np.median(cosine) > 0.3


def test_plane_of_exactly_representable_points_and_rows_of_fewer_than_three():
    L.require_gpu()
    x, y = np.meshgrid(np.arange(40), np.arange(30), indexing="ij")
    plane = np.stack([x.reshape(-1) * 0.25, y.reshape(-1) * 0.5, np.full(1200, 2.0)], 1).astype(F)
    lone = np.array([[100.0, 100.0, 100.0], [100.25, 100.0, 100.0], [500.0, 0.0, 0.0]], F)      # a pair and a single point: m = 2, 2, 1
    cloud = np.concatenate([plane, lone])
    normal, curv = postprocess.estimate_normals(_dev(cloud), k=9, radius=0.75, return_curvature=True)
    n, cu = normal.cpu().numpy(), curv.cpu().numpy()
    assert (n[:1200] == np.array([0.0, 0.0, 1.0], F)).all() and (cu[:1200] == 0).all()
    assert (n[1200:] == 0).all() and (cu[1200:] == 0).all()
    down = postprocess.estimate_normals(_dev(cloud), k=9, radius=0.75, viewpoint=(3.0, 3.0, -10.0)).cpu().numpy()
    assert (down[:1200] == np.array([0.0, 0.0, -1.0], F)).all() and (down[1200:] == 0).all()
    res = postprocess.knn_neighbours(_dev(cloud), _dev(cloud), 9, 0.75)
    _, _, cov, used = ops.knn_normals(_dev(cloud), _dev(cloud), res.index, covariance=True, used=True)
    assert used[1200:].tolist() == [2, 2, 1] and bool((used[:1200] >= 6).all())
    assert bool((cov[:1200][:, [2, 4, 5]] == 0).all()) and bool((cov[1202] == 0).all())
    table = _dev(np.array([[0, 1, 40, -1], [0, 5000, -1, 1], [-1, -1, -1, -1]], np.int32))       # skipped entries; m = 3, 2, 0
    nrm, _, cov, used = ops.knn_normals(_dev(cloud[:3]), _dev(cloud), table, covariance=True, used=True)
    want_c, want_m = twin.covariance(cloud[:3], cloud, table.cpu().numpy())
    assert used.tolist() == [3, 2, 0] and cov.cpu().numpy().tobytes() == want_c.tobytes() and want_m.tolist() == [3, 2, 0]
    assert nrm.cpu().numpy().tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistical filter
# ---------------------------------------------------------------------------------------------------------------------------------

def _want_statistical(cloud, k, std_ratio, radius, valid=None):
    """numpy on the twin's table -> (mask, in the band |a - thr| <= 1e-9 thr, full rows)."""
    count, _, sq = twin.search(cloud, cloud, radius_twin.radius_sq(radius), k, valid, valid, exclude_self=True)
    full = count >= k
    with np.errstate(all="ignore"):
        a = np.sqrt(sq.astype(np.float64)).mean(1)
    thr = a[full].mean() + std_ratio * a[full].std()
    return full & (a <= thr), full & (np.abs(a - thr) <= 1e-9 * thr), full


def test_statistical_outlier_mask_and_removal_against_numpy(tmp_path):
    L.require_gpu()
    rng = np.random.default_rng(11)
    surface = np.stack([rng.random(3000) * 4, rng.random(3000) * 4, np.zeros(3000)], 1) + rng.normal(0.0, 0.01, (3000, 3))
    floaters = np.stack([rng.random(60) * 4, rng.random(60) * 4, 0.15 + rng.random(60) * 0.2], 1)          # within the radius of the surface, but sparse
    isolated = np.array([[50.0, 50.0, 50.0], [-30.0, 2.0, 1.0]])                                            # nothing within the radius: count < k
    cloud = np.concatenate([surface, floaters, isolated]).astype(F)
    perm = rng.permutation(len(cloud))
    cloud, kind = cloud[perm], np.concatenate([np.zeros(3000, int), np.ones(60, int), np.full(2, 2)])[perm]
    cloud[7] = np.nan
    k, radius = 8, 0.6
    for std_ratio, valid in ((2.0, None), (1.0, None), (2.0, rng.random(len(cloud)) < 0.9)):
        want, band, full = _want_statistical(cloud, k, std_ratio, radius, valid)
        got = postprocess.statistical_outlier_mask(_dev(cloud), k=k, std_ratio=std_ratio, radius=radius, valid=_dev(valid)).cpu().numpy()
        assert got.dtype == bool and got.shape == (len(cloud),)
        assert band.sum() <= 2 and (got[~band] == want[~band]).all(), (int(band.sum()), int((got != want).sum()))
        assert not got[~full].any() and (~full).sum() >= 3                  # count < k: an outlier, whatever its distances
    want, band, full = _want_statistical(cloud, k, 2.0, radius)
    assert not band.any()
    assert not want[kind == 2].any() and not want[7] and want[kind == 1].mean() < 0.2 and want[kind == 0].mean() > 0.95
    shaped = postprocess.statistical_outlier_mask(_dev(cloud.reshape(2, -1, 3)), k=k, std_ratio=2.0, radius=radius)
    assert shaped.shape == (2, len(cloud) // 2) and shaped.cpu().numpy().reshape(-1).tobytes() == want.tobytes()
    colors = rng.integers(0, 256, (len(cloud), 3)).astype(np.uint8)
    conf = rng.random(len(cloud)).astype(F)
    scale = torch.tensor(2.0, device="cuda")
    pc = postprocess.PointCloud(_dev(cloud), _dev(colors), torch.tensor(0.5, device="cuda"), scale, np.eye(4), torch.zeros(2, 3, 4, device="cuda"),
                                _dev(np.arange(len(cloud), dtype=np.int64) * 3 + 1), _dev(conf))
    out = postprocess.remove_statistical_outliers(pc, k=k, std_ratio=2.0, radius=radius)
    keep = np.nonzero(want)[0]
    assert len(out) == len(keep) and out.points.cpu().numpy().tobytes() == cloud[keep].tobytes()
    assert out.colors.cpu().numpy().tobytes() == colors[keep].tobytes() and out.conf.cpu().numpy().tobytes() == conf[keep].tobytes()
    assert out.indices.cpu().numpy().tolist() == (keep * 3 + 1).tolist()
    assert out.scene_scale is scale and out.extrinsic is pc.extrinsic and out.transform is pc.transform and out.conf_threshold is pc.conf_threshold
    rel = postprocess.remove_statistical_outliers(pc, k=k, std_ratio=2.0, rel_radius=0.3)                   # f32(0.3) * f32(2.0)
    want_rel = _want_statistical(cloud, k, 2.0, float(F(0.3) * F(2.0)))[0]
    assert rel.indices.cpu().numpy().tolist() == (np.nonzero(want_rel)[0] * 3 + 1).tolist()
    path = str(tmp_path / "kept.ply")
    normals = postprocess.estimate_normals(out, k=8, radius=radius)
    postprocess.write_ply(path, out, normals=normals)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex %d\n" % len(keep) in head and b"property float nz\n" in head and len(body) == len(keep) * 27
