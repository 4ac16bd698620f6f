"""ovg_radius_search / postprocess.radius_neighbours, radius_outlier_mask, remove_radius_outliers and cloud_fscore on the device
against the brute force of tests/radius_twin.py: count, index and sqdist byte for byte -- shapes around the query block and the
hash table's minimum, both radii, both cell edges, a moved origin, crafted inputs (the inclusive boundary, duplicates, far offsets,
clamped cells, one cell, no usable reference), the grid's statistics, the work guard, guard bytes behind the workspace and the three
outputs, a medium case, agreement with the exhaustive search, floater removal on real views and F-scores against numpy."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import nn_twin
import radius_twin as twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
QB = L.RS_QUERY_BLOCK
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
ZERO = (0.0, 0.0, 0.0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("count", "index", "sqdist")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape)
        assert g.tobytes() == w.tobytes(), (name, what, int((g.view(np.int32) != w.view(np.int32)).sum()))


def _run(q, r, r2, cell=None, origin=None, qv=None, rv=None, exclude_self=False, max_pairs=1 << 40):
    """BUILD, the statistics, SEARCH through the thin wrapper, in an exact-size workspace. -> ([flags, cells, largest, pairs], outputs)"""
    cell = twin.reach(r2) if cell is None else cell
    ws = torch.empty(ops.radius_workspace_bytes(len(q), len(r)), device="cuda", dtype=torch.uint8)
    args = dict(query=_dev(q), reference=_dev(r), radius_sq=float(r2), cell=float(cell), ws=ws, query_valid=_dev(qv), reference_valid=_dev(rv),
                origin=None if origin is None else _dev(np.asarray(origin, F)), exclude_self=exclude_self)
    stats = ops.radius_search(L.RS_BUILD, **args)[0].cpu().tolist()
    out = ops.radius_search(L.RS_SEARCH, max_pairs=max_pairs, **args)
    assert out[0] is None
    return stats, out[1:]


def _check(q, r, r2, cell=None, origin=None, qv=None, rv=None, exclude_self=False, name=""):
    want = twin.search(q, r, r2, qv, rv, exclude_self=exclude_self)
    stats, got = _run(q, r, r2, cell, origin, qv, rv, exclude_self)
    _same(got, want, name)
    occupied, largest, pairs, _ = twin.box_stats(q, r, r2, twin.reach(r2) if cell is None else cell, ZERO if origin is None else origin, qv, rv)
    assert stats == [0, occupied, largest, pairs], (name, stats, (occupied, largest, pairs))
    assert pairs >= int(want[0].sum())
    return want


@pytest.mark.parametrize("nr", [1, 65, 511, 513, 1025])
def test_shapes_around_the_block_and_the_table_minimum_match_twin_bit_exactly(nr):
    """nq around the query block of 256 threads; nr = 1, 65 and 511 stay in the 1024-slot minimum table, 513 is the first nr whose 2 nr
    slots exceed it, 1025 takes a second tile of the scan."""
    L.require_gpu()
    assert QB == 256 and L.RS_MIN_SLOTS == 1024
    nqs = (1, 63, QB - 1, QB, QB + 1, 2 * QB + 1)
    q, r, qv, rv = nn_twin.scene(max(nqs), 1025, seed=0)
    some = 0
    for nq in nqs:
        for radius in (0.25, 0.5):
            r2 = twin.radius_sq(radius)
            for cell in (twin.reach(r2), F(2) * twin.reach(r2)):
                name = "%d x %d radius %g cell %g" % (nq, nr, radius, cell)
                want = _check(q[:nq], r[:nr], r2, cell, None, qv[:nq], rv[:nr], name=name + " masks")
                _check(q[:nq], r[:nr], r2, cell, name=name)
                some += int((want[0] > 0).sum())
        _check(q[:nq], r[:nr], twin.radius_sq(0.25), None, (0.37, -5.0, 1e3), qv[:nq], rv[:nr], name="%d x %d moved origin" % (nq, nr))
    assert some > 0 or nr == 1


def test_two_calls_and_every_cell_edge_give_identical_bytes():
    L.require_gpu()
    q, r, qv, rv = nn_twin.scene(700, 900, seed=1)
    r2 = twin.radius_sq(0.5)
    first = _run(q, r, r2, None, None, qv, rv)
    for cell, origin in ((None, None), (F(0.7), None), (F(3.0), (1.0, 2.0, 3.0)), (F(1e6), None), (None, (-1e4, 1e4, 0.5))):
        again = _run(q, r, r2, cell, origin, qv, rv)
        for a, b in zip(first[1], again[1]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (cell, origin)
    assert _run(q, r, r2, None, None, qv, rv)[0] == first[0]
    one = _run(q, r, r2, F(1e6), None, qv, rv)[0]                            # an edge of 1e6: the near points share cell 0 / -1 per axis
    assert one[1] < first[0][1] and one[3] >= first[0][3]


def test_crafted_inputs_match_twin():
    L.require_gpu()
    rng = np.random.default_rng(1)
    ql, rl = (rng.integers(-8, 9, (5000, 3)) / 4.0).astype(F), (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    want = _check(ql, rl, twin.radius_sq(0.25), name="lattice boundary")
    assert ((want[2] == F(0.0625)) & (want[0] > 0)).sum() > 100             # nearest exactly at d == radius_sq: the inclusive bound
    c, _, cv, _ = nn_twin.scene(3 * QB + 17, 0, seed=2, same=True)
    assert len(np.unique(c[np.isfinite(c).all(1)], axis=0)) < np.isfinite(c).all(1).sum()
    want = _check(c, c, twin.radius_sq(0.25), None, None, cv, cv, exclude_self=True, name="exclude-self with duplicates")
    ok = want[1] >= 0
    assert (want[1][ok] != np.nonzero(ok)[0]).all() and (want[2][ok] == 0).any()
    plain = _check(c, c, twin.radius_sq(0.25), None, None, cv, cv, name="same cloud")
    assert (plain[0] >= want[0]).all() and (plain[0][nn_twin.usable(c, cv)] == want[0][nn_twin.usable(c, cv)] + 1).all()
    far = (rng.random((900, 3)) * 0.6 + 16384.0).astype(F)
    want = _check(far[:400], far[400:], twin.radius_sq(0.05), name="offset 16384")
    assert (want[0] > 0).mean() > 0.3
    _check(far[:400], far[400:], twin.radius_sq(0.05), None, (16384.0, 16384.0, 16384.0), name="offset 16384, origin there")
    big = np.array([[1e20, 0, 0], [1e20, 0.1, 0], [-1e20, 0, 0], [0, 9e20, 0.1], [0, 9e20, 0], [3e38, 3e38, -3e38], [0, 0, 0], [0.1, 0, 0]], F)
    want = _check(big, big, twin.radius_sq(0.25), name="clamped cells")
    assert want[0].tolist() == [2, 2, 1, 2, 2, 1, 2, 2]
    _check(big, big, twin.radius_sq(0.25), None, (1e20, -1e20, 3e38), exclude_self=True, name="clamped cells, far origin")
    ball = (rng.random((700, 3)) * 0.2).astype(F)
    stats, got = _run(ball[:300], ball[300:], twin.radius_sq(0.25), F(0.6))
    assert stats == [0, 1, 400, 300 * 400]                                   # every reference in ONE cell, every query scans it
    _same(got, twin.search(ball[:300], ball[300:], twin.radius_sq(0.25)), "one cell")
    r = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    stats, got = _run(ball[:5], r, twin.radius_sq(0.25))
    assert stats == [0, 0, 0, 0]
    _same(got, twin.search(ball[:5], r, twin.radius_sq(0.25)), "all references unusable")
    stats, got = _run(ball[:5], ball[5:9], twin.radius_sq(0.25), rv=np.zeros(4, np.uint8))
    assert stats == [0, 0, 0, 0] and (got[0] == 0).all() and (got[1] == -1).all() and torch.isposinf(got[2]).all()


def test_public_entry_shapes_masks_clouds_and_empty_sides():
    L.require_gpu()
    rng = np.random.default_rng(1)
    ql, rl = (rng.integers(-8, 9, (5000, 3)) / 4.0).astype(F), (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    want = twin.search(ql, rl, twin.radius_sq(0.25))
    res = postprocess.radius_neighbours(_dev(ql.reshape(50, 100, 3)), _dev(rl.reshape(7, 100, 3)), 0.25, reference_valid=_dev(np.ones((7, 100), bool)))
    assert res.count.shape == res.index.shape == res.sqdist.shape == (50, 100)
    _same((res.count.reshape(-1), res.index.reshape(-1), res.sqdist.reshape(-1)), want, "leading shapes")
    res = postprocess.radius_neighbours(_dev(ql), _dev(rl), 0.25, cell_size=0.9, origin=(0.1, -3.0, 77.0), max_pairs=int(5000 * 700))
    _same((res.count, res.index, res.sqdist), want, "cell_size, origin, max_pairs")
    res = postprocess.radius_neighbours(_dev(ql), _dev(rl), 0.25, origin=_dev(np.array([0.1, -3.0, 77.0], F)))
    _same((res.count, res.index, res.sqdist), want, "device origin")
    with pytest.raises(ValueError, match="origin"):
        postprocess.radius_neighbours(_dev(ql), _dev(rl), 0.25, origin=_dev(np.array([0.1, np.nan, 77.0], F)))
    qv = rng.random(5000) < 0.7
    res = postprocess.radius_neighbours(_dev(ql), _dev(rl), 0.25, query_valid=_dev(qv))
    _same((res.count, res.index, res.sqdist), twin.search(ql, rl, twin.radius_sq(0.25), qv), "bool mask")
    cloud = postprocess.PointCloud(_dev(rl), None, None, None, None, None)
    res = postprocess.radius_neighbours(cloud, cloud, 0.5, exclude_self=True)
    _same((res.count, res.index, res.sqdist), twin.search(rl, rl, twin.radius_sq(0.5), exclude_self=True), "PointCloud")
    res = postprocess.radius_neighbours(_dev(ql[:8]), _dev(rl[:0]), 0.25)
    assert (res.count == 0).all() and (res.index == -1).all() and torch.isposinf(res.sqdist).all()
    assert res.count.dtype == res.index.dtype == torch.int32 and res.sqdist.dtype == torch.float32 and res.index.shape == (8,)
    assert postprocess.radius_neighbours(_dev(ql[:0]), _dev(rl), 0.25).count.shape == (0,)


def test_nothing_is_written_behind_the_workspace_or_the_outputs():
    L.require_gpu()
    nq, nr = QB + 3, 5 * 512 + 1
    q, r, qv, rv = nn_twin.scene(nq, nr, seed=4)
    r2 = twin.radius_sq(0.5)
    want = twin.search(q, r, r2, qv, rv)
    need = ops.radius_workspace_bytes(nq, nr)
    ws = torch.full((need + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
    count, check_c = guarded((1, nq), torch.int32, "cuda")
    index, check_i = guarded((1, nq), torch.int32, "cuda")
    sqdist, check_s = guarded((1, nq), torch.float32, "cuda")
    stats, check_t = guarded((1, 4), torch.int64, "cuda")
    args = dict(query=_dev(q), reference=_dev(r), radius_sq=float(r2), cell=float(twin.reach(r2)), ws=ws[:need], query_valid=_dev(qv),
                reference_valid=_dev(rv))
    # SEARCH on a workspace no BUILD has filled: refused, nothing written, and said so
    out = ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, out_stats=stats[0], count=count[0], index=index[0], sqdist=sqdist[0], **args)
    torch.cuda.synchronize()
    assert stats[0].tolist() == [L.RS_NOT_BUILT, 0, 0, 0]
    for t in (count, index, sqdist):
        assert bool((t.view(torch.int32) == -0x5A5A5A5B).all())
    got = ops.radius_search(L.RS_BUILD | L.RS_SEARCH, max_pairs=1 << 40, out_stats=stats[0], count=count[0], index=index[0], sqdist=sqdist[0], **args)
    torch.cuda.synchronize()
    for chk, what in ((check_c, "count"), (check_i, "index"), (check_s, "sqdist"), (check_t, "out_stats")):
        chk(what)
    assert bool((ws[need:] == 0xA5).all())
    _same(got[1:], want, "guarded")
    occupied, largest, pairs, _ = twin.box_stats(q, r, r2, twin.reach(r2), ZERO, qv, rv)
    assert got[0].tolist() == [0, occupied, largest, pairs]


def test_work_guard_refuses_before_the_search():
    L.require_gpu()
    pts = np.tile(np.array([[0.3, -0.2, 1.5]], F), (4096, 1))
    with pytest.raises(ValueError) as e:
        postprocess.radius_neighbours(_dev(pts), _dev(pts), 0.1, max_pairs=1000)
    msg = str(e.value)
    assert str(4096 * 4096) in msg and "1000" in msg and "4096" in msg, msg    # the pair count, the budget, the largest cell
    r2 = twin.radius_sq(0.1)
    ws = torch.empty(ops.radius_workspace_bytes(4096, 4096), device="cuda", dtype=torch.uint8)
    args = dict(query=_dev(pts), reference=_dev(pts), radius_sq=float(r2), cell=float(twin.reach(r2)), ws=ws)
    stats = ops.radius_search(L.RS_BUILD, **args)[0]
    assert stats.tolist() == [0, 1, 4096, 4096 * 4096]
    count = torch.full((4096,), 77, device="cuda", dtype=torch.int32)
    index = torch.full((4096,), 78, device="cuda", dtype=torch.int32)
    sqdist = torch.full((4096,), 79.0, device="cuda", dtype=torch.float32)
    ops.radius_search(L.RS_SEARCH, max_pairs=1000, out_stats=stats, count=count, index=index, sqdist=sqdist, **args)
    assert stats.tolist() == [L.RS_OVER_BUDGET, 1, 4096, 4096 * 4096]
    assert bool((count == 77).all()) and bool((index == 78).all()) and bool((sqdist == 79.0).all())
    ops.radius_search(L.RS_SEARCH, max_pairs=4096 * 4096, out_stats=stats, count=count, index=index, sqdist=sqdist, **args)   # exactly the budget
    assert stats.tolist() == [0, 1, 4096, 4096 * 4096]
    assert bool((count == 4096).all()) and bool((index == 0).all()) and bool((sqdist == 0).all())


def test_medium_case_rules_everywhere_twin_on_a_sample_and_the_exhaustive_search():
    L.require_gpu()
    nq, nr = 65537, 70001
    q, r, qv, rv = nn_twin.scene(nq, nr, seed=5)
    r2 = twin.radius_sq(0.1)
    stats, (count, index, sqdist) = _run(q, r, r2, None, None, qv, rv)
    nn_index, nn_sqdist = ops.nearest_neighbours(_dev(q), _dev(r), _dev(qv), _dev(rv))
    inside = (nn_index >= 0) & (nn_sqdist <= float(r2))                      # where the exhaustive search finds something within the radius
    assert bool(inside.any()) and bool((~inside).any())
    assert torch.equal(index[inside], nn_index[inside]) and torch.equal(sqdist[inside].view(torch.int32), nn_sqdist[inside].view(torch.int32))
    assert bool((index[~inside] == -1).all()) and bool((count[~inside] == 0).all())
    count, idx, sq = count.cpu().numpy(), index.cpu().numpy(), sqdist.cpu().numpy()
    q_ok, r_ok = nn_twin.usable(q, qv), nn_twin.usable(r, rv)
    assert ((idx >= -1) & (idx < nr)).all() and not np.isnan(sq).any() and (sq >= 0).all() and (count >= 0).all()
    assert ((count >= 1) == (idx >= 0)).all() and (idx[~q_ok] == -1).all() and np.isposinf(sq[idx == -1]).all()
    assert r_ok[idx[idx >= 0]].all() and (sq[idx >= 0] <= r2).all()          # never an unusable reference, never beyond the radius
    hit = np.nonzero(idx >= 0)[0]
    dx, dy, dz = (q[hit, k] - r[idx[hit], k] for k in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F and d.tobytes() == sq[hit].tobytes()                 # sqdist is the rule's d of the reported pair, everywhere
    assert stats[0] == 0 and stats[3] >= int(count.sum()) and 0 < stats[1] <= r_ok.sum() and stats[2] >= 1
    rows = np.random.default_rng(6).choice(nq, 2048, replace=False)
    want = twin.search(q, r, r2, qv, rv, rows=rows)
    assert count[rows].tobytes() == want[0].tobytes() and idx[rows].tobytes() == want[1].tobytes() and sq[rows].tobytes() == want[2].tobytes()
    assert (want[0] > 1).any() and (want[0] == 0).any()


def test_radius_outliers_of_real_views_with_planted_floaters():
    L.require_gpu()
    g = np.load(REAL)
    depth = g["depth"].astype(F)
    pts = ctwin.unproject64(depth, g["extrinsics"][0], g["intrinsics"][0])
    P = np.concatenate([pts[v][::6, ::6].reshape(-1, 3) for v in (0, 1)]).astype(F)     # every 6th pixel of views 0 and 1
    valid = np.concatenate([depth[v][::6, ::6].reshape(-1) > 0 for v in (0, 1)])
    rng = np.random.default_rng(8)
    floaters = (np.array([9.0, 14.0, 6.0]) + 1.5 * np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3)).astype(F)
    assert len(floaters) == 50
    where = np.sort(rng.choice(len(P) + 50, 50, replace=False))              # planted among the real points
    cloud = np.empty((len(P) + 50, 3), F)
    is_floater = np.zeros(len(cloud), bool)
    is_floater[where] = True
    cloud[is_floater], cloud[~is_floater] = floaters, P
    ok = np.ones(len(cloud), bool)
    ok[~is_floater] = valid
    cloud[~ok] = np.nan                                                      # pixels without depth: not finite, like a masked prediction
    radius = 0.3
    want = twin.search(cloud, cloud, twin.radius_sq(radius), exclude_self=True)[0] >= 2
    assert not want[is_floater].any() and want[~is_floater & ok].mean() > 0.9 and not want[~ok].any()
    mask = postprocess.radius_outlier_mask(_dev(cloud), radius=radius)
    assert mask.dtype == torch.bool and mask.shape == (len(cloud),) and mask.cpu().numpy().tobytes() == want.tobytes()
    v8 = rng.random(len(cloud)) < 0.8
    want_v = twin.search(cloud, cloud, twin.radius_sq(radius), v8, v8, exclude_self=True)[0] >= 3
    got_v = postprocess.radius_outlier_mask(_dev(cloud.reshape(2, -1, 3)), radius=radius, min_neighbours=3, valid=_dev(v8.reshape(2, -1)))
    assert got_v.shape == (2, len(cloud) // 2) and got_v.cpu().numpy().reshape(-1).tobytes() == want_v.tobytes()
    colors = rng.integers(0, 256, (len(cloud), 3)).astype(np.uint8)
    conf = rng.random(len(cloud)).astype(F)
    scale = torch.tensor(2.5, device="cuda")
    ext = torch.zeros(2, 3, 4, device="cuda")
    pc = postprocess.PointCloud(_dev(cloud), _dev(colors), torch.tensor(0.5, device="cuda"), scale, np.eye(4), ext, None, _dev(conf))
    out = postprocess.remove_radius_outliers(pc, radius=radius)
    keep = np.nonzero(want)[0]
    assert len(out) == len(keep) and out.points.cpu().numpy().tobytes() == cloud[keep].tobytes()
    assert out.colors.cpu().numpy().tobytes() == colors[keep].tobytes() and out.conf.cpu().numpy().tobytes() == conf[keep].tobytes()
    assert out.indices.dtype == torch.int64 and out.indices.cpu().numpy().tolist() == keep.tolist()
    assert out.scene_scale is scale and out.extrinsic is ext and out.transform is pc.transform and out.conf_threshold is pc.conf_threshold
    pc.indices = _dev(np.arange(len(cloud), dtype=np.int64) * 3 + 1)
    rel = postprocess.remove_radius_outliers(pc, rel_radius=0.12)            # f32(0.12) * f32(2.5), one float32 multiply
    want_rel = np.nonzero(twin.search(cloud, cloud, twin.radius_sq(F(0.12) * F(2.5)), exclude_self=True)[0] >= 2)[0]
    assert rel.indices.cpu().numpy().tolist() == (want_rel * 3 + 1).tolist() and rel.points.cpu().numpy().tobytes() == cloud[want_rel].tobytes()
    assert not is_floater[want_rel].any()


def _want_fscore(pred, gt, thr):
    out = {}
    for name, share, (a, b) in (("accuracy", "precision", (pred, gt)), ("completeness", "recall", (gt, pred))):
        count, _, sq = twin.search(a, b, twin.radius_sq(thr))
        ok = np.isfinite(a).all(1)
        out["n_" + name] = n = int(ok.sum())
        out[share] = int((count[ok] >= 1).sum()) / n if n else float("nan")
        out[name] = np.minimum(np.sqrt(sq[ok].astype(np.float64)), thr).mean() if n else float("nan")
    out["chamfer"] = (out["accuracy"] + out["completeness"]) / 2
    p, r = out["precision"], out["recall"]
    out["fscore"] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out


def test_cloud_fscore_against_numpy():
    L.require_gpu()
    rng = np.random.default_rng(7)
    gt = rng.normal(0.0, 1.0, (3001, 3)).astype(F)
    pred = (gt[rng.permutation(3001)[:2500]] + rng.normal(0.0, 0.02, (2500, 3))).astype(F)
    pred[::97] = np.nan                                                      # unusable points leave every figure
    gt[5] = np.inf
    for a, b, thr in ((pred, gt, 0.03), (pred[:-1], gt[:-1], 0.03), (pred, gt, 0.05), (pred[1:3], gt[:2], 10.0)):
        got, want = postprocess.cloud_fscore(_dev(a), _dev(b), thr), _want_fscore(a, b, thr)
        assert got.n_pred == want["n_accuracy"] == np.isfinite(a).all(1).sum() and got.n_gt == want["n_completeness"] == np.isfinite(b).all(1).sum()
        assert got.precision == want["precision"] and got.recall == want["recall"] and got.fscore == want["fscore"]      # integer ratios: exact
        for k in ("accuracy", "completeness", "chamfer"):
            assert abs(getattr(got, k) - want[k]) <= 1e-9 * abs(want[k]), (k, getattr(got, k), want[k])
        assert got.accuracy_median is None and got.completeness_median is None and got.threshold == thr
        assert 0 < got.precision <= 1 and 0 < got.recall <= 1 and got.accuracy <= thr and got.completeness <= thr
    clean = gt[np.isfinite(gt).all(1)]
    same = postprocess.cloud_fscore(_dev(clean), _dev(clean), 1e-3)
    assert same.accuracy == 0 and same.completeness == 0 and same.chamfer == 0
    assert same.fscore == 1 and same.precision == 1 and same.recall == 1 and same.n_pred == same.n_gt == len(clean)
    empty = postprocess.cloud_fscore(_dev(np.full((4, 3), np.nan, F)), _dev(clean[:10]), 0.1)
    assert empty.n_pred == 0 and empty.n_gt == 10 and np.isnan(empty.accuracy) and abs(empty.completeness - 0.1) < 1e-12 and empty.recall == 0 and empty.fscore == 0
    with pytest.raises(ValueError, match="candidate pairs"):
        postprocess.cloud_fscore(_dev(clean), _dev(clean), 10.0, max_pairs=1000)
