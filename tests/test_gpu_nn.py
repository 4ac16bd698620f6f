"""ovg_nearest_neighbours / postprocess.nearest_neighbours, reciprocal_matches and cloud_distance on the device against
tests/nn_twin.py: index and sqdist byte for byte -- shapes around the tile constants, every split count, crafted inputs (ties,
duplicates, non-finite coordinates, masks, distances that overflow), the search inside one cloud, guard bytes behind the workspace and
both outputs, a medium case, mutual matches of two real views and cloud-to-cloud figures against numpy float64."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import nn_twin as twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
QT, RT = L.NN_QUERY_TILE, L.NN_REFERENCE_TILE
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, name):
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.dtype == np.int32 and gs.dtype == F and gi.shape == want[0].shape and gs.shape == want[1].shape, (name, gi.dtype, gs.dtype, gi.shape)
    assert gi.tobytes() == want[0].tobytes(), (name, "index", int((gi != want[0]).sum()))
    assert gs.tobytes() == want[1].tobytes(), (name, "sqdist", int((gs.view(np.uint32) != want[1].view(np.uint32)).sum()))


def _check(q, r, qv=None, rv=None, exclude_self=False, name="", splits=(0,)):
    want = twin.nearest(q, r, qv, rv, exclude_self=exclude_self)
    dq, dr, dqv, drv = _dev(q), _dev(r), _dev(qv), _dev(rv)
    for s in splits:
        _same(ops.nearest_neighbours(dq, dr, dqv, drv, exclude_self=exclude_self, splits=s), want, "%s splits=%d" % (name, s))
    return want


def test_shapes_around_the_tiles_match_twin_bit_exactly():
    L.require_gpu()
    assert QT >= 128 and RT >= 128
    nqs = (1, 63, 65, QT - 1, QT, QT + 1, 2 * QT + 1)
    nrs = (1, 63, 65, RT - 1, RT, RT + 1, 2 * RT + 1)
    q, r, qv, rv = twin.scene(max(nqs), max(nrs), seed=0)
    for nq in nqs:
        for nr in nrs:
            want = _check(q[:nq], r[:nr], qv[:nq], rv[:nr], name="%d x %d" % (nq, nr))
            if nq >= QT - 1 and nr >= 63:
                assert (want[0] == -1).any() and (want[0] >= 0).any()
    _check(q, r, name="without masks")


def test_every_split_count_gives_identical_bytes():
    L.require_gpu()
    nq, nr = 2 * QT + 1, 9 * RT + 5                                          # 10 reference tiles: 2 -> 5 + 5, 7 -> 2 x 5, auto, 1000 -> 10
    q, r, qv, rv = twin.scene(nq, nr, seed=1)
    want = _check(q, r, qv, rv, name="splits", splits=(1, 2, 7, 0, 3, 10, 1000))
    assert np.isposinf(want[1][want[0] >= 0]).any() and (want[1] == 0).any()
    # the search inside a cloud with duplicates, every split count
    c, _, cv, _ = twin.scene(3 * QT + 17, 0, seed=2, same=True)
    assert len(np.unique(c[np.isfinite(c).all(1)], axis=0)) < np.isfinite(c).all(1).sum()
    want = _check(c, c, cv, cv, exclude_self=True, name="exclude-self", splits=(1, 2, 7, 0))
    ok = want[0] >= 0
    assert (want[0][ok] != np.nonzero(ok)[0]).all() and (want[1][ok] == 0).any()
    plain = _check(c, c, cv, cv, name="same cloud", splits=(1, 0))
    assert (plain[1][plain[0] >= 0] == 0).all()                              # every usable point finds itself or an earlier duplicate


def test_crafted_inputs_match_twin():
    L.require_gpu()
    rng = np.random.default_rng(1)
    ql, rl = (rng.integers(-8, 9, (5000, 3)) / 4.0).astype(F), (rng.integers(-8, 9, (700, 3)) / 4.0).astype(F)
    _check(ql, rl, name="lattice ties", splits=(0, 1, 2))
    r = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e20, 0, 0]], F)
    q = np.array([[0.9, 0, 0], [0, 0, 0], [np.nan, 1, 1], [0, -np.inf, 0], [-3e38, 0, 0], [0, 1.0, 0], [1e20, 1e20, 0], [1e20, 1e10, 0]], F)
    want = _check(q, r, name="crafted")
    assert want[0].tolist() == [1, 0, -1, -1, 0, 0, 0, 7]
    _check(q, r, np.array([1, 1, 1, 1, 1, 0, 1, 1], np.uint8), np.array([0, 0, 1, 1, 1, 1, 1, 1], np.uint8), name="crafted masks")
    want = _check(q, r[4:7], name="all references unusable")
    assert (want[0] == -1).all()
    _check(q, r, None, np.zeros(8, np.uint8), name="all references masked")
    _check(r, r, exclude_self=True, name="crafted exclude-self")
    _check(r[:1], r[:1], exclude_self=True, name="one point, exclude-self")
    # the public entry: leading shapes, bool masks, PointClouds, empty sides
    res = postprocess.nearest_neighbours(_dev(ql.reshape(50, 100, 3)), _dev(rl.reshape(7, 100, 3)), reference_valid=_dev(np.ones((7, 100), bool)))
    assert res.index.shape == (50, 100) and res.sqdist.shape == (50, 100)
    _same((res.index.reshape(-1), res.sqdist.reshape(-1)), twin.nearest(ql, rl), "leading shapes")
    cloud = postprocess.PointCloud(_dev(r), None, None, None, None, None)
    res = postprocess.nearest_neighbours(cloud, cloud, exclude_self=True)
    _same((res.index, res.sqdist), twin.nearest(r, r, exclude_self=True), "PointCloud")
    res = postprocess.nearest_neighbours(_dev(q), _dev(r[:0]))
    assert (res.index == -1).all() and torch.isposinf(res.sqdist).all() and res.index.dtype == torch.int32 and res.index.shape == (8,)
    assert postprocess.nearest_neighbours(_dev(q[:0]), _dev(r)).index.shape == (0,)


def test_nothing_is_written_behind_the_workspace_or_the_outputs():
    L.require_gpu()
    nq, nr = QT + 3, 5 * RT + 1
    q, r, qv, rv = twin.scene(nq, nr, seed=4)
    want = twin.nearest(q, r, qv, rv)
    need = ops.nn_workspace_bytes(nq, nr)
    assert need == (8 * nq + 15) // 16 * 16
    for splits in (1, 3, 0):
        ws = torch.full((need + 4096,), 0xA5, device="cuda", dtype=torch.uint8)
        index, check_i = guarded((1, nq), torch.int32, "cuda")
        sqdist, check_s = guarded((1, nq), torch.float32, "cuda")
        got = ops.nearest_neighbours(_dev(q), _dev(r), _dev(qv), _dev(rv), splits=splits, ws=ws[:need], index=index[0], sqdist=sqdist[0])
        torch.cuda.synchronize()
        check_i("index splits=%d" % splits)
        check_s("sqdist splits=%d" % splits)
        assert bool((ws[need:] == 0xA5).all()), splits
        _same(got, want, "guarded splits=%d" % splits)


def test_medium_case_rules_everywhere_and_twin_on_a_sample():
    L.require_gpu()
    nq, nr = 65537, 70001
    q, r, qv, rv = twin.scene(nq, nr, seed=5)
    idx, sq = ops.nearest_neighbours(_dev(q), _dev(r), _dev(qv), _dev(rv))
    again = ops.nearest_neighbours(_dev(q), _dev(r), _dev(qv), _dev(rv), splits=1)
    assert torch.equal(idx, again[0]) and torch.equal(sq.view(torch.int32), again[1].view(torch.int32))
    idx, sq = idx.cpu().numpy(), sq.cpu().numpy()
    q_ok, r_ok = twin.usable(q, qv), twin.usable(r, rv)
    assert ((idx >= -1) & (idx < nr)).all() and not np.isnan(sq).any() and (sq >= 0).all()
    assert (idx[~q_ok] == -1).all() and (idx[q_ok] >= 0).all() and np.isposinf(sq[idx == -1]).all()
    assert r_ok[idx[idx >= 0]].all()                                         # never an unusable reference
    hit = np.nonzero(idx >= 0)[0]
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[hit, k] - r[idx[hit], k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F and d.tobytes() == sq[hit].tobytes()                 # sqdist is the rule's d of the reported pair, everywhere
    rows = np.random.default_rng(6).choice(nq, 2048, replace=False)
    want = twin.nearest(q, r, qv, rv, rows=rows)
    assert idx[rows].tobytes() == want[0].tobytes() and sq[rows].tobytes() == want[1].tobytes()


def test_reciprocal_matches_of_two_real_views():
    L.require_gpu()
    g = np.load(REAL)
    depth = g["depth"].astype(F)
    pts = ctwin.unproject64(depth, g["extrinsics"][0], g["intrinsics"][0])
    P1, P2 = pts[0][::4, ::4].reshape(-1, 3), pts[1][::4, ::4].reshape(-1, 3)     # every 4th pixel of views 0 and 1
    v1, v2 = (depth[0][::4, ::4].reshape(-1) > 0), (depth[1][::4, ::4].reshape(-1) > 0)
    assert len(P1) == len(P2) == 74 * 130 and v1.any() and not v1.all()
    want = twin.reciprocal(P1, P2, v1, v2)
    rec, nn2, count = postprocess.reciprocal_matches(_dev(P1), _dev(P2), _dev(v1), _dev(v2))
    assert rec.dtype == torch.bool and nn2.dtype == torch.int32 and rec.shape == nn2.shape == (len(P2),)
    assert rec.cpu().numpy().tobytes() == want[0].tobytes() and nn2.cpu().numpy().tobytes() == want[1].tobytes()
    assert int(count) == want[2] and 0 < want[2] < len(P2)
    # the symmetric count of the reference's own assertion
    rec1, _, count1 = postprocess.reciprocal_matches(_dev(P2), _dev(P1))
    assert int(count1) == int(postprocess.reciprocal_matches(_dev(P1), _dev(P2))[2]) and rec1.shape == (len(P1),)
    # no usable point on one side: -1 everywhere, nothing reciprocal
    rec, nn2, count = postprocess.reciprocal_matches(_dev(np.full((5, 3), np.nan, F)), _dev(P2[:100]))
    assert (nn2 == -1).all() and not rec.any() and int(count) == 0


def _want_distance(pred, gt, threshold):
    out = {}
    sides = {}
    for name, (a, b) in (("accuracy", (pred, gt)), ("completeness", (gt, pred))):
        idx, sq = twin.nearest(a, b)
        d = np.sqrt(sq[idx >= 0].astype(np.float64))
        sides[name] = d
        out[name], out[name + "_median"] = d.mean(), np.median(d)
    out["chamfer"] = (out["accuracy"] + out["completeness"]) / 2
    out["n_pred"], out["n_gt"] = len(sides["accuracy"]), len(sides["completeness"])
    if threshold is not None:
        p, r = (sides["accuracy"] < threshold).mean(), (sides["completeness"] < threshold).mean()
        out.update(precision=p, recall=r, fscore=2 * p * r / (p + r))
    return out


def test_cloud_distance_against_numpy_float64():
    L.require_gpu()
    rng = np.random.default_rng(7)
    gt = rng.normal(0.0, 1.0, (3001, 3)).astype(F)
    pred = (gt[rng.permutation(3001)[:2500]] + rng.normal(0.0, 0.02, (2500, 3))).astype(F)
    pred[::97] = np.nan                                                      # unmatched points leave every figure
    gt[5] = np.inf
    for a, b, thr in ((pred, gt, 0.03), (pred[:-1], gt[:-1], 0.03), (pred, gt, None), (pred[1:3], gt[:2], 10.0)):
        got, want = postprocess.cloud_distance(_dev(a), _dev(b), threshold=thr), _want_distance(a, b, thr)
        assert got.n_pred == want["n_pred"] and got.n_gt == want["n_gt"]
        assert got.n_pred == np.isfinite(a).all(1).sum() and got.n_gt == np.isfinite(b).all(1).sum()
        for k in ("accuracy", "accuracy_median", "completeness", "completeness_median", "chamfer") + (("precision", "recall", "fscore") if thr else ()):
            assert abs(getattr(got, k) - want[k]) <= 1e-9 * abs(want[k]), (k, getattr(got, k), want[k])
        if thr is None:
            assert got.precision is None and got.recall is None and got.fscore is None
        else:
            assert 0 < got.precision <= 1 and 0 < got.recall <= 1
    clean = gt[np.isfinite(gt).all(1)]
    same = postprocess.cloud_distance(_dev(clean), _dev(clean), threshold=1e-3)
    assert same.accuracy == 0 and same.completeness == 0 and same.chamfer == 0 and same.accuracy_median == 0
    assert same.fscore == 1 and same.precision == 1 and same.recall == 1 and same.n_pred == same.n_gt == len(clean)
    empty = postprocess.cloud_distance(_dev(np.full((4, 3), np.nan, F)), _dev(clean[:10]), threshold=0.1)
    assert empty.n_pred == 0 and empty.n_gt == 0 and np.isnan(empty.accuracy) and np.isnan(empty.chamfer) and empty.fscore == 0
