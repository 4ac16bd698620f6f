"""Plane segmentation (ovg_plane_*, postprocess.segment_plane / segment_planes / remove_plane / floor_alignment), host side: the
brute-force twin (tests/plane_twin.py) checked against the pinned hash vectors, the void and orientation rules on crafted triples and
the synthetic room, its two refit solvers against each other; the C ABI without a device (exported symbols, struct layout, enums,
argument checks that return before any HIP call) and the Python API's argument checks."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi_layout
import common
import plane_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
ENTRIES = ("ovg_plane_hypotheses", "ovg_plane_score", "ovg_plane_select", "ovg_plane_mask", "ovg_plane_fit")


def test_pinned_hash_vectors():
    assert twin.mix(0) == 0xE220A8397B1DCDAF
    assert twin.draws(0, 1000, 4).tolist() == [[883, 566, 591], [113, 431, 386], [739, 389, 618], [682, 33, 316]]
    assert twin.draws(7, 3, 3).tolist() == [[1, 1, 2], [0, 0, 1], [2, 1, 1]]
    assert twin.draws(2 ** 64 - 1, 2 ** 31 - 1, 2).tolist() == [[1919727802, 1896895515, 1216681717], [1269570286, 243632753, 926544312]]
    z = np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15], np.uint64)
    assert [int(v) for v in twin.mix(z)] == [twin.mix(int(v)) for v in z]                  # the array form wraps like the integer form


def test_draws_stay_inside_the_candidates():
    for m in (1, 2, 3, 7, 1000, 2 ** 31 - 1):
        for seed in (0, 5, 2 ** 63, 2 ** 64 - 1):
            d = twin.draws(seed, m, 200)
            assert d.min() >= 0 and d.max() < m
            # the hash of the counter seed + 3 h + j: seed + 3 is the same stream one hypothesis later
            assert (twin.draws((seed + 3) % 2 ** 64, m, 199) == d[1:]).all()
    assert len(np.unique(twin.draws(1, 1000, 300))) > 400


def _rows(points, valid=None, axis=None, min_abs_cos=0.0):
    """The hypotheses over a cloud of three points whose draws are a permutation of (0, 1, 2), and one with a repeated draw."""
    planes, index = twin.hypotheses(points, 200, 7, valid, None, axis, min_abs_cos)
    perm = np.array([sorted(r) == [0, 1, 2] for r in index.tolist()])
    assert perm.sum() >= 20 and (~perm).sum() >= 100 and len({tuple(r) for r in index[perm].tolist()}) >= 4
    assert np.isnan(planes[~perm]).all()                                                  # a repeated index is void
    return planes[perm], index[perm]


def test_void_rules_on_crafted_triples():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    planes, index = _rows(tri)
    assert (planes == np.array([0, 0, 1, 0], F)).all() and planes.dtype == F and index.dtype == np.int32
    assert twin.hypotheses(tri, 3, 7)[1].tolist() == [[1, 1, 2], [0, 0, 1], [2, 1, 1]]
    assert np.isnan(_rows(np.array([[0, 0, 0], [0.25, 0.25, 0], [0.5, 0.5, 0]], F))[0]).all()          # three points of a lattice line
    assert np.isnan(_rows(np.array([[1, 2, 3], [2, 4, 6], [-3, -6, -9]], F))[0]).all()                 # exactly collinear
    # the 2^-20 bound: a = 0, b = (1, 0, 0), c = (1, s, 0) has l2 = s^2, |u|^2 = 1, |v|^2 = 1 + s^2, all exact in float64
    for s, void in ((F(2.0 ** -10), True), (F(2.0 ** -10 * (1 + 2.0 ** -19)), False), (F(2.0 ** -11), True), (F(2.0 ** -9), False)):
        exact = Fraction(float(s)) ** 2 > Fraction(1, 2 ** 20) * (1 + Fraction(float(s)) ** 2)
        assert exact == (not void)
        o, x, c = np.zeros(3, F), np.array([1, 0, 0], F), np.array([1, s, 0], F)
        for p in (twin.plane_of(o, x, c), twin.plane_of(o, c, x)):                                     # the angle at a = o is the small one
            assert np.isnan(p).all() if void else p.tolist() == [0, 0, 1, 0], s
        assert twin.plane_of(x, o, c).tolist() == [0, 0, 1, 0]                                         # the angle at a = x is a right angle
    for bad in (np.nan, np.inf, -np.inf):
        pts = tri.copy()
        pts[1, 2] = bad
        assert np.isnan(_rows(pts)[0]).all()
    assert np.isnan(_rows(tri, valid=np.array([1, 0, 1], np.uint8))[0]).all()                           # a masked point
    assert not np.isnan(_rows(tri, valid=np.array([1, 2, 255], np.uint8))[0]).any()
    # an index outside [0, n) in the candidate list
    planes, index = twin.hypotheses(tri, 50, 0, candidates=np.array([0, 1, 2, 3, -1], np.int32))
    out = ((index < 0) | (index >= 3)).any(1)
    assert out.any() and np.isnan(planes[out]).all() and set(index.reshape(-1).tolist()) <= {0, 1, 2, 3, -1}
    # the axis constraint on each side of min_abs_cos: the normal is (0, 0, 1) exactly, so d is the axis' z exactly
    axis = np.array([np.sin(0.3), 0.0, np.cos(0.3)], F)
    at, above = float(axis[2]), float(np.nextafter(axis[2], F(1)))
    assert (_rows(tri, axis=axis, min_abs_cos=at)[0] == np.array([0, 0, 1, 0], F)).all()
    assert np.isnan(_rows(tri, axis=axis, min_abs_cos=above)[0]).all()
    assert (_rows(tri, axis=-axis, min_abs_cos=at)[0] == np.array([0, 0, -1, 0], F)).all()             # |d|: either side of the axis
    assert np.isnan(_rows(tri, axis=np.array([np.nan, 0, 1], F))[0]).all()


def test_both_orientation_rules():
    a, b, c = np.array([0.5, 0.5, 2], F), np.array([1.5, 1.5, 2], F), np.array([0.5, 0.5, 3], F)      # normal along (1, -1, 0)
    r = np.float64(1.0) / np.sqrt(np.float64(2.0))
    for p in (twin.plane_of(a, b, c), twin.plane_of(a, c, b), twin.plane_of(c, b, a)):
        # |n0| == |n1|: the tie goes to the LOWEST component, which becomes positive
        assert p[0] == F(r) and p[1] == -F(r) and p[2] == 0 and p[3] == 0
    o = np.array([1, 1, 1], F)                                                                          # u x v = (3, -9, 1.5)
    for q in (twin.plane_of(o, o + np.array([3, 1, 0], F), o + np.array([0, 0.5, 3], F)), twin.plane_of(o, o + np.array([0, 0.5, 3], F), o + np.array([3, 1, 0], F))):
        assert q[1] > 0 and abs(q[1]) > abs(q[0]) and q[0] < 0                                          # the largest component is positive
    up, down = np.array([0, -1, 0], F), np.array([0, 1, 0], F)
    for pts in ((a, b, c), (a, c, b)):
        assert twin.plane_of(*pts, axis=up)[1] == -F(r) and twin.plane_of(*pts, axis=down)[1] == F(r)   # n . axis > 0
        flat = twin.plane_of(*pts, axis=np.array([0, 0, 1], F))                                         # n . axis == 0: the rule without an axis
        assert flat[0] == F(r) and flat[1] == -F(r)
        assert np.isnan(twin.plane_of(*pts, axis=np.array([0, 0, 1], F), min_abs_cos=2.0 ** -20)).all()
    g = np.array([2.0, -1.0, 0.5], F)
    p = twin.plane_of(g, g + np.array([0, 1, 0], F), g + np.array([0, 0, 1], F))
    assert p.tolist() == [1.0, 0.0, 0.0, -2.0]                                                          # w = -n . a
    assert (twin.residual(np.stack([g, g + F(1)]), p) == np.array([0, 1], F)).all()


def test_inlier_rule_is_inclusive_and_nan_is_never_an_inlier():
    t = F(0.125)
    z = np.array([t, np.nextafter(t, F(1)), -t, np.nextafter(-t, F(-1)), 0, np.nan, np.inf], F)
    pts = np.stack([np.arange(7, dtype=F), np.ones(7, F), z], 1)
    plane = np.array([0, 0, 1, 0], F)
    inl, dist, cnt = twin.mask(pts, plane, t)
    assert inl.tolist() == [1, 0, 1, 0, 1, 0, 0] and cnt.tolist() == [3] and np.isnan(dist[5:]).all() and (dist[:5] == z[:5]).all()
    assert twin.mask(pts, plane, 0.0)[0].tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert twin.mask(pts, plane, t, valid=np.array([0, 1, 1, 1, 1, 1, 1]))[0].tolist() == [0, 0, 1, 0, 1, 0, 0]
    assert twin.mask(pts, plane, t, gate=twin.NONE)[2].tolist() == [0] and np.isnan(twin.mask(pts, plane, t, gate=twin.NONE)[1]).all()
    assert twin.mask(pts, plane, t, gate=twin.FEW)[2].tolist() == [3]
    void = np.full(4, np.nan, F)
    planes = np.stack([plane, void, plane, np.array([0, 0, 1, np.inf], F), np.array([0, 0, 0, 0], F)])
    assert twin.score(pts, planes, t).tolist() == [3, 0, 3, 0, 5] and twin.score(pts, planes, t).dtype == np.int32
    assert twin.select([3, 0, 3, 0, 2], planes)[:1] + twin.select([3, 0, 3, 0, 2], planes)[2:] == (0, 3, 0)            # ties: lowest h
    best, p, c, status = twin.select([3, 0, 3, 0, 2], planes, 4)
    assert (best, c, status) == (-1, 3, twin.NONE) and p.tolist() == [0, 0, 0, 0]
    assert twin.select([0, 9, 0, 0, 0], planes)[0] == -1 and twin.select([0, 0, 0, 0, 0], planes, 3)[3] == twin.NONE


def test_jacobi_fit_agrees_with_eigh_and_refit_recovers_the_room():
    n, t = 3000, 0.01
    for s in (0, 1, 2):
        pts, floor_n, wall_n, part = twin.scene(n, s)
        assert pts.dtype == F and pts.shape == (n, 3) and (part == 0).sum() == n // 2 and (part == 1).sum() == n // 4
        first = twin.segment_plane(pts, t, H=64, seed=0, refit=0)
        counts = np.sort(first["counts"])[::-1]
        # what a CPU run gave: 1501 / 1462 / 1491 inliers, |cos| >= 0.999994, the runner-up at most 1391
        assert first["count"] >= 0.48 * n and first["count"] == counts[0] > counts[1] and first["status"] == 0
        assert abs(first["plane"][:3].astype(np.float64) @ floor_n) >= 0.9999
        N, sums, centre = twin.inlier_moments(pts, first["inlier"])
        assert int(N[0]) == first["count"] and twin.eigen_gap(N, sums, centre) > 100
        a, rms_a, eig_a, st_a = twin.fit(N, sums, centre, first["plane"])
        b, rms_b, eig_b, st_b = twin.fit_eigh(N, sums, centre, first["plane"])
        assert st_a == st_b == 0 and (np.abs(a.view(np.int32) - b.view(np.int32)) <= 1).all()
        assert abs(rms_a - rms_b) <= 1e-9 * rms_b and np.allclose(eig_a, eig_b, rtol=1e-9, atol=0) and 0.002 < rms_a < 0.005
        assert abs(a[:3].astype(np.float64) @ floor_n) >= 0.999999
        both = [twin.segment_plane(pts, t, H=64, seed=0, refit=2, fit_fn=f) for f in (twin.fit, twin.fit_eigh)]
        assert (both[0]["inlier"] == both[1]["inlier"]).all() and both[0]["count"] >= first["count"] and both[0]["status"] == 0
        assert both[0]["count"] == int((twin.mask(pts, both[0]["plane"], t)[0]).sum())
        # with the axis: the same plane, pointing to the axis' side
        for sign in (1.0, -1.0):
            ax = (sign * floor_n).astype(F)
            r = twin.segment_plane(pts, t, H=64, seed=0, refit=2, axis=ax, min_abs_cos=float(F(np.cos(np.deg2rad(10.0)))))
            assert r["plane"][:3].astype(np.float64) @ ax > 0.9999 and (r["inlier"] == both[0]["inlier"]).all()
        wall = twin.segment_plane(pts, t, H=1024, seed=0, refit=2, axis=wall_n.astype(F), min_abs_cos=float(F(np.cos(np.deg2rad(10.0)))))
        assert 0.23 * n <= wall["count"] < 0.3 * n and wall["plane"][:3].astype(np.float64) @ wall_n >= 0.9999


def test_twin_extracts_floor_then_wall_then_stops():
    n, t = 3000, 0.01
    for s in (0, 1, 2):
        pts, floor_n, wall_n, part = twin.scene(n, s)
        for refit in (0, 2):
            planes, labels, res = twin.segment_planes(pts, t, max_planes=4, min_inliers=n // 20, H=64, seed=0, refit=refit)
            assert planes.shape == (2, 4) and planes.dtype == F and labels.dtype == np.int32 and set(labels.tolist()) == {-1, 0, 1}
            assert res[0]["count"] >= 0.48 * n and res[1]["count"] >= 0.23 * n
            assert abs(planes[0][:3].astype(np.float64) @ floor_n) >= 0.9999 and abs(planes[1][:3].astype(np.float64) @ wall_n) >= 0.9999
            assert ((labels == 0).sum(), (labels == 1).sum()) == (res[0]["count"], res[1]["count"])
            assert (part[labels == 0] == 0).mean() > 0.98 and (part[labels == 1] == 1).mean() > 0.98
        assert len(twin.segment_planes(pts, t, max_planes=1, min_inliers=n // 20, H=64)[0]) == 1
        more = twin.segment_planes(pts, t, max_planes=3, min_inliers=3, H=64, refit=0)
        assert len(more[0]) == 3 and more[2][2]["count"] < 40                              # the third plane is clutter
    assert len(twin.segment_planes(pts, t, min_inliers=n, H=64)[0]) == 0


def test_degenerate_refits_keep_the_plane():
    keep = np.array([0, 0, 1, -5], F)
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [0, 1, 0]], F)
    for fit in (twin.fit, twin.fit_eigh):
        N, s, c = twin.inlier_moments(pts, np.array([1, 1, 0, 0, 0], np.uint8))
        assert fit(N, s, c, keep)[3] == twin.FEW and (fit(N, s, c, keep)[0] == keep).all()
        N, s, c = twin.inlier_moments(pts, np.array([1, 1, 1, 1, 0], np.uint8))
        p, rms, eig, st = fit(N, s, c, keep)
        assert st == twin.NO_SPREAD and (p == keep).all() and rms == 0 and (eig == 0).all()
        N, s, c = twin.inlier_moments(pts, np.array([1, 1, 1, 1, 1], np.uint8))
        p, rms, eig, st = fit(N, s, c, keep)
        assert st == 0 and p.tolist() == [0, 0, 1, 0] and rms == 0
        bad = s.copy()
        bad[7] = np.inf
        assert fit(N, bad, c, keep)[3] == twin.NOT_FINITE and (fit(N, bad, c, keep)[0] == keep).all()
        assert fit(np.array([2]), bad, c, keep)[3] == twin.FEW | twin.NOT_FINITE


def _layout(struct, cname, extra):
    return abi_layout.check({cname: struct}, extra)[0]


def test_library_exports_the_entries_and_ctypes_layout_matches_c():
    lib = L.load()
    assert lib.ovg_abi_version() == 13 == L.ABI_VERSION
    for name in ENTRIES:
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    enums = ["OVG_PLANE_HYP_TILE", "OVG_PLANE_POINT_TILE", "OVG_PLANE_NONE", "OVG_PLANE_FEW", "OVG_PLANE_NO_SPREAD", "OVG_PLANE_NOT_FINITE",
             "OVG_KNN_NORMALS_SWEEPS", "OVG_ALIGN_SUMS", "OVG_ABI_VERSION"]
    want = [L.PLANE_HYP_TILE, L.PLANE_POINT_TILE, L.PLANE_NONE, L.PLANE_FEW, L.PLANE_NO_SPREAD, L.PLANE_NOT_FINITE, twin.SWEEPS, L.ALIGN_SUMS, 13]
    for struct, cname in ((L.PlaneHypothesesParams, "ovg_plane_hypotheses_params"), (L.PlaneScoreParams, "ovg_plane_score_params"),
                          (L.PlaneSelectParams, "ovg_plane_select_params"), (L.PlaneMaskParams, "ovg_plane_mask_params"),
                          (L.PlaneFitParams, "ovg_plane_fit_params")):
        assert _layout(struct, cname, enums) == want, cname
    assert (L.PLANE_NONE, L.PLANE_FEW, L.PLANE_NO_SPREAD, L.PLANE_NOT_FINITE) == (twin.NONE, twin.FEW, twin.NO_SPREAD, twin.NOT_FINITE)
    assert (postprocess.PLANE_NONE, postprocess.PLANE_FEW, postprocess.PLANE_NO_SPREAD, postprocess.PLANE_NOT_FINITE) == (1, 2, 4, 8)
    assert L.PLANE_COLLINEAR_EPS == twin.COLLINEAR_EPS == 2.0 ** -20 and L.PLANE_SPREAD_EPS == twin.SPREAD_EPS == 2.0 ** -40
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (name, name), text), name
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert re.search(r"#define\s+OVG_PLANE_COLLINEAR_EPS\s+9\.5367431640625e-07\b", text) and 2.0 ** -20 == 9.5367431640625e-07
    assert re.search(r"#define\s+OVG_PLANE_SPREAD_EPS\s+9\.094947017729282e-13\b", text) and 2.0 ** -40 == 9.094947017729282e-13


def test_argument_validation_of_the_entries_without_gpu():
    lib = L.load()
    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks
    nan, inf = float("nan"), float("inf")

    def run(name, struct, base, **kw):
        p = struct(**base)
        for k, v in kw.items():
            setattr(p, k, v)
        return getattr(lib, name)(ctypes.byref(p), None)

    for name in ENTRIES:
        assert getattr(lib, name)(None, None) == -1
    base = dict(points=big, valid=big + 1, candidates=big, axis=big, n=1000, m=10, H=64, seed=1, min_abs_cos=0.5, planes=big, index=big)
    for bad in (dict(points=None), dict(planes=None), dict(index=None), dict(n=0), dict(n=1 << 31), dict(n=-1), dict(H=0), dict(H=1 << 31), dict(H=-5),
                dict(m=0), dict(m=1 << 31), dict(m=-1), dict(candidates=None), dict(candidates=None, m=999), dict(min_abs_cos=-0.5),
                dict(min_abs_cos=1.5), dict(min_abs_cos=nan), dict(axis=None), dict(points=big + 2), dict(candidates=big + 2), dict(axis=big + 1),
                dict(planes=big + 2), dict(index=big + 3)):
        assert run("ovg_plane_hypotheses", L.PlaneHypothesesParams, base, **bad) == -1, bad
    base = dict(points=big, valid=big + 1, planes=big, n=1000, H=64, threshold=0.5, splits=0, count=big)
    for bad in (dict(points=None), dict(planes=None), dict(count=None), dict(n=0), dict(n=1 << 31), dict(H=0), dict(H=1 << 31), dict(threshold=-1.0),
                dict(threshold=nan), dict(threshold=inf), dict(threshold=-0.0 - 1e-30), dict(splits=-1), dict(points=big + 1), dict(planes=big + 2),
                dict(count=big + 2)):
        assert run("ovg_plane_score", L.PlaneScoreParams, base, **bad) == -1, bad
    base = dict(count=big, planes=big, H=64, min_inliers=3, best=big, plane=big, best_count=big, status=big)
    for bad in (dict(count=None), dict(planes=None), dict(best=None), dict(plane=None), dict(best_count=None), dict(status=None), dict(H=0),
                dict(H=1 << 31), dict(min_inliers=2), dict(min_inliers=0), dict(min_inliers=-7), dict(count=big + 2), dict(planes=big + 1),
                dict(best=big + 2), dict(plane=big + 2), dict(best_count=big + 1), dict(status=big + 3)):
        assert run("ovg_plane_select", L.PlaneSelectParams, base, **bad) == -1, bad
    base = dict(points=big, valid=big + 1, plane=big, gate=big, n=1000, threshold=0.0, inlier=big + 1, distance=big, out_count=big)
    for bad in (dict(points=None), dict(plane=None), dict(inlier=None), dict(out_count=None), dict(n=0), dict(n=1 << 31), dict(threshold=-1.0),
                dict(threshold=nan), dict(threshold=inf), dict(points=big + 2), dict(plane=big + 2), dict(gate=big + 1), dict(distance=big + 2),
                dict(out_count=big + 4)):
        assert run("ovg_plane_mask", L.PlaneMaskParams, base, **bad) == -1, bad
    base = dict(count=big, sums=big, centre=big, axis=big, plane=big, out_rms=big, out_eigen=big, status=big)
    for bad in (dict(count=None), dict(sums=None), dict(plane=None), dict(count=big + 4), dict(sums=big + 4), dict(centre=big + 4), dict(axis=big + 2),
                dict(plane=big + 2), dict(out_rms=big + 4), dict(out_eigen=big + 4), dict(status=big + 2)):
        assert run("ovg_plane_fit", L.PlaneFitParams, base, **bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    q = torch.zeros(5, 3)
    scale = torch.tensor(2.0)
    cloud = postprocess.PointCloud(q, torch.zeros(5, 3, dtype=torch.uint8), None, scale, None, None)
    bad_kw = (dict(), dict(threshold=0.1, rel_threshold=0.1), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
              dict(threshold=True), dict(threshold="x"), dict(threshold=1e39), dict(rel_threshold=0.0), dict(rel_threshold=float("nan")),
              dict(threshold=0.1, hypotheses=0), dict(threshold=0.1, hypotheses=1.5), dict(threshold=0.1, hypotheses=True),
              dict(threshold=0.1, hypotheses=(1 << 24) + 1), dict(threshold=0.1, seed=-1), dict(threshold=0.1, seed=1 << 64),
              dict(threshold=0.1, seed=0.5), dict(threshold=0.1, refit=-1), dict(threshold=0.1, refit=1.0), dict(threshold=0.1, refit=None),
              dict(threshold=0.1, min_inliers=2), dict(threshold=0.1, min_inliers=3.0), dict(threshold=0.1, min_inliers=1 << 31),
              dict(threshold=0.1, valid=torch.ones(4, dtype=torch.bool)), dict(threshold=0.1, valid=torch.ones(5)),
              dict(threshold=0.1, axis=(0, 0)), dict(threshold=0.1, axis=(0, 0, 0)), dict(threshold=0.1, axis=(0, float("nan"), 1)),
              dict(threshold=0.1, axis="up"), dict(threshold=0.1, axis=torch.zeros(2)), dict(threshold=0.1, axis=torch.zeros(3, dtype=torch.int32)),
              dict(threshold=0.1, max_angle_deg=10), dict(threshold=0.1, axis=(0, 1, 0), max_angle_deg=0), dict(threshold=0.1, axis=(0, 1, 0), max_angle_deg=91),
              dict(threshold=0.1, axis=(0, 1, 0), max_angle_deg=True), dict(threshold=0.1, candidates=[0, 1, 2]),
              dict(threshold=0.1, candidates=torch.zeros(3)), dict(threshold=0.1, candidates=torch.zeros(2, 2, dtype=torch.int32)))
    for kw in bad_kw:
        with pytest.raises(ValueError):
            postprocess.segment_plane(cloud, **kw)
        with pytest.raises(ValueError):
            postprocess.segment_planes(cloud, **kw)
    with pytest.raises(ValueError):
        postprocess.segment_plane(cloud, threshold=0.1, return_distance=1)
    for kw in (dict(max_planes=0), dict(max_planes=1.0), dict(max_planes=True), dict(min_inliers=2)):
        with pytest.raises(ValueError):
            postprocess.segment_planes(cloud, threshold=0.1, **kw)
    for bad in (torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.float64), [[0.0, 0.0, 0.0]], None):
        with pytest.raises(ValueError):
            postprocess.segment_plane(bad, threshold=0.1)
        with pytest.raises(ValueError):
            postprocess.segment_planes(bad, threshold=0.1)
    with pytest.raises(ValueError):
        postprocess.segment_plane(q, rel_threshold=0.1)                       # rel_threshold needs a PointCloud
    good = (dict(threshold=0.1), dict(threshold=0), dict(rel_threshold=0.01), dict(threshold=0.1, axis=(0, 2, 0), max_angle_deg=10.0),
            dict(threshold=0.1, axis=torch.tensor([0.0, 1.0, 0.0])), dict(threshold=0.1, candidates=torch.arange(5)),
            dict(threshold=0.1, hypotheses=7, seed=(1 << 64) - 1, refit=0, min_inliers=3, valid=torch.ones(5, dtype=torch.bool)))
    for kw in good:
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.segment_plane(cloud, **kw)
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.segment_planes(cloud, **kw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.segment_plane(torch.zeros(0, 3), threshold=0.1)
    # the thin wrappers
    p4, cnt = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32)
    for call in (lambda: ops.plane_hypotheses(q, 8), lambda: ops.plane_score(q, p4, 0.1), lambda: ops.plane_select(cnt, p4),
                 lambda: ops.plane_mask(q, p4[0], 0.1), lambda: ops.plane_fit(torch.zeros(1, dtype=torch.int64), torch.zeros(18, dtype=torch.float64), p4[0].clone()),
                 lambda: ops.plane_hypotheses(q.double(), 8), lambda: ops.plane_hypotheses(q, 0), lambda: ops.plane_hypotheses(q, 8, seed=-1),
                 lambda: ops.plane_hypotheses(q, 8, min_abs_cos=0.5), lambda: ops.plane_hypotheses(q, 8, candidates=torch.zeros(0, dtype=torch.int32)),
                 lambda: ops.plane_score(q, p4[:, :3], 0.1), lambda: ops.plane_score(q, p4, -0.1), lambda: ops.plane_score(q, p4, float("nan")),
                 lambda: ops.plane_score(q, p4, 0.1, splits=-1), lambda: ops.plane_score(q[:0], p4, 0.1), lambda: ops.plane_select(cnt, p4, min_inliers=2),
                 lambda: ops.plane_select(cnt.long(), p4), lambda: ops.plane_mask(q, p4[0, :3], 0.1), lambda: ops.plane_mask(q, p4[0], float("inf")),
                 lambda: ops.plane_fit(torch.zeros(1, dtype=torch.int64), torch.zeros(17, dtype=torch.float64), p4[0].clone())):
        with pytest.raises(L.OvgError):
            call()


def test_remove_plane_and_floor_alignment_without_gpu():
    pts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 5]])
    cloud = postprocess.PointCloud(pts, torch.arange(12, dtype=torch.uint8).reshape(4, 3), None, torch.tensor(1.0), None, None,
                                   torch.tensor([10, 11, 12, 13]), torch.tensor([0.1, 0.2, 0.3, 0.4]))
    z = torch.zeros(())
    res = postprocess.PlaneResult(torch.tensor([0.0, 0, 1, 0]), torch.tensor([True, True, True, False]), z, z, z, z)
    out = postprocess.remove_plane(cloud, res)
    assert out.points.tolist() == [[0, 0, 5]] and out.indices.tolist() == [13] and out.colors.tolist() == [[9, 10, 11]]
    assert abs(out.conf.item() - 0.4) < 1e-7 and out.scene_scale is cloud.scene_scale
    inl = postprocess.remove_plane(cloud, res, keep="inliers")
    assert inl.indices.tolist() == [10, 11, 12] and len(inl) == 3
    for bad in (dict(cloud=pts, result=res), dict(cloud=cloud, result=None), dict(cloud=cloud, result=res, keep="all"),
                dict(cloud=cloud, result=postprocess.PlaneResult(res.plane, res.inlier[:3], z, z, z, z))):
        with pytest.raises(ValueError):
            postprocess.remove_plane(**bad)
    # floor_alignment is a few float64 torch operations on the plane's device: checked here on the host
    rng = np.random.default_rng(0)
    for up in ((0.0, 1.0, 0.0), (0.0, 0.0, 2.0), (1.0, -2.0, 0.5)):
        u = np.array(up) / np.linalg.norm(up)
        normals = [rng.normal(size=3) for _ in range(6)] + [u, -u, np.array([1.0, 0, 0]), np.array([-1.0, 0, 0]), np.array([0, -1.0, 0])]
        for nrm in normals:
            nrm = nrm / np.linalg.norm(nrm)
            plane = torch.tensor(np.append(nrm, 0.7).astype(F))
            sim = postprocess.floor_alignment(plane, up=up)
            M = sim.matrix.numpy()
            assert sim.matrix.dtype == torch.float64 and M.shape == (4, 4) and float(sim.scale) == 1.0 and int(sim.status) == 0
            R = M[:3, :3]
            n32 = plane[:3].double().numpy()
            n32 = n32 / np.linalg.norm(n32)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and (M[3] == [0, 0, 0, 1]).all()
            assert np.abs(R @ n32 - u).max() < 1e-12
            p = rng.normal(size=(5, 3))
            height = (p @ R.T + M[:3, 3]) @ u
            w = float(plane[3]) / np.linalg.norm(plane[:3].double().numpy())
            assert np.abs(height - (p @ n32 + w)).max() < 1e-12                             # the up coordinate is the signed distance
    same = postprocess.floor_alignment(res, up=(0, 0, 1)).matrix
    assert torch.equal(same, torch.eye(4, dtype=torch.float64))
    for bad in (dict(plane=torch.zeros(3)), dict(plane=[0, 0, 1, 0]), dict(plane=res.plane, up=(0, 0, 0)), dict(plane=res.plane, up=(0, 1)),
                dict(plane=res.plane, up="y"), dict(plane=res.plane.int())):
        with pytest.raises(ValueError):
            postprocess.floor_alignment(**bad)
