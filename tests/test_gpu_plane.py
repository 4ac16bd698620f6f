"""ovg_plane_hypotheses / _score / _select / _mask / _fit and postprocess.segment_plane, segment_planes, remove_plane, floor_alignment on
the device against the brute force of tests/plane_twin.py: draws, planes, counts, winner and masks byte for byte, the refit within one
float32 ulp of numpy's eigh; every case into exact-size guarded outputs and run twice with identical bytes -- shapes around the point
and hypothesis tiles of the score kernel and every split count, crafted inputs (the inclusive bound at +-t and one float32 step
beyond, t = 0, no usable point, a plane twice, ties, no plane, degenerate refits), the synthetic room, the Python layer and a cloud
un-projected from real views."""
import math
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as ctwin
import nn_twin
import plane_twin as twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
HT, PT = L.PLANE_HYP_TILE, L.PLANE_POINT_TILE
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
T = 0.01
_CACHE = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _twice(run, names):
    """run() -> tuple of device tensors, called twice: the two runs must give identical bytes. -> the first run as numpy arrays"""
    first, second = run(), run()
    for a, b, what in zip(first, second, names):
        assert _host(a).tobytes() == _host(b).tobytes(), ("two runs differ", what)
    return tuple(_host(a) for a in first)


def _same_planes(got, want, name):
    """Byte for byte, the NaN pattern of void planes counted as a void check, not as payload."""
    assert got.dtype == want.dtype == F and got.shape == want.shape, (name, got.shape, want.shape)
    void = np.isnan(want).all(-1)
    assert (np.isnan(got).all(-1) == void).all() and not np.isnan(got[~void]).any(), (name, "void rows differ")
    diff = got[~void].view(np.uint32) != want[~void].view(np.uint32)
    assert not diff.any(), (name, "%d components of %d planes differ" % (diff.sum(), diff.any(-1).sum()))
    return int(void.sum())


def _hypotheses(pts, H, seed, valid, cand, axis, mac):
    def run():
        planes, check_p = guarded((H, 4), torch.float32, "cuda", guard_bytes=4096)
        index, check_i = guarded((H, 3), torch.int32, "cuda", guard_bytes=4096)
        out = ops.plane_hypotheses(pts, H, seed, valid=valid, candidates=cand, axis=axis, min_abs_cos=mac, planes=planes, index=index)
        torch.cuda.synchronize()
        check_p("planes"), check_i("index")
        assert out[0] is planes and out[1] is index
        return planes, index
    return _twice(run, ("planes", "index"))


@pytest.mark.parametrize("n", [3, 257, 3000])
def test_hypotheses_match_twin_bit_exactly(n):
    """nn_twin.scene clouds: blobs, lattice ties, duplicates, NaN / inf / 1e20 coordinates and a mask with holes; H around the block
    of 256 threads; with and without a candidate list (which holds out-of-range entries and repeats) and an axis. n = 3 voids most
    hypotheses by repeated draws."""
    L.require_gpu()
    c, _, cv, _ = nn_twin.scene(n, 0, seed=3, same=True)
    if n == 3:
        c, cv = np.array([[0.5, 0.25, 0], [1, 0, 0.75], [0, 1, 0.5]], F), np.ones(3, np.uint8)
    rng = np.random.default_rng(n)
    cand = np.concatenate([rng.integers(0, n, max(5, n // 3)), [-1, n, n + 5, 0, 0]]).astype(np.int32)
    rng.shuffle(cand)
    axis = np.array([0.36, 0.48, 0.8], F)
    pts, valid, dcand, daxis = _dev(c), _dev(cv), _dev(cand), _dev(axis)
    voids, total = 0, 0
    for H in (1, 255, 256, 257, 1000):
        for use_cand in (False, True):
            for use_axis in (False, True):
                seed = 1000 * H + 2 * use_cand + use_axis
                mac = 0.5 if use_axis else 0.0
                want_p, want_i = twin.hypotheses(c, H, seed, cv, cand if use_cand else None, axis if use_axis else None, mac)
                got_p, got_i = _hypotheses(pts, H, seed, valid, dcand if use_cand else None, daxis if use_axis else None, mac)
                name = "n %d H %d candidates %s axis %s" % (n, H, use_cand, use_axis)
                assert got_i.dtype == np.int32 and got_i.tobytes() == want_i.tobytes(), name
                voids += _same_planes(got_p, want_p, name)
                total += H
                if use_axis:
                    live = ~np.isnan(want_p).all(-1)
                    assert (want_p[live, :3].astype(np.float64) @ axis.astype(np.float64) >= 0.5 - 1e-6).all()
    print("n %d: %d of %d hypotheses void" % (n, voids, total))
    assert voids > total // 2 if n == 3 else 0 < voids < total
    # the extremes of the seed, and an unmasked cloud
    for seed in (0, (1 << 64) - 1):
        want_p, want_i = twin.hypotheses(c, 64, seed)
        got_p, got_i = _hypotheses(pts, 64, seed, None, None, None, 0.0)
        assert got_i.tobytes() == want_i.tobytes()
        _same_planes(got_p, want_p, "seed %d" % seed)


def _dirty(n, seed):
    """The synthetic room with everything the inlier rule speaks of: NaN / inf / 1e20 coordinates and a mask with holes."""
    pts = twin.scene(n, seed)[0].copy()
    rng = np.random.default_rng(100 + seed)
    for share, value in ((0.01, np.nan), (0.005, np.inf), (0.005, -np.inf), (0.01, 3e20)):
        bad = np.nonzero(rng.random(n) < share)[0]
        pts[bad, rng.integers(0, 3, len(bad))] = value
    return pts, (rng.random(n) >= 0.03).astype(np.uint8)


def _score_planes():
    """1000 planes for the score tests: the twin's hypotheses over the 3000-point room (void rows among them), one plane twice, a plane
    with an infinite offset and the plane of zeros."""
    if "planes" not in _CACHE:
        pts, valid = _dirty(3000, 0)
        planes = twin.hypotheses(pts, 1000, 11, valid)[0]
        live = np.nonzero(~np.isnan(planes).all(-1))[0]
        assert 50 < 1000 - len(live) < 500
        planes[HT - 1] = planes[live[3]]                                      # the same plane in two hypothesis tiles
        planes[HT] = planes[live[3]]
        planes[7] = np.array([0, 0, 1, np.inf], F)
        planes[8] = 0
        _CACHE["planes"] = planes
    return _CACHE["planes"]


def _score(pts, planes, t, valid, splits):
    H = planes.shape[0]

    def run():
        count, check = guarded((1, H), torch.int32, "cuda", guard_bytes=4096)
        out = ops.plane_score(pts, planes, t, valid=valid, splits=splits, count=count[0])
        torch.cuda.synchronize()
        check("count")
        assert out.data_ptr() == count.data_ptr()
        return (count[0],)
    return _twice(run, ("count",))[0]


@pytest.mark.parametrize("n", [1, PT - 1, PT, PT + 1, 3000, 70000])
def test_score_matches_twin_for_every_shape_and_split(n):
    """n around the point tile, H around the hypothesis tile, splits 0 (auto), 1, 2 and 7: count is byte-identical to the twin and the
    same for every split. 70 000 points are 137 point tiles: the auto split and 7 both leave ragged last splits."""
    L.require_gpu()
    assert (HT, PT) == (512, 512)
    planes = _score_planes()
    c, cv = _dirty(n, 1)
    want = twin.score(c, planes, T, cv)
    assert want.dtype == np.int32 and (want[np.isnan(planes).any(-1)] == 0).all() and want[7] == 0
    assert want[HT - 1] == want[HT] and (n < 3000 or want[HT] > 10) and (n < 3000 or want.max() > n // 5)
    pts, valid, dplanes = _dev(c), _dev(cv), _dev(planes)
    for H in (1, HT - 1, HT, HT + 1, 1000):
        sub = dplanes[:H].contiguous()
        for splits in (0, 1, 2, 7):
            got = _score(pts, sub, T, valid, splits)
            assert got.dtype == np.int32 and got.tobytes() == want[:H].tobytes(), ("n %d H %d splits %d" % (n, H, splits), int((got != want[:H]).sum()))
    free = twin.score(c, planes[:HT + 1], T)
    assert _score(pts, dplanes[:HT + 1].contiguous(), T, None, 0).tobytes() == free.tobytes() and (n < 3000 or (free != want[:HT + 1]).any())


def test_score_crafted_bounds_unusable_points_and_twin_planes():
    L.require_gpu()
    t = F(0.125)
    z = np.array([t, np.nextafter(t, F(1)), -t, np.nextafter(-t, F(-1)), 0, np.nextafter(F(0), F(1)), -np.nextafter(F(0), F(1))], F)
    c = np.stack([np.linspace(-3, 3, 7).astype(F), np.full(7, 1e6, F), z], 1)
    planes = np.array([[0, 0, 1, 0], [0, 0, -1, 0], [0, 0, 1, 0], [np.nan] * 4, [0, 0, 1, 0.125], [0, 0, 0, 0.125], [0, 0, 0, 0.2]], F)
    pts, dplanes = _dev(c), _dev(planes)
    for thr, want in ((float(t), [5, 5, 5, 0, 5, 7, 0]), (0.0, [1, 1, 1, 0, 1, 0, 0])):
        assert twin.score(c, planes, thr).tolist() == want                    # inclusive at +-t, out one float32 step beyond; t = 0: e == 0 only
        for splits in (0, 1, 2):
            assert _score(pts, dplanes, thr, None, splits).tolist() == want
    bad = c.copy()
    bad[:, 0] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, np.nan]
    assert _score(_dev(bad), dplanes, float(t), None, 0).tolist() == [0] * 7                           # no usable point
    assert _score(pts, dplanes, float(t), _dev(np.zeros(7, np.uint8)), 0).tolist() == [0] * 7
    assert _score(pts, dplanes, float(t), _dev(np.array([1, 1, 0, 0, 0, 0, 0], np.uint8)), 0).tolist() == [1, 1, 1, 0, 0, 2, 0]
    with pytest.raises(L.OvgError):
        ops.plane_score(pts, dplanes, -1.0)


def _select(count, planes, min_inliers):
    def run():
        outs = [guarded((1, k), dt, "cuda", guard_bytes=4096) for k, dt in ((1, torch.int32), (4, torch.float32), (1, torch.int32), (1, torch.int32))]
        ops.plane_select(count, planes, min_inliers, *(o[0][0] for o in outs))
        torch.cuda.synchronize()
        for (_, check), what in zip(outs, ("best", "plane", "best_count", "status")):
            check(what)
        return tuple(o[0][0] for o in outs)
    best, plane, best_count, status = _twice(run, ("best", "plane", "best_count", "status"))
    return int(best[0]), plane, int(best_count[0]), int(status[0])


def test_select_ties_none_and_min_inliers():
    L.require_gpu()
    rng = np.random.default_rng(5)
    for H in (1, 255, 256, 257, 1000):
        planes = rng.normal(size=(H, 4)).astype(F)
        count = rng.integers(0, 50, H).astype(np.int32)
        top = int(count.max())
        cases = [(count, planes, 3), (count, planes, top), (count, planes, top + 1)]                   # one above the best count: none
        tied = count.copy()
        tied[rng.integers(0, H, 5)] = 77                                       # ties go to the lowest h
        cases.append((tied, planes, 3))
        last = np.zeros(H, np.int32)
        last[H - 1] = 9
        cases.append((last, planes, 3))
        void = planes.copy()
        void[int(tied.argmax())] = np.nan                                      # the winner's plane is not finite: none, and never a NaN
        cases.append((tied, void, 3))
        cases.append((np.zeros(H, np.int32), np.full((H, 4), np.nan, F), 3))    # all void
        cases.append((-count - 1, planes, 3))                                  # negative counts read as 0
        for cnt, pl, mn in cases:
            want = twin.select(cnt, pl, mn)
            got = _select(_dev(cnt), _dev(pl), mn)
            assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:], (H, mn, got, want)
            assert not np.isnan(got[1]).any() and (got[0] >= 0 or ((got[1] == 0).all() and got[3] == L.PLANE_NONE))
        assert _select(_dev(tied), _dev(planes), 3)[0] == int(np.nonzero(tied == 77)[0][0])
        assert _select(_dev(count), _dev(planes), top + 1)[0] == -1


def _mask(pts, plane, t, valid, gate, want_distance=True):
    n = pts.shape[0]

    def run():
        inlier, check_i = guarded((1, n), torch.uint8, "cuda", guard_bytes=4096)
        dist, check_d = guarded((1, n), torch.float32, "cuda", guard_bytes=4096)
        total, check_t = guarded((1, 1), torch.int64, "cuda", guard_bytes=4096)
        out = ops.plane_mask(pts, plane, t, valid=valid, gate=gate, inlier=inlier[0], distance=dist[0] if want_distance else None, out_count=total[0])
        torch.cuda.synchronize()
        check_i("inlier"), check_d("distance"), check_t("out_count")
        assert want_distance or (out[1] is None and bool((dist.view(torch.uint8) == 0xA5).all()))
        return inlier[0], dist[0], total[0]
    return _twice(run, ("inlier", "distance", "out_count"))


def _same_mask(got, want, name):
    inl, dist, cnt = got
    assert inl.dtype == np.uint8 and inl.tobytes() == want[0].tobytes(), (name, int((inl != want[0]).sum()))
    nan = np.isnan(want[1])
    assert (np.isnan(dist) == nan).all() and dist[~nan].tobytes() == want[1][~nan].tobytes(), name
    assert cnt.tolist() == want[2].tolist() == [int(inl.sum())], name


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3000, 70000])
def test_mask_matches_twin_and_the_score_count(n):
    """n around the 1024 points of a workgroup. The plane is read from device memory; out_count equals inlier.sum() and the score
    kernel's count of that plane."""
    L.require_gpu()
    planes = _score_planes()
    c, cv = _dirty(n, 1)
    counts = twin.score(c, planes, T, cv)
    pts, valid = _dev(c), _dev(cv)
    for h in sorted({int(counts.argmax()), int(np.argsort(counts)[-2]), 7, 8, int(np.nonzero(np.isnan(planes).all(-1))[0][0]), 20}):
        for v, dv in ((cv, valid), (None, None)):
            want = twin.mask(c, planes[h], T, v)
            got = _mask(pts, _dev(planes[h]), T, dv, None)
            _same_mask(got, want, "n %d plane %d" % (n, h))
            if v is not None:
                assert got[2][0] == counts[h]
                assert _score(pts, _dev(planes[h:h + 1]), T, dv, 0).tolist() == [got[2][0]]
    h = int(counts.argmax())
    for gate in (L.PLANE_NONE, L.PLANE_NONE | L.PLANE_FEW, L.PLANE_FEW, 0):
        got = _mask(pts, _dev(planes[h]), T, valid, _dev(np.array([gate], np.int32)))
        _same_mask(got, twin.mask(c, planes[h], T, cv, gate), "gate %d" % gate)
        assert (got[2][0] == 0 and np.isnan(got[1]).all()) if gate & L.PLANE_NONE else got[2][0] == counts[h]
    inl = _mask(pts, _dev(planes[h]), T, valid, None, want_distance=False)[0]
    assert inl.tobytes() == twin.mask(c, planes[h], T, cv)[0].tobytes()


def _fit(count, sums, centre, plane, axis=None):
    def run():
        outs = [guarded((1, k), dt, "cuda", guard_bytes=4096) for k, dt in ((4, torch.float32), (1, torch.float64), (3, torch.float64), (1, torch.int32))]
        outs[0][0][0].copy_(plane)
        ops.plane_fit(count, sums, outs[0][0][0], centre=centre, axis=axis, rms=outs[1][0][0], eigen=outs[2][0][0], status=outs[3][0][0])
        torch.cuda.synchronize()
        for (_, check), what in zip(outs, ("plane", "rms", "eigen", "status")):
            check(what)
        return tuple(o[0][0] for o in outs)
    plane, rms, eigen, status = _twice(run, ("plane", "rms", "eigen", "status"))
    return plane, float(rms[0]), eigen, int(status[0])


def _moments(pts, inlier):
    """The two passes of the refit on the device. -> (count, sums, centre) device tensors"""
    n0, s0 = ops.align_moments(pts, pts, source_valid=inlier)
    centre = s0[:6] / n0.clamp_min(1).to(torch.float64)
    n1, s1 = ops.align_moments(pts, pts, source_valid=inlier, centre=centre)
    return n1, s1, centre


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_is_within_one_ulp_of_eigh(seed):
    """The refit of the room's floor from the inliers of the first winner. The eigen-gap is above 100, so the float64 error of either
    solver is far below half a float32 ulp: the device's plane equals the float32 rounding of the eigh plane up to one ulp per
    component (a double rounding at a tie). The Jacobi twin restates the device operation for operation: printed, and equal bytes
    where the device's float64 divide and square root round correctly."""
    L.require_gpu()
    c = twin.scene(3000, seed)[0]
    first = twin.segment_plane(c, T, H=64, seed=0, refit=0)
    pts = _dev(c)
    N, s, centre = _moments(pts, _dev(first["inlier"]))
    tN, ts, tc = twin.inlier_moments(c, first["inlier"])
    wN, ws, wc = _host(N), _host(s), _host(centre)                          # the twin solves the device's own moments
    assert wN.tolist() == tN.tolist() and np.allclose(ws, ts, rtol=1e-12, atol=1e-12) and np.allclose(wc, tc, rtol=1e-15, atol=0)
    assert twin.eigen_gap(wN, ws, wc) > 100
    for axis in (None, np.array([0.0, 0.0, -1.0], F)):
        want, want_rms, want_eig, st = twin.fit_eigh(wN, ws, wc, first["plane"], axis)
        jac = twin.fit(wN, ws, wc, first["plane"], axis)
        plane, rms, eig, status = _fit(N, s, centre, _dev(first["plane"]), _dev(axis))
        print("seed %d: ulps to eigh %s, to the Jacobi twin %s" % (seed, _ulps(plane, want).tolist(), _ulps(plane, jac[0]).tolist()))
        assert status == st == 0 and (_ulps(plane, want) <= 1).all()
        assert abs(rms - want_rms) <= 1e-9 * want_rms and np.allclose(eig, want_eig, rtol=1e-9, atol=0)
        assert axis is None or plane[:3].astype(np.float64) @ axis > 0
        assert (_ulps(plane, jac[0]) <= 1).all() and abs(rms - jac[1]) <= 1e-12 * jac[1]


def test_fit_degenerate_cases_keep_the_plane():
    L.require_gpu()
    keep = np.array([0, 0.6, 0.8, -5], F)
    c = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [0, 1, 0]], F)
    pts = _dev(c)
    for inl, bits in (([1, 1, 0, 0, 0], L.PLANE_FEW), ([0, 0, 0, 0, 0], L.PLANE_FEW), ([1, 1, 1, 1, 0], L.PLANE_NO_SPREAD), ([1, 1, 1, 1, 1], 0)):
        inl = np.array(inl, np.uint8)
        N, s, centre = _moments(pts, _dev(inl))
        plane, rms, eig, status = _fit(N, s, centre, _dev(keep))
        want = twin.fit(*twin.inlier_moments(c, inl), keep)
        assert status == bits == want[3] and plane.tobytes() == want[0].tobytes() and rms == want[1] == 0 and (bits == 0 or (eig == 0).all())
        assert (plane == keep).all() if bits else plane.tolist() == [0, 0, 1, 0]
    # coincident inliers, and non-finite sums forced into the entry directly (a float32 coordinate cannot overflow a float64 sum)
    same = _dev(np.ones((4, 3), F))
    N, s, centre = _moments(same, _dev(np.ones(4, np.uint8)))
    assert _fit(N, s, centre, _dev(keep))[3] == L.PLANE_NO_SPREAD
    N, s, centre = _moments(pts, _dev(np.ones(5, np.uint8)))
    for k, value in ((0, np.inf), (7, np.nan), (17, -np.inf)):
        bad = s.clone()
        bad[k] = value
        plane, rms, eig, status = _fit(N, bad, centre, _dev(keep))
        assert status == L.PLANE_NOT_FINITE and (plane == keep).all() and rms == 0
    bad_centre = centre.clone()
    bad_centre[4] = np.nan
    assert _fit(N, s, bad_centre, _dev(keep))[3] == L.PLANE_NOT_FINITE
    few = torch.tensor([2], device="cuda", dtype=torch.int64)
    assert _fit(few, bad, centre, _dev(keep))[3] == L.PLANE_FEW | L.PLANE_NOT_FINITE
    assert _fit(N, s, None, _dev(keep))[3] == 0                              # no centre: zeros


def _result(res):
    return dict(plane=_host(res.plane), inlier=_host(res.inlier).reshape(-1).astype(np.uint8), count=int(res.count), hypothesis=int(res.hypothesis),
                rms=float(res.rms), status=int(res.status), distance=None if res.distance is None else _host(res.distance).reshape(-1))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_segment_plane_matches_twin_on_the_room(seed):
    L.require_gpu()
    n = 3000
    c, floor_n, wall_n, part = twin.scene(n, seed)
    pts = _dev(c)
    want = twin.segment_plane(c, T, H=64, seed=0, refit=0)
    runs = [_result(postprocess.segment_plane(pts, threshold=T, hypotheses=64, seed=0, refit=0, return_distance=True)) for _ in range(2)]
    got = runs[0]
    for k in ("plane", "inlier", "distance"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes()
    assert (got["hypothesis"], got["count"], got["status"], got["rms"]) == (want["hypothesis"], want["count"], 0, 0.0)
    assert got["plane"].tobytes() == want["plane"].tobytes() and got["inlier"].tobytes() == want["inlier"].tobytes()
    nan = np.isnan(want["distance"])
    assert (np.isnan(got["distance"]) == nan).all() and got["distance"][~nan].tobytes() == want["distance"][~nan].tobytes()
    print("seed %d: %d floor inliers, |cos| %.7f" % (seed, got["count"], abs(got["plane"][:3].astype(np.float64) @ floor_n)))
    assert got["count"] >= 0.48 * n and abs(got["plane"][:3].astype(np.float64) @ floor_n) >= 0.9999
    # refit = 2 (the default): the mask is the twin's mask of the DEVICE's refit plane
    res = postprocess.segment_plane(pts.reshape(3, 1000, 3), threshold=T, hypotheses=64)
    assert res.inlier.shape == (3, 1000) and res.inlier.dtype == torch.bool and res.distance is None and res.plane.dtype == torch.float32
    assert res.count.dtype == torch.int64 and res.hypothesis.dtype == torch.int32 and res.rms.dtype == torch.float64 and res.status.dtype == torch.int32
    assert all(v.dim() == 0 and v.is_cuda for v in (res.count, res.hypothesis, res.rms, res.status))
    got2 = _result(res)
    m = twin.mask(c, got2["plane"], T)
    assert got2["inlier"].tobytes() == m[0].tobytes() and got2["count"] == int(m[2][0]) and got2["status"] == 0 and got2["hypothesis"] == want["hypothesis"]
    full = twin.segment_plane(c, T, H=64, seed=0, refit=2)
    eigh = twin.segment_plane(c, T, H=64, seed=0, refit=2, fit_fn=twin.fit_eigh)
    print("seed %d refit 2: %d inliers (twin %d), ulps to the Jacobi twin %s, to eigh %s, rms %.6f" % (
        seed, got2["count"], full["count"], _ulps(got2["plane"], full["plane"]).tolist(), _ulps(got2["plane"], eigh["plane"]).tolist(), got2["rms"]))
    assert (_ulps(got2["plane"], eigh["plane"]) <= 1).all() and got2["count"] >= 0.48 * n and 0.002 < got2["rms"] < 0.005
    assert abs(got2["plane"][:3].astype(np.float64) @ floor_n) >= 0.999999
    # the axis along the wall normal within 10 degrees returns the wall, not the larger floor
    wall = _result(postprocess.segment_plane(pts, threshold=T, axis=tuple(float(v) for v in wall_n), max_angle_deg=10.0))
    assert 0.23 * n <= wall["count"] < 0.3 * n and wall["plane"][:3].astype(np.float64) @ wall_n >= 0.9999 and wall["status"] == 0
    ax = (wall_n / np.sqrt((wall_n[0] * wall_n[0] + wall_n[1] * wall_n[1]) + wall_n[2] * wall_n[2])).astype(F)
    twall = twin.segment_plane(c, T, H=1024, seed=0, refit=0, axis=ax, min_abs_cos=float(F(math.cos(math.radians(10.0)))))
    dwall = _result(postprocess.segment_plane(pts, threshold=T, axis=_dev(wall_n), max_angle_deg=10.0, refit=0))
    assert dwall["hypothesis"] == twall["hypothesis"] and dwall["inlier"].tobytes() == twall["inlier"].tobytes()
    assert (_ulps(dwall["plane"], twall["plane"]) <= 1).all()                # the tensor axis is normalised on the device
    # floor_alignment puts the inliers on the ground and the normal on `up`
    for up in ((0.0, 1.0, 0.0), (0.0, 0.0, -1.0)):
        sim = postprocess.floor_alignment(res, up=up)
        assert sim.matrix.is_cuda and sim.matrix.dtype == torch.float64
        moved = _host(sim.apply(pts))
        u = np.array(up)
        assert np.abs(moved[got2["inlier"] != 0] @ u).max() <= T + 1e-5
        assert np.abs(_host(sim.matrix)[:3, :3] @ got2["plane"][:3].astype(np.float64) - u).max() <= 1e-6
        assert np.abs(moved @ u - (c.astype(np.float64) @ got2["plane"][:3].astype(np.float64) + float(got2["plane"][3]))).max() <= 1e-5


def test_segment_planes_labels_match_twin():
    L.require_gpu()
    n = 3000
    for seed in (0, 1, 2):
        c, floor_n, wall_n, part = twin.scene(n, seed)
        pts = _dev(c)
        for refit in (0, 2):
            want_p, want_l, want_r = twin.segment_planes(c, T, max_planes=4, min_inliers=n // 20, H=64, seed=0, refit=refit)
            planes, labels = postprocess.segment_planes(pts.reshape(30, 100, 3), max_planes=4, min_inliers=n // 20, threshold=T, hypotheses=64, refit=refit)
            assert planes.shape == (2, 4) and planes.dtype == torch.float32 and labels.shape == (30, 100) and labels.dtype == torch.int32
            got_p, got_l = _host(planes), _host(labels).reshape(-1)
            if refit == 0:
                assert got_p.tobytes() == want_p.tobytes() and got_l.tobytes() == want_l.tobytes()
            else:
                # the labels of the device's own planes, extracted in order; the twin's Jacobi refit restates the device's
                own = np.full(n, -1, np.int32)
                for k in range(2):
                    own[(twin.mask(c, got_p[k], T, own < 0)[0] != 0)] = k
                assert got_l.tobytes() == own.tobytes() and (_ulps(got_p, want_p) <= 1).all()
                print("seed %d: plane ulps to the twin %s, %d labels differ" % (seed, _ulps(got_p, want_p).tolist(), int((got_l != want_l).sum())))
                assert got_l.tobytes() == want_l.tobytes()
            assert (got_l == 0).sum() >= 0.48 * n and (got_l == 1).sum() >= 0.23 * n
            assert abs(got_p[0][:3].astype(np.float64) @ floor_n) >= 0.9999 and abs(got_p[1][:3].astype(np.float64) @ wall_n) >= 0.9999
        col = postprocess.cluster_colors(labels)
        assert col.shape == (30, 100, 3) and bool((col[labels < 0] == 128).all())
    planes, labels = postprocess.segment_planes(pts, max_planes=1, threshold=T, hypotheses=64)
    assert planes.shape == (1, 4) and set(_host(labels).tolist()) == {-1, 0}
    planes, labels = postprocess.segment_planes(pts, min_inliers=n, threshold=T, hypotheses=64)
    assert planes.shape == (0, 4) and bool((labels == -1).all())
    cand = np.random.default_rng(0).permutation(n)[:1500].astype(np.int32)
    want_p, want_l, _ = twin.segment_planes(c, T, max_planes=3, min_inliers=n // 20, H=64, seed=5, refit=0, candidates=cand)
    planes, labels = postprocess.segment_planes(pts, max_planes=3, min_inliers=n // 20, threshold=T, hypotheses=64, seed=5, refit=0, candidates=_dev(cand.astype(np.int64)))
    assert _host(planes).tobytes() == want_p.tobytes() and _host(labels).tobytes() == want_l.tobytes() and len(want_p) == 2


def test_python_layer_seeds_masks_candidates_and_removal():
    L.require_gpu()
    n = 3000
    c, cv = _dirty(n, 2)
    pts, valid = _dev(c), _dev(cv)
    a = ops.plane_hypotheses(pts, 64, 5, valid=valid)
    b = ops.plane_hypotheses(pts, 64, 5, valid=valid)
    other = ops.plane_hypotheses(pts, 64, 6, valid=valid)
    assert torch.equal(a[1], b[1]) and _host(a[0]).tobytes() == _host(b[0]).tobytes() and not torch.equal(a[1], other[1])
    cand = np.nonzero(cv)[0][::3].astype(np.int32)
    want = twin.segment_plane(c, T, H=64, seed=9, refit=0, valid=cv, candidates=cand, min_inliers=50)
    for dc in (_dev(cand), _dev(cand.astype(np.int64))):
        got = _result(postprocess.segment_plane(pts, threshold=T, hypotheses=64, seed=9, refit=0, valid=valid.bool(), candidates=dc, min_inliers=50))
        assert got["hypothesis"] == want["hypothesis"] >= 0 and got["plane"].tobytes() == want["plane"].tobytes()
        assert got["inlier"].tobytes() == want["inlier"].tobytes() and got["count"] == want["count"] and not got["inlier"][cv == 0].any()
    # no hypothesis reaches min_inliers: no plane, zeros, nothing is an inlier, and the refit keeps the zeros
    for refit in (0, 2):
        none = _result(postprocess.segment_plane(pts, threshold=T, hypotheses=64, seed=9, refit=refit, valid=valid, min_inliers=n, return_distance=True))
        tw = twin.segment_plane(c, T, H=64, seed=9, refit=refit, valid=cv, min_inliers=n)
        assert none["hypothesis"] == -1 and (none["plane"] == 0).all() and none["count"] == 0 and not none["inlier"].any()
        assert none["status"] == tw["status"] == (L.PLANE_NONE | (L.PLANE_FEW if refit else 0)) and np.isnan(none["distance"]).all()
    empty = postprocess.segment_plane(pts[:0], threshold=T, return_distance=True)
    assert int(empty.status) == L.PLANE_NONE and empty.inlier.shape == (0,) and int(empty.hypothesis) == -1 and empty.distance.shape == (0,)
    assert int(postprocess.segment_plane(pts, threshold=T, candidates=_dev(cand[:0])).status) == L.PLANE_NONE
    assert postprocess.segment_planes(pts[:0], threshold=T)[0].shape == (0, 4)
    # a PointCloud: rel_threshold = f32(rel) * scene_scale, and the gather of remove_radius_outliers
    ok = np.isfinite(c).all(1)
    cloud = c[ok]
    colors = np.random.default_rng(0).integers(0, 256, (len(cloud), 3)).astype(np.uint8)
    conf = np.random.default_rng(1).random(len(cloud)).astype(F)
    scale = torch.tensor(2.0, device="cuda")
    pc = postprocess.PointCloud(_dev(cloud), _dev(colors), torch.tensor(0.5, device="cuda"), scale, np.eye(4), torch.zeros(2, 3, 4, device="cuda"),
                                _dev(np.arange(len(cloud), dtype=np.int64) * 3 + 1), _dev(conf))
    t_rel = float(F(0.005) * F(2.0))
    want = twin.segment_plane(cloud, t_rel, H=64, seed=0, refit=0)
    res = postprocess.segment_plane(pc, rel_threshold=0.005, hypotheses=64, refit=0)
    assert _host(res.inlier).astype(np.uint8).tobytes() == want["inlier"].tobytes() and _host(res.plane).tobytes() == want["plane"].tobytes()
    for keep, sel in (("outliers", want["inlier"] == 0), ("inliers", want["inlier"] != 0)):
        out = postprocess.remove_plane(pc, res, keep=keep)
        idx = np.nonzero(sel)[0]
        assert 0 < len(idx) < len(cloud) and len(out) == len(idx) and _host(out.points).tobytes() == cloud[idx].tobytes()
        assert _host(out.colors).tobytes() == colors[idx].tobytes() and _host(out.conf).tobytes() == conf[idx].tobytes()
        assert _host(out.indices).tolist() == (idx * 3 + 1).tolist()
        assert out.scene_scale is scale and out.extrinsic is pc.extrinsic and out.transform is pc.transform and out.conf_threshold is pc.conf_threshold
    bare = postprocess.PointCloud(_dev(cloud), None, None, scale, None, None)
    assert _host(postprocess.remove_plane(bare, res).indices).tolist() == np.nonzero(want["inlier"] == 0)[0].tolist()
    moved = postprocess.floor_alignment(res).apply(pc)
    assert isinstance(moved, postprocess.PointCloud) and moved.colors is pc.colors and np.abs(_host(moved.points)[want["inlier"] != 0, 1]).max() <= t_rel + 1e-5


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
    t = 0.02
    want = twin.segment_plane(P, t, H=256, seed=0, refit=0)
    got = _result(postprocess.segment_plane(_dev(P), threshold=t, hypotheses=256, seed=0, refit=0))
    planes, index = ops.plane_hypotheses(_dev(P), 256, 0)
    assert _host(index).tobytes() == want["index"].tobytes()
    _same_planes(_host(planes), twin.hypotheses(P, 256, 0)[0], "real views")
    assert _host(ops.plane_score(_dev(P), planes, t)).tobytes() == want["counts"].tobytes()
    assert got["hypothesis"] == want["hypothesis"] >= 0 and got["count"] == want["count"] and got["plane"].tobytes() == want["plane"].tobytes()
    assert got["inlier"].tobytes() == want["inlier"].tobytes()
    res = _result(postprocess.segment_plane(_dev(P), threshold=t, hypotheses=256))
    assert res["inlier"].tobytes() == twin.mask(P, res["plane"], t)[0].tobytes() and res["status"] == 0
    print("real views: %d points, the winner holds %d, %d after two refits, rms %.4f" % (len(P), got["count"], res["count"], res["rms"]))
