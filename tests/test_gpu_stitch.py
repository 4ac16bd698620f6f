"""ovg_align_wmoments / _wsolve / _move_maps / _move_cameras and postprocess.fit_similarity_robust, stitch_predictions and
OmniVGGT.forward_chunked on the device against tests/stitch_twin.py: the weighted moments and the two moves byte for byte in exact-size
guarded buffers, the weighted solve against the twin's independent weighted Umeyama / SVD fit, the refit loop iteration by iteration
from the twin's previous transform, the robust fixture (30 % one-sided outliers), synthetic chunks of a known scene stitched in both
prediction modes and both select modes, a depth-2 model run in chunks, and the four entries under the stream contract."""
import os

import numpy as np
import pytest
import torch

import align_twin
import common
import small_grids as sg
import stitch_twin as twin
import stream_contract as sc
import test_gpu_stream_contract as tsc
from kernel_guards import guarded
from omnivggt_official_amd import camera_math, ops, postprocess
from omnivggt_official_amd import lib as L

pytestmark = pytest.mark.gpu
F = np.float32
TILE, THREADS = L.ALIGN_TILE, L.ALIGN_THREADS


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wmoments(p, q, weight=None, source_valid=None, target_valid=None, transform=None, delta=None, delta_scale=1.0, cauchy=False, centre=None):
    """ovg_align_wmoments into exact-size guarded outputs and an exact-size guarded workspace. -> (count int64 [1], sums f64 [20]) numpy"""
    count, check_c = guarded((1, 1), torch.int64, "cuda", guard_bytes=4096)
    sums, check_s = guarded((1, L.WALIGN_SUMS), torch.float64, "cuda", guard_bytes=4096)
    ws, check_w = guarded((1, ops.align_wmoments_workspace_bytes(len(p))), torch.uint8, "cuda", guard_bytes=4096)
    out = ops.align_wmoments(_dev(p), _dev(q), _dev(weight), _dev(source_valid), _dev(target_valid), _dev(transform),
                             None if delta is None else _dev(np.asarray(delta, np.float64).reshape(1)), delta_scale, cauchy, _dev(centre),
                             ws=ws[0], count=count[0], sums=sums[0])
    torch.cuda.synchronize()
    check_c("count"), check_s("sums"), check_w("workspace")
    assert out[0].data_ptr() == count.data_ptr() and out[1].data_ptr() == sums.data_ptr()
    return count[0].cpu().numpy(), sums[0].cpu().numpy()


def _same(got, want, name):
    assert got[0].dtype == want[0].dtype == np.int64 and got[0].tolist() == want[0].tolist(), (name, got[0], want[0])
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes(), (name, np.nonzero(got[1] != want[1])[0].tolist(), got[1], want[1])


def _wsolve(count, sums, centre=None, with_scale=True, keep=False, transform=None, scale=None):
    """ovg_align_wsolve into guarded outputs; transform / scale: what the buffers hold before the call (KEEP leaves them there).
    -> dict like the twin's"""
    T, check_t = guarded((4, 4), torch.float64, "cuda", guard_bytes=4096)
    outs = [guarded((1, 1), dt, "cuda", guard_bytes=4096) for dt in (torch.float64,) * 4 + (torch.int64, torch.int32)]
    T.copy_(_dev(np.eye(4) * 7 if transform is None else np.asarray(transform, np.float64)))
    outs[0][0].fill_(-3.0 if scale is None else scale)
    ops.align_wsolve(_dev(np.asarray(count, np.int64).reshape(1)), _dev(np.asarray(sums, np.float64)), T, _dev(centre), with_scale, keep,
                     *(o[0][0] for o in outs))
    torch.cuda.synchronize()
    check_t("transform")
    for (_, check), name in zip(outs, ("scale", "rms", "fit_rms", "weight", "count", "status")):
        check(name)
    v = [o[0][0].cpu().numpy()[0] for o in outs]
    return dict(transform=T.cpu().numpy(), scale=v[0], rms=v[1], fit_rms=v[2], weight=v[3], count=v[4], status=v[5])


def _close(got, want, extent, name):
    """ovg_align_solve's own gate (test_gpu_align._compare_with_svd): rotation, scale and translation / extent within 1e-12."""
    T, s, R, rs = got["transform"], got["scale"], want["transform"] if isinstance(want, dict) else want[0], want["scale"] if isinstance(want, dict) else want[1]
    dR, ds, dt = np.abs(T[:3, :3] / s - R[:3, :3] / rs).max(), abs(s - rs), np.abs(T[:3, 3] - R[:3, 3]).max() / extent
    print("%s: dR %.3g ds %.3g dt/extent %.3g" % (name, dR, ds, dt))
    assert max(dR, ds, dt) <= 1e-12 and (T[3] == [0, 0, 0, 1]).all(), (name, dR, ds, dt)


def _clouds(n, seed):
    """A source cloud, a target that is a noisy Sim(3) of it (so a transform leaves small residuals), weights over three decades."""
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(n, 3)) * [3, 2, 1] + [10, -4, 7]).astype(F)
    T0, _ = _sim3(rng, 35.0, 1.3, 2.0)
    q = (p.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3] + rng.normal(size=(n, 3)) * 0.05).astype(F)
    w = (10.0 ** rng.uniform(-1.5, 1.5, n)).astype(F)
    T1 = T0.copy()
    T1[:3] += rng.normal(size=(3, 4)) * 0.01                                 # a transform near the truth: residuals of the size of delta
    return rng, p, q, w, T1


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049, THREADS * TILE + 1])
def test_wmoments_match_twin_bit_exactly(n):
    """n around the 256 threads of a workgroup and the 1024 pairs of a tile; 2049 is three tiles; 256 * 1024 + 1 is 257 tiles, so thread 0
    of the fold adds two partials."""
    assert (TILE, THREADS) == (1024, 256)
    big = n > 4096
    rng, p, q, w, T1 = _clouds(n, n)
    centre = np.concatenate([p.astype(np.float64).mean(0), q.astype(np.float64).mean(0)]) + 0.1
    # unit weights, no flag: sums [0..17] and the count are ovg_align_moments' bytes
    got = _wmoments(p, q)
    _same(got, twin.wmoments(p, q), "plain")
    _same(_wmoments(p, q), got, "second call")
    old = align_twin.moments(p, q)
    assert got[0].tolist() == old[0].tolist() == [n] and got[1][:18].tobytes() == old[1].tobytes() and got[1][18] == n == got[1][19]
    cnt, sums = ops.align_moments(_dev(p), _dev(q))
    assert sums.cpu().numpy().tobytes() == got[1][:18].tobytes() and cnt.cpu().numpy().tolist() == [n]
    kw = dict(weight=w, transform=T1, cauchy=True, delta=np.array([0.2]), delta_scale=0.5, centre=centre)
    got = _wmoments(p, q, **kw)
    _same(got, twin.wmoments(p, q, **kw), "weights, transform, device delta, centre")
    _same(_wmoments(p, q, **kw), got, "second call, reweighted")
    if big:
        return
    # weights with 0, a negative, NaN and +inf; masks with holes; non-finite coordinates
    bad_p, bad_q, bw = p.copy(), q.copy(), w.copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        bad_p[rng.integers(0, n, max(1, n // 50)), k] = v
        bad_q[rng.integers(0, n, max(1, n // 50)), 2 - k] = v
    for v in (0.0, -1.0, np.nan, np.inf, -0.0):
        bw[rng.integers(0, n, max(1, n // 40))] = v
    sv, tv = (rng.random(n) >= 0.1).astype(np.uint8) * 7, (rng.random(n) >= 0.1).astype(np.uint8)
    cases = [("weights", dict(weight=bw)), ("bad entries", dict(weight=bw, source_valid=sv, target_valid=tv)),
             ("bad entries, centre", dict(weight=bw, source_valid=sv, target_valid=tv, centre=centre)),
             ("masks alone", dict(source_valid=sv, target_valid=tv)),
             ("transform without the flag", dict(weight=bw, transform=T1, centre=centre)),
             ("cauchy, device delta", dict(weight=bw, source_valid=sv, transform=T1, cauchy=True, delta=np.array([0.07]), delta_scale=0.5, centre=centre)),
             ("cauchy, absolute delta", dict(weight=bw, transform=T1, cauchy=True, delta_scale=0.11)),
             ("cauchy without a transform", dict(weight=bw, cauchy=True, delta_scale=30.0))]
    for name, kw in cases:
        with np.errstate(all="ignore"):
            want = twin.wmoments(bad_p, bad_q, **kw)
        _same(_wmoments(bad_p, bad_q, **kw), want, name)
        assert n < 255 or 0 < int(want[0][0]) < n, name
    # a delta of 0, NaN, +inf or below zero reweights nothing: the bytes of the unweighted call under the same transform
    base = _wmoments(bad_p, bad_q, weight=bw, transform=T1, centre=centre)
    for d, ds in ((0.0, 0.5), (np.nan, 0.5), (np.inf, 0.5), (-2.0, 0.5), (0.3, 0.0), (0.3, np.inf), (1e-170, 1e-10), (None, 0.0)):
        got = _wmoments(bad_p, bad_q, weight=bw, transform=T1, centre=centre, cauchy=True, delta=None if d is None else np.array([d]), delta_scale=ds)
        _same(got, base, "delta %r x %r" % (d, ds))
        _same(got, twin.wmoments(bad_p, bad_q, weight=bw, transform=T1, centre=centre, cauchy=True, delta=None if d is None else np.array([d]), delta_scale=ds),
              "twin, delta %r x %r" % (d, ds))
    # no used pair: count 0 and every sum +0.0 -- also when no moved point is finite
    off = T1.copy()
    off[1, 3] = np.inf
    for kw in (dict(weight=np.zeros(n, F)), dict(source_valid=np.zeros(n, np.uint8)), dict(weight=np.full(n, np.nan, F), cauchy=True, transform=T1),
               dict(weight=w, transform=off), dict(transform=off, cauchy=True, delta_scale=0.3)):
        got = _wmoments(p, q, centre=centre, **kw)
        assert got[0].tolist() == [0] and got[1].tobytes() == np.zeros(20).tobytes(), kw.keys()
    with pytest.raises(L.OvgError):
        ops.align_wmoments(_dev(p), _dev(q), delta_scale=float("nan"), cauchy=True)


def _fit_at_entries(p, q, with_scale=True, keep=False, transform=None, scale=None, **kw):
    n0, s0 = _wmoments(p, q, **kw)
    centre = s0[:6] / (s0[18] if s0[18] > 0 else 1.0)
    n1, s1 = _wmoments(p, q, centre=centre, **kw)
    return _wsolve(n1, s1, centre, with_scale, keep, transform, scale), (n1, s1, centre)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_wsolve_matches_the_weighted_svd_solution_and_the_residual(seed):
    rng, p, q, w, T1 = _clouds(500, 100 + seed)
    extent = np.abs(q.astype(np.float64)).max()
    for with_scale in (True, False):
        got, (n1, s1, centre) = _fit_at_entries(p, q, with_scale, weight=w)
        assert got["status"] == 0 and got["count"] == 500 and align_twin.gap(n1, s1 / s1[18] * 500) >= 1e-3
        _close(got, twin.wsolve_svd(p, q, w, with_scale), extent, "seed %d scale %d against the SVD" % (seed, with_scale))
        want = twin.wsolve(n1, s1, centre, with_scale)
        _close(got, want, extent, "seed %d scale %d against the twin" % (seed, with_scale))
        assert (with_scale or got["scale"] == 1.0) and got["weight"] == s1[18]
        # rms: the weighted residual under the transform the weights came from (none: the identity)
        assert abs(got["rms"] - np.sqrt(s1[17] / s1[18])) <= 1e-15 * got["rms"]
        # fit_rms against the twin's directly summed weighted residual, within the cancellation bound 64 * 2^-53 * vb / E on E
        E, rms = twin.weighted_residual(got["transform"], p, q, w.astype(np.float64))
        rel = 64 * 2.0 ** -53 * want["vb"] / E
        print("seed %d scale %d: vb %.6g E %.6g, bound on E %.3g relative; fit_rms %.17g direct %.17g" % (seed, with_scale, want["vb"], E, rel, got["fit_rms"], rms))
        assert abs(got["fit_rms"] ** 2 * s1[18] - E) <= rel * E


def test_wsolve_with_unit_weights_is_align_solve_byte_for_byte():
    rng, p, q, w, T1 = _clouds(777, 7)
    for with_scale in (True, False):
        got, (n1, s1, centre) = _fit_at_entries(p, q, with_scale)
        assert s1[18] == 777.0
        T = torch.empty(4, 4, device="cuda", dtype=torch.float64)
        scale, rms = torch.empty(1, device="cuda", dtype=torch.float64), torch.empty(1, device="cuda", dtype=torch.float64)
        ops.align_solve(_dev(n1), _dev(s1[:18]), T, _dev(centre), with_scale, False, scale, rms)
        assert T.cpu().numpy().tobytes() == got["transform"].tobytes() and scale.item() == got["scale"] and rms.item() == got["rms"]
        sim = postprocess.fit_similarity(_dev(p), _dev(q), with_scale=with_scale)
        fit = postprocess.fit_similarity_robust(_dev(p), _dev(q), with_scale=with_scale, iterations=0)
        assert sim.matrix.cpu().numpy().tobytes() == fit.transform.matrix.cpu().numpy().tobytes() == got["transform"].tobytes()
        assert fit.count.tolist() == [777] and fit.status.tolist() == [0] and fit.effective_pairs.tolist() == [777.0]


def test_wsolve_degenerate_statuses_with_and_without_keep():
    P = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 10], [0, 1, 0], [2, 2, 2]], F)
    held = np.eye(4)
    held[:3] = np.arange(12).reshape(3, 4) + 0.5
    ok_n, ok_s = _wmoments(P, P + 1, weight=np.arange(1, 6).astype(F))
    cases = [("two pairs", _wmoments(P[:2], P[:2] + 1), L.ALIGN_FEW_PAIRS), ("coincident", _wmoments(np.tile(P[:1], (5, 1)), P), L.ALIGN_NO_SPREAD),
             ("five pairs of weight zero", _wmoments(P, P + 1, weight=np.zeros(5, F)), L.ALIGN_FEW_PAIRS)]
    for k, v in ((0, np.inf), (7, np.nan), (15, np.inf), (17, -np.inf), (19, np.inf)):
        bad = ok_s.copy()
        bad[k] = v
        cases.append(("sums[%d] = %r" % (k, v), (ok_n, bad), L.ALIGN_NOT_FINITE))
    for v, want in ((np.nan, L.ALIGN_FEW_PAIRS | L.ALIGN_NOT_FINITE), (np.inf, L.ALIGN_NOT_FINITE), (-1.0, L.ALIGN_FEW_PAIRS), (0.0, L.ALIGN_FEW_PAIRS)):
        bad = ok_s.copy()
        bad[18] = v
        cases.append(("W = %r" % v, (ok_n, bad), want))
    cases.append(("count 2 with weight", (np.array([2]), ok_s), L.ALIGN_FEW_PAIRS))
    for name, (n_, s_), want in cases:
        for with_scale in (True, False):
            r = _wsolve(n_, s_, None, with_scale)
            assert r["status"] == want == twin.wsolve(n_, s_, None, with_scale)["status"], (name, r["status"])
            assert r["transform"].tobytes() == np.eye(4).tobytes() and r["scale"] == 1.0 and r["fit_rms"] == 0.0 and np.isfinite(r["rms"]), name
            assert r["count"] == n_[0] and (r["weight"] == s_[18] or (np.isnan(r["weight"]) and np.isnan(s_[18]))), name
            k = _wsolve(n_, s_, None, with_scale, keep=True, transform=held, scale=2.5)
            assert k["status"] == want and k["transform"].tobytes() == held.tobytes() and k["scale"] == 2.5 and k["fit_rms"] == 0.0, name
    assert _wsolve(ok_n, ok_s, centre=np.array([0, 0, np.nan, 0, 0, 0.0]))["status"] == L.ALIGN_NOT_FINITE
    # a regular solve with KEEP writes like one without
    a, b = _wsolve(ok_n, ok_s), _wsolve(ok_n, ok_s, keep=True, transform=held, scale=2.5)
    assert a["status"] == b["status"] == 0 and a["transform"].tobytes() == b["transform"].tobytes() and a["scale"] == b["scale"] != 2.5


def _check_refits(p, q, name, weight=None, source_valid=None, target_valid=None, with_scale=True, iterations=6, rel_delta=0.5):
    """Every iteration at the entries, started from the TWIN's previous transform and fit_rms: the two moment passes byte for byte, the
    solve within 1e-12. -> the twin's per-iteration results"""
    want = twin.fit_robust(p, q, weight, source_valid, target_valid, with_scale, iterations, rel_delta)
    extent = np.abs(np.asarray(q, np.float64)[np.isfinite(q).all(1)]).max()
    for k, w in enumerate(want):
        kw = dict(weight=weight, source_valid=source_valid, target_valid=target_valid)
        prev = None
        if k:
            prev = want[k - 1]
            kw.update(transform=prev["transform"], cauchy=True, delta=np.array([prev["fit_rms"]]), delta_scale=rel_delta)
        n0, s0 = _wmoments(p, q, **kw)
        _same((n0, s0), twin.wmoments(p, q, **kw), "%s, iteration %d, first pass" % (name, k))
        centre = s0[:6] / (s0[18] if s0[18] > 0 else 1.0)
        n1, s1 = _wmoments(p, q, centre=centre, **kw)
        _same((n1, s1), twin.wmoments(p, q, centre=centre, **kw), "%s, iteration %d, second pass" % (name, k))
        got = _wsolve(n1, s1, centre, with_scale, keep=k > 0, transform=None if prev is None else prev["transform"], scale=None if prev is None else prev["scale"])
        assert got["status"] == w["status"] == 0 and got["count"] == w["count"], (name, k)
        _close(got, w, extent, "%s, iteration %d" % (name, k))
        assert abs(got["rms"] - w["rms"]) <= 1e-12 * max(w["rms"], 1e-300) and abs(got["weight"] - w["weight"]) <= 1e-12 * w["weight"]
    return want


def test_robust_fit_on_the_fixture():
    """n = 4096, 30 % of the targets displaced by uniform(0, 1)^3: the plain fit is off by 0.15, six refits reach the noise floor."""
    p, q, T = twin.robust_fixture()
    want = _check_refits(p, q, "fixture")
    fit = postprocess.fit_similarity_robust(_dev(p), _dev(q))
    plain = postprocess.fit_similarity(_dev(p), _dev(q))
    torch.cuda.synchronize()
    got = fit.transform.matrix.cpu().numpy()
    e_plain, e_got, e_twin = np.abs(plain.matrix.cpu().numpy() - T).max(), np.abs(got - T).max(), np.abs(want[-1]["transform"] - T).max()
    print("fixture: max |T - T_true| plain %.3g, robust %.3g, the twin's %.3g; device against twin over the whole loop %.3g" % (
        e_plain, e_got, e_twin, np.abs(got - want[-1]["transform"]).max()))
    print("fit_rms device", fit.fit_rms.tolist(), "\nfit_rms twin  ", [w["fit_rms"] for w in want])
    print("effective pairs", fit.effective_pairs.tolist())
    assert e_got <= e_plain / 100.0 and e_got <= 10.0 * e_twin
    assert fit.status.tolist() == [0] * 7 and fit.count.tolist() == [4096] * 7 and fit.weight[0].item() == 4096.0
    assert fit.transform.scale.item() == np.linalg.norm(got[:3, 0]) or abs(fit.transform.scale.item() - np.linalg.norm(got[:3, 0])) <= 1e-12
    eff = fit.effective_pairs.cpu().numpy()
    assert eff[0] == 4096.0 and (eff[1:] < 4096.0).all() and (eff[1:] > 1000.0).all()
    assert fit.rms[0].item() == plain.rms.item() and bool((fit.fit_rms[1:] < fit.fit_rms[:-1]).all())
    # the absolute form, weights and masks through the public entry; a second call gives the same bytes
    w = np.random.default_rng(2).uniform(0.5, 2.0, len(p)).astype(F)
    sv = np.random.default_rng(3).random(len(p)) > 0.1
    a = postprocess.fit_similarity_robust(_dev(p), _dev(q), weights=_dev(w), source_valid=_dev(sv), delta=0.01, iterations=4)
    b = postprocess.fit_similarity_robust(_dev(p), _dev(q), weights=_dev(w), source_valid=_dev(sv), delta=0.01, iterations=4)
    assert a.transform.matrix.cpu().numpy().tobytes() == b.transform.matrix.cpu().numpy().tobytes() and a.fit_rms.tolist() == b.fit_rms.tolist()
    assert np.abs(a.transform.matrix.cpu().numpy() - T).max() <= e_plain / 100.0 and a.count.tolist() == [int(sv.sum())] * 5
    # a degenerate refit keeps the last regular transform: the same points three times are a fit without spread from the start
    flat = postprocess.fit_similarity_robust(_dev(np.tile(p[:1], (9, 1))), _dev(q[:9]), iterations=2)
    assert flat.status.tolist() == [L.ALIGN_NO_SPREAD] * 3 and flat.transform.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes()
    empty = postprocess.fit_similarity_robust(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), iterations=2)
    assert empty.status.tolist() == [L.ALIGN_FEW_PAIRS] * 3 and empty.count.tolist() == [0] * 3


def _sim3(rng, angle_deg=20.0, scale=1.3, shift=0.5):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K), rng.normal(size=3) * shift
    return T, scale


@pytest.mark.parametrize("views,hw", [(1, (1, 1)), (3, (1, 1)), (1, (3, 5)), (3, (3, 5)), (1, (14, 19)), (3, (14, 19))])
def test_move_maps_and_cameras_match_twin_bit_exactly(views, hw):
    rng = np.random.default_rng(views * 100 + hw[1])
    n = views * hw[0] * hw[1]
    M, s = _sim3(rng)
    pts, depth = (rng.normal(size=(n, 3)) * 3).astype(F), rng.uniform(0.5, 5, n).astype(F)
    pc, dc = rng.uniform(1, 9, n).astype(F), rng.uniform(1, 9, n).astype(F)
    if n > 4:
        pts[1, 0], pts[2, 1], depth[3], dc[4] = np.inf, np.nan, np.inf, np.nan
    maps = dict(points=pts, depth=depth, points_conf=pc, depth_conf=dc)
    shapes = dict(points=(n, 3), depth=(1, n), points_conf=(1, n), depth_conf=(1, n))
    for absent in (None, "points", "depth", "points_conf", "depth_conf", ("points", "points_conf"), ("depth", "depth_conf", "points_conf")):
        use = {k: (None if absent is not None and k in absent else v) for k, v in maps.items()}
        outs = {k: guarded(shapes[k], torch.float32, "cuda", guard_bytes=4096) for k, v in use.items() if v is not None}
        got = ops.align_move_maps(n, _dev(M), _dev(np.array([s])), *(_dev(use[k]) for k in maps),
                                  *(outs[k][0].reshape(use[k].shape) if k in outs else None for k in maps))
        torch.cuda.synchronize()
        want = twin.move_maps(M, s, *(use[k] for k in maps))
        for k, g, w in zip(maps, got, want):
            if use[k] is None:
                assert g is None and w is None
            else:
                outs[k][1](k)
                assert g.cpu().numpy().tobytes() == w.tobytes(), (absent, k)
    # in place
    live = {k: _dev(v) for k, v in maps.items()}
    got = ops.align_move_maps(n, _dev(M), _dev(np.array([s])), *live.values(), *live.values())
    for (k, t), g, w in zip(live.items(), got, twin.move_maps(M, s, *maps.values())):
        assert g is t and t.cpu().numpy().tobytes() == w.tobytes(), k
    # cameras
    E = np.stack([_sim3(rng, 40.0, 1.0, 2.0)[0][:3] for _ in range(views)]).astype(F)
    out, check = guarded((views, 3, 4), torch.float32, "cuda", guard_bytes=4096)
    assert ops.align_move_cameras(_dev(E), _dev(M), _dev(np.array([s])), out=out) is out
    torch.cuda.synchronize()
    check("cameras")
    want = twin.move_cameras(E, M, s)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    inplace = _dev(E)
    assert ops.align_move_cameras(inplace, _dev(M), _dev(np.array([s])), out=inplace) is inplace and inplace.cpu().numpy().tobytes() == want.tobytes()
    # The moved camera projects the moved points to s times the old depth. In exact arithmetic z' = s z. Rounding: the moved point has a
    # relative error of 2^-24 per coordinate of magnitude <= |M| |x| (f32 store), the moved camera row 2^-24 per entry of magnitude <= 1
    # and its translation 2^-24 of |t'|; the float64 evaluation below adds nothing of that size. So |z' - s z| <= 2^-24 (3 |x'|_max +
    # 3 |x'|_max + |t'|) and the depth map itself, f32(depth s), is within 2^-24 s z of s z.
    X = (rng.normal(size=(50, 3)) * 3).astype(F)
    z = X.astype(np.float64) @ E[0, 2, :3].astype(np.float64) + float(E[0, 2, 3])
    X2 = ops.align_apply(_dev(X), _dev(M)).cpu().numpy().astype(np.float64)
    z2 = X2 @ want[0, 2, :3].astype(np.float64) + float(want[0, 2, 3])
    bound = 2.0 ** -24 * (6 * np.abs(X2).max() + abs(float(want[0, 2, 3])))
    print("camera move: max |z' - s z| %.3g, bound %.3g" % (np.abs(z2 - s * z).max(), bound))
    assert np.abs(z2 - s * z).max() <= bound
    d = ops.align_move_maps(50, scale=_dev(np.array([s])), depth=_dev(np.abs(z).astype(F)))[1].cpu().numpy()
    assert np.abs(d - s * np.abs(z)).max() <= 2.0 ** -23 * s * np.abs(z).max()


# ---------------------------------------------------------------------------------------------
# stitch_predictions on synthetic chunks of a known scene
# ---------------------------------------------------------------------------------------------
SIGMA = 1e-3
S_ALL, HW, CHUNK, OVERLAP = 7, (8, 10), 4, 2


def _quat(R):
    return camera_math.rotation_to_quaternion(torch.from_numpy(R)).numpy()


def scene(seed=11):
    """Seven views of 8 x 10 pixels of a smooth surface about 3 in front of cameras on an arc: the true world points, z-depths and
    world-to-camera matrices in the frame of chunk 0, and per chunk c the similarity G_c (chunk frame -> true frame; G_0 the
    identity). Each chunk holds the scene under inv(G_c) with N(0, SIGMA) noise on points and depth, confidences in [1, 3], and a
    fifth of its pixels displaced by up to 0.5 with a confidence in [0.1, 0.5] (below the median: never a valid pair).
    -> (truth dict, [chunk dict of numpy arrays with the batch dimension], plan)"""
    rng = np.random.default_rng(seed)
    H, W = HW
    plan = twin.chunk_plan(S_ALL, CHUNK, OVERLAP)
    fov_h, fov_w = 0.9, 1.1
    fy, fx = (H / 2) / np.tan(fov_h / 2), (W / 2) / np.tan(fov_w / 2)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ext, depth, pts = np.zeros((S_ALL, 3, 4)), np.zeros((S_ALL, H, W)), np.zeros((S_ALL, H, W, 3))
    for k in range(S_ALL):
        E = _sim3(rng, 4.0 * k, 1.0, 0.0)[0]
        E[:3, 3] = [0.1 * k, -0.05 * k, 0.02 * k]
        ext[k] = E[:3]
        depth[k] = 3.0 + 0.4 * np.sin(0.7 * u + k) * np.cos(0.5 * v) + 0.05 * k
        cam = np.stack([(u - W / 2) / fx * depth[k], (v - H / 2) / fy * depth[k], depth[k]], -1)
        pts[k] = (cam - E[:3, 3]) @ E[:3, :3]                                                            # R^T (cam - t)
    truth = dict(points=pts, depth=depth, extrinsic=ext)
    chunks, Gs = [], []
    for c, (a, b) in enumerate(plan):
        G, s = (np.eye(4), 1.0) if c == 0 else _sim3(rng, 15.0 + 10 * c, 1.3 - 0.25 * c, 0.5)
        Gi = np.linalg.inv(G)
        n = b - a
        P = pts[a:b].reshape(-1, 3) @ Gi[:3, :3].T + Gi[:3, 3] + rng.normal(size=(n * H * W, 3)) * SIGMA
        D = depth[a:b] / s + rng.normal(size=(n, H, W)) * SIGMA
        E = twin.move_cameras(ext[a:b].astype(F), Gi, 1.0 / s)
        conf_p, conf_d = rng.uniform(1, 3, (n, H, W)), rng.uniform(1, 3, (n, H, W))
        bad = rng.random((n, H, W)) < 0.2
        P = P.reshape(n, H, W, 3)
        P[bad] += rng.uniform(-0.5, 0.5, (int(bad.sum()), 3))
        D[bad] += rng.uniform(0.1, 0.5, int(bad.sum()))
        conf_p[bad], conf_d[bad] = rng.uniform(0.1, 0.5, int(bad.sum())), rng.uniform(0.1, 0.5, int(bad.sum()))
        enc = np.concatenate([E[:, :, 3], np.stack([_quat(E[k, :, :3].astype(np.float64)) for k in range(n)]).astype(F),
                              np.full((n, 1), fov_h, F), np.full((n, 1), fov_w, F)], 1).astype(F)
        chunks.append({"world_points": P.astype(F)[None], "world_points_conf": conf_p.astype(F)[None], "depth": D.astype(F)[None, ..., None],
                       "depth_conf": conf_d.astype(F)[None], "pose_enc": enc[None], "pose_enc_list": [(enc * F(0.5))[None], enc[None]],
                       "images": rng.random((1, n, 3, H, W)).astype(F), "bad": bad})
        Gs.append((G, s))
    truth["G"] = Gs
    return truth, chunks, plan


def _to_device(chunk):
    return {k: [_dev(e) for e in v] if isinstance(v, list) else _dev(v) for k, v in chunk.items() if k != "bad"}


def _chain_bound(scales, fits, n_min):
    """|merged - truth| per coordinate for a pixel that is no outlier: its own noise, N(0, SIGMA) times the chunk's scale, stays under
    5 SIGMA s (3 x 560 draws); every fit on the way to chunk 0 adds the error of a 7-parameter least-squares transform from n >=
    n_min pairs with noise SIGMA sqrt 2 (both sides are noisy), sigma_T = SIGMA sqrt 2 sqrt(7 / n_min) at the data's centre, taken at
    4 standard deviations and at a leverage of 3 (owned views lie next to the overlap views, not among them)."""
    return max(scales) * SIGMA * (5.0 + fits * 4.0 * 3.0 * np.sqrt(2.0) * np.sqrt(7.0 / n_min))


@pytest.mark.parametrize("mode", ["Predicted Pointmap", "Depthmap and Camera Branch"])
@pytest.mark.parametrize("select", ["first", "last"])
def test_stitch_predictions_on_synthetic_chunks(mode, select):
    truth, chunks, plan = scene()
    assert plan == [(0, 4), (2, 6), (4, 7)] == postprocess.chunk_plan(S_ALL, CHUNK, OVERLAP)
    H, W = HW
    dev = [_to_device(c) for c in chunks]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                  # no device -> host synchronisation anywhere
    try:
        out = postprocess.stitch_predictions(dev, plan, prediction_mode=mode, select=select)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    # keys and shapes
    assert out["chunks"] == plan and len(out["chunk_transforms"]) == 3 and len(out["pose_enc_list"]) == 2
    shapes = dict(world_points=(1, 7, H, W, 3), world_points_conf=(1, 7, H, W), depth=(1, 7, H, W, 1), depth_conf=(1, 7, H, W), images=(1, 7, 3, H, W),
                  extrinsic=(1, 7, 3, 4), intrinsic=(1, 7, 3, 3), pose_enc=(1, 7, 9))
    for k, s in shapes.items():
        assert tuple(out[k].shape) == s and out[k].dtype == torch.float32, k
    assert all(tuple(e.shape) == (1, 7, 9) for e in out["pose_enc_list"])
    fits = out["chunk_transforms"]
    assert fits[0].transform.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes() and fits[0].status.tolist() == [0] * 7
    Ts = [f.transform.matrix.cpu().numpy() for f in fits]
    ss = [float(f.transform.scale.item()) for f in fits]
    pointmap = "Pointmap" in mode
    pk, ck = ("world_points", "world_points_conf") if pointmap else ("depth", "depth_conf")
    ext_c, intr_c = zip(*(camera_math.pose_decoding(d["pose_enc"], HW) for d in dev))
    host = [dict({k: c[k][0] for k in ("world_points", "world_points_conf", "depth", "depth_conf")}, extrinsic=e[0].cpu().numpy()) for c, e in zip(chunks, ext_c)]
    n_min = 1 << 30
    for c in (1, 2):
        a, b = plan[c]
        ov = plan[c - 1][1] - a
        before = twin.stitch(host[:c], plan[:c], Ts[:c], ss[:c], select)                                  # the merged maps as chunk c finds them
        cs, ct = host[c][ck][:ov], before[ck][a:a + ov]
        if pointmap:
            src, tgt = host[c][pk][:ov], before[pk][a:a + ov]
        else:                                                                # the device's own un-projection of the same bytes
            K = intr_c[c][0, :ov]
            src = postprocess.unproject_depth_map_to_point_map(_dev(host[c][pk][:ov]), ext_c[c][0, :ov], K, check_skew=False).cpu().numpy()
            tgt = postprocess.unproject_depth_map_to_point_map(_dev(before[pk][a:a + ov]), _dev(before["extrinsic"][a:a + ov]), K, check_skew=False).cpu().numpy()
        sv, tv = cs >= np.percentile(cs, 50.0), ct >= np.percentile(ct, 50.0)
        w = np.minimum(cs, ct).reshape(-1)
        src, tgt, sv, tv = src.reshape(-1, 3), tgt.reshape(-1, 3), sv.reshape(-1).astype(np.uint8), tv.reshape(-1).astype(np.uint8)
        want = _check_refits(src, tgt, "%s %s chunk %d" % (mode, select, c), w, sv, tv)
        direct = postprocess.fit_similarity_robust(_dev(src), _dev(tgt), weights=_dev(w), source_valid=_dev(sv), target_valid=_dev(tv))
        assert direct.transform.matrix.cpu().numpy().tobytes() == Ts[c].tobytes(), "the stitch fitted other pairs than the rule names"
        assert direct.fit_rms.tolist() == fits[c].fit_rms.tolist() and direct.count.tolist() == fits[c].count.tolist()
        print("chunk %d: device against twin over the whole loop %.3g; pairs %d, effective %.1f" % (
            c, np.abs(Ts[c] - want[-1]["transform"]).max(), fits[c].count[-1].item(), fits[c].effective_pairs[-1].item()))
        assert fits[c].status.tolist() == [0] * 7 and ov * H * W * 0.15 < fits[c].count[-1].item() < ov * H * W * 0.5
        n_min = min(n_min, int(fits[c].count[-1].item()))
        print("chunk %d: max |T - G| %.3g, scale %.6f against %.6f" % (c, np.abs(Ts[c] - truth["G"][c][0]).max(), ss[c], truth["G"][c][1]))
    # the merged maps and cameras: the twin's merge with the DEVICE's transforms, byte for byte
    want = twin.stitch(host, plan, Ts, ss, select)
    for k in ("world_points", "world_points_conf", "depth", "depth_conf", "extrinsic"):
        assert out[k][0].cpu().numpy().tobytes() == want[k].tobytes(), k
    owner = [0, 0, 0, 0, 1, 1, 2] if select == "first" else [0, 0, 1, 1, 2, 2, 2]
    imgs = np.concatenate([chunks[c]["images"][:, k - plan[c][0]:k - plan[c][0] + 1] for k, c in enumerate(owner)], 1)
    assert out["images"].cpu().numpy().tobytes() == imgs.tobytes()
    # cameras and encodings: chunk 0's bytes; the translation of an encoding is its camera's; decoding gives the camera back
    enc = out["pose_enc"].cpu().numpy()
    n0 = owner.count(0)
    assert enc[0, :n0].tobytes() == chunks[0]["pose_enc"][0, :n0].tobytes()
    assert out["pose_enc_list"][0].cpu().numpy()[0, :n0].tobytes() == chunks[0]["pose_enc_list"][0][0, :n0].tobytes()
    assert enc[0, :, :3].tobytes() == np.ascontiguousarray(want["extrinsic"][:, :, 3]).tobytes()
    back, K = camera_math.pose_decoding(out["pose_enc"], HW)
    assert np.abs(back[0].cpu().numpy() - want["extrinsic"]).max() <= 1e-5 and np.abs(enc[0, :, 7:] - [0.9, 1.1]).max() <= 1e-5
    assert all(out["intrinsic"][0, k].cpu().numpy().tobytes() == intr_c[0][0, 0].cpu().numpy().tobytes() for k in range(7))
    first = out["pose_enc_list"][0].cpu().numpy()
    moved_half = twin.move_cameras(camera_math.pose_decoding(dev[2]["pose_enc_list"][0], HW)[0][0].cpu().numpy(), Ts[2], ss[2])
    assert first[0, 6, :3].tobytes() == moved_half[-1, :, 3].tobytes()
    # the merged scene against the truth, for pixels that are no outliers
    bound = _chain_bound([1.0] + [s for _, s in truth["G"][1:]], 2, n_min)
    good = np.concatenate([~chunks[c]["bad"][k - plan[c][0]][None] for k, c in enumerate(owner)])
    err = np.abs(out["world_points"][0].cpu().numpy() - truth["points"])[good].max()
    err_d = np.abs(out["depth"][0, ..., 0].cpu().numpy() - truth["depth"])[good].max()
    print("%s %s: merged points within %.3g of the truth, depth within %.3g; bound %.3g (n_min %d)" % (mode, select, err, err_d, bound, n_min))
    assert err <= bound and err_d <= bound
    # the moved cameras see the merged points at the merged depth (outliers included: a camera knows nothing of them)
    E = out["extrinsic"][0].cpu().numpy().astype(np.float64)
    z = np.einsum("shwk,sk->shw", truth["points"], E[:, 2, :3]) + E[:, 2, 3][:, None, None]
    assert np.abs(z - truth["depth"]).max() <= bound


# ---------------------------------------------------------------------------------------------
# forward_chunked on a depth-2 model
# ---------------------------------------------------------------------------------------------
def test_forward_chunked_on_a_depth_2_model():
    torch.set_num_threads(min(32, os.cpu_count()))
    m = sg.build(common.reduced_state_dict(2, 2), torch.float32)
    inp = sg.device_inputs(1, 6, (28, 42))
    args = lambda a, b: tuple(inp[k][:, a:b] for k in ("images", "extrinsics", "intrinsics", "depth", "mask"))
    with torch.no_grad():
        full = m.forward_chunked(*args(0, 6), depth_gt_index=[1, 4], camera_gt_index=[0, 2, 5], chunk_size=4, overlap=2)
        first = m(*args(0, 4), [1], [0, 2])
        second = m(*args(2, 6), [2], [0, 3])
        manual = postprocess.stitch_predictions([first, second], [(0, 4), (2, 6)])
        one = m.forward_chunked(*args(0, 4), depth_gt_index=[1], camera_gt_index=[0, 2], chunk_size=4, overlap=2)
        one5 = m.forward_chunked(inp["images"][0, :4], *args(0, 4)[1:], depth_gt_index=[1], camera_gt_index=[0, 2], chunk_size=5, overlap=1)
    torch.cuda.synchronize()
    same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    assert full["chunks"] == [(0, 4), (2, 6)] and len(full["chunk_transforms"]) == 2
    for k in sg.DENSE + ("pose_enc", "images"):
        assert tuple(full[k].shape[:2]) == (1, 6), k
        assert same(full[k][:, :4], first[k]), "views 0-3 of %s are not forward(views 0..3)'s bytes" % k
        assert same(full[k], manual[k]), "views 4-5 of %s are not the manual stitch's bytes" % k
        assert same(one[k], first[k]) and same(one5[k], first[k]), "one chunk is not forward's own bytes: %s" % k
    for i, e in enumerate(full["pose_enc_list"]):
        assert same(e[:, :4], first["pose_enc_list"][i]) and same(e, manual["pose_enc_list"][i])
        assert same(one["pose_enc_list"][i], first["pose_enc_list"][i])
    assert same(full["extrinsic"], manual["extrinsic"]) and same(full["intrinsic"], manual["intrinsic"])
    assert "chunks" not in one and "extrinsic" not in one and set(one) == set(first)
    assert torch.equal(full["chunk_transforms"][1].transform.matrix, manual["chunk_transforms"][1].transform.matrix)
    # views 4-5 are the second chunk's maps under the fitted transform: not its own bytes, unless the fit is the identity
    T = full["chunk_transforms"][1].transform.matrix.cpu().numpy()
    moved = twin.move_maps(T, float(full["chunk_transforms"][1].transform.scale.item()), second["world_points"][0, 2:].cpu().numpy())[0]
    assert full["world_points"][0, 4:].cpu().numpy().tobytes() == moved.tobytes()
    assert bool(torch.isfinite(full["world_points"]).all()) and bool(torch.isfinite(full["pose_enc"]).all())
    two = torch.cat([inp["images"], inp["images"]], 0)
    with pytest.raises(ValueError):
        m.forward_chunked(two, chunk_size=4, overlap=2)
    with pytest.raises(ValueError):
        m.forward_chunked(inp["images"], chunk_size=4, overlap=4)


# ---------------------------------------------------------------------------------------------
# the stream and no-sync contract (recorded for test_gpu_stream_contract's coverage test)
# ---------------------------------------------------------------------------------------------
def test_stitch_entries_are_gated():
    n = 1500
    rng = np.random.default_rng(900)
    cloud = lambda seed: (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) - 0.5)
    src, tgt = (cloud(1), cloud(1).flip(0) + 0.03), (cloud(2), cloud(2).flip(0) + 0.03)
    Ta, Tb = torch.from_numpy(_sim3(rng)[0]), torch.from_numpy(_sim3(rng)[0])

    def wmoments():
        c = sc.Case("align_wmoments 1500 pairs, weights, cauchy, device delta")
        s, t = c.inp(*src), c.inp(*tgt)
        w = c.inp(torch.rand(n, generator=torch.Generator().manual_seed(3)) + 0.1)
        T, d = c.inp(Ta, Tb), c.inp(torch.tensor([0.4], dtype=torch.float64), torch.tensor([0.9], dtype=torch.float64))
        ws = c.ws(ops.align_wmoments_workspace_bytes(n))
        cnt, sums = c.out((1,), torch.int64), c.out((20,), torch.float64)
        c.call = lambda: ops.align_wmoments(s, t, weight=w, transform=T, delta=d, delta_scale=0.5, cauchy=True, ws=ws, count=cnt, sums=sums)
        return c

    def wsolve():
        c = sc.Case("align_wsolve with scale, every output")
        ma = ops.align_wmoments(src[0].cuda(), tgt[0].cuda())
        mb = ops.align_wmoments(src[1].cuda(), tgt[1].cuda())
        torch.cuda.synchronize()
        cnt, sums = c.inp(ma[0].cpu(), mb[0].cpu()), c.inp(ma[1].cpu(), mb[1].cpu())
        outs = [c.out((4, 4), torch.float64)] + [c.out((1,), dt) for dt in (torch.float64,) * 4 + (torch.int64, torch.int32)]
        c.call = lambda: ops.align_wsolve(cnt, sums, outs[0], None, True, False, *outs[1:])
        return c

    def move_maps():
        c = sc.Case("align_move_maps 1500 pixels, four maps")
        p, d, pc, dc = c.inp(*src), c.inp(torch.rand(n) + 1), c.inp(torch.rand(n) + 2), c.inp(torch.rand(n) + 3)
        T, s = c.inp(Ta, Tb), c.inp(torch.tensor([1.3], dtype=torch.float64), torch.tensor([0.7], dtype=torch.float64))
        outs = [c.out((n, 3), torch.float32)] + [c.out((n,), torch.float32) for _ in range(3)]
        c.call = lambda: ops.align_move_maps(n, T, s, p, d, pc, dc, *outs)
        return c

    def move_cameras():
        c = sc.Case("align_move_cameras 5 views")
        E = c.inp(torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(4)))
        T, s = c.inp(Ta, Tb), c.inp(torch.tensor([1.3], dtype=torch.float64), torch.tensor([0.7], dtype=torch.float64))
        out = c.out((5, 3, 4), torch.float32)
        c.call = lambda: ops.align_move_cameras(E, T, s, out=out)
        return c

    cases = tsc.family([wmoments, wsolve, move_maps, move_cameras], "stitching")
    entries = {"ovg_align_wmoments", "ovg_align_wsolve", "ovg_align_move_maps", "ovg_align_move_cameras"}
    assert {e for c in cases for e in c.entries} == entries and all(e in tsc.COVERED for e in entries)
    want = twin.wmoments(src[0].numpy(), tgt[0].numpy(), weight=cases[0].real[2].cpu().numpy(), transform=Ta.numpy(), delta=np.array([0.4]), delta_scale=0.5, cauchy=True)
    assert cases[0].outs[0].cpu().numpy().tolist() == want[0].tolist() and cases[0].outs[1].cpu().numpy().tobytes() == want[1].tobytes()
