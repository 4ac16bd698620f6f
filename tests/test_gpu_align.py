"""ovg_align_moments / ovg_align_solve / ovg_align_apply and postprocess.fit_similarity, icp, aligned_cloud_distance and trajectory_ate
on the device against tests/align_twin.py: the moments and the apply byte for byte in exact-size guarded buffers (sizes around the
thread block, the tile and the second stage's stride; index, centre, masks, non-finite coordinates, the inclusive gate, no used pair),
the solve against the twin's independent Umeyama / SVD solution (exact, general, mirrored, degenerate, collinear, composed), and the
public entries on a known Sim(3), the ICP fixture, aligned scores and a camera trajectory."""
import numpy as np
import pytest
import torch

import align_twin as twin
from kernel_guards import guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
TILE, THREADS = L.ALIGN_TILE, L.ALIGN_THREADS


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _moments(p, q, index=None, source_valid=None, target_valid=None, sqdist=None, max_sqdist=None, centre=None):
    """ovg_align_moments into exact-size guarded outputs and an exact-size guarded workspace. -> (count int64 [1], sums f64 [18]) numpy"""
    count, check_c = guarded((1, 1), torch.int64, "cuda", guard_bytes=4096)
    sums, check_s = guarded((1, L.ALIGN_SUMS), torch.float64, "cuda", guard_bytes=4096)
    ws, check_w = guarded((1, ops.align_workspace_bytes(len(p))), torch.uint8, "cuda", guard_bytes=4096)
    out = ops.align_moments(_dev(p), _dev(q), _dev(index), _dev(source_valid), _dev(target_valid), _dev(sqdist), max_sqdist, _dev(centre),
                            ws=ws[0], count=count[0], sums=sums[0])
    torch.cuda.synchronize()
    check_c("count"), check_s("sums"), check_w("workspace")
    assert out[0] is not None and out[0].data_ptr() == count.data_ptr() and out[1].data_ptr() == sums.data_ptr()
    return count[0].cpu().numpy(), sums[0].cpu().numpy()


def _same_moments(got, want, name):
    assert got[0].dtype == want[0].dtype == np.int64 and got[0].tolist() == want[0].tolist(), (name, got[0], want[0])
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes(), (name, np.nonzero(got[1] != want[1])[0].tolist(), got[1], want[1])


def _solve(count, sums, centre=None, with_scale=True, transform=None):
    """ovg_align_solve into guarded outputs; transform: None writes the step, an array composes onto it.
    -> (T [4, 4], scale, rms, count, status)"""
    T, check_t = guarded((4, 4), torch.float64, "cuda", guard_bytes=4096)
    outs = [guarded((1, 1), dt, "cuda", guard_bytes=4096) for dt in (torch.float64, torch.float64, torch.int64, torch.int32)]
    if transform is not None:
        T.copy_(_dev(np.asarray(transform, np.float64)))
    ops.align_solve(_dev(np.asarray(count, np.int64).reshape(1)), _dev(np.asarray(sums, np.float64)), T, _dev(centre), with_scale,
                    transform is not None, *(o[0][0] for o in outs))
    torch.cuda.synchronize()
    check_t("transform")
    for (_, check), name in zip(outs, ("scale", "rms", "count", "status")):
        check(name)
    return (T.cpu().numpy(),) + tuple(o[0][0].cpu().numpy()[0] for o in outs)


def _fit(p, q, with_scale=True, **kw):
    """fit_similarity's two passes at the entries. -> (T, scale, rms, count, status, gap)"""
    n0, s0 = _moments(p, q, **kw)
    centre = s0[:6] / max(int(n0[0]), 1)
    n1, s1 = _moments(p, q, centre=centre, **kw)
    return _solve(n1, s1, centre, with_scale) + (twin.gap(n1, s1) if n1[0] >= 3 else 0.0,)


def _clouds(n, m, seed):
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(n, 3)) * [3, 2, 1] + [10, -4, 7]).astype(F)
    q = (rng.normal(size=(m, 3)) * [1, 2, 3] + [-5, 4, 20]).astype(F)
    return rng, p, q


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049, THREADS * TILE + 1])
def test_moments_match_twin_bit_exactly(n):
    """n around the 256 threads of a workgroup and the 1024 pairs of a tile; 2049 is three tiles; 256 * 1024 + 1 is 257 tiles, so that
    thread 0 of the second stage folds two partials (its strided loop runs twice)."""
    L.require_gpu()
    assert (TILE, THREADS) == (1024, 256)
    big = n > 4096
    rng, p, q = _clouds(n, n + 5, n)
    centre = np.concatenate([p.astype(np.float64).mean(0), q.astype(np.float64).mean(0)]) + 0.1
    got = _moments(p, q[:n])
    _same_moments(got, twin.moments(p, q[:n]), "plain")
    _same_moments(_moments(p, q[:n]), got, "second call")
    assert int(got[0][0]) == n
    index = rng.integers(0, n + 5, n).astype(np.int32)
    _same_moments(_moments(p, q, index, centre=centre), twin.moments(p, q, index, centre=centre), "index, centre")
    if big:
        return
    _same_moments(_moments(p, q[:n], centre=centre), twin.moments(p, q[:n], centre=centre), "centre")
    _same_moments(_moments(p, q, index), twin.moments(p, q, index), "index")
    # out-of-range index entries, non-finite coordinates on either side, masks with holes
    bad_p, bad_q, idx = p.copy(), q.copy(), index.copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        bad_p[rng.integers(0, n, max(1, n // 50)), k] = v
        bad_q[rng.integers(0, n + 5, max(1, n // 50)), 2 - k] = v
    idx[rng.integers(0, n, max(1, n // 20))] = -1
    idx[rng.integers(0, n, max(1, n // 20))] = n + 5
    idx[rng.integers(0, n, max(1, n // 40))] = np.iinfo(np.int32).max
    idx[rng.integers(0, n, max(1, n // 40))] = np.iinfo(np.int32).min
    sv, tv = (rng.random(n) >= 0.1).astype(np.uint8) * 7, (rng.random(n + 5) >= 0.1).astype(np.uint8)
    for name, kw in (("bad entries", dict(index=idx)), ("masks", dict(index=idx, source_valid=sv, target_valid=tv)),
                     ("masks, centre", dict(index=idx, source_valid=sv, target_valid=tv, centre=centre))):
        want = twin.moments(bad_p, bad_q, **kw)
        _same_moments(_moments(bad_p, bad_q, **kw), want, name)
        assert n < 255 or 0 < int(want[0][0]) < n
    _same_moments(_moments(bad_p, bad_q[:n], source_valid=sv, target_valid=tv[:n]), twin.moments(bad_p, bad_q[:n], source_valid=sv, target_valid=tv[:n]),
                  "masks without an index")
    # the gate at an exactly representable squared distance is inclusive; a NaN distance is not used
    sq = rng.choice(np.array([0.25, 0.5, 0.75, np.nan, np.inf], F), n)
    want = twin.moments(p, q, index, sqdist=sq, max_sqdist=0.5)
    _same_moments(_moments(p, q, index, sqdist=sq, max_sqdist=0.5), want, "gate")
    assert int(want[0][0]) == int((sq <= F(0.5)).sum())
    _same_moments(_moments(p, q, index, sqdist=sq, max_sqdist=float("inf")), twin.moments(p, q, index, sqdist=sq, max_sqdist=np.inf), "gate at +inf")
    # no used pair: count 0 and every sum +0.0
    for kw in (dict(index=np.full(n, -1, np.int32)), dict(index=index, sqdist=sq, max_sqdist=0.125), dict(index=index, source_valid=np.zeros(n, np.uint8))):
        got = _moments(p, q, centre=centre, **kw)
        assert got[0].tolist() == [0] and got[1].tobytes() == np.zeros(18).tobytes(), kw.keys()


@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_apply_matches_twin_bit_exactly(n):
    L.require_gpu()
    rng, p, _ = _clouds(n, 1, n)
    T = np.eye(4)
    T[:3, :3] = 1.7 * np.linalg.qr(rng.normal(size=(3, 3)))[0] + rng.normal(size=(3, 3)) * 0.01           # general: scale, a little shear
    T[:3, 3] = [1.5, -20.25, 300.125]
    if n > 4:
        p[1, 0], p[2, 1], p[3, 2], p[4] = np.inf, np.nan, 3e38, (1e-30, -0.0, 0.0)
    for M, name in ((T, "general"), (np.eye(4), "identity")):
        out, check = guarded((n, 3), torch.float32, "cuda", guard_bytes=4096)
        assert ops.align_apply(_dev(p), _dev(M), out=out) is out
        torch.cuda.synchronize()
        check(name)
        with np.errstate(all="ignore"):
            assert out.cpu().numpy().tobytes() == twin.apply(M, p).tobytes(), name
    # the identity returns the input bytes (of finite points: 0 x inf is NaN; and -0.0 + 0.0 is +0.0)
    ok = np.isfinite(p).all(1) & ~((p == 0) & np.signbit(p)).any(1)
    same = ops.align_apply(_dev(p), _dev(np.eye(4))).cpu().numpy()
    assert same[ok].tobytes() == p[ok].tobytes() and ok.sum() >= n - 4 and (n < 5 or ok[3])
    inplace = _dev(p)
    assert ops.align_apply(inplace, _dev(T), out=inplace) is inplace and inplace.cpu().numpy().tobytes() == twin.apply(T, p).tobytes()


def test_solve_exact_case_is_recovered():
    """Small-integer source points; the target is a quarter turn about z, times 2, plus an integer translation: every moment is an
    integer below 2^53, so the sums are exact and the transform follows from them to the solve's own rounding."""
    L.require_gpu()
    rng = np.random.default_rng(0)
    p = rng.integers(-8, 9, (300, 3)).astype(F)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 2.0 * np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), [5, -7, 11]
    q = (p.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F)
    count, sums = _moments(p, q)
    assert sums.tobytes() == twin.moments(p, q)[1].tobytes() and (sums == np.round(sums)).all()
    T, scale, rms, n, status = _solve(count, sums)
    err = np.abs(T - M).max()
    print("exact case: |T - truth| %.3g, scale - 2 %.3g" % (err, scale - 2))
    assert status == 0 and n == 300 and err <= 1e-12 and abs(scale - 2) <= 1e-12
    assert abs(rms - np.sqrt(((q.astype(np.float64) - p) ** 2).sum(1).mean())) <= 1e-12 * rms
    moved = ops.align_apply(_dev(p), _dev(T)).cpu().numpy()
    assert moved.tobytes() == q.tobytes()
    after = _solve(*_moments(moved, q), with_scale=False)
    assert after[2] == 0.0 and after[4] == 0 and np.abs(after[0] - np.eye(4)).max() <= 1e-12           # rms after applying is 0


def _compare_with_svd(p, q, with_scale, name):
    T, scale, rms, n, status, g = _fit(p, q, with_scale)
    ref, ref_scale = twin.solve_svd(p, q, with_scale)
    assert g >= 1e-3, (name, g)
    extent = np.abs(q.astype(np.float64)).max()
    dR, ds, dt = np.abs(T[:3, :3] / scale - ref[:3, :3] / ref_scale).max(), abs(scale - ref_scale), np.abs(T[:3, 3] - ref[:3, 3]).max() / extent
    print("%s scale %d: gap %.3g dR %.3g ds %.3g dt/extent %.3g" % (name, with_scale, g, dR, ds, dt))
    assert status == 0 and n == len(p) and max(dR, ds, dt) <= 1e-12, (name, dR, ds, dt)
    assert (T[3] == [0, 0, 0, 1]).all() and (with_scale or scale == 1.0)
    return T, scale, ref


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solve_general_case_matches_the_svd_solution(seed):
    """Anisotropic Gaussian clouds of 500 points, 10 away from the origin, the target with 1 % noise: rigid and similarity."""
    L.require_gpu()
    rng = np.random.default_rng(seed)
    p = (rng.normal(size=(500, 3)) * [3, 2, 1] + 10 * np.array([1, -1, 1]) / np.sqrt(3)).astype(F)
    R0 = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R0 *= np.linalg.det(R0)
    q = (1.4 * p.astype(np.float64) @ R0.T + [1, 2, 3] + rng.normal(size=p.shape) * 0.03).astype(F)
    for with_scale in (True, False):
        _compare_with_svd(p, q, with_scale, "seed %d" % seed)


def test_mirrored_target_gives_a_proper_rotation_with_umeyamas_residual():
    L.require_gpu()
    rng = np.random.default_rng(5)
    p = (rng.normal(size=(500, 3)) * [3, 2, 1] + [10, -4, 7]).astype(F)
    q = (1.7 * (p.astype(np.float64) * [1, 1, -1]) + [1, 2, 3] + rng.normal(size=p.shape) * 0.03).astype(F)
    for with_scale in (True, False):
        T, scale, ref = _compare_with_svd(p, q, with_scale, "mirrored")
        assert abs(np.linalg.det(T[:3, :3] / scale) - 1.0) <= 1e-12
        r, want = twin.residual(T, p, q), twin.residual(ref, p, q)
        assert want > 0.1 and abs(r - want) <= 1e-12 * want


def test_degenerate_inputs_give_identity_steps():
    L.require_gpu()
    P = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 10], [0, 1, 0], [2, 2, 2]], F)
    running = np.eye(4)
    running[:3] = np.arange(12).reshape(3, 4) + 0.5
    cases = [("two pairs", _moments(P[:2], P[:2] + 1), L.ALIGN_FEW_PAIRS), ("coincident", _moments(np.tile(P[:1], (5, 1)), P), L.ALIGN_NO_SPREAD)]
    count, sums = _moments(P, P + 1)
    for k, v in ((0, np.inf), (7, np.nan), (15, np.inf), (17, -np.inf)):
        bad = sums.copy()
        bad[k] = v
        cases.append(("sums[%d] = %r" % (k, v), (count, bad), L.ALIGN_NOT_FINITE))
    for name, (count_, sums_), want in cases:
        for with_scale in (True, False):
            T, scale, rms, n, status = _solve(count_, sums_, None, with_scale)
            assert status == want and T.tobytes() == np.eye(4).tobytes() and scale == 1.0 and np.isfinite(rms) and n == count_[0], name
            T = _solve(count_, sums_, None, with_scale, transform=running)[0]
            assert T.tobytes() == running.tobytes(), name                    # composed: the running transform keeps its bytes
    assert _solve(count, sums, centre=np.array([0, 0, np.nan, 0, 0, 0.0]))[4] == L.ALIGN_NOT_FINITE
    assert _solve(np.array([0]), np.zeros(18))[1:] == (1.0, 0.0, 0, L.ALIGN_FEW_PAIRS)
    # A float32 coordinate cannot push a float64 moment out of range (3e38 squared is 9e76): such a pair is summed like any other and
    # the fit stays regular and finite. A non-finite moment can only arrive from outside, as above.
    far = P.copy()
    far[0, 0] = 3e38
    count, sums = _moments(far, P)
    assert np.isfinite(sums).all() and sums.tobytes() == twin.moments(far, P)[1].tobytes()
    for with_scale in (True, False):
        T, scale, rms, n, status = _solve(count, sums, None, with_scale)
        assert np.isfinite(T).all() and np.isfinite(scale) and np.isfinite(rms) and status in (0, L.ALIGN_NOT_FINITE, L.ALIGN_NO_SPREAD)
    sim = postprocess.fit_similarity(_dev(far), _dev(P))
    assert bool(torch.isfinite(sim.matrix).all()) and bool(torch.isfinite(sim.rms))


def test_collinear_points_give_a_finite_proper_rotation():
    """All source points on one line: the rotation about the line is free (the two largest eigenvalues coincide), the residual is not."""
    L.require_gpu()
    rng = np.random.default_rng(3)
    p = (np.arange(-20, 21)[:, None] * np.array([[1.0, 2.0, 3.0]]) * 0.25 + [4, 5, 6]).astype(F)
    R0 = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R0 *= np.linalg.det(R0)
    q = (p.astype(np.float64) @ R0.T + [1, -2, 3] + rng.normal(size=p.shape) * 0.01).astype(F)
    for with_scale in (True, False):
        T, scale, rms, n, status, g = _fit(p, q, with_scale)
        ref = twin.fit(p, q, with_scale)[0]
        r, want = twin.residual(T, p, q), twin.residual(ref, p, q)
        print("collinear scale %d: gap %.3g residual %.6g twin %.6g" % (with_scale, g, r, want))
        assert status == 0 and np.isfinite(T).all() and abs(np.linalg.det(T[:3, :3] / scale) - 1.0) <= 1e-12
        assert want > 1e-3 and abs(r - want) <= 1e-9 * want


def test_composition_onto_a_running_transform():
    L.require_gpu()
    rng, p, q = _clouds(300, 300, 11)
    count, sums = _moments(p, q)
    step = _solve(count, sums)[0]
    running = np.eye(4)
    running[:3, :3] = 0.8 * np.linalg.qr(rng.normal(size=(3, 3)))[0]
    running[:3, 3] = [3, -1, 2]
    T = _solve(count, sums, transform=running)[0]
    want = step @ running
    assert np.abs(T - want).max() <= 1e-14 * np.abs(want).max() and (T[3] == [0, 0, 0, 1]).all()


def _known_sim3():
    source = twin.icp_fixture()[1][:2000]
    ang, ax = 0.9, np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = 2.5 * (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K)
    M[:3, 3] = [4.0, -3.0, 1.5]
    return source, (source.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F), M


def test_fit_similarity_recovers_a_known_sim3():
    """2000 points of the surface fixture moved by a known Sim(3) in float64 and rounded to float32: 2^-24 per coordinate, averaged over
    2000 points; 1e-6 relative to scale and extent is about ten times that floor."""
    L.require_gpu()
    source, target, M = _known_sim3()
    sim = postprocess.fit_similarity(_dev(source), _dev(target))
    T = sim.matrix.cpu().numpy()
    extent = np.abs(target.astype(np.float64)).max()
    err_r, err_t = np.abs(T[:3, :3] - M[:3, :3]).max() / 2.5, np.abs(T[:3, 3] - M[:3, 3]).max() / extent
    print("fit_similarity: |sR - truth| / s %.3g, |t - truth| / extent %.3g, scale - 2.5 %.3g, rms %.6g" % (err_r, err_t, float(sim.scale) - 2.5, float(sim.rms)))
    assert sim.matrix.dtype == torch.float64 and sim.matrix.is_cuda and int(sim.count) == 2000 and int(sim.status) == 0
    assert max(err_r, err_t) <= 1e-6 and abs(float(sim.scale) - 2.5) <= 2.5e-6
    assert abs(float(sim.rms) - np.sqrt(((target.astype(np.float64) - source) ** 2).sum(1).mean())) <= 1e-12 * float(sim.rms)
    want = twin.fit(source, target)[0]
    assert np.abs(T - want).max() <= 1e-12 * extent
    moved = sim.apply(_dev(source))
    assert moved.dtype == torch.float32 and moved.cpu().numpy().tobytes() == twin.apply(T, source).tobytes()
    # masks: the masked pairs do not enter; a rigid fit of a scaled target keeps scale 1
    sv = np.arange(2000) % 3 != 0
    bad = target.copy()
    bad[~sv] = 77.0
    masked = postprocess.fit_similarity(_dev(source.reshape(40, 50, 3)), _dev(bad.reshape(40, 50, 3)), source_valid=_dev(sv.reshape(40, 50)))
    assert int(masked.count) == int(sv.sum()) and np.abs(masked.matrix.cpu().numpy() - M).max() <= 1e-5
    rigid = postprocess.fit_similarity(_dev(source), _dev(target), with_scale=False)
    assert float(rigid.scale) == 1.0 and abs(np.linalg.det(rigid.matrix.cpu().numpy()[:3, :3]) - 1.0) <= 1e-12
    cloud = postprocess.PointCloud(_dev(source), torch.zeros(2000, 3, dtype=torch.uint8, device="cuda"), None, torch.tensor(2.0, device="cuda"),
                                   np.eye(4), None, torch.arange(2000, device="cuda"), None)
    out = sim.apply(cloud)
    assert isinstance(out, postprocess.PointCloud) and out.points.cpu().numpy().tobytes() == moved.cpu().numpy().tobytes()
    assert out.colors is cloud.colors and out.indices is cloud.indices and out.scene_scale is cloud.scene_scale and out.transform is cloud.transform


def test_icp_on_the_fixture():
    """The surface fixture (tests/align_twin.py icp_fixture; tests/test_align_host.py runs the same loop in numpy): 3 degrees and a small
    shift, rigid, exhaustive search, no gate, 20 iterations. The float32 floor of the moved points is sqrt(3) 2^-24 3.6 = 3.7e-7."""
    L.require_gpu()
    source, target, T0 = twin.icp_fixture()
    res = postprocess.icp(_dev(source), _dev(target), iterations=20)
    rms, count, T = res.rms.cpu().numpy(), res.count.cpu().numpy(), res.transform.matrix.cpu().numpy()
    print("icp rms", " ".join("%.2e" % r for r in rms), "|T T0 - I| %.3g" % np.abs(T @ T0 - np.eye(4)).max())
    assert res.rms.dtype == torch.float64 and res.count.dtype == torch.int64 and rms.shape == count.shape == (20,)
    assert all(rms[i + 1] <= rms[i] * (1 + 1e-6) + 1e-7 for i in range(19))
    assert rms[0] > 1e-2 and rms[19] <= 1e-6
    assert np.abs(T @ T0 - np.eye(4)).max() <= 1e-6
    assert (count == 2025).all() and (res.status.cpu().numpy() == 0).all() and int(res.transform.status) == 0
    assert abs(float(res.transform.scale) - 1.0) <= 1e-12 and float(res.transform.rms) == rms[19] and int(res.transform.count) == 2025
    want_T, want_rms, _, _ = twin.icp(source, target, 20)
    assert np.abs(rms[:8] - want_rms[:8]).max() <= 1e-9 and np.abs(T - want_T).max() <= 1e-6
    # every correspondence is far inside a gate of 0.5: the grid search finds the same pairs
    grid = postprocess.icp(_dev(source), _dev(target), iterations=20, search="grid", max_distance=0.5)
    assert np.abs(grid.transform.matrix.cpu().numpy() - T).max() <= 1e-9 and (grid.count.cpu().numpy() == 2025).all()
    gated = postprocess.icp(_dev(source), _dev(target), iterations=20, max_distance=0.5)
    assert gated.transform.matrix.cpu().numpy().tobytes() == T.tobytes()
    # a gate of 1e-4 leaves fewer than three pairs: identity steps, the flag set, the transform is init
    init = np.eye(4)
    init[:3, 3] = [0.25, 0.0, 0.0]
    for search in ("exhaustive", "grid"):
        none = postprocess.icp(_dev(source), _dev(target), init=_dev(init), iterations=3, max_distance=1e-4, search=search)
        assert (none.count.cpu().numpy() < 3).all() and (none.status.cpu().numpy() == L.ALIGN_FEW_PAIRS).all(), search
        assert none.transform.matrix.cpu().numpy().tobytes() == init.tobytes() and int(none.transform.status) == L.ALIGN_FEW_PAIRS
    sim = postprocess.Similarity(_dev(init), None, None, None, None)
    again = postprocess.icp(_dev(source), _dev(target), init=sim, iterations=1, max_distance=1e-4)
    assert again.transform.matrix.cpu().numpy().tobytes() == init.tobytes() and again.transform.matrix.data_ptr() != sim.matrix.data_ptr()


def test_aligned_cloud_distance():
    L.require_gpu()
    source, target, M = _known_sim3()
    plain = postprocess.cloud_distance(_dev(source), _dev(target))
    dist, sim = postprocess.aligned_cloud_distance(_dev(source), _dev(target))
    print("aligned accuracy %.3g completeness %.3g; unaligned %.3g %.3g" % (dist.accuracy, dist.completeness, plain.accuracy, plain.completeness))
    assert plain.accuracy > 1e-2 and plain.completeness > 1e-2
    assert dist.accuracy <= 1e-5 and dist.completeness <= 1e-5 and dist.n_pred == dist.n_gt == 2000
    assert np.abs(sim.matrix.cpu().numpy() - M).max() <= 1e-5
    valid = np.arange(2000) % 4 != 1
    bad = source.copy()
    bad[~valid] = np.nan
    dist, sim = postprocess.aligned_cloud_distance(_dev(bad.reshape(20, 100, 3)), _dev(target.reshape(20, 100, 3)), valid=_dev(valid.reshape(20, 100)),
                                                   threshold=1e-3, icp_iterations=2, max_distance=0.1)
    assert dist.accuracy <= 1e-5 and dist.completeness <= 1e-5 and dist.n_pred == dist.n_gt == int(valid.sum()) and dist.fscore == 1.0
    assert int(sim.count) == int(valid.sum()) and np.abs(sim.matrix.cpu().numpy() - M).max() <= 1e-5


def test_trajectory_ate():
    """Eight cameras on a circle, each turned by a multiple of a quarter turn about z (so that -R^T t is exact in any order of operations),
    against the same trajectory moved by a known Sim(3)."""
    L.require_gpu()
    k = np.arange(8)
    centres = np.stack([2 * np.cos(k * np.pi / 4), 2 * np.sin(k * np.pi / 4), 0.1 * k], 1).astype(F)
    quarter = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])

    def cameras(c):
        e = np.zeros((8, 3, 4), F)
        for i in range(8):
            R = np.linalg.matrix_power(quarter, i % 4)
            e[i, :, :3], e[i, :, 3] = R, -(R @ c[i].astype(np.float64))
            assert (e[i, :, 3].astype(np.float64) == -(R @ c[i].astype(np.float64))).all()
        return e

    ang = 0.4
    M = np.eye(4)
    M[:3, :3] = 1.5 * np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    M[:3, 3] = [3, 1, -2]
    moved = (centres.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F)
    gt, pred = cameras(moved), cameras(centres)
    ate, sim = postprocess.trajectory_ate(_dev(pred), _dev(gt))
    print("ate %.3g, scale - 1.5 %.3g" % (float(ate), float(sim.scale) - 1.5))
    assert ate.is_cuda and ate.dtype == torch.float64 and float(ate) <= 1e-6 and abs(float(sim.scale) - 1.5) <= 1e-5 and int(sim.count) == 8
    full = np.zeros((8, 4, 4))
    full[:, :3], full[:, 3, 3] = pred, 1
    ate, sim = postprocess.trajectory_ate(_dev(full), _dev(gt), with_scale=False)
    step = twin.fit(centres, moved, with_scale=False)[0]
    want = twin.residual(step, centres, moved)
    print("rigid ate %.9g twin %.9g" % (float(ate), want))
    assert want > 0.1 and abs(float(ate) - want) <= 1e-9 * want and float(sim.scale) == 1.0


def test_public_entries_on_the_device_errors_and_empty_sides():
    L.require_gpu()
    p, q = torch.zeros(5, 3, device="cuda"), torch.zeros(6, 3, device="cuda")
    for fn, kw in ((postprocess.fit_similarity, dict(source=p, target=q)), (postprocess.fit_similarity, dict(source=p.double(), target=p)),
                   (postprocess.fit_similarity, dict(source=p, target=p, source_valid=torch.ones(4, device="cuda", dtype=torch.bool))),
                   (postprocess.icp, dict(source=p, target=q.half())), (postprocess.icp, dict(source=p, target=q, search="grid")),
                   (postprocess.aligned_cloud_distance, dict(pred_points=p, gt_points=q)),
                   (postprocess.trajectory_ate, dict(pred_extrinsic=torch.zeros(3, 3, 4, device="cuda"), gt_extrinsic=torch.zeros(4, 3, 4, device="cuda")))):
        with pytest.raises(ValueError):
            fn(**kw)
    for fn, kw in ((postprocess.fit_similarity, dict(source=p, target=p.cpu())), (postprocess.icp, dict(source=p.cpu(), target=q)),
                   (postprocess.icp, dict(source=p, target=q, init=torch.eye(4, dtype=torch.float64))),
                   (postprocess.aligned_cloud_distance, dict(pred_points=p, gt_points=p.cpu()))):
        with pytest.raises(L.OvgError):
            fn(**kw)
    with pytest.raises(L.OvgError):
        ops.align_moments(p, q)                                              # n != m without an index, at the thin wrapper
    empty = torch.zeros(0, 3, device="cuda")
    sim = postprocess.fit_similarity(empty, empty)
    assert sim.matrix.is_cuda and sim.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes() and int(sim.count) == 0
    assert int(sim.status) == L.ALIGN_FEW_PAIRS and float(sim.scale) == 1.0 and sim.apply(empty).shape == (0, 3)
    for a, b in ((empty, q), (p, empty)):
        res = postprocess.icp(a, b, iterations=2)
        assert res.transform.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes() and res.count.tolist() == [0, 0]
        assert res.status.tolist() == [L.ALIGN_FEW_PAIRS] * 2 and res.rms.tolist() == [0.0, 0.0]
    few = postprocess.fit_similarity(p[:2], q[:2])
    assert int(few.count) == 2 and int(few.status) == L.ALIGN_FEW_PAIRS and few.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes()
    same = postprocess.fit_similarity(p, p + 1)                              # five coincident points
    assert int(same.status) == L.ALIGN_NO_SPREAD and same.matrix.cpu().numpy().tobytes() == np.eye(4).tobytes()
