"""Registration (ovg_align_moments / ovg_align_solve / ovg_align_apply), host side: the C ABI without a device (struct layouts, enums,
argument checks that return before any HIP call), the Python wrappers' argument checks, and the numpy twin (tests/align_twin.py)
checked against what it restates: its ordered sums against exact rational sums, its Horn solve against an independent Umeyama / SVD
solve, and its ICP loop on the fixture the device test uses."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi_layout
import align_twin as twin
import common
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def _layout(struct, cname, extra):
    enums, (eps,) = abi_layout.check({cname: struct}, extra, ["OVG_ALIGN_SPREAD_EPS"])
    assert eps == L.ALIGN_SPREAD_EPS == twin.SPREAD_EPS == 2.0 ** -40
    return enums


def test_ctypes_struct_layouts_and_enums_match_c_align():
    names = ["OVG_ALIGN_THREADS", "OVG_ALIGN_TILE", "OVG_ALIGN_JACOBI_SWEEPS", "OVG_ALIGN_SUMS", "OVG_ALIGN_PARTIAL_BYTES", "OVG_ALIGN_GATE",
             "OVG_ABI_VERSION"]
    want = [L.ALIGN_THREADS, L.ALIGN_TILE, L.ALIGN_JACOBI_SWEEPS, L.ALIGN_SUMS, L.ALIGN_PARTIAL_BYTES, L.ALIGN_GATE, L.ABI_VERSION]
    assert _layout(L.AlignMomentsParams, "ovg_align_moments_params", names) == want
    flags = ["OVG_ALIGN_SCALE", "OVG_ALIGN_COMPOSE", "OVG_ALIGN_FEW_PAIRS", "OVG_ALIGN_NO_SPREAD", "OVG_ALIGN_NOT_FINITE"]
    assert _layout(L.AlignSolveParams, "ovg_align_solve_params", flags) == [L.ALIGN_SCALE, L.ALIGN_COMPOSE, L.ALIGN_FEW_PAIRS,
                                                                              L.ALIGN_NO_SPREAD, L.ALIGN_NOT_FINITE]
    assert _layout(L.AlignApplyParams, "ovg_align_apply_params", ["OVG_ABI_VERSION"]) == [13]
    assert L.ABI_VERSION == 13 and (L.ALIGN_THREADS, L.ALIGN_TILE, L.ALIGN_SUMS) == (twin.THREADS, twin.TILE, twin.SUMS) == (256, 1024, 18)
    assert (L.ALIGN_FEW_PAIRS, L.ALIGN_NO_SPREAD, L.ALIGN_NOT_FINITE) == (twin.FEW_PAIRS, twin.NO_SPREAD, twin.NOT_FINITE)
    assert (postprocess.ALIGN_FEW_PAIRS, postprocess.ALIGN_NO_SPREAD, postprocess.ALIGN_NOT_FINITE) == (1, 2, 4)
    assert L.ALIGN_TILE % L.ALIGN_THREADS == 0 and L.ALIGN_THREADS == 4 * 64 and L.ALIGN_PARTIAL_BYTES >= 8 * (1 + L.ALIGN_SUMS)
    text = open(HEADER).read()
    for entry, params in (("ovg_align_moments", "ovg_align_moments_params"), ("ovg_align_solve", "ovg_align_solve_params"),
                          ("ovg_align_apply", "ovg_align_apply_params")):
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (entry, params), text)
        assert entry in L.SYMBOLS
    assert re.search(r"int64_t\s+ovg_align_workspace_bytes\s*\(\s*int64_t\s+n\s*\)\s*;", text) and "ovg_align_workspace_bytes" in L.SYMBOLS
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert L.load().ovg_abi_version() == 13


def test_argument_validation_of_the_three_entries_without_gpu():
    lib = L.load()
    ws_bytes = lib.ovg_align_workspace_bytes
    assert [ws_bytes(n) for n in (1, 1024, 1025, 256 * 1024 + 1, (1 << 31) - 1)] == [256, 256, 512, 41216, (1 << 21) * 160]
    assert [ws_bytes(n) for n in (0, -1, 1 << 31, -(1 << 63), (1 << 63) - 1)] == [-1] * 5
    assert ops.align_workspace_bytes(2049) == 512
    for bad in (0, -5, 1 << 31, 1 << 70):
        with pytest.raises(L.OvgError):
            ops.align_workspace_bytes(bad)
    big = 1 << 40                                                            # fake, never dereferenced: every call below fails its checks
    need = ws_bytes(5000)

    def moments(**kw):
        p = L.AlignMomentsParams(source=big, target=big, index=big, source_valid=big + 1, target_valid=big + 3, sqdist=big, centre=big,
                                 n=5000, m=700, max_sqdist=0.25, flags=L.ALIGN_GATE, ws=big, ws_bytes=need, out_count=big, out_sums=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_align_moments(ctypes.byref(p), None)

    assert lib.ovg_align_moments(None, None) == -1
    for bad in (dict(source=None), dict(target=None), dict(ws=None), dict(out_count=None), dict(out_sums=None),
                dict(n=0), dict(m=0), dict(n=-1), dict(m=-3), dict(n=1 << 31, ws_bytes=1 << 50), dict(m=1 << 31), dict(n=-(1 << 63)),
                dict(index=None), dict(index=None, m=4999), dict(index=None, m=5001),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(sqdist=None), dict(max_sqdist=float("nan")),
                dict(source=big + 2), dict(target=big + 1), dict(index=big + 2), dict(sqdist=big + 3), dict(centre=big + 4),
                dict(out_count=big + 4), dict(out_sums=big + 4), dict(ws=big + 8), dict(ws=big + 4),
                dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-256)):
        assert moments(**bad) == -1, bad

    def solve(**kw):
        p = L.AlignSolveParams(count=big, sums=big, centre=big, flags=L.ALIGN_SCALE | L.ALIGN_COMPOSE, transform=big, out_scale=big, out_rms=big,
                               out_count=big, out_status=big + 4)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_align_solve(ctypes.byref(p), None)

    assert lib.ovg_align_solve(None, None) == -1
    for bad in (dict(count=None), dict(sums=None), dict(transform=None), dict(flags=4), dict(flags=7), dict(flags=-1), dict(flags=1 << 40),
                dict(count=big + 4), dict(sums=big + 4), dict(centre=big + 4), dict(transform=big + 4), dict(out_scale=big + 4),
                dict(out_rms=big + 2), dict(out_count=big + 4), dict(out_status=big + 2)):
        assert solve(**bad) == -1, bad

    def apply(**kw):
        p = L.AlignApplyParams(points=big, transform=big, n=5000, out=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_align_apply(ctypes.byref(p), None)

    assert lib.ovg_align_apply(None, None) == -1
    for bad in (dict(points=None), dict(transform=None), dict(out=None), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(n=-(1 << 63)),
                dict(points=big + 2), dict(transform=big + 4), dict(out=big + 1)):
        assert apply(**bad) == -1, bad


def test_ops_wrappers_check_their_arguments_before_any_device_call():
    p, q = torch.zeros(5, 3), torch.zeros(7, 3)
    idx = torch.zeros(5, dtype=torch.int32)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    for kw in (dict(source=torch.zeros(5, 4)), dict(source=p.double()), dict(source=torch.zeros(0, 3)), dict(source=torch.zeros(2, 5, 3)),
               dict(source=torch.zeros(5, 6)[:, ::2]), dict(target=torch.zeros(0, 3)), dict(target=[[0.0, 0.0, 0.0]]),
               dict(index=None), dict(index=idx.long()), dict(index=idx[:4]), dict(source_valid=torch.ones(5, dtype=torch.bool)),
               dict(source_valid=torch.ones(7, dtype=torch.uint8)), dict(target_valid=torch.ones(5, dtype=torch.uint8)),
               dict(sqdist=torch.zeros(5)), dict(max_sqdist=1.0), dict(sqdist=torch.zeros(5), max_sqdist=float("nan")),
               dict(sqdist=torch.zeros(7), max_sqdist=1.0), dict(sqdist=f64(5), max_sqdist=1.0),
               dict(centre=f64(3)), dict(centre=torch.zeros(6)), dict(count=i64(2)), dict(count=torch.zeros(1, dtype=torch.int32)),
               dict(sums=f64(19)), dict(sums=torch.zeros(18)), dict(ws=torch.zeros(256))):
        with pytest.raises(L.OvgError, match="must be|need"):
            ops.align_moments(**dict(dict(source=p, target=q, index=idx), **kw))
    for kw in (dict(), dict(source_valid=torch.ones(5, dtype=torch.uint8), target_valid=torch.ones(7, dtype=torch.uint8)),
               dict(sqdist=torch.zeros(5), max_sqdist=0.5), dict(centre=f64(6)), dict(target=p, index=None)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            ops.align_moments(**dict(dict(source=p, target=q, index=idx), **kw))
    ok = dict(count=i64(1), sums=f64(18), transform=f64(4, 4))
    for kw in (dict(count=i64(2)), dict(count=torch.zeros(1)), dict(sums=f64(17)), dict(transform=f64(3, 4)), dict(transform=torch.zeros(4, 4)),
               dict(transform=f64(4, 8)[:, ::2]), dict(centre=f64(5)), dict(scale=f64(2)), dict(rms=torch.zeros(1)), dict(out_count=f64(1)),
               dict(status=i64(1))):
        with pytest.raises(L.OvgError, match="must be"):
            ops.align_solve(**dict(ok, **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        ops.align_solve(**ok)
    for kw in (dict(points=torch.zeros(5, 2)), dict(points=p.double()), dict(points=torch.zeros(0, 3)), dict(transform=torch.zeros(4, 4)),
               dict(transform=f64(3, 4)), dict(out=torch.zeros(4, 3)), dict(out=f64(5, 3))):
        with pytest.raises(L.OvgError, match="must be"):
            ops.align_apply(**dict(dict(points=p, transform=f64(4, 4)), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        ops.align_apply(p, f64(4, 4))


def test_public_entries_check_their_arguments_and_refuse_cpu_tensors():
    p, q = torch.zeros(5, 3), torch.zeros(2, 4, 3)
    cloud = postprocess.PointCloud(p, torch.zeros(5, 3, dtype=torch.uint8), None, torch.tensor(2.0), None, None)
    for kw in (dict(target=q), dict(source=p.double()), dict(source=torch.zeros(5, 2)), dict(target=[[0.0] * 3] * 5),
               dict(source_valid=torch.ones(4, dtype=torch.bool)), dict(target_valid=torch.ones(5)), dict(source=torch.zeros(0, 3))):
        with pytest.raises(ValueError):
            postprocess.fit_similarity(**dict(dict(source=p, target=p), **kw))
    for kw in (dict(), dict(with_scale=False), dict(source=cloud), dict(source_valid=torch.ones(5, dtype=torch.bool)),
               dict(source=torch.zeros(0, 3), target=torch.zeros(0, 3))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.fit_similarity(**dict(dict(source=p, target=p), **kw))
    for kw in (dict(iterations=0), dict(iterations=-1), dict(iterations=2.0), dict(iterations=True), dict(search="kdtree"), dict(search=None),
               dict(search="grid"), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(max_distance="1"),
               dict(source=p.double()), dict(target=torch.zeros(5, 4)), dict(init=torch.eye(4)), dict(init=torch.eye(3, dtype=torch.float64)),
               dict(init="identity")):
        with pytest.raises(ValueError):
            postprocess.icp(**dict(dict(source=p, target=q), **kw))
    for kw in (dict(), dict(max_distance=0.5), dict(search="grid", max_distance=0.5), dict(with_scale=True), dict(iterations=1),
               dict(source=cloud), dict(init=torch.eye(4, dtype=torch.float64)), dict(source=torch.zeros(0, 3))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.icp(**dict(dict(source=p, target=q), **kw))
    for kw in (dict(gt_points=q), dict(pred_points=p.double()), dict(valid=torch.ones(4, dtype=torch.bool)), dict(icp_iterations=-1),
               dict(icp_iterations=1.0), dict(icp_iterations=True)):
        with pytest.raises(ValueError):
            postprocess.aligned_cloud_distance(**dict(dict(pred_points=p, gt_points=p), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.aligned_cloud_distance(p, p, valid=torch.ones(5, dtype=torch.bool), threshold=0.1)
    e = torch.eye(4)[None].repeat(3, 1, 1)
    for kw in (dict(gt_extrinsic=e[:2]), dict(pred_extrinsic=e[0]), dict(pred_extrinsic=e[:, :2]), dict(pred_extrinsic=e.half()),
               dict(pred_extrinsic=e.numpy())):
        with pytest.raises(ValueError):
            postprocess.trajectory_ate(**dict(dict(pred_extrinsic=e, gt_extrinsic=e[:, :3]), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.trajectory_ate(e, e[:, :3].double())
    sim = postprocess.Similarity.identity("cpu", postprocess.ALIGN_FEW_PAIRS)
    assert sim.matrix.dtype == torch.float64 and sim.matrix.tolist() == np.eye(4).tolist() and int(sim.count) == 0 and float(sim.scale) == 1.0
    assert int(sim.status) == postprocess.ALIGN_FEW_PAIRS and float(sim.rms) == 0.0
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        sim.apply(p)
    with pytest.raises(ValueError):
        sim.apply(p.double())


def _exact(p, q, use, j, centre):
    """The 18 sums as exact rationals from the float64 values a, b, d the rule forms (their subtraction's own rounding included), and
    the sum of the terms' magnitudes."""
    P, Q = p.astype(np.float64), q[j].astype(np.float64)
    c = np.zeros(6) if centre is None else centre
    a, b, d = P - c[:3], Q - c[3:], Q - P
    fr = lambda x: [[Fraction(float(v)) for v in row] for row in x]
    total, mag = [Fraction(0)] * 18, [Fraction(0)] * 18
    for i in np.nonzero(use)[0]:
        ai, bi, di = fr([a[i]])[0], fr([b[i]])[0], fr([d[i]])[0]
        t = ai + bi + [ai[r] * bi[k] for r in range(3) for k in range(3)] + [sum(v * v for v in ai), sum(v * v for v in bi), sum(v * v for v in di)]
        m = [abs(v) for v in ai + bi] + [abs(ai[r] * bi[k]) for r in range(3) for k in range(3)] + t[15:]
        total = [x + y for x, y in zip(total, t)]
        mag = [x + y for x, y in zip(mag, m)]
    return total, mag


@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_twin_moments_against_exact_sums(n):
    """Every term is a product of two float64 values that hold centred float32 coordinates: without a centre it is exact in float64
    (24 + 24 bits), so the ordered sum differs from the exact one only by its additions: at most n of them on any path, each within
    2^-53 of a partial sum that never exceeds the sum of the magnitudes -> n 2^-52 sum|term| with room to spare (|a|^2 of ONE pair is
    two additions: 2 x 2^-53). With a centre the values a, b carry 53 bits: each product rounds once more (2^-53 |term|), which the
    three-term sums triple at most: + 2 x 2^-52 sum|term|. The reference treats the rounded a, b, d as the inputs (the subtraction's own
    rounding is part of the rule and enters both sides)."""
    rng = np.random.default_rng(n)
    p = (rng.normal(size=(n, 3)) * [3, 2, 1] + [10, -4, 7]).astype(F)
    q = (rng.normal(size=(n + 3, 3)) * [1, 2, 3] + [-5, 4, 20]).astype(F)
    index = rng.integers(0, n + 3, n).astype(np.int32)
    if n > 4:
        index[1], index[3] = -1, n + 3
        p[2, 1] = np.nan
    worst = 0.0
    for centre in (None, np.concatenate([p[np.isfinite(p).all(1)].astype(np.float64).mean(0), q.astype(np.float64).mean(0)])):
        count, sums = twin.moments(p, q, index=index, centre=centre)
        use, j = twin.used(p, q, index)
        assert int(count[0]) == int(use.sum()) == (n if n <= 4 else n - 3)
        total, mag = _exact(p, q, use, j, centre)
        for k in range(18):
            bound = (n + (0 if centre is None else 2)) * Fraction(2) ** -52 * mag[k]
            err = abs(Fraction(float(sums[k])) - total[k])
            assert err <= bound, (n, centre is not None, k, float(err), float(bound))
            worst = max(worst, float(err / bound)) if bound else worst
    print("n %d: worst share of the bound %.3g" % (n, worst))
    # the same pairs without an index; the order is part of the result but the value barely moves
    count, sums = twin.moments(p, q[:n])
    assert int(count[0]) == int(np.isfinite(p).all(1).sum()) and np.isfinite(sums).all()
    empty = twin.moments(p, q, index=np.full(n, -1, np.int32))
    assert int(empty[0][0]) == 0 and empty[1].tobytes() == np.zeros(18).tobytes()               # +0.0, every one


def _cases():
    rng = np.random.default_rng(7)
    ang = 0.7
    R0 = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]])
    out = {}
    P = (rng.normal(size=(500, 3)) * [3, 2, 1] + [10, -4, 7]).astype(F)
    out["random"] = (P, (1.7 * P.astype(np.float64) @ R0.T + [1, 2, 3]).astype(F))
    out["noisy"] = (P, (0.6 * P.astype(np.float64) @ R0.T + [1, 2, 3] + rng.normal(size=P.shape) * 0.03).astype(F))
    out["mirrored"] = (P, (1.7 * (P.astype(np.float64) * [1, 1, -1]) @ R0.T + [1, 2, 3] + rng.normal(size=P.shape) * 0.03).astype(F))
    flat = (rng.normal(size=(500, 3)) * [3, 2, 0] + [10, -4, 7]).astype(F)
    out["planar"] = (flat, (1.3 * flat.astype(np.float64) @ R0.T + [0, 5, -3] + rng.normal(size=P.shape) * 0.01).astype(F))
    return out


@pytest.mark.parametrize("name", ["random", "noisy", "mirrored", "planar"])
@pytest.mark.parametrize("with_scale", [True, False])
def test_twin_horn_solve_against_twin_svd_solve(name, with_scale):
    P, Q = _cases()[name]
    n0, s0 = twin.moments(P, Q)
    centre = s0[:6] / int(n0[0])
    n1, s1 = twin.moments(P, Q, centre=centre)
    g = twin.gap(n1, s1)
    assert g >= 1e-3, g                                                       # the condition under which the bound below is claimed
    step, scale, rms, status = twin.solve(n1, s1, centre, with_scale)
    ref, ref_scale = twin.solve_svd(P, Q, with_scale)
    extent = np.abs(Q.astype(np.float64)).max()
    dR = np.abs(step[:3, :3] / scale - ref[:3, :3] / ref_scale).max()
    ds, dt = abs(scale - ref_scale), np.abs(step[:3, 3] - ref[:3, 3]).max() / extent
    print("%s scale %d: gap %.3g dR %.3g ds %.3g dt/extent %.3g" % (name, with_scale, g, dR, ds, dt))
    assert status == 0 and max(dR, ds, dt) <= 1e-12
    assert abs(np.linalg.det(step[:3, :3] / scale) - 1.0) <= 1e-12                                    # proper, also for the mirrored target
    assert abs(rms - np.sqrt(((Q.astype(np.float64) - P.astype(np.float64)) ** 2).sum(1).mean())) <= 1e-12 * rms
    assert abs(twin.residual(step, P, Q) - twin.residual(ref, P, Q)) <= 1e-12 * twin.residual(ref, P, Q) + 1e-14


def test_twin_solve_degenerate_inputs_are_identity_steps():
    P = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 10], [0, 1, 0]], F)
    for p, q, want in ((P[:2], P[:2] + 1, twin.FEW_PAIRS), (np.tile(P[:1], (5, 1)), np.tile(P, (2, 1))[:5], twin.NO_SPREAD)):
        step, scale, rms, status = twin.solve(*twin.moments(p, q))
        assert status == want and (step == np.eye(4)).all() and scale == 1.0 and np.isfinite(rms)
    count, sums = twin.moments(P, P + 1)
    for k, v in ((0, np.inf), (7, np.nan), (17, -np.inf)):
        bad = sums.copy()
        bad[k] = v
        step, scale, rms, status = twin.solve(count, bad)
        assert status == twin.NOT_FINITE and (step == np.eye(4)).all() and np.isfinite(rms)
    assert twin.solve(count, sums, centre=[0, 0, np.nan, 0, 0, 0])[3] == twin.NOT_FINITE
    assert twin.solve(np.array([0]), np.zeros(18))[2:] == (0.0, twin.FEW_PAIRS)
    # a float32 coordinate cannot make a float64 moment overflow: 3e38 squares to 9e76, and the fit stays regular and finite
    far = P.copy()
    far[0, 0] = 3e38
    step, scale, rms, status = twin.solve(*twin.moments(far, P))
    assert status == 0 and np.isfinite(step).all() and np.isfinite(rms)


def test_twin_icp_converges_on_the_fixture():
    """The CPU proof that the device test's bounds are reachable by the rule alone. Measured with this twin: rms 3.1e-2 at the start,
    below 1e-6 from iteration 8 on, then 1.3e-8 .. 2.5e-8; never rising; |T T0 - I| = 2.8e-9."""
    source, target, T0 = twin.icp_fixture()
    assert source.dtype == target.dtype == F and source.shape == target.shape == (2025, 3)
    T, rms, count, status = twin.icp(source, target, 20)
    print("rms", " ".join("%.2e" % r for r in rms), "|T T0 - I| %.3g" % np.abs(T @ T0 - np.eye(4)).max())
    assert all(rms[i + 1] <= rms[i] * (1 + 1e-6) + 1e-7 for i in range(19))
    assert rms[0] > 1e-2 and rms[19] <= 1e-6 and np.abs(T @ T0 - np.eye(4)).max() <= 1e-6
    assert (count == 2025).all() and (status == 0).all()
    # a gate far below the first distances leaves no pair: identity steps, the transform stays what it was
    init = np.eye(4)
    init[:3, 3] = [0.5, 0, 0]
    T, rms, count, status = twin.icp(source, target, 3, max_distance=1e-4, init=init)
    assert (count < 3).all() and (status == twin.FEW_PAIRS).all() and (T == init).all()
