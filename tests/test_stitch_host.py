"""Weighted registration and chunk stitching (ovg_align_wmoments / _wsolve / _move_maps / _move_cameras, postprocess.chunk_plan /
stitch_predictions, OmniVGGT.forward_chunked), host side: the C ABI without a device (struct layouts, enums, the argument checks
that return before any HIP call), the chunk plan checked exhaustively, the index remapping, the Python argument checks, and the numpy
twin (tests/stitch_twin.py) against what it restates: its Horn solve against an independent weighted Umeyama / SVD fit, and its refit
loop on the fixture the device test uses -- where the plain fit must be at least 100 times worse than six refits."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import align_twin
import common
import stitch_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess
from omnivggt_official_amd.model import OmniVGGT

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
ENTRIES = (("ovg_align_wmoments", "ovg_align_wmoments_params", L.AlignWMomentsParams), ("ovg_align_wsolve", "ovg_align_wsolve_params", L.AlignWSolveParams),
           ("ovg_align_move_maps", "ovg_align_move_maps_params", L.AlignMoveMapsParams),
           ("ovg_align_move_cameras", "ovg_align_move_cameras_params", L.AlignMoveCamerasParams))


def test_ctypes_struct_layouts_and_enums_match_c_stitch():
    names = ["OVG_WALIGN_SUMS", "OVG_WALIGN_PARTIAL_BYTES", "OVG_WALIGN_CAUCHY", "OVG_WALIGN_KEEP", "OVG_ALIGN_SCALE", "OVG_ALIGN_TILE",
             "OVG_ALIGN_THREADS", "OVG_ABI_VERSION"]
    got, _ = abi_layout.check({c: s for _, c, s in ENTRIES}, names)
    assert got == [L.WALIGN_SUMS, L.WALIGN_PARTIAL_BYTES, L.WALIGN_CAUCHY, L.WALIGN_KEEP, L.ALIGN_SCALE, L.ALIGN_TILE, L.ALIGN_THREADS, L.ABI_VERSION]
    assert got == [20, 176, 1, 4, 1, 1024, 256, 13]
    assert (twin.SUMS, twin.TILE, twin.THREADS) == (20, 1024, 256) and L.WALIGN_PARTIAL_BYTES >= 8 * (1 + L.WALIGN_SUMS)
    assert L.WALIGN_KEEP & (L.ALIGN_SCALE | L.ALIGN_COMPOSE) == 0


def test_entries_are_bound_and_named_before_the_abi_define():
    text = open(HEADER).read()
    head = text[:text.index("#define OVG_ABI_VERSION")]
    for entry, params, _ in ENTRIES:
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (entry, params), text)
        assert entry in L.SYMBOLS and re.search(r"\b%s\b" % entry, head), entry
    assert re.search(r"int64_t\s+ovg_align_wmoments_workspace_bytes\s*\(\s*int64_t\s+n\s*\)\s*;", text)
    assert "ovg_align_wmoments_workspace_bytes" in L.SYMBOLS and "ovg_align_wmoments_workspace_bytes" in head
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text) and L.load().ovg_abi_version() == 13


def test_argument_validation_of_the_four_entries_without_gpu():
    lib = L.load()
    q = lib.ovg_align_wmoments_workspace_bytes
    assert [q(n) for n in (1, 1024, 1025, 256 * 1024 + 1, (1 << 31) - 1)] == [256, 256, 512, 45312, (1 << 21) * 176]
    assert [q(n) for n in (0, -1, 1 << 31, -(1 << 63))] == [-1] * 4
    assert ops.align_wmoments_workspace_bytes(2049) == 768
    with pytest.raises(L.OvgError):
        ops.align_wmoments_workspace_bytes(0)
    big, need = 1 << 40, q(5000)                                             # fake pointers, never dereferenced: every call fails its checks

    def call(name, cls, base, bads):
        fn = getattr(lib, name)
        assert fn(None, None) == -1
        for bad in bads:
            p = cls(**dict(base, **bad))
            assert fn(ctypes.byref(p), None) == -1, (name, bad)

    base = dict(source=big, target=big, weight=big, source_valid=big + 1, target_valid=big + 3, transform=big, delta=big, centre=big,
                delta_scale=0.5, n=5000, flags=1, ws=big, ws_bytes=need, out_count=big, out_sums=big)
    call("ovg_align_wmoments", L.AlignWMomentsParams, base,
         [dict(source=None), dict(target=None), dict(ws=None), dict(out_count=None), dict(out_sums=None), dict(n=0), dict(n=-1), dict(n=1 << 31, ws_bytes=1 << 50),
          dict(flags=2), dict(flags=-1), dict(delta_scale=float("nan")), dict(source=big + 2), dict(weight=big + 2), dict(transform=big + 4),
          dict(delta=big + 4), dict(centre=big + 4), dict(out_sums=big + 4), dict(ws=big + 8), dict(ws_bytes=need - 1)])
    base = dict(count=big, sums=big, centre=big, flags=5, transform=big, out_scale=big, out_rms=big, out_fit_rms=big, out_weight=big, out_count=big,
                out_status=big + 4)
    call("ovg_align_wsolve", L.AlignWSolveParams, base,
         [dict(count=None), dict(sums=None), dict(transform=None), dict(flags=2), dict(flags=8), dict(count=big + 4), dict(out_fit_rms=big + 4),
          dict(out_weight=big + 4), dict(out_status=big + 2)])
    base = dict(points=big, depth=big, points_conf=big, depth_conf=big, transform=big, scale=big, n=100, out_points=big, out_depth=big,
                out_points_conf=big, out_depth_conf=big)
    none = dict(points=None, depth=None, points_conf=None, depth_conf=None, out_points=None, out_depth=None, out_points_conf=None, out_depth_conf=None)
    call("ovg_align_move_maps", L.AlignMoveMapsParams, base,
         [dict(n=0), dict(n=1 << 31), none, dict(out_points=None), dict(points=None), dict(depth_conf=None), dict(out_points_conf=None), dict(transform=None),
          dict(scale=None), dict(points=big + 2), dict(scale=big + 4), dict(out_depth=big + 1)])
    base = dict(extrinsic=big, transform=big, scale=big, views=3, out=big)
    call("ovg_align_move_cameras", L.AlignMoveCamerasParams, base,
         [dict(extrinsic=None), dict(transform=None), dict(scale=None), dict(out=None), dict(views=0), dict(views=1 << 31), dict(out=big + 2),
          dict(transform=big + 4)])


def test_wrapper_argument_checks_without_gpu():
    p, w = torch.zeros(5, 3), torch.zeros(5)
    for bad in (dict(target=torch.zeros(4, 3)), dict(weight=torch.zeros(4)), dict(weight=w.double()), dict(transform=torch.eye(4)),
                dict(delta=torch.zeros(1)), dict(delta_scale=float("nan")), dict(centre=torch.zeros(6)), dict(sums=torch.zeros(18, dtype=torch.float64))):
        with pytest.raises(L.OvgError):
            ops.align_wmoments(**dict(dict(source=p, target=p), **bad))
    with pytest.raises(L.OvgError):                                          # CPU tensors: no fallback
        ops.align_wmoments(p, p)
    cnt, sums, T = torch.zeros(1, dtype=torch.int64), torch.zeros(20, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
    for bad in (dict(sums=sums[:18].clone()), dict(transform=T[:3].clone()), dict(fit_rms=torch.zeros(1)), dict(status=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(L.OvgError):
            ops.align_wsolve(**dict(dict(count=cnt, sums=sums, transform=T), **bad))
    s = torch.ones(1, dtype=torch.float64)
    for bad in (dict(), dict(points=torch.zeros(4, 3)), dict(points=p, transform=None), dict(depth=w, scale=None), dict(out_depth=w),
                dict(points_conf=w, out_points_conf=torch.zeros(4)), dict(n=0)):
        with pytest.raises(L.OvgError):
            ops.align_move_maps(**dict(dict(n=5, transform=T, scale=s), **bad))
    for bad in (dict(extrinsic=torch.zeros(2, 4, 4)), dict(extrinsic=torch.zeros(0, 3, 4)), dict(scale=torch.ones(1)), dict(out=torch.zeros(3, 3, 4))):
        with pytest.raises(L.OvgError):
            ops.align_move_cameras(**dict(dict(extrinsic=torch.zeros(2, 3, 4), transform=T, scale=s), **bad))
    with pytest.raises(L.OvgError):
        postprocess.fit_similarity_robust(p, p)
    for bad in (dict(weights=w[:4]), dict(weights=w.double()), dict(iterations=-1), dict(iterations=1.5), dict(rel_delta=0.0), dict(rel_delta=float("nan")),
                dict(delta=-1.0), dict(delta=float("inf")), dict(target=torch.zeros(4, 3)), dict(source_valid=torch.zeros(4, dtype=torch.bool))):
        with pytest.raises(ValueError):
            postprocess.fit_similarity_robust(**dict(dict(source=p, target=p), **bad))


def test_chunk_plan_exhaustively():
    for chunk in range(2, 13):
        for overlap in range(1, chunk):
            for S in range(1, 41):
                plan = postprocess.chunk_plan(S, chunk, overlap)
                assert plan == twin.chunk_plan(S, chunk, overlap)
                assert plan[0][0] == 0 and plan[-1][1] == S and all(0 < b - a <= chunk for a, b in plan)
                assert sorted(set(v for a, b in plan for v in range(a, b))) == list(range(S))               # cover
                assert all(b == S or b - a == chunk for a, b in plan) and [b for a, b in plan].count(S) == 1
                for (a0, b0), (a1, b1) in zip(plan, plan[1:]):
                    assert b0 - a1 == overlap and a1 - a0 == chunk - overlap and b1 > b0                    # exact overlap, a new view
                assert (len(plan) == 1) == (S <= chunk)
    for S, chunk, overlap in ((0, 4, 2), (-1, 4, 2), (5, 4, 0), (5, 4, 4), (5, 4, 5), (5, 4, -1), (5, 0, 0), (5.0, 4, 2), (5, 4, True)):
        with pytest.raises(ValueError):
            postprocess.chunk_plan(S, chunk, overlap)


def test_index_remapping():
    plan = postprocess.chunk_plan(6, 4, 2)
    assert plan == [(0, 4), (2, 6)]
    assert [postprocess.chunk_indices([1, 4], a, b) for a, b in plan] == [[1], [2]]
    assert [postprocess.chunk_indices([0, 2, 5], a, b) for a, b in plan] == [[0, 2], [0, 3]]
    assert postprocess.chunk_indices(None, 0, 4) == [] and postprocess.chunk_indices([5, 3, 3], 2, 6) == [3, 1, 1]
    for index in ([1, 4], [0, 2, 5], [7, 0, 3]):
        for a, b in postprocess.chunk_plan(9, 5, 2):
            assert postprocess.chunk_indices(index, a, b) == twin.chunk_indices(index, a, b)
            assert [i + a for i in postprocess.chunk_indices(index, a, b)] == [i for i in index if a <= i < b]


def _chunk(S, H=2, W=3):
    return {"world_points": torch.zeros(1, S, H, W, 3), "world_points_conf": torch.ones(1, S, H, W), "depth": torch.ones(1, S, H, W, 1),
            "depth_conf": torch.ones(1, S, H, W), "pose_enc": torch.zeros(1, S, 9), "images": torch.zeros(1, S, 3, H, W)}


def test_stitch_and_forward_chunked_value_errors():
    plan = [(0, 4), (2, 6)]
    good = [_chunk(4), _chunk(4)]
    with pytest.raises(L.OvgError):                                          # well-formed, but on the CPU
        postprocess.stitch_predictions(good, plan)
    for kw in (dict(select="middle"), dict(weights="conf"), dict(conf_percentile=101.0), dict(conf_percentile=None), dict(prediction_mode=None),
               dict(plan=[(0, 4)]), dict(plan=[(1, 4), (2, 6)]), dict(plan=[(0, 4), (4, 6)]), dict(plan=[(0, 4), (2, 4)]), dict(plan=5),
               dict(chunks=good[:1]), dict(chunks=[_chunk(4), _chunk(3)]), dict(chunks=[_chunk(4), {k: v for k, v in _chunk(4).items() if k != "pose_enc"}]),
               dict(chunks=[_chunk(4), {k: v for k, v in _chunk(4).items() if k != "depth"}]),
               dict(chunks=[_chunk(4), dict(_chunk(4), world_points_conf=torch.ones(1, 4, 2, 3, dtype=torch.float64))]),
               dict(chunks=[dict(_chunk(4), images=torch.zeros(2, 4, 3, 2, 3)), _chunk(4)]), dict(iterations=-2)):
        with pytest.raises(ValueError):
            postprocess.stitch_predictions(**dict(dict(chunks=good, plan=plan), **kw))
    with pytest.raises(ValueError):
        postprocess.stitch_predictions([{k: v for k, v in c.items() if not k.startswith("world")} for c in good], plan)      # Pointmap mode without points
    m = OmniVGGT.__new__(OmniVGGT)                                           # the checks below return before the model is touched
    for images, kw in ((torch.zeros(2, 6, 3, 28, 42), {}), (torch.zeros(6, 28, 42), {}), (torch.zeros(6, 3, 28, 42), dict(chunk_size=4, overlap=4)),
                       (torch.zeros(6, 3, 28, 42), dict(chunk_size=4, overlap=0)), (torch.zeros(6, 3, 28, 42), dict(extrinsics=torch.zeros(1, 5, 3, 4))),
                       (torch.zeros(6, 3, 28, 42), dict(depth=torch.zeros(6, 28, 42)))):
        with pytest.raises(ValueError):
            OmniVGGT.forward_chunked(m, images, **kw)


def _random_moments(seed, n=500, with_outliers=False):
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(n, 3)).astype(F)
    T0, _ = twin.wsolve_svd(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)))
    Q = (P.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3] + rng.normal(size=(n, 3)) * 0.01).astype(F)
    w = (10.0 ** rng.uniform(-1.5, 1.5, n)).astype(F)
    return P, Q, w


@pytest.mark.parametrize("with_scale", [True, False])
def test_twin_wsolve_agrees_with_the_weighted_umeyama_fit(with_scale):
    for seed in range(6):
        P, Q, w = _random_moments(seed)
        r, (n1, s1, centre) = twin.fit_step(P, Q, with_scale, weight=w)
        want, scale = twin.wsolve_svd(P, Q, w, with_scale)
        assert r["status"] == 0 and r["count"] == len(P)
        assert np.abs(r["transform"] - want).max() <= 1e-12 and abs(r["scale"] - scale) <= 1e-12
        # fit_rms from the moments alone against the residual summed directly, within the cancellation of vb - tr^2 / var
        E, rms = twin.weighted_residual(r["transform"], P, Q, w.astype(np.float64))
        assert abs(r["E"] - E) <= 64 * 2.0 ** -53 * r["vb"] and abs(r["fit_rms"] - rms) <= 1e-9 * rms
        assert abs(r["weight"] - w.astype(np.float64).sum()) <= 1e-12 * r["weight"]
    # unit weights: the 18 first sums and the solve are align_twin's
    P, Q, _ = _random_moments(9)
    n0, s0 = twin.wmoments(P, Q)
    m0, t0 = align_twin.moments(P, Q)
    assert n0 == m0 and s0[:18].tobytes() == t0.tobytes() and s0[18] == len(P) == s0[19]
    step, scale, rms, status = align_twin.solve(m0, t0, None, with_scale)
    r = twin.wsolve(n0, s0, None, with_scale)
    assert np.array_equal(r["transform"], step) and r["scale"] == scale and r["rms"] == rms and r["status"] == status == 0


def test_twin_degenerate_solves_and_keep():
    P, Q, w = _random_moments(3, n=40)
    prev = (np.diag([2.0, 2.0, 2.0, 1.0]), 2.0)
    for kw, want in ((dict(weight=np.zeros(40, F)), twin.FEW_PAIRS), (dict(source_valid=np.arange(40) < 2), twin.FEW_PAIRS),
                     (dict(weight=np.where(np.arange(40) < 1, 1, np.nan).astype(F)), twin.FEW_PAIRS)):
        n, s = twin.wmoments(P, Q, **kw)
        r = twin.wsolve(n, s)
        assert r["status"] == want and np.array_equal(r["transform"], np.eye(4)) and r["scale"] == 1.0 and r["fit_rms"] == 0.0
        k = twin.wsolve(n, s, keep=True, previous=prev)
        assert k["status"] == want and np.array_equal(k["transform"], prev[0]) and k["scale"] == 2.0
    n, s = twin.wmoments(np.tile(P[:1], (40, 1)), Q, weight=w)
    assert twin.wsolve(n, s)["status"] == twin.NO_SPREAD
    s = s.copy()
    s[7] = np.inf
    assert twin.wsolve(n, s)["status"] & twin.NOT_FINITE
    n, s = twin.wmoments(P, Q, weight=w)
    assert twin.wsolve(n, s, centre=np.array([0, 0, np.nan, 0, 0, 0.0]))["status"] == twin.NOT_FINITE
    # a delta that is zero, NaN or infinite reweights nothing; a perfect previous fit keeps every weight
    base = twin.wmoments(P, Q, weight=w, transform=np.eye(4))[1]
    for d in (0.0, np.nan, np.inf, -1.0, 1e-200):
        assert twin.wmoments(P, Q, weight=w, transform=np.eye(4), cauchy=True, delta=np.array([d]))[1].tobytes() == base.tobytes()
    assert twin.wmoments(P, Q, weight=w, transform=np.eye(4), cauchy=True, delta=np.array([0.3]))[1][18] < base[18]


def test_robust_fixture_is_meaningful_on_the_twin_alone():
    P, Q, T = twin.robust_fixture()
    fits = twin.fit_robust(P, Q, iterations=6)
    err = [np.abs(f["transform"] - T).max() for f in fits]
    print("robust fixture, max |T - T_true| per iteration:", " ".join("%.3g" % e for e in err))
    print("fit_rms per iteration:", " ".join("%.3g" % f["fit_rms"] for f in fits))
    assert all(f["status"] == 0 and f["count"] == 4096 for f in fits)
    assert err[0] / err[6] >= 100.0
    assert err[0] > 0.05 and err[6] < 2e-4
    plain = align_twin.fit(P, Q)
    assert np.array_equal(plain[0], fits[0]["transform"])                    # iteration 0 without weights is the plain fit
    # the absolute form: the same loop with delta fixed at half the noise-free extent of an inlier's residual
    fixed = twin.fit_robust(P, Q, iterations=6, delta=0.01)
    assert np.abs(fixed[6]["transform"] - T).max() < err[0] / 100.0


def test_twin_camera_move_sees_the_moved_points_at_the_scaled_depth():
    rng = np.random.default_rng(5)
    M, s = twin.wsolve_svd(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)))
    E, _ = twin.wsolve_svd(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)), with_scale=False)
    X = rng.normal(size=(50, 3))
    cam = X @ E[:3, :3].T + E[:3, 3]
    moved = twin.move_cameras(E[None, :3].astype(F), M, s)[0].astype(np.float64)
    X2 = X @ M[:3, :3].T + M[:3, 3]
    cam2 = X2 @ moved[:, :3].T + moved[:, 3]
    assert np.abs(cam2 - s * cam).max() <= 1e-5 * max(1.0, np.abs(cam2).max())
    pts, depth, pc, dc = twin.move_maps(M, s, X.astype(F), cam[:, 2].astype(F), None, np.ones(50, F))
    assert pc is None and np.array_equal(dc, np.ones(50, F)) and np.array_equal(pts, align_twin.apply(M, X.astype(F)))
    assert np.array_equal(depth, (cam[:, 2].astype(F).astype(np.float64) * s).astype(F))
