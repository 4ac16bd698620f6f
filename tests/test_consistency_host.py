"""Multi-view depth consistency, host side: the numpy twin (tests/consistency_twin.py) on hand-made two-camera cases whose every
intermediate is exact in float32, the rule on the real four-view infinigen fixture (untouched and with seeded floaters), the C ABI
without a device (struct layout, the workspace query, argument checks that return before any HIP call) and the Python API's argument
checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import consistency_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
REAL = os.path.join(common.ROOT, "tests", "golden", "real", "infinigen_294_aux_inputs.npz")
F = np.float32
H = W = 5


def _two_cameras():
    """fx = fy = 4, cx = cy = 2, 5 x 5 pixels; camera 0 at the origin, camera 1 with t = (0.5, 0, 0): xc = x + 0.5. On the plane
    z = 2 pixel (u, w) of camera 0 is the point ((u - 2) / 2, (w - 2) / 2, 2) and lands in camera 1 at u1 = floor(4 (x + .5) / 2 + 2.5)
    = u + 1, same row; pixel (u, w) of camera 1 is ((u - 3) / 2, (w - 2) / 2, 2) and lands in camera 0 at u - 1. Every product,
    quotient and sum is exact in f32."""
    e = np.zeros((2, 3, 4))
    e[:, :, :3] = np.eye(3)
    e[1, 0, 3] = 0.5
    k = np.array([[4.0, 0, 2.0], [0, 4.0, 2.0], [0, 0, 1.0]])
    return twin.pack_cams(e, k)


def _plane(z=2.0):
    w, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pts = np.empty((2, H, W, 3), F)
    for s, shift in ((0, 2.0), (1, 3.0)):
        pts[s] = np.stack([(u - shift) / 2 * (z / 2), (w - 2.0) / 2 * (z / 2), np.full(u.shape, z)], -1)
    return pts


def _run(pts, tol=0.25, near=1e-3, valid=None):
    out = twin.consistency(pts, _two_cameras(), tol, near=near, valid=valid)
    for o in out:
        assert o.dtype == np.int16 and o.shape == (2, H, W)
    return out


def test_twin_plane_seen_by_two_cameras_supports_itself_where_the_frames_overlap():
    for tol in (0.25, 0.0):                                                  # zc == d == 2 exactly: a tie, kept at tol = 0
        sup, vio, occ = _run(_plane(), tol=tol)
        want = np.zeros((2, H, W), np.int16)
        want[0, :, :4] = 1                                                   # column 4 of camera 0 lands at u = 5: out of frame
        want[1, :, 1:] = 1                                                   # column 0 of camera 1 lands at u = -1
        assert np.array_equal(sup, want) and not vio.any() and not occ.any()


def test_twin_pulled_point_is_a_violation_and_pushed_point_is_occluded():
    pts = _plane()
    pts[0, 2, 2] = [0.0, 0.0, 1.0]                                           # pixel (2, 2) of camera 0 pulled along its ray to z = 1
    sup, vio, occ = _run(pts)
    # in camera 1: xc = 0.5, zc = 1, u = floor(4 * 0.5 + 2.5) = 4 -> pixel (4, 2), d = 2, diff = -1 < -0.5: camera 1 looks through it
    assert (sup[0, 2, 2], vio[0, 2, 2], occ[0, 2, 2]) == (0, 1, 0)
    # pixel (3, 2) of camera 1 lands on (2, 2) of camera 0 with zc = 2 against d = 1: diff = 1 > band = 0.25: hidden behind the floater
    assert (sup[1, 2, 3], vio[1, 2, 3], occ[1, 2, 3]) == (0, 0, 1)
    # pixel (4, 2) of camera 1, where the floater lands, still lands on (3, 2) of camera 0 itself: untouched support
    assert (sup[1, 2, 4], vio[1, 2, 4], occ[1, 2, 4]) == (1, 0, 0)
    assert vio.sum() == 1 and occ.sum() == 1 and sup.sum() == 2 * 20 - 2

    pts = _plane()
    pts[0, 2, 2] = [0.0, 0.0, 4.0]                                           # pushed back to z = 4
    sup, vio, occ = _run(pts)
    # in camera 1: xc = 0.5, zc = 4, u = floor(4 * 0.125 + 2.5) = 3 -> pixel (3, 2), d = 2, diff = 2 > 0.5: occluded
    assert (sup[0, 2, 2], vio[0, 2, 2], occ[0, 2, 2]) == (0, 0, 1)
    # pixel (3, 2) of camera 1 lands on (2, 2) of camera 0 with zc = 2 against d = 4: diff = -2 < -1: a violation
    assert (sup[1, 2, 3], vio[1, 2, 3], occ[1, 2, 3]) == (0, 1, 0)
    assert vio.sum() == 1 and occ.sum() == 1 and sup.sum() == 2 * 20 - 2


def test_twin_band_is_inclusive_and_tol_zero_keeps_only_ties():
    """d = 2, tol = 0.25: band = 0.5 exactly. The source is pixel (2, 2) of camera 0 moved along its ray (x = y = 0) to z = zc; in
    camera 1 it lands at u = floor(4 (0.5 / zc) + 2.5) = 3 for every zc tried (0.5 / zc in [0.2, 0.34]), where d = 2."""
    up, down = np.nextafter(F(2.5), F(np.inf)), np.nextafter(F(1.5), F(-np.inf))
    for zc, want in ((F(2.5), (1, 0, 0)), (up, (0, 0, 1)), (F(1.5), (1, 0, 0)), (down, (0, 1, 0)), (F(2.0), (1, 0, 0))):
        pts = _plane()
        pts[0, 2, 2] = [0.0, 0.0, zc]
        sup, vio, occ = _run(pts, tol=0.25)
        assert (sup[0, 2, 2], vio[0, 2, 2], occ[0, 2, 2]) == want, zc
    for zc, want in ((F(2.0), (1, 0, 0)), (np.nextafter(F(2.0), F(3.0)), (0, 0, 1)), (np.nextafter(F(2.0), F(1.0)), (0, 1, 0))):
        pts = _plane()
        pts[0, 2, 2] = [0.0, 0.0, zc]
        sup, vio, occ = _run(pts, tol=0.0)
        assert (sup[0, 2, 2], vio[0, 2, 2], occ[0, 2, 2]) == want, zc


def test_twin_unusable_pixels_count_nowhere_as_targets_and_give_zero_rows_as_sources():
    """Each bad point replaces pixel (2, 2) of camera 0: as a source it has three zeros; pixel (3, 2) of camera 1, which lands on it,
    loses its only target and has three zeros too. Everything else keeps its support."""
    base_sup = _run(_plane())[0]
    cases = [([np.nan, 0, 2], None), ([0, np.inf, 2], None), ([0, 0, -np.inf], None), ([0, 0, np.nan], None),
             ([0, 0, -1.0], None),                                           # behind its own camera
             ([0, 0, 0.5], 0.5),                                             # z > near is strict
             ([0, 0, 0.25], 0.5)]
    for p, near in cases:
        pts = _plane()
        pts[0, 2, 2] = p
        sup, vio, occ = _run(pts, near=1e-3 if near is None else near)
        want = base_sup.copy()
        want[0, 2, 2] = want[1, 2, 3] = 0
        assert np.array_equal(sup, want) and not vio.any() and not occ.any(), p
    # valid = 0 does the same as a bad coordinate
    valid = np.ones((2, H, W), np.uint8)
    valid[0, 2, 2] = 0
    sup, vio, occ = _run(_plane(), valid=valid)
    want = base_sup.copy()
    want[0, 2, 2] = want[1, 2, 3] = 0
    assert np.array_equal(sup, want) and not vio.any() and not occ.any()
    # usable in its own view (own depth 2), out of camera 1's frame: u = floor(4 * 2.5 / 2 + 2.5) = 7, and pixels far beyond int32
    for p in ([2.0, 0.0, 2.0], [1e30, 0.0, 2.0], [3e38, 0.0, 2.0]):
        pts = _plane()
        pts[0, 2, 2] = p
        sup, vio, occ = _run(pts)
        assert (sup[0, 2, 2], vio[0, 2, 2], occ[0, 2, 2]) == (0, 0, 0), p
        assert sup[1, 2, 3] == 1                                             # as a target it is still usable: its own depth is 2
    # a camera behind which the plane lies: camera 1 turned round (R = diag(-1, 1, -1)) sees every point of camera 0 at zc = -2
    e = np.zeros((2, 3, 4))
    e[0, :, :3] = np.eye(3)
    e[1, :, :3] = np.diag([-1.0, 1.0, -1.0])
    cams = twin.pack_cams(e, np.array([[4.0, 0, 2.0], [0, 4.0, 2.0], [0, 0, 1.0]]))
    pts = _plane()
    pts[1, :, :, 2] = -2.0                                                   # in front of camera 1 (zc = 2), behind camera 0
    sup, vio, occ = twin.consistency(pts, cams, 0.25)
    assert not sup.any() and not vio.any() and not occ.any()
    assert not np.isnan(twin.zmap(pts, cams, 1e-3)).any()                    # every pixel is usable: the pairs fail in the other view


def _real_scene():
    g = np.load(REAL)
    ext, intr, depth = g["extrinsics"][0], g["intrinsics"][0], g["depth"]
    assert depth.shape == (4, 294, 518) and ext.shape == (4, 3, 4) and intr.shape == (4, 3, 3)
    return ext, intr, depth.astype(F), depth > 0


def test_rule_separates_floaters_from_surfaces_on_real_views():
    """The four infinigen views with ground-truth depth, rel_tol = 0.02. The gates are conditions that keep the test from being
    empty (the rule must confirm most of a consistent scene and flag most floaters), not a measurement of the device code."""
    ext, intr, depth, valid = _real_scene()
    cams = twin.pack_cams(ext, intr)
    sup, vio, _ = twin.consistency(twin.unproject64(depth, ext, intr), cams, 0.02, valid=valid)
    s1, v1 = float((sup[valid] >= 1).mean()), float((vio[valid] >= 1).mean())
    print("untouched: support >= 1 %.3f, violations >= 1 %.3f" % (s1, v1))
    assert not sup[~valid].any() and not vio[~valid].any()
    assert s1 >= 0.75 and v1 <= 0.03

    depth2, moved = twin.perturb_depth(depth, valid, share=0.05, factor=0.7, seed=0)
    sup, vio, _ = twin.consistency(twin.unproject64(depth2, ext, intr), cams, 0.02, valid=valid)
    rest = valid & ~moved
    mv, ms = float((vio[moved] >= 1).mean()), float((sup[moved] >= 1).mean())
    rs, rv = float((sup[rest] >= 1).mean()), float((vio[rest] >= 1).mean())
    print("perturbed: moved pixels violations >= 1 %.3f, support >= 1 %.3f; unmoved support >= 1 %.3f, violations >= 1 %.3f"
          % (mv, ms, rs, rv))
    assert 0.04 <= moved.sum() / valid.sum() <= 0.06
    assert mv >= 0.70 and ms <= 0.05 and rs >= 0.75 and rv <= 0.03
    # the mask the pipeline uses keeps the surfaces and drops the floaters
    keep = (sup >= 1) & (vio <= 0)
    assert keep[moved].mean() <= 0.05 and keep[rest].mean() >= 0.70


def test_synthetic_scene_exercises_every_class():
    """The scene of the device test, checked where it is built: at each tolerance every class holds >= 5 % of the counted pairs and
    >= 5 % of all pairs leave the frame; some fall behind the other cameras."""
    pts, ext, intr, valid = twin.synthetic_scene()
    assert pts.shape == (6, 70, 98, 3) and np.isnan(pts).any() and np.isinf(pts).any() and np.nanmax(np.abs(pts[np.isfinite(pts)])) > 1e29
    for tol in (0.0, 0.01, 0.05):
        st = {}
        twin.consistency(pts, twin.pack_cams(ext, intr), tol, valid=valid, stats=st)
        print(tol, st)
        for k in ("support", "violations", "occluded"):
            assert st[k] >= 0.05 * st["counted"], (tol, k)
        assert st["support"] + st["violations"] + st["occluded"] == st["counted"]
        assert st["in_front"] - st["in_frame"] >= 0.05 * st["pairs"] and st["pairs"] - st["in_front"] >= 0.05 * st["pairs"]


def test_ctypes_struct_layout_matches_c_consistency():
    enums, _ = abi_layout.check({"ovg_consistency_params": L.ConsistencyParams},
                                ["OVG_MVC_MAX_VIEWS", "OVG_MVC_TILE_DEFAULT", "OVG_MVC_TILE_256x1", "OVG_MVC_TILE_16x16", "OVG_MVC_TILE_8x32",
                                 "OVG_MVC_TILE_32x8", "OVG_MVC_ROTATE_TARGETS", "OVG_MVC_KEEP_MAP", "OVG_ABI_VERSION"])
    assert enums == [L.MVC_MAX_VIEWS, L.MVC_TILE_DEFAULT, L.MVC_TILE_256x1, L.MVC_TILE_16x16, L.MVC_TILE_8x32,
                     L.MVC_TILE_32x8, L.MVC_ROTATE_TARGETS, L.MVC_KEEP_MAP, L.ABI_VERSION]
    assert L.ABI_VERSION == 13
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+ovg_consistency_workspace_bytes\s*\(\s*int32_t\s+S,\s*int32_t\s+H,\s*int32_t\s+W\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_multiview_consistency\s*\(\s*const\s+ovg_consistency_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_multiview_consistency" in L.SYMBOLS and "ovg_consistency_workspace_bytes" in L.SYMBOLS


def test_consistency_workspace_query_and_argument_validation_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    q = lib.ovg_consistency_workspace_bytes
    for S, h, w in ((1, 1, 1), (2, 1, 2), (4, 294, 518), (64, 518, 518), (3, 3, 5), (7, 1, 9), (32767, 16, 16), (1, 46340, 46340)):
        assert q(S, h, w) == (4 * S * h * w + 15) // 16 * 16, (S, h, w)
    assert q(1, 1, 1) == 16 and q(64, 518, 518) == 4 * 64 * 518 * 518
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3), (2, 1 << 15, 1 << 15), (1, 1 << 16, 1 << 15),
                (8004, 518, 518), (32768, 1, 1), (40000, 2, 2), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        assert q(*bad) == -1, bad
    assert q(8003, 518, 518) > 0                                           # 8003 * 518^2 < 2^31 <= 8004 * 518^2

    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks

    def run(**kw):
        p = L.ConsistencyParams(points=big, cams=big, valid=big, S=4, H=16, W=24, src_first=0, src_count=4, tol=0.02, near=1e-3,
                                ws=big, ws_bytes=q(4, 16, 24), support=big, violations=big, occluded=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_multiview_consistency(ctypes.byref(p), None)

    assert lib.ovg_multiview_consistency(None, None) == -1
    for bad in (dict(points=None), dict(cams=None), dict(ws=None), dict(support=None), dict(violations=None),
                dict(S=0), dict(H=0), dict(W=0), dict(S=-1), dict(H=-5), dict(W=-1), dict(S=32768, H=1, W=1, ws_bytes=1 << 50),
                dict(S=1 << 15, H=1 << 8, W=1 << 8, ws_bytes=1 << 50), dict(S=1 << 14, H=1 << 20, W=1 << 20, ws_bytes=1 << 62),
                dict(src_first=-1), dict(src_first=4), dict(src_count=0), dict(src_count=-1), dict(src_count=5), dict(src_first=2, src_count=3),
                dict(src_first=3, src_count=(1 << 31) - 1),
                dict(tol=-1e-9), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-float("inf")),
                dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(near=-0.0),
                dict(ws_bytes=q(4, 16, 24) - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8),
                dict(tile=-1), dict(tile=5), dict(flags=4), dict(flags=-1), dict(support=big + 1), dict(occluded=big + 1)):
        assert run(**bad) == -1, bad


def test_python_argument_checks_and_cpu_tensors():
    S, h, w = 3, 6, 8
    pts = torch.zeros(S, h, w, 3)
    E, K = np.tile(np.eye(4)[:3], (S, 1, 1)), np.array([[10.0, 0, 4], [0, 10.0, 3], [0, 0, 1]])
    good = dict(points=pts, extrinsic=E, intrinsic=K)
    for kw in (dict(points=torch.zeros(S, h, w)), dict(points=torch.zeros(S, h, w, 4)), dict(points=torch.zeros(0, h, w, 3)),
               dict(points=np.zeros((S, h, w, 3), F)), dict(extrinsic=E[:2]), dict(extrinsic=np.tile(np.eye(4), (S, 1, 1))),
               dict(intrinsic=np.zeros((2, 3, 3))), dict(intrinsic=np.zeros((3, 4))),
               dict(valid=torch.ones(S, h, w + 1, dtype=torch.bool)), dict(valid=torch.ones(S, h, w)), dict(valid=np.ones((S, h, w), bool)),
               dict(frame=3), dict(frame=-4), dict(frame=1.5), dict(frame=True),
               dict(rel_tol=-0.01), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(rel_tol=1e60), dict(rel_tol="x"),
               dict(near=0.0), dict(near=-1e-3), dict(near=float("nan")), dict(near=1e-60)):
        with pytest.raises(ValueError):
            postprocess.multiview_consistency(**dict(good, **kw))
    for kw in (dict(), dict(frame=1), dict(frame=-1), dict(valid=torch.ones(S, h, w, dtype=torch.bool)), dict(intrinsic=np.tile(K, (S, 1, 1))),
               dict(rel_tol=0.0, return_occluded=True), dict(extrinsic=torch.from_numpy(E), intrinsic=K.tolist())):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.multiview_consistency(**dict(good, **kw))          # CPU tensors: no fallback

    r = postprocess.ConsistencyResult(torch.tensor([[2, 0, 1]], dtype=torch.int16), torch.tensor([[0, 0, 1]], dtype=torch.int16))
    assert r.occluded is None
    assert postprocess.consistency_mask(r).tolist() == [[True, False, False]]
    assert postprocess.consistency_mask(r, min_support=2).tolist() == [[True, False, False]]
    assert postprocess.consistency_mask(r, min_support=0, max_violations=1).tolist() == [[True, True, True]]
    assert postprocess.consistency_mask(r).dtype == torch.bool

    pred = {"images": torch.zeros(1, S, 3, h, w), "world_points": torch.zeros(1, S, h, w, 3), "extrinsic": torch.zeros(1, S, 3, 4),
            "intrinsic": torch.zeros(1, S, 3, 3)}
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.prediction_consistency(pred)
    with pytest.raises(ValueError):
        postprocess.prediction_consistency(pred, batch_index=1)
    with pytest.raises(ValueError):
        postprocess.prediction_consistency([pred])
    for km in (torch.ones(S, h, w + 1, dtype=torch.bool), torch.ones(S, h, w), torch.ones(S, h, w, dtype=torch.uint8),
               np.ones((S, h, w), bool), torch.ones(1, S, h, w, dtype=torch.bool)):
        with pytest.raises(ValueError):
            postprocess.predictions_to_point_cloud(pred, keep_mask=km)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.predictions_to_point_cloud(pred, keep_mask=torch.ones(S, h, w, dtype=torch.bool))
