"""Point-cloud extraction on the MI355X (ovg_percentile / ovg_point_filter through postprocess.predictions_to_point_cloud): every golden
case of the REAL reference export, the headline 64 x 518^2 size against the CPU twin, percentiles where torch.quantile refuses, and
determinism. Selection, colours and threshold are compared for identity; the points are copies, so they are compared bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

import common
import pointcloud_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
import postprocess_oracle as ppo  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).tobytes()


def _same_f32(a, b):
    """Bit-identical f32 values, except that any NaN equals any NaN (the sign of a NaN made by inf - inf is the machine's: x86 and the
    GPU make different ones, numpy's own NaN is positive)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def _check(cloud, tw, pts_flat, name):
    idx = cloud.indices.cpu().numpy()
    assert np.array_equal(idx, tw["indices"]), name
    assert np.array_equal(cloud.colors.cpu().numpy(), tw["colors"]), name
    assert _bits(cloud.points) == np.ascontiguousarray(pts_flat[idx]).tobytes(), name
    assert _same_f32(cloud.conf_threshold.cpu().numpy(), tw["conf_threshold"]), name
    assert np.abs(cloud.transform - tw["transform"]).max() <= 1e-12, name


def test_every_golden_case_matches_the_reference_selection():
    L.require_gpu()
    g = dict(np.load(os.path.join(common.GOLD, "pointcloud.npz")))
    import json
    cases = json.loads(str(g["cases"]))
    for i, case in enumerate(cases):
        p, m = "c%d_" % i, case["map"]
        depth_mode = case["mode"] == "Predicted Depth"
        if depth_mode:
            # the device computes its own f32 world points from pose_enc + depth: the same selection, points within 1e-6 of the oracle
            pred = {"pose_enc": _dev(g[m + "_pose_enc"])[None], "depth": _dev(g[m + "_depth"])[None], "depth_conf": _dev(g[m + "_depth_conf"])[None],
                    "images": _dev(g[m + "_images"])[None]}
        else:
            pred = {"world_points": _dev(g[m + "_world_points"])[None], "world_points_conf": _dev(g[m + "_world_points_conf"])[None],
                    "images": _dev(g[m + "_images"])[None], "extrinsic": _dev(g[m + "_extrinsic"])[None]}
        sky = g.get(p + "sky")
        cloud = postprocess.predictions_to_point_cloud(pred, conf_thres=case["conf_thres"], filter_by_frames=case["filter_by_frames"],
                                                       mask_black_bg=case["mask_black_bg"], mask_white_bg=case["mask_white_bg"],
                                                       prediction_mode=case["mode"], sky_mask=None if sky is None else _dev(sky),
                                                       return_indices=True)
        name = case["name"]
        assert np.array_equal(cloud.indices.cpu().numpy(), g[p + "indices"].astype(np.int64)), name
        assert np.array_equal(cloud.colors.cpu().numpy(), g[p + "colors"]), name
        assert _same_f32(cloud.conf_threshold.cpu().numpy(), g[p + "threshold"]), name
        if depth_mode:
            pts_dev = cloud.points.cpu().numpy()
            ref = g[m + "_world_points_from_depth"].reshape(-1, 3)[g[p + "indices"]]
            assert common.max_rel(pts_dev, ref) <= 1e-6, name
            # the transform comes from the device's own pose decoding (f32): within its rounding of the reference's extrinsic
            assert np.abs(cloud.transform - g[p + "transform"]).max() <= 1e-5, name
            want = twin.scene_scale(pts_dev)
        else:
            pts = g[m + "_world_points"].reshape(-1, 3)
            assert _bits(cloud.points) == np.ascontiguousarray(pts[g[p + "indices"]]).tobytes(), name
            assert np.abs(cloud.transform - g[p + "transform"]).max() <= 1e-12, name
            want = g[p + "scene_scale"] if not case["empty"] else np.float32(1.0)
        assert _same_f32(cloud.scene_scale.cpu().numpy(), want), (name, float(cloud.scene_scale), want)
        assert len(cloud) == g[p + "indices"].size, name


def _headline(S=64, H=518, W=518, seed=0):
    rng = np.random.default_rng(seed)
    conf = (np.float32(1.0) + np.floor(rng.random((S, H, W), dtype=np.float32) * np.float32(40.0)) / np.float32(4.0)).astype(np.float32)
    conf[rng.random((S, H, W)) < 0.01] = np.inf
    pts = rng.standard_normal((S, H, W, 3), dtype=np.float32)
    img = rng.random((S, 3, H, W), dtype=np.float32)
    black = rng.random((S, H, W)) < 0.05
    white = rng.random((S, H, W)) < 0.05
    img[np.broadcast_to(black[:, None], img.shape)] = 0.01
    img[np.broadcast_to(white[:, None], img.shape)] = 0.99
    sky = (rng.random((S, H, W)) < 0.9).astype(np.uint8)
    sky[np.isinf(conf)] = 1                                              # inf * 0 would be NaN: numpy's threshold, and the cloud, empty
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    ext = np.tile(np.concatenate([rot, rng.standard_normal((3, 1))], 1).astype(np.float32), (S, 1, 1))
    return conf, pts, img, sky, ext


def test_headline_size_matches_twin():
    """64 views x 518^2 = 17 172 736 pixels (above torch.quantile's 2^24 limit): quantised conf with many ties and some +inf, black
    and white pixels, a sky mask, both background tests, five thresholds and a frame filter, against the twin bit for bit."""
    L.require_gpu()
    conf, pts, img, sky, ext = _headline()
    pred = {"world_points": _dev(pts)[None], "world_points_conf": _dev(conf)[None], "images": _dev(img)[None], "extrinsic": _dev(ext)[None]}
    sky_d = _dev(sky)
    flat = pts.reshape(-1, 3)
    for t in (0.0, 25.0, 37.3, 50.0, 100.0):
        kw = dict(conf_thres=t, mask_black_bg=True, mask_white_bg=True, sky_mask=sky if t in (37.3, 50.0) else None)
        cloud = postprocess.predictions_to_point_cloud(pred, return_indices=True, **{**kw, "sky_mask": sky_d if kw["sky_mask"] is not None else None})
        tw = twin.select(pts, conf, img, ext, **kw)
        _check(cloud, tw, flat, "conf_thres %s" % t)
        if len(cloud):
            assert _same_f32(cloud.scene_scale.cpu().numpy(), twin.scene_scale(np.ascontiguousarray(flat[tw["indices"]]))), t
    cloud = postprocess.predictions_to_point_cloud(pred, conf_thres=50.0, filter_by_frames="17: x.png", return_indices=True)
    _check(cloud, twin.select(pts, conf, img, ext, conf_thres=50.0, frame=17), flat, "frame 17")


def test_predicted_depth_mode_at_headline_size():
    L.require_gpu()
    S, H, W = 64, 518, 518
    rng = np.random.default_rng(3)
    enc = np.zeros((1, S, 9), np.float32)
    enc[..., :3] = rng.standard_normal((1, S, 3)) * 0.5
    q = rng.standard_normal((1, S, 4)).astype(np.float32)
    enc[..., 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    enc[..., 7:] = 0.7 + 0.5 * rng.random((1, S, 2))
    depth = (1.0 + 4.0 * rng.random((1, S, H, W, 1), dtype=np.float32)).astype(np.float32)
    dconf = (np.float32(1.0) + np.floor(rng.random((1, S, H, W), dtype=np.float32) * np.float32(64.0))).astype(np.float32)
    img = rng.random((1, S, 3, H, W), dtype=np.float32)
    pred = {"pose_enc": _dev(enc), "depth": _dev(depth), "depth_conf": _dev(dconf), "images": _dev(img)}
    cloud = postprocess.predictions_to_point_cloud(pred, conf_thres=50.0, prediction_mode="Predicted Depth", return_indices=True)
    full = postprocess.get_world_points_from_depth(dict(pred))
    ext = full["extrinsic"][0].cpu().numpy()
    intr = full["intrinsic"][0].cpu().numpy()
    wp = full["world_points_from_depth"][0].cpu().numpy()
    sel = np.random.default_rng(0).choice(S, 4, replace=False)
    ref = ppo.unproject_depth_map_to_point_map(depth[0][sel], ext[sel], intr[sel])
    assert common.max_rel(wp[sel], ref) <= 1e-6
    tw = twin.select(wp, dconf[0], img[0], ext, conf_thres=50.0)
    _check(cloud, tw, wp.reshape(-1, 3), "depth mode")


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, (1 << 20) + 1, 64 * 518 * 518])
def test_percentile_matches_twin(n):
    L.require_gpu()
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    if n > 300:
        tie = rng.random(n) < 0.3
        x[tie] = np.round(x[tie])                                       # ties
        x[rng.integers(0, n, 3)] = np.inf
    qs = [0.0, 5.0, 37.3, 100.0]
    got = postprocess.percentile(_dev(x), qs).cpu().numpy()
    assert _same_f32(got, twin.percentile(x, qs)), n
    assert postprocess.percentile(_dev(x), 95.0).shape == ()
    if n > (1 << 24):
        with pytest.raises(RuntimeError):
            torch.quantile(_dev(x[:n]), 0.5)
    # strided (n, 3) columns, as the scene scale reads the kept vertices
    m = min(n, 1 << 20)
    v = rng.standard_normal((m, 3)).astype(np.float32)
    got = postprocess.percentile(_dev(v), [5.0, 95.0], dim=0).cpu().numpy()
    want = np.stack([twin.percentile(v[:, c], [5.0, 95.0]) for c in range(3)], 1)
    assert got.shape == (2, 3) and _same_f32(got, want), n


def test_percentile_nan_and_inf_follow_numpy():
    L.require_gpu()
    x = np.array([1.0, 2.0, np.inf, np.inf, 3.0], np.float32)
    for qs in ([0.0, 50.0, 60.0, 100.0], [10.0, 99.0]):
        assert _same_f32(postprocess.percentile(_dev(x), qs).cpu().numpy(), twin.percentile(x, qs)), qs
    x[1] = np.nan
    assert np.isnan(postprocess.percentile(_dev(x), [0.0, 50.0]).cpu().numpy()).all()


def test_two_calls_are_bit_identical():
    L.require_gpu()
    conf, pts, img, sky, ext = _headline(S=8, seed=5)
    pred = {"world_points": _dev(pts)[None], "world_points_conf": _dev(conf)[None], "images": _dev(img)[None], "extrinsic": _dev(ext)[None]}
    a = postprocess.predictions_to_point_cloud(pred, conf_thres=37.3, sky_mask=_dev(sky), mask_black_bg=True, return_indices=True)
    b = postprocess.predictions_to_point_cloud(pred, conf_thres=37.3, sky_mask=_dev(sky), mask_black_bg=True, return_indices=True)
    for k in ("points", "colors", "indices", "conf_threshold", "scene_scale"):
        assert _bits(getattr(a, k)) == _bits(getattr(b, k)), k
    assert len(a) > 0
