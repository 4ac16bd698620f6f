"""ovg_multiview_consistency / postprocess.multiview_consistency on the device against tests/consistency_twin.py: support, violations
and occluded counts byte for byte -- a synthetic orbit with floaters, pushed-back pixels, non-finite rows, huge coordinates, points
behind other cameras and a holed valid mask at an awkward size; the real infinigen views, untouched and perturbed; 64 x 518^2 inside
the queried workspace; and the pipeline predictions -> consistency mask -> point cloud -> voxel grid / GLB."""
import os

import numpy as np
import pytest
import torch

import common
import consistency_twin as twin
import pointcloud_twin as pctwin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
REAL = os.path.join(common.ROOT, "tests", "golden", "real")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("support", "violations", "occluded")):
        g = g.cpu().numpy()
        assert g.dtype == np.int16 and w.dtype == np.int16 and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, int((g != w).sum()))


def _check(pts, ext, intr, tol, name, valid=None, near=1e-3, frame=None, want=None):
    """Device against twin, the three maps byte for byte. -> (device result, twin result)."""
    res = postprocess.multiview_consistency(_dev(pts), ext, intr, valid=None if valid is None else _dev(valid), rel_tol=tol, near=near,
                                            frame=frame, return_occluded=True)
    if want is None:
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        want = twin.consistency(pts, twin.pack_cams(host(ext), host(intr)), tol, near=near, valid=valid,
                                sources=None if frame is None else [frame % len(pts)])
    _same((res.support, res.violations, res.occluded), want, name)
    return res, want


def test_synthetic_orbit_matches_twin_bit_exactly():
    L.require_gpu()
    pts, ext, intr, valid = twin.synthetic_scene()
    S, H, W = pts.shape[:3]
    assert (S, H, W) == (6, 70, 98)
    cams = twin.pack_cams(ext, intr)
    for tol in (0.0, 0.01, 0.05):
        st = {}
        want = twin.consistency(pts, cams, tol, valid=valid, stats=st)
        for k in ("support", "violations", "occluded"):                      # non-emptiness, on the twin's own output
            assert st[k] >= 0.05 * st["counted"], (tol, k, st)
        assert st["in_front"] - st["in_frame"] >= 0.05 * st["pairs"], st
        res, _ = _check(pts, ext, intr, tol, "synthetic tol=%g" % tol, valid=valid, want=want)
        # without `occluded`, every tile shape and both target orders: the same bytes
        dp, dc, dv = _dev(pts), _dev(cams), _dev(valid)
        for tile in (L.MVC_TILE_DEFAULT, L.MVC_TILE_256x1, L.MVC_TILE_16x16, L.MVC_TILE_8x32, L.MVC_TILE_32x8):
            for flags in (0, L.MVC_ROTATE_TARGETS):
                sup, vio, occ = ops.multiview_consistency(dp, dc, tol, valid=dv, occluded=flags != 0, tile=tile, flags=flags)
                assert torch.equal(sup, res.support) and torch.equal(vio, res.violations), (tol, tile, flags)
                assert occ is None or torch.equal(occ, res.occluded)
    _check(pts, ext, intr, 0.01, "synthetic without valid")
    _check(pts, ext, intr, 0.01, "synthetic near=2.5", valid=valid, near=2.5)      # a near plane that cuts into the scene
    # a source range, and the maps of an earlier call reused
    dp, dc = _dev(pts), _dev(cams)
    ws = torch.empty(ops.consistency_workspace_bytes(S, H, W), device="cuda", dtype=torch.uint8)
    full = ops.multiview_consistency(dp, dc, 0.05, occluded=True, ws=ws)
    part = ops.multiview_consistency(dp, dc, 0.05, occluded=True, ws=ws, src_first=2, src_count=3, flags=L.MVC_KEEP_MAP)
    for a, b in zip(full, part):
        assert b.shape == (3, H, W) and torch.equal(a[2:5], b)


def _real():
    g = np.load(os.path.join(REAL, "infinigen_294_aux_inputs.npz"))
    depth = g["depth"].astype(F)
    return g["extrinsics"][0], g["intrinsics"][0], depth, depth > 0


def test_real_views_match_twin_and_frame_selects_a_row():
    L.require_gpu()
    ext, intr, depth, valid = _real()
    depth2, moved = twin.perturb_depth(depth, valid)
    for name, d in (("untouched", depth), ("perturbed", depth2)):
        pts = twin.unproject64(d, ext, intr)
        res, want = _check(pts, ext, intr, 0.02, name, valid=valid.astype(np.uint8))
        assert res.support.shape == (4, 294, 518)
        # bool mask, device-resident f32 cameras, host float64 cameras: the same bytes; two calls give identical bytes
        dp = _dev(pts)
        for e, k in ((_dev(ext), _dev(intr)), (ext.astype(np.float64), intr.astype(np.float64)), (ext.tolist(), intr[0])):
            if not isinstance(e, torch.Tensor) and np.asarray(k).ndim == 2:
                continue                                                     # the views' intrinsics differ: no (3, 3) form here
            again = postprocess.multiview_consistency(dp, e, k, valid=_dev(valid), rel_tol=0.02, return_occluded=True)
            _same((again.support, again.violations, again.occluded), want, name)
        for k in (0, 2, -1):
            one = postprocess.multiview_consistency(dp, ext, intr, valid=_dev(valid), rel_tol=0.02, frame=k, return_occluded=True)
            assert one.support.shape == (1, 294, 518)
            for a, b in zip((one.support, one.violations, one.occluded), (res.support, res.violations, res.occluded)):
                assert torch.equal(a[0], b[k])
        _check(pts, ext, intr, 0.02, name + " without valid")
        assert postprocess.multiview_consistency(dp, ext, intr).occluded is None
    # float64 cameras that are NOT f32 values are rounded to f32 first, as the twin's pack_cams does
    e64, k64 = ext.astype(np.float64) * (1 + 1e-9), intr.astype(np.float64) * (1 + 1e-9)
    _check(twin.unproject64(depth, ext, intr), e64, k64, 0.02, "float64 cameras", valid=valid.astype(np.uint8))
    # one (3, 3) intrinsic for all views
    _check(twin.unproject64(depth, ext, intr), _dev(ext), intr[0], 0.02, "shared intrinsic", valid=valid.astype(np.uint8), frame=1)


def test_full_size_64_views_inside_the_queried_workspace():
    L.require_gpu()
    S, H, W = 64, 518, 518
    pts, ext, intr = twin.device_scene(S, H, W)
    cams = _dev(twin.pack_cams(ext, intr))
    need = ops.consistency_workspace_bytes(S, H, W)
    assert need == 4 * S * H * W
    guard = 4096
    buf = torch.full((need + guard,), 0xA5, device="cuda", dtype=torch.uint8)
    sup, vio, occ = ops.multiview_consistency(pts, cams, 0.02, occluded=True, ws=buf[:need])
    assert bool((buf[need:] == 0xA5).all())                                   # nothing written behind the queried size
    assert sup.shape == (S, H, W) and sup.dtype == torch.int16
    hp, hc = pts.cpu().numpy(), cams.cpu().numpy()
    zm = twin.zmap(hp, hc, 1e-3)
    assert np.array_equal(np.isnan(zm), np.isnan(buf[:need].view(torch.float32).reshape(S, H, W).cpu().numpy()))
    want = twin.count_pixels(hp[37].reshape(-1, 3), ~np.isnan(zm[37].reshape(-1)), 37, zm, hc, 0.02, 1e-3)
    _same((sup[37].reshape(-1), vio[37].reshape(-1), occ[37].reshape(-1)), want, "64 views, frame 37")
    assert want[0].max() >= 8 and want[1].max() >= 3 and want[2].max() >= 1    # many views agree; the floaters are seen through
    # frame=37 through the public entry is that row
    one = postprocess.multiview_consistency(pts, ext, intr, frame=37, return_occluded=True)
    assert torch.equal(one.support[0], sup[37]) and torch.equal(one.violations[0], vio[37]) and torch.equal(one.occluded[0], occ[37])
    # 4 096 seeded source pixels of the other views
    rng = np.random.default_rng(1)
    views, pix = rng.integers(0, S, 4096), rng.integers(0, H * W, 4096)
    hs, hv, ho = (a.reshape(S, H * W).cpu().numpy() for a in (sup, vio, occ))
    for i in np.unique(views):
        q = pix[views == i]
        want = twin.count_pixels(hp[i].reshape(-1, 3)[q], ~np.isnan(zm[i].reshape(-1)[q]), int(i), zm, hc, 0.02, 1e-3)
        for g, w, what in zip((hs[i, q], hv[i, q], ho[i, q]), want, ("support", "violations", "occluded")):
            assert g.tobytes() == w.tobytes(), (int(i), what)


def _predictions(seed=0):
    """A prediction dict from the infinigen fixture: ground-truth depth, the fixture's cameras, the four frames, a seeded confidence
    map; world_points is a second, slightly different point map (depth x 1.001) so that the two prediction modes differ."""
    from PIL import Image
    ext, intr, depth, valid = _real()
    S, H, W = depth.shape
    rng = np.random.default_rng(seed)
    img = np.stack([np.asarray(Image.open(os.path.join(REAL, "infinigen_%d.png" % i)).convert("RGB"), F) / F(255) for i in range(S)])
    assert img.shape == (S, H, W, 3)
    conf = (1.0 + 4.0 * rng.random((S, H, W))).astype(F)
    pred = {"images": _dev(img.transpose(0, 3, 1, 2))[None], "depth": _dev(depth)[None, ..., None], "depth_conf": _dev(conf)[None],
            "world_points_conf": _dev(conf[:, ::-1].copy())[None], "extrinsic": _dev(ext)[None], "intrinsic": _dev(intr)[None],
            "world_points_from_depth": _dev(twin.unproject64(depth, ext, intr))[None],
            "world_points": _dev(twin.unproject64(depth * F(1.001), ext, intr))[None]}
    return pred, _dev(valid)


def test_pipeline_keep_mask_selects_rows_of_the_unmasked_cloud(tmp_path):
    L.require_gpu()
    pred, valid = _predictions()
    S, H, W = valid.shape
    for mode in ("Predicted Pointmap", "Depthmap and Camera Branch"):
        res = postprocess.prediction_consistency(pred, prediction_mode=mode, valid=valid)
        key = "world_points" if "Pointmap" in mode else "world_points_from_depth"
        ref = postprocess.multiview_consistency(pred[key][0], pred["extrinsic"][0], pred["intrinsic"][0], valid=valid)
        assert torch.equal(res.support, ref.support) and torch.equal(res.violations, ref.violations)
        mask = postprocess.consistency_mask(res)
        assert mask.shape == (S, H, W) and mask.dtype == torch.bool and 0.3 < float(mask.float().mean()) < 0.95
        for conf_thres in (0.0, 50.0):
            for frames in ("all", "1:"):
                kw = dict(conf_thres=conf_thres, prediction_mode=mode, filter_by_frames=frames, return_indices=True, return_conf=True)
                base = postprocess.predictions_to_point_cloud(pred, **kw)
                cloud = postprocess.predictions_to_point_cloud(pred, keep_mask=mask, **kw)
                assert cloud.conf_threshold.cpu().numpy().tobytes() == base.conf_threshold.cpu().numpy().tobytes()
                rows = mask.reshape(-1)[base.indices]
                assert 0 < int(rows.sum()) < len(base) and len(cloud) == int(rows.sum())
                for a, b in ((cloud.points, base.points), (cloud.colors, base.colors), (cloud.indices, base.indices), (cloud.conf, base.conf)):
                    assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b[rows].cpu().numpy().tobytes()
                # scene_scale: the percentile rule (pointcloud_twin.scene_scale) on the kept rows, bit for bit
                want = pctwin.scene_scale(cloud.points.cpu().numpy())
                assert np.asarray(cloud.scene_scale.cpu().numpy(), F).tobytes() == np.asarray(want, F).tobytes()
                # keep_mask=None is the path without it
                same = postprocess.predictions_to_point_cloud(pred, keep_mask=None, **kw)
                assert torch.equal(same.points, base.points) and torch.equal(same.indices, base.indices)
        none = postprocess.predictions_to_point_cloud(pred, prediction_mode=mode, keep_mask=torch.zeros_like(mask), conf_thres=0.0)
        assert len(none) == 0
    # the kept cloud goes on through the voxel grid and the GLB writer unchanged
    cloud = postprocess.predictions_to_point_cloud(pred, keep_mask=mask, return_conf=True)
    small = postprocess.voxel_downsample(cloud, rel_size=0.01, conf=cloud.conf)
    assert 0 < len(small) < len(cloud)
    path = str(tmp_path / "kept.glb")
    postprocess.write_glb(path, small)
    assert os.path.getsize(path) > 12 + 15 * len(small) and open(path, "rb").read(4) == b"glTF"
