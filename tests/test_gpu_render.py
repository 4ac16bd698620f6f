"""ovg_render_points / postprocess.render_point_cloud on the device against tests/render_twin.py: images, depth maps and index maps
bit for bit -- a random cloud with ties, non-finite rows, points behind the cameras and huge coordinates; real selections of the golden
point-cloud cases from their own cameras and from an orbit; the edge sizes; determinism; and the 64 x 518^2 cloud inside the queried
workspace."""
import json
import os

import numpy as np
import pytest
import torch

import common
import render_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
FULL = 64 * 518 * 518
BG = (12, 200, 77)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cloud(pts, col=None, indices=None):
    pts = np.asarray(pts, F).reshape(-1, 3)
    if col is None:
        col = (np.arange(3 * len(pts), dtype=np.int64).reshape(-1, 3) * 7 % 256).astype(np.uint8)
    return postprocess.PointCloud(_dev(pts), _dev(col), torch.zeros((), device="cuda"), torch.ones((), device="cuda"), np.eye(4),
                                  torch.eye(4, device="cuda")[:3][None], None if indices is None else _dev(indices))


def _intrinsic(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def _check(cloud, ext, intr, size, r, name, near=1e-3, bg=BG):
    """Render on the device and with the twin; rgb, depth and index must agree byte for byte. -> (device result, twin result)."""
    H, W = size
    res = postprocess.render_point_cloud(cloud, ext, intr, size, point_radius=r, near=near, background=bg, return_depth=True,
                                         return_index=True)
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    cams = twin.pack_cams(host(ext), host(intr))
    want = twin.render(cloud.points.cpu().numpy(), cloud.colors.cpu().numpy(), cams, H, W, r, near, bg)
    got = (res.rgb.cpu().numpy(), res.depth.cpu().numpy(), res.index.cpu().numpy())
    V = len(cams)
    assert got[0].shape == (V, H, W, 3) and got[1].shape == (V, H, W) and got[2].shape == (V, H, W), name
    for g, w, what in zip(got, want, ("rgb", "depth", "index")):
        assert g.dtype == w.dtype, (name, what)
        assert g.tobytes() == w.tobytes(), (name, what, int((g != w).sum()))
    return res, want


def random_scene(n=300_000, seed=0):
    """300 000 points N(0, (1, 1, 0.5)) around z = 3 seen by three cameras (identity, shifted in x, moved back along z), with exact
    duplicates (depth ties), NaN / inf rows, points behind the cameras and coordinates near 1e30."""
    rng = np.random.default_rng(seed)
    pts = (rng.standard_normal((n, 3)) * [1.0, 1.0, 0.5] + [0.0, 0.0, 3.0]).astype(F)
    pts[100_000:150_000] = pts[:50_000]                                   # exact duplicates: equal depth on one pixel
    pts[150_000:160_000, 2] = pts[150_000:160_000, 2].round(1)            # many points on a few depth planes
    pts[::1000] = np.nan
    rows = np.arange(1, n, 1000)
    pts[rows, rng.integers(0, 3, len(rows))] = np.inf
    pts[2::1000, 0] = -np.inf
    pts[5::997, 2] = -F(1.0) - pts[5::997, 2]                             # behind the cameras
    pts[7::991] *= F(1e30)
    pts[11::983, 2] = F(1e-4)                                             # in front, but nearer than the near plane
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    ext = np.tile(np.eye(4)[:3], (3, 1, 1))
    ext[1, 0, 3], ext[2, 2, 3] = 0.3, -1.0
    return pts, col, ext, _intrinsic(200.0, 128.0, 96.0)


def test_random_cloud_matches_twin_bit_exactly():
    L.require_gpu()
    pts, col, ext, intr = random_scene()
    H, W = 192, 256
    cloud = _cloud(pts, col)
    for r in (0, 1, 3):
        _, (rgb, depth, index) = _check(cloud, ext, intr, (H, W), r, ("random", r))
        if r == 0:
            # the comparison is not empty: in the twin's own output every view has >= 25 % of its pixels hit and >= 25 % of its
            # in-frame points lose a depth test
            cams = twin.pack_cams(ext, intr)
            for v in range(3):
                hit = int((index[v] >= 0).sum())
                inframe = len(twin.project(pts, cams[v], H, W, 0, 1e-3)[0])
                print("view %d: %d of %d pixels hit, %d points in frame, %d lose" % (v, hit, H * W, inframe, inframe - hit))
                assert hit >= 0.25 * H * W and hit < H * W and inframe - hit >= 0.25 * inframe
    # tilted cameras and non-square pixels, device-resident camera tensors, a (V, 3, 3) intrinsic
    ext2 = postprocess.orbit_cameras(ext[1], (0.0, 0.0, 3.0), 12, axis=(0.3, 1.0, 0.1))[[1, 2, 11]].astype(F)      # 30, 60, -30 degrees
    intr2 = np.stack([_intrinsic(150.0 + 40 * v, 100.0 + 9.25 * v, 80.0 - 3.5 * v) for v in range(3)])
    intr2[:, 1, 1] *= 1.25
    _check(cloud, _dev(ext2), _dev(intr2.astype(F)), (H, W), 1, "tilted")
    _check(cloud, ext2.astype(np.float64) + 1e-9, intr2, (H, W), 2, "float64 cameras are rounded to f32 first")


def test_on_real_selections_of_the_golden_cases():
    L.require_gpu()
    g = dict(np.load(os.path.join(common.GOLD, "pointcloud.npz")))
    cases = json.loads(str(g["cases"]))
    used = reprojected = 0
    for i, case in enumerate(cases):
        if case["empty"]:
            continue
        m = case["map"]
        depth_mode = case["mode"] == "Predicted Depth"
        images = _dev(g[m + "_images"])[None]
        S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
        if depth_mode:
            pred = {"world_points_from_depth": _dev(g[m + "_world_points_from_depth"].astype(F))[None], "depth_conf": _dev(g[m + "_depth_conf"])[None],
                    "images": images, "extrinsic": _dev(g[m + "_extrinsic"])[None]}
            # the predicted cameras: intrinsics decoded from the pose encoding at the map size
            intr = postprocess.pose_encoding_to_extri_intri(_dev(g[m + "_pose_enc"])[None], (H, W))[1][0]
        else:
            pred = {"world_points": _dev(g[m + "_world_points"])[None], "world_points_conf": _dev(g[m + "_world_points_conf"])[None],
                    "images": images, "extrinsic": _dev(g[m + "_extrinsic"])[None]}
            intr = _intrinsic(float(W), (W - 1) / 2.0, (H - 1) / 2.0)      # these maps carry no intrinsics: a 53-degree pinhole
        sky = g.get("c%d_sky" % i)
        kw = dict(conf_thres=case["conf_thres"], filter_by_frames=case["filter_by_frames"], mask_black_bg=case["mask_black_bg"],
                  mask_white_bg=case["mask_white_bg"], prediction_mode=case["mode"], sky_mask=None if sky is None else _dev(sky))
        cloud = postprocess.predictions_to_point_cloud(pred, return_indices=True, **kw)
        assert len(cloud) == case["n_kept"]
        ext = pred["extrinsic"][0]
        for r in (0, 2):
            res, (_, _, index) = _check(cloud, ext, intr, (H, W), r, (case["name"], "own cameras", r))
            if depth_mode and r == 0 and cloud.extrinsic.shape[0] == 1:
                # one frame of a depth-mode cloud seen by its own camera: every kept pixel shows its own point and nothing else is
                # hit (the f64 un-projection rounded to f32 and the f32 projection are good to ~1e-4 of a pixel; a centre is 0.5 from the edge)
                frame = int(cloud.indices[0]) // (H * W)
                local = cloud.indices.cpu().numpy() - frame * H * W
                want = np.full(H * W, -1, np.int64)
                want[local] = np.arange(len(local))
                assert np.array_equal(index[frame].reshape(-1), want), case["name"]
                # index names positions in the cloud; composed with cloud.indices it names pixels of the maps
                shown = res.index[frame][res.index[frame] >= 0]
                assert torch.equal(cloud.indices[shown], torch.sort(cloud.indices).values)
                reprojected += 1
        finite = torch.isfinite(cloud.points).all(dim=1)
        if int(finite.sum()) == len(cloud):
            centre = postprocess.cloud_centre(cloud)
            med = np.median(cloud.points.cpu().numpy().astype(np.float64), axis=0)
            # numpy's float32 linear percentile (the rule ovg_percentile restates), not the float64 one
            assert np.array_equal(centre.cpu().numpy(), np.percentile(cloud.points.cpu().numpy(), 50, axis=0)), case["name"]
            assert np.abs(centre.cpu().numpy() - med).max() <= 1e-5 * max(1.0, np.abs(med).max())
        else:
            centre = torch.tensor([0.0, 0.0, 5.0])
        orbit = postprocess.orbit_cameras(ext[0], centre.cpu(), 4)
        _check(cloud, orbit, intr[0] if depth_mode else intr, (H, W), 1, (case["name"], "orbit"))      # the first camera's intrinsics
        used += 1
    assert used >= 10 and reprojected >= 1


def test_edge_sizes():
    L.require_gpu()
    E = np.eye(4)[:3][None]
    K = _intrinsic(16.0, 8.0, 6.0)
    empty = _cloud(np.zeros((0, 3), F))
    res, _ = _check(empty, E, K, (12, 16), 1, "M = 0")
    assert bool((res.index == -1).all()) and bool((res.depth == 0).all())
    assert bool((res.rgb == torch.tensor(BG, device="cuda", dtype=torch.uint8)).all())
    plain = postprocess.render_point_cloud(empty, E, K, (12, 16), return_depth=False)
    assert plain.depth is None and plain.index is None and bool((plain.rgb == 255).all())      # the default background is white
    one = _cloud([[0.25, -0.125, 2.0]])                                   # u = floor(2 + 8.5) = 10, w = floor(-1 + 6.5) = 5
    for r in (0, 1, 8):
        res, _ = _check(one, E, K, (12, 16), r, ("M = 1", r))
        hit = torch.nonzero(res.index[0] >= 0)
        assert hit.min(0).values.tolist() == [max(5 - r, 0), max(10 - r, 0)] and hit.max(0).values.tolist() == [min(5 + r, 11), min(10 + r, 15)]
        assert len(hit) == (hit.max(0).values - hit.min(0).values + 1).prod()
    rng = np.random.default_rng(3)
    pts = (rng.standard_normal((5000, 3)) * [0.4, 0.4, 0.3] + [0, 0, 2.0]).astype(F)
    cloud = _cloud(pts)
    _check(cloud, E, K, (12, 16), 2, "V = 1")
    for r in (0, 3):
        res, _ = _check(cloud, E, _intrinsic(16.0, 0.0, 0.0), (1, 1), r, ("1 x 1 image", r))
        assert int(res.index[0, 0, 0]) >= 0
    _check(cloud, E, K, (1, 16), 1, "one row")
    _check(cloud, E, K, (12, 1), 1, "one column")
    _check(cloud, np.tile(E, (5, 1, 1)), K, (3, 5), 1, "odd pixel count: the last 16 bytes of the workspace are half used")
    # r = 8 at the image corners: splats centred up to 8 pixels outside each corner paint only their inside part
    H, W = 24, 32
    corners = []
    for u in (-8, -3, 0, W - 1, W + 2, W + 7):
        for w in (-8, -1, 0, H - 1, H + 4, H + 7):
            corners.append([(u - 8.0) / 16.0 * 2.0, (w - 6.0) / 16.0 * 2.0, 2.0])     # exact: (u - cx) / f * z
    corners = np.asarray(corners, F)
    res, (_, _, index) = _check(_cloud(corners), E, K, (H, W), 8, "r = 8 at the corners")
    # all on one depth plane: ties go to the smaller index, and the middle columns are out of every splat's reach
    assert index[0, 0, 0] == 0 and index[0, H - 1, W - 1] >= 0 and (index[0, :, 9:23] < 0).all()
    _check(_cloud(corners), E, K, (H, W), 7, "r = 7: the outermost centres no longer reach the frame")
    with pytest.raises(ValueError):
        postprocess.render_point_cloud(cloud, E, K, (12, 16), point_radius=9)


def test_two_runs_give_identical_bytes_and_index_properties():
    L.require_gpu()
    pts, col, ext, intr = random_scene(seed=4)
    cloud = _cloud(pts, col, indices=np.arange(len(pts), dtype=np.int64)[::-1].copy())
    near = 0.5
    a = postprocess.render_point_cloud(cloud, ext, intr, (192, 256), point_radius=1, near=near, background=BG, return_index=True)
    b = postprocess.render_point_cloud(cloud, ext, intr, (192, 256), point_radius=1, near=near, background=BG, return_index=True)
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.index, b.index)
    hit = a.index >= 0
    assert a.index.dtype == torch.int64 and int(a.index.max()) < len(cloud) and int(a.index.min()) >= -1
    assert torch.equal(a.rgb[hit], cloud.colors[a.index[hit]])             # positions in the cloud, although it carries `indices`
    assert bool((a.rgb[~hit] == torch.tensor(BG, device="cuda", dtype=torch.uint8)).all())
    assert torch.equal(a.depth > near, hit) and bool((a.depth[~hit] == 0).all())
    c = postprocess.render_point_cloud(cloud, ext, intr, (192, 256), point_radius=1, near=near, background=BG, return_depth=False)
    assert c.depth is None and c.index is None and torch.equal(c.rgb, a.rgb)
    # the lab switch of the probe: without the plain pre-read the images are the same
    cams = _dev(twin.pack_cams(ext, intr))
    rgb, dep, idx = ops.render_points(cloud.points, cloud.colors, cams, 192, 256, radius=1, near=near, background=BG, index=True,
                                      flags=L.RENDER_NO_PREREAD)
    assert torch.equal(rgb, a.rgb) and torch.equal(dep, a.depth) and torch.equal(idx, a.index)


def test_full_size_within_queried_workspace_and_exact():
    """64 x 518^2 = 17.2 M seeded points into one 518^2 view at r = 0 through the raw entry, with a workspace of exactly the queried
    size between two guard regions, compared with the twin (one np.minimum.at over <= 17.2 M keys: 0.6 s of host time where it was measured, 2 s on a slower host)."""
    L.require_gpu()
    n, H, W = FULL, 518, 518
    gen = torch.Generator(device="cuda").manual_seed(11)
    pts = torch.randn(n, 3, device="cuda", generator=gen) * torch.tensor([1.0, 1.0, 0.5], device="cuda") + torch.tensor([0.0, 0.0, 3.0], device="cuda")
    pts[:, 2] = torch.round(pts[:, 2] * 64.0) / 64.0                       # depth planes 1/64 apart: ties on most pixels
    col = torch.randint(0, 256, (n, 3), device="cuda", generator=gen, dtype=torch.uint8)
    cams = _dev(twin.pack_cams(np.eye(4)[:3][None], _intrinsic(400.0, 258.5, 258.5)))
    need = ops.render_workspace_bytes(1, H, W)
    assert need == 8 * H * W
    guard = 1 << 20
    buf = torch.full((need + 2 * guard,), 0xA5, device="cuda", dtype=torch.uint8)
    rgb, dep, idx = ops.render_points(pts, col, cams, H, W, radius=0, near=1e-3, background=BG, index=True, ws=buf[guard:guard + need])
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())     # nothing outside the queried bytes
    want = twin.render(pts.cpu().numpy(), col.cpu().numpy(), cams.cpu().numpy(), H, W, 0, 1e-3, BG)
    assert (want[2] >= 0).mean() > 0.9
    for g, w, what in zip((rgb, dep, idx), want, ("rgb", "depth", "index")):
        assert g.cpu().numpy().tobytes() == w.tobytes(), what
