"""Point-cloud rendering, host side: the numpy twin (tests/render_twin.py) on hand-made clouds and on a projection case whose every
intermediate is exact in float32, the C ABI without a device (struct layout, the workspace query, argument checks that return before
any HIP call), orbit_cameras, write_png and the Python API's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import render_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32
BG = (9, 8, 7)


def _cam(fx=4.0, fy=4.0, cx=2.0, cy=2.0, t=(0.0, 0.0, 0.0), R=None):
    e = np.zeros((3, 4))
    e[:, :3] = np.eye(3) if R is None else R
    e[:, 3] = t
    return twin.pack_cams(e[None], np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))


def _render(pts, H=5, W=5, r=0, near=1e-3, cam=None, col=None):
    pts = np.asarray(pts, F).reshape(-1, 3)
    col = (np.arange(3 * len(pts)).reshape(-1, 3) % 200 + 10).astype(np.uint8) if col is None else col
    rgb, depth, index = twin.render(pts, col, _cam() if cam is None else cam, H, W, r, near, BG)
    assert rgb.dtype == np.uint8 and depth.dtype == F and index.dtype == np.int64
    assert rgb.shape == (1, H, W, 3) and depth.shape == (1, H, W) and index.shape == (1, H, W)
    hit = index >= 0
    assert np.array_equal(rgb[hit], col[index[hit]]) and np.all(rgb[~hit] == np.array(BG, np.uint8))
    assert np.all(depth[~hit] == 0) and np.all(depth[hit] > 0)
    return rgb[0], depth[0], index[0]


def test_twin_nearest_point_wins_and_ties_go_to_the_smaller_index():
    # all three project to pixel (2, 2): x / z = 0 -> u = floor(0 * 4 + 2 + 0.5) = 2
    _, depth, index = _render([[0, 0, 3.0], [0, 0, 2.0], [0, 0, 2.5]])
    assert index[2, 2] == 1 and depth[2, 2] == F(2.0) and (index >= 0).sum() == 1
    _, depth, index = _render([[0, 0, 3.0], [0, 0, 2.0], [0, 0, 2.0], [0, 0, 2.0]])
    assert index[2, 2] == 1 and depth[2, 2] == F(2.0)
    # depth is compared, not distance: the farther-off-axis point with the smaller z wins
    _, _, index = _render([[0.0, 0.0, 1.0], [0.05, 0.05, 0.99]])
    assert index[2, 2] == 1


def test_twin_culls_behind_near_and_non_finite():
    pts = [[0, 0, -1.0], [0, 0, 0.0], [0, 0, 0.5], [0, 0, 0.25], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.nan], [0, 0, np.inf],
           [-np.inf, 0, 1], [1e30, 1e30, 1.0]]
    _, _, index = _render(pts, near=0.5)                                   # zc > near is strict: 0.5 itself is culled
    assert (index >= 0).sum() == 0
    _, depth, index = _render(pts, near=0.25)
    assert index[2, 2] == 2 and depth[2, 2] == F(0.5) and (index >= 0).sum() == 1
    # a camera translation that overflows the camera coordinates culls the point (inf is not finite)
    _, _, index = _render([[3e38, 0, 1.0]], cam=_cam(t=(3e38, 0, 0)))
    assert (index >= 0).sum() == 0


def test_twin_radius_zero_paints_one_pixel_and_empty_pixels():
    rgb, depth, index = _render([[0.25, -0.25, 1.0]], r=0)                 # u = floor(1 + 2 + .5) = 3, w = floor(-1 + 2 + .5) = 1
    assert np.argwhere(index >= 0).tolist() == [[1, 3]]
    assert rgb[0, 0].tolist() == list(BG) and depth[0, 0] == 0 and index[0, 0] == -1
    rgb, depth, index = _render(np.zeros((0, 3)))
    assert np.all(index == -1) and np.all(depth == 0) and np.all(rgb == np.array(BG, np.uint8))


def test_twin_splat_centred_outside_the_frame_paints_its_inside_part():
    # u = 4 * (x / 1) + 2 + .5 floored: x = 1.0 -> u = 6 = W - 1 + 2; y = -1 -> w = -2
    _, _, index = _render([[1.0, -1.0, 1.0]], r=2)
    assert np.argwhere(index >= 0).tolist() == [[0, 4]]                    # only the corner pixel of the 5 x 5 square is inside
    _, _, index = _render([[1.0, -1.0, 1.0]], r=1)                         # one pixel too far for r = 1
    assert (index >= 0).sum() == 0
    _, _, index = _render([[1.25, 0.0, 1.0]], r=2)                         # u = 7 > W - 1 + r
    assert (index >= 0).sum() == 0
    _, _, index = _render([[-1.0, 0.0, 1.0]], r=2)                         # u = -2: columns 0 of rows 0 .. 4
    assert np.argwhere(index >= 0).tolist() == [[y, 0] for y in range(5)]
    _, _, index = _render([[0.0, 0.0, 1.0]], r=8)                          # a splat larger than the image covers it
    assert np.all(index == 0)


def test_twin_pinned_projection_with_exact_intermediates():
    """z in {1, 2, 4}, fx = fy = 4, cx = 3, cy = 2, coordinates multiples of 1/4: every product, quotient and sum is exact in f32,
    so the pixels can be written down by hand: u = floor(4 x / z + 3.5), w = floor(4 y / z + 2.5)."""
    cam = _cam(fx=4.0, fy=4.0, cx=3.0, cy=2.0)
    pts = np.array([[0.0, 0.0, 1.0],        # (3, 2)
                    [0.5, 0.25, 1.0],       # (5, 3)
                    [-0.75, -0.5, 1.0],     # (0, 0)
                    [1.0, 1.0, 2.0],        # (5, 4)
                    [1.0, 0.5, 2.0],        # (5, 3): behind point 1 (z = 1), loses
                    [-3.0, 2.0, 4.0],       # (0, 4)
                    [0.25, 0.0, 2.0],       # 4 * 0.125 + 3.5 = 4.0 -> (4, 2): a projection exactly on a pixel boundary goes up
                    [4.0, 0.0, 4.0],        # u = 7 = W: outside at r = 0
                    [0.0, -1.0, 1.0]], F)   # w = floor(-1.5) = -2: outside
    _, depth, index = _render(pts, H=5, W=7, r=0, cam=cam)
    want = np.full((5, 7), -1, np.int64)
    for i, (u, w) in {0: (3, 2), 1: (5, 3), 2: (0, 0), 3: (5, 4), 5: (0, 4), 6: (4, 2)}.items():
        want[w, u] = i
    assert np.array_equal(index, want)
    assert depth[2, 3] == 1 and depth[4, 5] == 2 and depth[4, 0] == 4 and depth[3, 5] == 1
    # the same cloud seen by a camera moved by t = (0, 0, 1) along z with the axes x -> y -> x swapped: yc = x, xc = y, zc = z + 1
    R = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    _, depth, index = _render([[1.0, 0.5, 1.0], [0.0, 0.0, 3.0]], H=5, W=7, r=0, cam=_cam(4.0, 4.0, 3.0, 2.0, t=(0, 0, 1.0), R=R))
    assert np.argwhere(index >= 0).tolist() == [[2, 3], [4, 4]]            # point 1 at (3, 2) depth 4; point 0: u = 4 * .5 / 2 + 3.5 -> 4, w = 4 / 2 + 2.5 -> 4
    assert index[4, 4] == 0 and depth[4, 4] == 2 and index[2, 3] == 1 and depth[2, 3] == 4


def test_twin_views_are_independent_and_radius_grows_the_splat():
    cams = np.concatenate([_cam(), _cam(t=(0.25, 0, 0)), _cam(t=(0, 0, -2.0))])
    pts = np.array([[0, 0, 1.0]], F)
    col = np.array([[1, 2, 3]], np.uint8)
    rgb, depth, index = twin.render(pts, col, cams, 5, 5, 1, 1e-3, BG)
    assert (index[0] >= 0).sum() == 9 and np.argwhere(index[0] >= 0).min(0).tolist() == [1, 1]
    assert np.argwhere(index[1] >= 0).min(0).tolist() == [1, 2]            # shifted one pixel to the right
    assert (index[2] >= 0).sum() == 0 and np.all(rgb[2] == np.array(BG, np.uint8))     # behind the third camera
    assert np.all(depth[0][index[0] >= 0] == 1)


def test_ctypes_struct_layout_matches_c_render():
    enums, _ = abi_layout.check({"ovg_render_params": L.RenderParams}, ["OVG_RENDER_MAX_RADIUS", "OVG_RENDER_NO_PREREAD", "OVG_ABI_VERSION"])
    assert enums == [L.RENDER_MAX_RADIUS, L.RENDER_NO_PREREAD, L.ABI_VERSION]
    assert L.ABI_VERSION == 13
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+ovg_render_workspace_bytes\s*\(\s*int32_t\s+V,\s*int32_t\s+H,\s*int32_t\s+W\s*\)\s*;", text)
    assert re.search(r"int\s+ovg_render_points\s*\(\s*const\s+ovg_render_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+OVG_ABI_VERSION\s+13\b", text)
    assert "ovg_render_points" in L.SYMBOLS and "ovg_render_workspace_bytes" in L.SYMBOLS


def test_render_workspace_query_and_argument_validation_without_gpu():
    lib = L.load()
    assert lib.ovg_abi_version() == 13
    q = lib.ovg_render_workspace_bytes
    for V, H, W in ((1, 1, 1), (1, 1, 2), (3, 192, 256), (64, 518, 518), (1, 3, 5), (7, 1, 9), (1, 46340, 46340)):
        assert q(V, H, W) == (8 * V * H * W + 15) // 16 * 16, (V, H, W)
    assert q(1, 1, 1) == 16 and q(1, 3, 5) == 128 and q(64, 518, 518) == 8 * 64 * 518 * 518
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3), (2, 1 << 15, 1 << 15), (1, 1 << 16, 1 << 15),
                (8005, 518, 518), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        assert q(*bad) == -1, bad
    assert q(8003, 518, 518) > 0                                           # 8003 * 518^2 < 2^31 <= 8004 * 518^2
    assert q(8004, 518, 518) == -1

    big = 1 << 40                                                          # fake, never dereferenced: every call below fails its checks

    def run(**kw):
        p = L.RenderParams(points=big, colors=big, n=4096, cams=big, V=2, H=16, W=24, radius=1, near=1e-3, ws=big, ws_bytes=q(2, 16, 24),
                           out_rgb=big, out_depth=big, out_index=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_render_points(ctypes.byref(p), None)

    assert lib.ovg_render_points(None, None) == -1
    for bad in (dict(points=None), dict(colors=None), dict(cams=None), dict(ws=None), dict(out_rgb=None), dict(n=-1), dict(n=1 << 32),
                dict(n=(1 << 32) + 7), dict(V=0), dict(H=0), dict(W=0), dict(V=-1), dict(H=-5), dict(W=-1),
                dict(V=1 << 15, H=1 << 8, W=1 << 8, ws_bytes=1 << 50), dict(V=1 << 20, H=1 << 20, W=1 << 20, ws_bytes=1 << 62),
                dict(radius=-1), dict(radius=9), dict(radius=1 << 20),
                dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(near=-0.0),
                dict(ws_bytes=q(2, 16, 24) - 1), dict(ws_bytes=0), dict(ws_bytes=-8), dict(ws=big + 8), dict(flags=2), dict(flags=-1),
                dict(n=0, cams=None), dict(n=0, radius=9)):
        assert run(**bad) == -1, bad


class _Cloud:
    def __init__(self, M=10, seed=0):
        rng = np.random.default_rng(seed)
        self.points = torch.from_numpy(rng.standard_normal((M, 3)).astype(F))
        self.colors = torch.from_numpy(rng.integers(0, 256, (M, 3)).astype(np.uint8))
        self.indices = None


def test_render_point_cloud_arguments_and_cpu_tensors():
    cloud = _Cloud()
    E, K = np.eye(4)[:3][None], np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]])
    good = dict(extrinsic=E, intrinsic=K, size=(48, 64))
    for kw in (dict(size=(0, 64)), dict(size=(48, -1)), dict(size=(48,)), dict(size=48), dict(size=(48.5, 64)), dict(size=(48, 64, 3)),
               dict(point_radius=-1), dict(point_radius=9), dict(point_radius=1.5), dict(point_radius=True),
               dict(near=0.0), dict(near=-1e-3), dict(near=float("nan")), dict(near=float("inf")), dict(near=1e-60), dict(near="x"),
               dict(background=(255, 255)), dict(background=(0, 0, 256)), dict(background=(-1, 0, 0)), dict(background=(0.5, 0, 0)),
               dict(extrinsic=np.eye(4)[None]), dict(extrinsic=np.zeros((0, 3, 4))), dict(intrinsic=np.zeros((2, 3, 3))),
               dict(intrinsic=np.zeros((3, 4))), dict(extrinsic=np.zeros((9000, 3, 4)), size=(518, 518))):
        with pytest.raises(ValueError):
            postprocess.render_point_cloud(cloud, **dict(good, **kw))
    for kw in (dict(), dict(point_radius=0), dict(extrinsic=E[0]), dict(extrinsic=torch.from_numpy(E), intrinsic=K.tolist()),
               dict(return_index=True, return_depth=False)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            postprocess.render_point_cloud(cloud, **dict(good, **kw))      # CPU tensors: no fallback
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.cloud_centre(cloud)
    r = postprocess.RenderResult(1)
    assert r.rgb == 1 and r.depth is None and r.index is None


def _rigid(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.concatenate([q, rng.standard_normal((3, 1)) * 3.0], axis=1)


def test_orbit_cameras_is_a_rigid_circle_about_the_centre():
    """1e-12 and 1e-9 are float64 round-off for a product of four 4 x 4 matrices of entries of order 1 .. 10 (eps = 2.2e-16)."""
    for seed, n, axis in ((0, 8, None), (1, 5, (0.0, 0.0, 2.0)), (2, 1, None), (3, 12, (1.0, -2.0, 0.5))):
        E0 = _rigid(seed)
        c = np.random.default_rng(100 + seed).standard_normal(3) * 2.0
        E = postprocess.orbit_cameras(E0, c, n, axis=axis)
        assert E.shape == (n, 3, 4) and E.dtype == np.float64
        assert np.abs(E[0] - E0).max() <= 1e-12
        seen0 = E0[:, :3] @ c + E0[:, 3]
        centre0 = -E0[:, :3].T @ E0[:, 3]
        a = -E0[1, :3] if axis is None else np.asarray(axis) / np.linalg.norm(axis)
        for k in range(n):
            R, t = E[k][:, :3], E[k][:, 3]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
            cam_centre = -R.T @ t
            assert abs(np.linalg.norm(cam_centre - c) - np.linalg.norm(centre0 - c)) <= 1e-9
            assert np.abs((R @ c + t) - seen0).max() <= 1e-9                # the centre stays at one camera-frame point
            # the camera centre moved by the angle 2 pi k / n about the axis through c: its height along the axis is kept ...
            assert abs((cam_centre - c) @ a - (centre0 - c) @ a) <= 1e-9
            # ... and its part across the axis turned by exactly that angle (right-handed about `a`)
            p0 = (centre0 - c) - ((centre0 - c) @ a) * a
            pk = (cam_centre - c) - ((cam_centre - c) @ a) * a
            th = 2.0 * np.pi * k / n
            want = np.cos(th) * p0 + np.sin(th) * np.cross(a, p0)
            assert np.abs(pk - want).max() <= 1e-9
        if n > 2:
            assert np.abs(E[1] - E0).max() > 1e-3                          # the cameras do move
    t = postprocess.orbit_cameras(torch.from_numpy(_rigid(0)), torch.zeros(3), 3)
    assert isinstance(t, np.ndarray) and t.shape == (3, 3, 4)
    for bad in (dict(n=0), dict(n=-2), dict(n=2.5), dict(n=4, axis=(0, 0, 0)), dict(n=4, axis=(np.nan, 0, 1))):
        with pytest.raises(ValueError):
            postprocess.orbit_cameras(_rigid(0), np.zeros(3), **bad)


def test_write_png_round_trips_byte_for_byte(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    for name, src in (("a.png", img), ("t.png", torch.from_numpy(img)), ("v.png", torch.from_numpy(img)[::2, 1:])):
        path = str(tmp_path / name)
        postprocess.write_png(path, src)
        with Image.open(path) as im:
            assert im.format == "PNG" and im.mode == "RGB"
            back = np.asarray(im)
        want = src.numpy() if isinstance(src, torch.Tensor) else src
        assert back.dtype == np.uint8 and back.shape == want.shape and back.tobytes() == np.ascontiguousarray(want).tobytes()
    for bad in (img[:, :, 0], img.astype(np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((2, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            postprocess.write_png(str(tmp_path / "bad.png"), bad)
