"""Synthetic point maps for the map-geometry tests (a plain helper module): the host test checks on the twin that the scene the GPU
test compares is not trivial, so both must build the same arrays."""
import numpy as np

F = np.float32
NEAR = 1e-3


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pack_cam(R, t, fx, fy, cx, cy):
    """One [16] row as ovg_render_points reads it: world-to-camera rotation row-major, translation, fx, fy, cx, cy."""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), [fx, fy, cx, cy]]).astype(F)


def ray_cast(R, t, fx, fy, cx, cy, H, W, planes, box):
    """World points [H, W, 3] float64 of the nearest hit of every pixel's ray with the planes z = p0 + p1 x + p2 y or the
    axis-aligned box (lo, hi); camera X_c = R X_w + t."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    o = -R.T @ t
    d = d_cam @ R                                                             # R^T d_cam per pixel
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for p0, p1, p2 in planes:
            hit = (p0 + p1 * o[0] + p2 * o[1] - o[2]) / (d[..., 2] - p1 * d[..., 0] - p2 * d[..., 1])
            best = np.where((hit > 0) & (hit < best), hit, best)
        lo, hi = (np.asarray(b, np.float64) for b in box)
        t1, t2 = (lo - o) / d, (hi - o) / d
        enter, leave = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    hit = (enter <= leave) & (enter > 0)
    best = np.where(hit & (enter < best), enter, best)
    return o + best[..., None] * d


def box_scene(H=37, W=53, seed=5):
    """S = 3 views: a near box in front of a gently tilted plane that meets a steep one in a crease, seen by two different cameras, and a third view that repeats the
    first one's points behind a camera that looks the other way (z <= near everywhere). A band of valid = 0 with one live pixel
    inside it, a pixel whose horizontal neighbours are dead, scattered NaN / +-inf coordinates, random colours, a random keep mask.
    -> dict(points [3, H, W, 3] f32, cams [3, 16] f32, valid u8, keep u8, colors u8 [3, H, W, 3], depth [3, H, W] f32)."""
    rng = np.random.default_rng(seed)
    fx = fy = 40.0
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    planes, box = ((4.0, 0.03, 0.02), (5.3, -0.7, 0.0)), ((-0.6, -0.5, 2.0), (0.5, 0.4, 2.6))
    rigs = [(rotation([0, 1, 0], -5.0), np.array([0.8, -0.1, 0.0])),          # to the right of the box, turned towards it: sees its +x side
            (rotation([1, 0.3, 0], 2.0) @ rotation([0, 1, 0], 4.0), np.array([-0.9, 0.5, 0.2]))]
    pts, cams = [], []
    for Rwc, centre in rigs:
        R = Rwc.T                                                            # world-to-camera
        t = -R @ centre
        pts.append(ray_cast(R, t, fx, fy, cx, cy, H, W, planes, box))
        cams.append(pack_cam(R, t, fx, fy, cx, cy))
    back = np.diag([-1.0, 1.0, -1.0]) @ rigs[0][0].T                           # view 0's camera turned round: every depth negated
    pts.append(pts[0].copy())
    cams.append(pack_cam(back, -back @ rigs[0][1], fx, fy, cx, cy))
    points = np.stack(pts).astype(F)
    valid = np.ones((3, H, W), np.uint8)
    valid[:, 20:25, 5:30] = 0                                                # the band, five rows
    valid[:, 22, 12] = 1                                                     # a live pixel inside it: a corner no face can name
    valid[:, 8, 40] = valid[:, 8, 42] = 0                                    # (8, 41) has no usable horizontal neighbour: no normal
    for s in range(2):
        for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan)):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            points[s, y, x, k % 3] = bad
    keep = (rng.uniform(0.0, 1.0, (3, H, W)) < 0.85).astype(np.uint8)
    keep[:, 22, 12] = 1
    colors = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    cams = np.stack(cams)
    with np.errstate(all="ignore"):
        c = cams[:, :, None, None]
        depth = (((c[:, 6] * points[..., 0] + c[:, 7] * points[..., 1]) + c[:, 8] * points[..., 2]) + c[:, 11]).astype(F)
    return dict(points=points, cams=cams, valid=valid, keep=keep, colors=colors, depth=depth)


def prediction_scene(S=2, H=28, W=42, seed=14):
    """What a forward pass returns for S views of the box scene's geometry, without holes: points [S, H, W, 3] f32, extrinsic
    [S, 3, 4] and intrinsic [S, 3, 3] float64, conf [S, H, W] f32 in (1, 3), images [S, 3, H, W] f32 in [0, 1)."""
    rng = np.random.default_rng(seed)
    f, cx, cy = 32.0, (W - 1) / 2.0, (H - 1) / 2.0
    planes, box = ((4.0, 0.03, 0.02),), ((-0.6, -0.5, 2.0), (0.5, 0.4, 2.6))
    pts, ext = [], []
    for k in range(S):
        Rwc, centre = rotation([0.2, 1, 0], 4.0 * k - 3.0), np.array([0.5 * k - 0.3, 0.1 * k, 0.0])
        R = Rwc.T
        t = -R @ centre
        pts.append(ray_cast(R, t, f, f, cx, cy, H, W, planes, box))
        ext.append(np.concatenate([R, t[:, None]], axis=1))
    intrinsic = np.tile(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]]), (S, 1, 1))
    return dict(points=np.stack(pts).astype(F), extrinsic=np.stack(ext), intrinsic=intrinsic,
                conf=rng.uniform(1.0, 3.0, (S, H, W)).astype(F), images=rng.uniform(0.0, 1.0, (S, 3, H, W)).astype(F))


def stacked_views(H, W, seed=0, depths=(1.0, 10.0, 100.0)):
    """S = len(depths) small views of a bumpy fronto-parallel surface at wildly different depths, identity cameras: anything that
    leaks from one view (or from the previous row's end) into another changes a flag, a normal or a face."""
    rng = np.random.default_rng(seed)
    S = len(depths)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pts = np.zeros((S, H, W, 3))
    for s, d in enumerate(depths):
        z = d * (1.0 + 0.01 * rng.uniform(0.0, 1.0, (H, W)) + 0.002 * x)
        pts[s] = np.stack([(x - W / 2) * z / 4, (y - H / 2) * z / 4, z], -1)
    cams = np.stack([pack_cam(np.eye(3), np.zeros(3), 4.0, 4.0, W / 2, H / 2)] * S)
    return pts.astype(F), cams


def random_keep_scene(S=2, H=190, W=180, seed=9, fraction=0.7):
    """A smooth surface over more than 256 workgroups of 256 pixels with an unstructured random keep mask."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pts = np.zeros((S, H, W, 3))
    for s in range(S):
        z = 3.0 + s + 0.3 * np.sin(x / 17.0) * np.cos(y / 13.0)
        pts[s] = np.stack([(x - W / 2) * z / 150, (y - H / 2) * z / 150, z], -1)
    keep = (rng.uniform(0.0, 1.0, (S, H, W)) < fraction).astype(np.uint8)
    return pts.astype(F), keep


def sphere_patch(H=9, W=11, seed=3, radius=50.0, distance=5.0, focal=2000.0):
    """A patch of a sphere seen from outside, through a camera at `distance` from its surface, in a randomly turned world frame whose
    origin is the hit point of the central pixel (so float32 rounds the coordinates at the scale of the patch, not of the scene).
    The radius is large against the pixel pitch: the stencil's O((pitch / radius)^2) deviation from the analytic normal is far below
    1e-6 while the normal itself turns by about 1e-3 across the patch.
    -> world points [1, H, W, 3] float64, the analytic outward normals, cams [1, 16] f32, the camera centre (world)."""
    rng = np.random.default_rng(seed)
    sphere = np.array([0.3, -0.2, distance + radius])                        # in camera coordinates: x right, y down, z forward
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(u - cx) / focal, (v - cy) / focal, np.ones_like(u)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    b = d @ sphere
    hit = b - np.sqrt(b * b - (sphere @ sphere - radius ** 2))               # the near intersection of every ray
    cam_pts = hit[..., None] * d
    Q = rotation(rng.normal(size=3), rng.uniform(20.0, 160.0))               # camera axes -> world axes
    origin = cam_pts[H // 2, W // 2]
    world = (cam_pts - origin) @ Q.T
    normals = ((cam_pts - sphere) / radius) @ Q.T
    return world[None], normals[None], pack_cam(Q.T, origin, focal, focal, cx, cy)[None], -Q @ origin
