"""numpy float32 restatement of the multi-view depth-consistency rule (include/omnivggt_hip.h, ovg_multiview_consistency), the oracle
of the device kernels bit for bit. Elementwise float32 numpy operations round one at a time, which is what the kernels do (no fused
multiply-add). The projection is render_twin.project at radius 0 (its rules 1-4), unchanged:

  1. own depth z[j, q] = ((c6 x + c7 y) + c8 z) + c11, c = cams[j]; pixel (j, q) is usable when valid[j, q] != 0 (if given), z is
     finite and z > near;
  2. a usable source pixel (i, p) is projected into every other view j; the pair is skipped unless the projection passes the
     finiteness / near test, lands on a pixel (w, u) of the frame, and (j, (w, u)) is usable;
  3. d = z[j, (w, u)], band = tol * d, diff = zc - d: |diff| <= band is support, diff < -band a violation, diff > band occluded;
  4. support / violations / occluded int16 [S, H, W] count the views j of each class; unusable sources have all three 0.
"""
import numpy as np

import render_twin as rt

F = np.float32
pack_cams = rt.pack_cams


def zmap(points, cams, near, valid=None):
    """Rule 1: z [S, H, W] float32 with NaN at the pixels that are not usable."""
    points = np.asarray(points, F)
    S, H, W, _ = points.shape
    cams = np.asarray(cams, F).reshape(S, 16)
    z = np.empty((S, H, W), F)
    for s in range(S):
        c = cams[s]
        x, y, zz = points[s, :, :, 0], points[s, :, :, 1], points[s, :, :, 2]
        with np.errstate(all="ignore"):
            d = ((c[6] * x + c[7] * y) + c[8] * zz) + c[11]
            ok = np.isfinite(d) & (d > F(near))
        assert d.dtype == F
        if valid is not None:
            ok &= np.asarray(valid[s]) != 0
        z[s] = np.where(ok, d, F(np.nan))
    return z


def count_pixels(pts, usable, i, zm, cams, tol, near, stats=None):
    """Rules 2-4 for n source pixels of view i: pts [n, 3] their world points, usable [n] bool. -> three int16 arrays [n].
    stats: an optional dict that accumulates the pair counts `pairs` (usable sources x other views), `in_front` (passed the
    finiteness / near test), `in_frame`, `counted` (target usable too), `support`, `violations`, `occluded`."""
    S, H, W = zm.shape
    pts = np.asarray(pts, F).reshape(-1, 3)
    tol = F(tol)
    out = np.zeros((3, len(pts)), np.int64)
    for j in range(S):
        if j == i:
            continue
        sel, px, py, key = rt.project(pts, cams[j], H, W, 0, near)
        zc = (key >> np.uint64(32)).astype(np.uint32).view(F)
        d = zm[j][py, px]
        with np.errstate(all="ignore"):
            ok = usable[sel] & ~np.isnan(d)
            band = tol * d
            diff = zc - d
            assert band.dtype == F and diff.dtype == F
            classes = (ok & (np.abs(diff) <= band), ok & (diff < -band), ok & (diff > band))
        assert int((classes[0].astype(int) + classes[1] + classes[2] != ok).sum()) == 0      # exactly one class per counted pair
        for k, m in enumerate(classes):
            out[k, sel[m]] += 1                                              # sel holds every point at most once
        if stats is not None:
            front = rt.project(pts, cams[j], H, W, 1 << 30, near)[0]
            for name, v in (("pairs", usable.sum()), ("in_front", usable[front].sum()), ("in_frame", usable[sel].sum()),
                            ("counted", ok.sum()), ("support", classes[0].sum()), ("violations", classes[1].sum()),
                            ("occluded", classes[2].sum())):
                stats[name] = stats.get(name, 0) + int(v)
    return tuple(o.astype(np.int16) for o in out)


def consistency(points, cams, tol, near=1e-3, valid=None, sources=None, stats=None):
    """(support, violations, occluded), int16 [len(sources), H, W]; sources: the source views, all S by default. All S views are
    targets either way."""
    points = np.asarray(points, F)
    S, H, W, _ = points.shape
    cams = np.asarray(cams, F).reshape(S, 16)
    zm = zmap(points, cams, near, valid)
    sources = range(S) if sources is None else list(sources)
    out = np.zeros((3, len(sources), H * W), np.int16)
    for r, i in enumerate(sources):
        out[:, r] = count_pixels(points[i].reshape(-1, 3), ~np.isnan(zm[i].reshape(-1)), i, zm, cams, tol, near, stats)
    return tuple(o.reshape(len(sources), H, W) for o in out)


# ---------------------------------------------------------------------------------------------------------------------------------
# Scenes the host and the device tests share (float64 geometry, rounded to float32 once)
# ---------------------------------------------------------------------------------------------------------------------------------

def unproject64(depth, extrinsic, intrinsic):
    """World points [S, H, W, 3] float32 of depth maps [S, H, W]: pixel centres at integer coordinates, camera = ((u - cx) d / fx,
    (v - cy) d / fy, d), world = R^T (camera - t), all in float64 and rounded to float32 at the end."""
    depth = np.asarray(depth, np.float64)
    S, H, W = depth.shape
    ext = np.asarray(extrinsic, np.float64).reshape(S, 3, 4)
    k = np.broadcast_to(np.asarray(intrinsic, np.float64), (S, 3, 3))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((S, H, W, 3), F)
    for s in range(S):
        d = depth[s]
        cam = np.stack([(u - k[s, 0, 2]) * d / k[s, 0, 0], (v - k[s, 1, 2]) * d / k[s, 1, 1], d], -1)
        with np.errstate(all="ignore"):
            out[s] = ((cam - ext[s, :, 3]) @ ext[s, :, :3]).astype(F)
    return out


def perturb_depth(depth, valid, share=0.05, factor=0.7, seed=0):
    """A seeded `share` of the valid pixels moved to `factor` x their depth. -> (depth, moved mask)."""
    rng = np.random.default_rng(seed)
    moved = (rng.random(depth.shape) < share) & valid
    out = depth.copy()
    out[moved] *= F(factor)
    return out, moved


def look_at(eye, target, roll=0.0):
    """World-to-camera (3, 4), float64: z towards the target, x to the right, y down, rolled about the optical axis."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, -1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * x + s * y, -s * x + c * y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1)


def synthetic_scene(S=6, H=70, W=98, seed=0, step_deg=14.0, floaters=0.12, pushed=0.10):
    """S views (S - 1 distinct ones and a repeat of the first) on an orbit (tilted, rolled, non-square pixels) of a unit sphere at the origin inside a backdrop sphere of radius 6:
    both analytic, so the depth maps agree across the views. Then, seeded: floaters (pulled to 0.4 .. 0.8 of their depth), pixels
    pushed back (1.2 .. 1.6), NaN / +-inf rows, coordinates near 1e30, points mirrored behind the cameras, and a valid mask with
    holes. -> (points f32 [S, H, W, 3], extrinsic f64 [S, 3, 4], intrinsic f64 [S, 3, 3], valid u8 [S, H, W])."""
    rng = np.random.default_rng(seed)
    ext, intr = np.empty((S, 3, 4)), np.empty((S, 3, 3))
    depth = np.empty((S, H, W))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for s in range(S):
        a = np.deg2rad(step_deg * (s - (S - 1) / 2) + (150.0 if s == S - 2 else 0.0))   # one view from the far side: its backdrop is behind the others
        eye = np.array([3.0 * np.sin(a), -0.4 + 0.25 * s, -3.0 * np.cos(a)])
        ext[s] = look_at(eye, [0.1 * s - 0.2, 0.0, 0.0], roll=np.deg2rad(6.0 * s - 10.0))
        intr[s] = [[80.0 + 3 * s, 0, W / 2 - 0.5 + s], [0, 65.0 - 2 * s, H / 2 - 0.5 - s], [0, 0, 1]]
        ray = np.stack([(u - intr[s, 0, 2]) / intr[s, 0, 0], (v - intr[s, 1, 2]) / intr[s, 1, 1], np.ones_like(u)], -1)   # camera frame, z = 1
        dirs = ray @ ext[s, :, :3]                                          # world directions, |.| != 1: the parameter is the depth
        aa, bb = (dirs * dirs).sum(-1), (dirs * eye).sum(-1)
        hit = {}
        for r in (1.0, 6.0):
            disc = bb * bb - aa * (eye @ eye - r * r)
            root = np.sqrt(np.maximum(disc, 0.0))
            hit[r] = (np.where(disc > 0, (-bb - root) / aa, np.inf), (-bb + root) / aa)
        depth[s] = np.where(np.isfinite(hit[1.0][0]) & (hit[1.0][0] > 0), hit[1.0][0], hit[6.0][1])
    r = rng.random((S, H, W))
    scale = np.ones((S, H, W))
    scale = np.where(r < floaters, rng.uniform(0.4, 0.8, r.shape), scale)
    scale = np.where((r >= floaters) & (r < floaters + pushed), rng.uniform(1.2, 1.6, r.shape), scale)
    scale = np.where((r >= 0.90) & (r < 0.92), -1.0, scale)                 # mirrored through the camera centre: behind every nearby view
    pts = unproject64(depth * scale, ext, intr)
    pts[(r >= 0.92) & (r < 0.93)] = np.nan
    m = (r >= 0.93) & (r < 0.94)
    pts[m, rng.integers(0, 3, int(m.sum()))] = np.inf
    m = (r >= 0.94) & (r < 0.945)
    pts[m, 0] = -np.inf
    m = (r >= 0.945) & (r < 0.955)
    pts[m] *= F(1e30)
    # the last view repeats the first one, camera and points: its pixels land on themselves with zc == d exactly, the only way to
    # have support at tol = 0 (the valid masks below still differ)
    pts[S - 1], ext[S - 1], intr[S - 1] = pts[0], ext[0], intr[0]
    valid = (rng.random((S, H, W)) >= 0.04).astype(np.uint8)
    valid[:, 20:27, 40:55] = 0                                              # a block hole besides the scattered ones
    return pts, ext, intr, valid


def device_scene(S, H, W, seed=0):
    """A consistent scene made on the device: a unit sphere inside a backdrop sphere of radius 6 seen from S cameras on a circle of
    radius 3 (float64 rays, analytic intersections), with 6 % floaters and 3 % NaN rows. -> (points f32 (S,H,W,3) on the device,
    extrinsic f64 (S,3,4), intrinsic f64 (3,3))."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ext = np.stack([look_at([3.0 * np.sin(a), 0.6 * np.sin(3 * a), -3.0 * np.cos(a)], [0.0, 0.0, 0.0], roll=0.2 * np.sin(a))
                    for a in 2 * np.pi * np.arange(S) / S])
    intr = np.array([[0.9 * W, 0.0, W / 2 - 0.5], [0.0, 0.8 * W, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    v, u = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float64), torch.arange(W, device="cuda", dtype=torch.float64),
                          indexing="ij")
    ray = torch.stack([(u - intr[0, 2]) / intr[0, 0], (v - intr[1, 2]) / intr[1, 1], torch.ones_like(u)], -1)
    out = torch.empty(S, H, W, 3, device="cuda", dtype=torch.float32)
    for s in range(S):
        R, t = torch.from_numpy(ext[s, :, :3]).cuda(), torch.from_numpy(ext[s, :, 3]).cuda()
        eye = -(R.T @ t)
        dirs = ray @ R
        aa, bb, ee = (dirs * dirs).sum(-1), (dirs * eye).sum(-1), float(eye @ eye)
        d1 = bb * bb - aa * (ee - 1.0)
        near_hit = (-bb - d1.clamp_min(0).sqrt()) / aa
        far_hit = (-bb + (bb * bb - aa * (ee - 36.0)).sqrt()) / aa
        depth = torch.where((d1 > 0) & (near_hit > 0), near_hit, far_hit)
        r = torch.rand(H, W, device="cuda", generator=gen)
        depth = torch.where(r < 0.06, depth * (0.4 + 5.0 * r), depth)        # floaters at 0.4 .. 0.7 of the depth
        p = (ray * depth[..., None] - t) @ R
        p[(r >= 0.06) & (r < 0.09)] = float("nan")
        out[s] = p.float()
    return out, ext, intr
