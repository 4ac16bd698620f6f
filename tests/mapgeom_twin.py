"""The rules of ovg_map_depth / ovg_map_normals / ovg_map_edges / ovg_map_triangulate (include/omnivggt_hip.h) in numpy, written for
clarity: whole-map arrays shifted by one pixel offset at a time, no tiles, no scans. float32 steps are one numpy operation each
(numpy never fuses), the cross product and its length run in float64, comparisons with NaN fail. The device returns these bytes.

Maps are [S, H, W] (z, valid, keep, flags) or [S, H, W, 3] (points, normals, colors); pixel (s, y, x) has the flat index
g = (s H + y) W + x. A shifted map reads `fill` outside its view, so nothing ever comes from the previous row's end or another view."""
import math

import numpy as np

F = np.float32
UNUSABLE, DEPTH_EDGE, NORMAL_EDGE, NO_NORMAL = 1, 2, 4, 8
GREY = 128
NAN = F(np.nan)                                                               # 0x7FC00000, the bits the device writes


def min_cos(max_angle_deg):
    """The float32 threshold of an angle in degrees: the float64 cosine rounded once."""
    return F(math.cos(math.radians(float(max_angle_deg))))


def shifted(a, dy, dx, fill):
    """out[s, y, x] = a[s, y + dy, x + dx], `fill` where that leaves the view."""
    S, H, W = a.shape[:3]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[:, yd, xd] = a[:, ys, xs]
    return out


def camera_depth(points, cams):
    """camera_depth() of csrc/ovg_project.h: ((c6 x + c7 y) + c8 z) + c11 in float32, per view."""
    c = np.asarray(cams, F).reshape(-1, 16)[:, :, None, None]
    p = np.asarray(points, F)
    with np.errstate(all="ignore"):
        return ((c[:, 6] * p[..., 0] + c[:, 7] * p[..., 1]) + c[:, 8] * p[..., 2]) + c[:, 11]


def map_depth(points=None, cams=None, depth=None, valid=None, near=1e-3):
    assert (points is None) != (depth is None)
    z = camera_depth(points, cams) if depth is None else np.asarray(depth, F)
    with np.errstate(all="ignore"):
        usable = np.isfinite(z) & (z > F(near))
    if valid is not None:
        usable &= np.asarray(valid) != 0
    return np.where(usable, z, NAN).astype(F)


def _finite3(points):
    return np.isfinite(points).all(axis=-1)


def _differences(points, z, rel_tol, axis):
    """-> (d [S, H, W, 3] f32, have, one_sided) along x (axis 1) or y (axis 0): central when both neighbours are usable for the pixel,
    else forward, else backward."""
    dy, dx = (1, 0) if axis == 0 else (0, 1)
    fin = _finite3(points)
    with np.errstate(all="ignore"):
        band = F(rel_tol) * z

        def usable_for(sy, sx):
            zq = shifted(z, sy, sx, NAN)
            return ~np.isnan(zq) & shifted(fin, sy, sx, False) & (np.abs(zq - z) <= band)
        lo, hi = usable_for(-dy, -dx), usable_for(dy, dx)
        p_lo, p_hi = shifted(points, -dy, -dx, F(0)), shifted(points, dy, dx, F(0))
        central, forward, backward = p_hi - p_lo, p_hi - points, points - p_lo
    d = np.where((lo & hi)[..., None], central, np.where(hi[..., None], forward, np.where(lo[..., None], backward, F(0)))).astype(F)
    return d, lo | hi, lo ^ hi


def map_normals(points, z, rel_tol=0.03, return_one_sided=False):
    points, z = np.asarray(points, F), np.asarray(z, F)
    ok = ~np.isnan(z) & _finite3(points)
    dh, have_h, one_h = _differences(points, z, rel_tol, 1)
    dv, have_v, one_v = _differences(points, z, rel_tol, 0)
    h, v = dh.astype(np.float64), dv.astype(np.float64)
    with np.errstate(all="ignore"):
        n = np.stack([v[..., 1] * h[..., 2] - v[..., 2] * h[..., 1],
                      v[..., 2] * h[..., 0] - v[..., 0] * h[..., 2],
                      v[..., 0] * h[..., 1] - v[..., 1] * h[..., 0]], axis=-1)
        length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        good = ok & have_h & have_v & np.isfinite(length) & (length > 0)
        out = np.where(good[..., None], (n / length[..., None]).astype(F), F(0)).astype(F)
    if return_one_sided:
        return out, good & one_h, good & one_v
    return out


def _is_zero(normals):
    return (normals[..., 0] == 0) & (normals[..., 1] == 0) & (normals[..., 2] == 0)


def map_edges(z, normals=None, radius=1, rel_tol=0.03, min_cos=-np.inf):
    z = np.asarray(z, F)
    usable = ~np.isnan(z)
    zmin, zmax = z.copy(), z.copy()
    nedge = np.zeros(z.shape, bool)
    if normals is not None:
        normals = np.asarray(normals, F)
        has = ~_is_zero(normals)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                zq = shifted(z, dy, dx, NAN)
                zmin = np.where(zq < zmin, zq, zmin)
                zmax = np.where(zq > zmax, zq, zmax)
                if normals is not None:
                    nq = shifted(normals, dy, dx, F(0))
                    dot = (normals[..., 0] * nq[..., 0] + normals[..., 1] * nq[..., 1]) + normals[..., 2] * nq[..., 2]
                    nedge |= ~np.isnan(zq) & ~_is_zero(nq) & (dot < F(min_cos))
        flags = np.where(zmax - zmin > F(rel_tol) * z, DEPTH_EDGE, 0).astype(np.uint8)
    if normals is not None:
        flags |= np.where(has, np.where(nedge, NORMAL_EDGE, 0), NO_NORMAL).astype(np.uint8)
    return np.where(usable, flags, UNUSABLE).astype(np.uint8)


def corners(z, points, keep=None):
    c = ~np.isnan(np.asarray(z, F)) & _finite3(np.asarray(points, F))
    return c if keep is None else c & (np.asarray(keep) != 0)


def quad_faces(z, points, keep=None, rel_tol=0.03, return_causes=False):
    """-> (pix [S, H-1, W-1, 2, 3] int64 flat pixel indices of the faces (a, c, b) and (b, c, d) of every quad, emitted [S, H-1, W-1, 2])."""
    z = np.asarray(z, F)
    S, H, W = z.shape
    g = np.arange(S * H * W, dtype=np.int64).reshape(S, H, W)
    cor = corners(z, points, keep)
    quad = lambda m: (m[:, :-1, :-1], m[:, :-1, 1:], m[:, 1:, :-1], m[:, 1:, 1:])      # a, b, c, d
    (ga, gb, gc, gd), (ca, cb, cc, cd), (za, zb, zc, zd) = quad(g), quad(cor), quad(z)

    def torn(z0, z1, z2):
        with np.errstate(all="ignore"):
            mx, mn = np.maximum(np.maximum(z0, z1), z2), np.minimum(np.minimum(z0, z1), z2)
            return mx - mn > F(rel_tol) * mn
    pix = np.stack([np.stack([ga, gc, gb], -1), np.stack([gb, gc, gd], -1)], axis=3)
    all_corners = np.stack([ca & cc & cb, cb & cc & cd], axis=3)
    is_torn = np.stack([torn(za, zc, zb), torn(zb, zc, zd)], axis=3)
    emitted = all_corners & ~is_torn
    if return_causes:
        return pix, emitted, all_corners, is_torn
    return pix, emitted


def triangulate(z, points, keep=None, normals=None, colors=None, rel_tol=0.03):
    """-> dict(vertices [M, 3] f32, normals [M, 3] f32, colors [M, 3] u8, pixel_index [M] int64, faces [F, 3] int32)."""
    z, points = np.asarray(z, F), np.asarray(points, F)
    n = z.size
    pix, emitted = quad_faces(z, points, keep, rel_tol)
    face_pix = pix[emitted]                                                   # C order: ascending (view, y, x, which)
    referenced = np.zeros(n, bool)
    referenced[face_pix.reshape(-1)] = True
    pixel_index = np.nonzero(referenced)[0].astype(np.int64)
    vertex_of = np.full(n, -1, np.int64)
    vertex_of[pixel_index] = np.arange(len(pixel_index))
    M = len(pixel_index)
    return dict(vertices=points.reshape(-1, 3)[pixel_index],
                normals=np.zeros((M, 3), F) if normals is None else np.asarray(normals, F).reshape(-1, 3)[pixel_index],
                colors=np.full((M, 3), GREY, np.uint8) if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3)[pixel_index],
                pixel_index=pixel_index, faces=vertex_of[face_pix].astype(np.int32).reshape(-1, 3))


def pixel_triples(face_pix):
    """Faces as sorted pixel triples, duplicates removed, rows in lexicographic order: what the golden file records."""
    t = np.sort(np.asarray(face_pix, np.int64).reshape(-1, 3), axis=1)
    return np.unique(t, axis=0) if len(t) else t
