"""numpy float32 restatement of the two TSDF rules (include/omnivggt_hip.h, ovg_tsdf_integrate / ovg_tsdf_extract), the oracle of the
device kernels bit for bit. Elementwise float32 numpy operations round one at a time, which is what the kernels do (no fused
multiply-add). Vectorised over the volume, the view loop kept. min(a, b) below is `a < b ? a : b` on both sides.

INTEGRATE, per lattice point (i, j, k) of tsdf / weight [nz][ny][nx] (colour [nz][ny][nx][4]: r, g, b, colour weight), views ascending:
  1. p = origin + voxel * (f32) index per axis;
  2. the projection of csrc/ovg_project.h (render_twin.project's rules 1-3); skipped when culled or (u, w) outside the frame;
  3. d = depth[s][w][u]; skipped unless valid != 0 (if given), d finite and d > near; wobs = obs_weight[s][w][u] (skipped unless finite
     and > 0) or 1;
  4. sdf = d - zc; skipped when sdf < -trunc; t = min(sdf / trunc, 1);
  5. Wn = W + wobs; T = (T W + t wobs) / Wn; W = min(Wn, max_weight);
  6. with colours and sdf <= trunc: Cn = Cw + wobs; ch = (ch Cw + (f32) colour wobs) / Cn per channel; Cw = min(Cn, max_weight).

EXTRACT (naive surface nets): see extract() below; corner c = dx + 2 dy + 4 dz of cell (i, j, k) is lattice point (i + dx, j + dy, k + dz).
"""
import numpy as np

F = np.float32
GREY = 128
# the 12 edges of a cell as (lower corner a, upper corner b, axis): the four x edges, the four y edges, the four z edges, each group
# in the order (0, 0), (1, 0), (0, 1), (1, 1) of the two other offsets (lower axis first)
EDGES = ((0, 1, 0), (2, 3, 0), (4, 5, 0), (6, 7, 0), (0, 2, 1), (1, 3, 1), (4, 6, 1), (5, 7, 1), (0, 4, 2), (1, 5, 2), (2, 6, 2), (3, 7, 2))
# the four cells round a lattice edge along axis a, as offsets along (b, c) = ((a + 1) % 3, (a + 2) % 3): counter-clockwise seen from +a
RING = ((-1, -1), (0, -1), (0, 0), (-1, 0))


def fmin(a, b):
    return np.where(a < b, a, b)


def pack_cams(extrinsic, intrinsic):
    """[S][16] float32 rows (rotation row-major, translation, fx, fy, cx, cy), inputs rounded to float32 first (postprocess._pack_cams)."""
    e = np.asarray(extrinsic).astype(F).reshape(-1, 3, 4)
    k = np.broadcast_to(np.asarray(intrinsic).astype(F), (len(e), 3, 3))
    return np.concatenate([e[:, :, :3].reshape(-1, 9), e[:, :, 3], k[:, 0, 0:1], k[:, 1, 1:2], k[:, 0, 2:3], k[:, 1, 2:3]], axis=1).astype(F)


def fresh(dims, color=True):
    """A fresh volume for dims = (nx, ny, nz): tsdf = 1, everything else 0. -> (tsdf, weight, color or None)."""
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), F), np.zeros((nz, ny, nx), F), np.zeros((nz, ny, nx, 4), F) if color else None


def lattice(origin, voxel, shape):
    """Rule 1: the three coordinate arrays [nz][ny][nx] float32."""
    nz, ny, nx = shape
    o, v = np.asarray(origin, F), F(voxel)
    x, y, z = (o[a] + v * np.arange(n).astype(F) for a, n in enumerate((nx, ny, nz)))
    assert x.dtype == F
    return np.broadcast_to(x[None, None, :], shape), np.broadcast_to(y[None, :, None], shape), np.broadcast_to(z[:, None, None], shape)


def integrate(tsdf, weight, color, origin, voxel, trunc, max_weight, near, depth, cams, valid=None, obs_weight=None, colors=None,
              views=None):
    """Rules 1-6, in place on tsdf / weight (/ color when colours are given). views: the view indices, all S by default (ascending)."""
    depth = np.asarray(depth, F)
    S, H, W = depth.shape
    cams = np.asarray(cams, F).reshape(S, 16)
    trunc, max_weight, near = F(trunc), F(max_weight), F(near)
    X, Y, Z = (a.reshape(-1) for a in lattice(origin, voxel, tsdf.shape))
    T, Wt = tsdf.reshape(-1), weight.reshape(-1)
    assert tsdf.flags.c_contiguous and weight.flags.c_contiguous and (color is None or color.flags.c_contiguous)   # views, not copies
    C = None if color is None or colors is None else color.reshape(-1, 4)
    for s in (range(S) if views is None else views):
        c = cams[s]
        with np.errstate(all="ignore"):
            xc, yc, zc = (((c[3 * i] * X + c[3 * i + 1] * Y) + c[3 * i + 2] * Z) + c[9 + i] for i in range(3))
            ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > near)
            u = np.floor((c[12] * (xc / zc) + c[14]) + F(0.5))
            w = np.floor((c[13] * (yc / zc) + c[15]) + F(0.5))
            ok &= (u >= F(0)) & (u <= F(W - 1)) & (w >= F(0)) & (w <= F(H - 1))
        for a in (xc, zc, u, w):
            assert a.dtype == F
        sel = np.nonzero(ok)[0]
        ui, wi = u[sel].astype(np.int64), w[sel].astype(np.int64)
        d = depth[s][wi, ui]
        with np.errstate(all="ignore"):
            ok2 = np.isfinite(d) & (d > near)
            if valid is not None:
                ok2 &= np.asarray(valid)[s][wi, ui] != 0
            if obs_weight is not None:
                wobs = np.asarray(obs_weight, F)[s][wi, ui]
                ok2 &= np.isfinite(wobs) & (wobs > F(0))
            else:
                wobs = np.ones(len(sel), F)
            sdf = d - zc[sel]
            ok2 &= ~(sdf < -trunc)
            t = fmin(sdf / trunc, F(1))
            idx, t, wo, sd = sel[ok2], t[ok2], wobs[ok2], sdf[ok2]
            Wn = Wt[idx] + wo
            T[idx] = (T[idx] * Wt[idx] + t * wo) / Wn
            Wt[idx] = fmin(Wn, max_weight)
            assert t.dtype == F and Wn.dtype == F
            if C is not None:
                near_surface = sd <= trunc
                ci, cw = idx[near_surface], wo[near_surface]
                col = np.asarray(colors, np.uint8)[s][wi[ok2][near_surface], ui[ok2][near_surface]].astype(F)
                Cw = C[ci, 3]
                Cn = Cw + cw
                for ch in range(3):
                    C[ci, ch] = (C[ci, ch] * Cw + col[:, ch] * cw) / Cn
                C[ci, 3] = fmin(Cn, max_weight)
    return tsdf, weight, color


def _empty():
    return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)


def extract(tsdf, weight, color, origin, voxel, min_weight=1.0):
    """Naive surface nets of the zero level. -> (vertices f32 [M][3], normals f32 [M][3], colors u8 [M][3], faces int32 [2Q][3]).
    A lattice point is observed when W >= min_weight and inside when T < 0. A cell with 8 observed corners of mixed sign owns one
    vertex: the crossings r = Ta / (Ta - Tb) of its sign-changing edges (EDGES order, a the lower endpoint) as local offsets, summed
    per component in float32 in that order and divided by their number; position = origin + voxel ((f32) index + offset). Normal:
    per axis the four edge differences Tb - Ta summed in EDGES order, divided by the length sqrt((gx gx + gy gy) + gz gz); zeros
    unless that length is > 0. Colour: the mean of the corners (ascending c) with colour weight > 0, floor(x + 0.5) clamped to u8;
    GREY when there are none or no colour volume. Vertices leave in ascending cell index. Every lattice edge (ascending lattice
    index, then axis) with observed endpoints of different sign whose four cells (RING) exist and are active gives the quad
    (v0, v1, v2, v3) of their vertices, reversed to (v0, v3, v2, v1) when the inside endpoint is the upper one, as the triangles
    (q0, q1, q2), (q0, q2, q3)."""
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    nz, ny, nx = tsdf.shape
    if min(nx, ny, nz) < 2:
        return _empty()
    o, v = np.asarray(origin, F), F(voxel)
    obs, ins = weight >= F(min_weight), tsdf < F(0)

    def corner(a, c):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    n_ins = sum(corner(ins, c).astype(np.int32) for c in range(8))
    active = np.logical_and.reduce([corner(obs, c) for c in range(8)]) & (n_ins > 0) & (n_ins < 8)
    kk, jj, ii = np.nonzero(active)                                         # C order: ascending cell index
    M = len(ii)
    if M == 0:
        return _empty()
    Tc = [corner(tsdf, c)[active] for c in range(8)]
    Ic = [corner(ins, c)[active] for c in range(8)]
    off, cnt = [np.zeros(M, F) for _ in range(3)], np.zeros(M, F)
    with np.errstate(all="ignore"):
        for a, b, axis in EDGES:
            cross = Ic[a] != Ic[b]
            r = Tc[a] / (Tc[a] - Tc[b])
            e = [F(a & 1), F((a >> 1) & 1), F((a >> 2) & 1)]
            e[axis] = r
            for q in range(3):
                off[q] = np.where(cross, off[q] + e[q], off[q])
            cnt = np.where(cross, cnt + F(1), cnt)
        vert = np.stack([o[q] + v * (idx.astype(F) + off[q] / cnt) for q, idx in enumerate((ii, jj, kk))], 1)
        g = []
        for axis in range(3):
            d = [Tc[b] - Tc[a] for a, b, ax in EDGES if ax == axis]
            g.append(((d[0] + d[1]) + d[2]) + d[3])
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        good = length > F(0)
        nrm = np.stack([np.where(good, gq / length, F(0)) for gq in g], 1)
    assert vert.dtype == F and nrm.dtype == F
    col = np.full((M, 3), GREY, np.uint8)
    if color is not None:
        color = np.asarray(color, F)
        Cc = [color[(c >> 2 & 1):nz - 1 + (c >> 2 & 1), (c >> 1 & 1):ny - 1 + (c >> 1 & 1), (c & 1):nx - 1 + (c & 1)][active] for c in range(8)]
        acc, n = np.zeros((M, 3), F), np.zeros(M, F)
        with np.errstate(all="ignore"):
            for c in range(8):
                has = Cc[c][:, 3] > F(0)
                acc = np.where(has[:, None], acc + Cc[c][:, :3], acc)
                n = np.where(has, n + F(1), n)
            x = np.floor(acc / n[:, None] + F(0.5))
            x = np.where(~(x >= F(0)), F(0), np.where(x > F(255), F(255), x))
        col = np.where((n > 0)[:, None], x.astype(np.uint8), np.uint8(GREY)).astype(np.uint8)
    vidx = np.full((nz, ny, nx), -1, np.int64)
    vidx[kk, jj, ii] = np.arange(M)
    dims = (nx, ny, nz)
    K, J, I = np.indices((nz, ny, nx))
    coord = (I.reshape(-1), J.reshape(-1), K.reshape(-1))
    stride = (1, nx, nx * ny)
    obs_f, ins_f, vidx_f = obs.reshape(-1), ins.reshape(-1), vidx.reshape(-1)
    keys, quads = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        m = (coord[a] <= dims[a] - 2) & (coord[b] >= 1) & (coord[b] <= dims[b] - 2) & (coord[c] >= 1) & (coord[c] <= dims[c] - 2)
        lat = np.nonzero(m)[0]
        up = lat + stride[a]
        e = obs_f[lat] & obs_f[up] & (ins_f[lat] != ins_f[up])
        lat = lat[e]
        ring = np.stack([vidx_f[lat + db * stride[b] + dc * stride[c]] for db, dc in RING], 1) if len(lat) else np.zeros((0, 4), np.int64)
        full = (ring >= 0).all(1)
        lat, ring = lat[full], ring[full]
        flip = ~ins_f[lat]                                                  # the inside endpoint is the upper one
        ring = np.where(flip[:, None], ring[:, [0, 3, 2, 1]], ring)
        keys.append(lat * 3 + a)
        quads.append(ring)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind="stable")]
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    return vert, nrm, col, faces


# ---------------------------------------------------------------------------------------------------------------------------------
# Mesh checks
# ---------------------------------------------------------------------------------------------------------------------------------

def mesh_stats(vertices, faces):
    """V (referenced vertices), E, F, chi = V - E + F, `bad_edges` (undirected edges not in exactly two triangles), `dup_directed`
    (directed edges used more than once), `degenerate` (triangles with a repeated vertex), `volume` (signed, float64: positive when
    the triangle normals of an enclosed solid point outwards), `area`."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(vertices, np.float64)
    n = max(int(f.max()) + 1 if len(f) else 0, 1)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    dk = d[:, 0] * n + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])
    _, ucount = np.unique(und, return_counts=True)
    _, dcount = np.unique(dk, return_counts=True)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    cr = np.cross(b - a, c - a)
    return {"V": len(np.unique(f)), "E": len(ucount), "F": len(f), "chi": len(np.unique(f)) - len(ucount) + len(f),
            "bad_edges": int((ucount != 2).sum()), "dup_directed": int((dcount != 1).sum()),
            "degenerate": int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()),
            "volume": float((a * np.cross(b, c)).sum() / 6.0), "area": float(np.sqrt((cr * cr).sum(1)).sum() / 2.0)}


# ---------------------------------------------------------------------------------------------------------------------------------
# Generators the host and the device tests share (float64 geometry, rounded to float32 once)
# ---------------------------------------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """World-to-camera (3, 4), float64: z towards the target, x to the right, y down."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(z, [1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z]), (-np.stack([x, np.cross(z, x), z]) @ eye)[:, None]], axis=1)


def pinhole(H, W, fov_deg=60.0):
    """(3, 3) intrinsics of a pinhole with the given horizontal field of view, pixel centres at integer coordinates."""
    f = 0.5 * W / np.tan(np.deg2rad(fov_deg) / 2.0)
    return np.array([[f, 0.0, W / 2.0 - 0.5], [0.0, f, H / 2.0 - 0.5], [0.0, 0.0, 1.0]])


def sphere_cameras(centre, distance):
    """14 look-at cameras round `centre`: the 6 axis and the 8 corner directions at the given distance. -> (14, 3, 4) float64."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + \
           [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    centre = np.asarray(centre, np.float64)
    return np.stack([look_at(centre + distance * np.asarray(d, np.float64) / np.linalg.norm(d), centre) for d in dirs])


def _rays(ext, intr, H, W):
    """Camera centre and the world directions of the pixel rays scaled so that the ray parameter is the z-depth."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - intr[0, 2]) / intr[0, 0], (v - intr[1, 2]) / intr[1, 1], np.ones_like(u)], -1)
    R, t = ext[:, :3], ext[:, 3]
    return -(R.T @ t), ray @ R


def sphere_depth(ext, intr, H, W, centre, radius, miss=0.0):
    """Analytic z-depth [S][H][W] float32 of a sphere (ray-sphere intersection, the near root); `miss` where the ray passes it."""
    ext = np.asarray(ext, np.float64).reshape(-1, 3, 4)
    k = np.broadcast_to(np.asarray(intr, np.float64), (len(ext), 3, 3))
    out = np.empty((len(ext), H, W), F)
    for s in range(len(ext)):
        eye, dirs = _rays(ext[s], k[s], H, W)
        oc = eye - np.asarray(centre, np.float64)
        aa, bb = (dirs * dirs).sum(-1), (dirs * oc).sum(-1)
        disc = bb * bb - aa * (oc @ oc - radius * radius)
        root = (-bb - np.sqrt(np.maximum(disc, 0.0))) / aa
        out[s] = np.where((disc > 0) & (root > 0), root, miss).astype(F)
    return out


def plane_depth(ext, intr, H, W, normal, offset, miss=0.0):
    """Analytic z-depth of the plane normal . p + offset = 0; `miss` where the ray is parallel or the plane lies behind the camera."""
    ext = np.asarray(ext, np.float64).reshape(-1, 3, 4)
    k = np.broadcast_to(np.asarray(intr, np.float64), (len(ext), 3, 3))
    n = np.asarray(normal, np.float64)
    out = np.empty((len(ext), H, W), F)
    for s in range(len(ext)):
        eye, dirs = _rays(ext[s], k[s], H, W)
        den = dirs @ n
        with np.errstate(all="ignore"):
            t = -(eye @ n + offset) / den
        out[s] = np.where(np.isfinite(t) & (t > 0), t, miss).astype(F)
    return out


def corner_depth(ext, intr, H, W, miss=0.0):
    """Analytic z-depth of a two-wall corner: the nearer hit of the walls x = 0 and z = 0 seen from the quadrant x, z > 0."""
    a = plane_depth(ext, intr, H, W, (1.0, 0.0, 0.0), 0.0, np.inf)
    b = plane_depth(ext, intr, H, W, (0.0, 0.0, 1.0), 0.0, np.inf)
    d = np.minimum(a, b)
    return np.where(np.isfinite(d), d, F(miss)).astype(F)


def _grid64(dims, origin, voxel):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(*(origin[a] + voxel * np.arange(n, dtype=np.float64) for a, n in ((2, nz), (1, ny), (0, nx))), indexing="ij")
    return x, y, z


def sdf_volume(kind, n, trunc_voxels=3.0, **kw):
    """An analytic truncated SDF volume on the lattice [-1, 1]^3 of n^3 points (or dims=(nx, ny, nz), the longest axis over [-1, 1] and
    the others centred with the same voxel): tsdf = clip(sdf / trunc, -1, 1)
    rounded to float32, weight 1. kinds: "sphere" (radius), "torus" (major, minor; axis z), "slab" (half: |z| <= half), "two_spheres"
    (radius, at x = -+0.5). -> (tsdf, weight, origin f32 [3], voxel f32, true volume or None)."""
    dims = kw.pop("dims", (n, n, n))
    voxel = F(2.0 / (max(dims) - 1))
    origin = np.array([-1.0 if d == max(dims) else -0.5 * float(voxel) * (d - 1) for d in dims], F)      # centred on every axis
    x, y, z = _grid64(dims, origin.astype(np.float64), float(voxel))
    if kind == "sphere":
        r = kw.get("radius", 0.6)
        sdf, true = np.sqrt(x * x + y * y + z * z) - r, 4.0 / 3.0 * np.pi * r ** 3
    elif kind == "torus":
        R, r = kw.get("major", 0.55), kw.get("minor", 0.25)
        sdf, true = np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r, 2.0 * np.pi ** 2 * R * r * r
    elif kind == "slab":
        sdf, true = np.abs(z) - kw.get("half", 0.3), None
    elif kind == "two_spheres":
        r = kw.get("radius", 0.3)
        sdf = np.minimum(np.sqrt((x + 0.5) ** 2 + y * y + z * z), np.sqrt((x - 0.5) ** 2 + y * y + z * z)) - r
        true = 2 * 4.0 / 3.0 * np.pi * r ** 3
    else:
        raise ValueError(kind)
    tsdf = np.clip(sdf / (trunc_voxels * float(voxel)), -1.0, 1.0).astype(F)
    return tsdf, np.ones(tsdf.shape, F), origin, voxel, true


def sphere_scene(n, size, radius=0.5, trunc_voxels=3.0):
    """The integration scene of the tests: a sphere at the origin in front of a far backdrop (rays that pass it read 1000 r: free
    space), seen by the 14 cameras of sphere_cameras at distance 2 r. The field of view is 60 degrees: the tangent cone of the sphere
    from that distance has a half-angle of asin(1 / 2) = 30 degrees, so the sphere fills the size x size frame exactly. The lattice is
    n^3 points over [-1.2 r, 1.2 r]^3. -> dict(depth, ext, intr, cams, origin, voxel, trunc, dims, radius)."""
    ext = sphere_cameras((0.0, 0.0, 0.0), 2.0 * radius)
    intr = pinhole(size, size, 60.0)
    depth = sphere_depth(ext, intr, size, size, (0.0, 0.0, 0.0), radius, miss=1000.0 * radius)
    voxel = F(2.4 * radius / (n - 1))
    origin = np.full(3, -1.2 * radius, F)
    return dict(depth=depth, ext=ext, intr=intr, cams=pack_cams(ext, intr), origin=origin, voxel=voxel, trunc=F(trunc_voxels) * voxel,
                dims=(n, n, n), radius=radius)
