"""numpy restatement of the mesh rasterisation rule (include/omnivggt_hip.h, ovg_render_mesh), the oracle of the device kernels bit
for bit. Elementwise numpy operations round one at a time, which is what the kernels do (no fused multiply-add). Per view and face:

  1. a face with a vertex index outside [0, M) is skipped;
  2. per vertex xc, yc, zc as render_twin's rules 1-2 (float32; usable when finite and zc > near), sx = fx (xc / zc) + cx, sy
     likewise (float32), usable only when -16384 <= sx, sy <= 16384 (NaN fails); X = (int) floor(sx 256 + 0.5), Y likewise: 8 bits
     of sub-pixel fixed point. A face with an unusable vertex is not drawn in that view (no clipping);
  3. int64: area = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); zero is skipped; cull 1 drops area > 0 (back faces: x right, y down),
     cull 2 drops area < 0; the box is ceil(min / 256) .. floor(max / 256) per axis, intersected with the frame;
  4. the centre of pixel (px, py) is (256 px, 256 py); w0 over edge 1 -> 2, w1 over 2 -> 0, w2 over 0 -> 1, negated when area < 0
     (w0 + w1 + w2 = |area|); covered when all three are >= 0;
  5. float64: li = wi / |area|, ri = 1 / zci, ai = li ri, iz = (a0 + a1) + a2, zf = 1 / iz, z = (float32) zf;
     key = bits(z) << 32 | f; a pixel keeps the minimum of its keys, ~0 is empty;
  6. per hit pixel, steps 2-5 again for the winning face; bi = ai zf; an attribute is (b0 q0 + b1 q1) + b2 q2 in float64; the colour
     c (128 without colours), the normal n (without normals the face normal e1 x e2 from float64 differences of the float32 world
     vertices), len = sqrt((nx nx + ny ny) + nz nz), s = |(nx c6 + ny c7) + nz c8| / len (1 unless len is finite and > 0);
     shading 0: floor(c + 0.5); 1: floor((0.25 + 0.75 s) c + 0.5); 2: floor((0.5 (nk / len) + 0.5) 255 + 0.5) or 128; clamped to
     [0, 255]. Depth is z, index f; an empty pixel takes the background, depth 0 and index -1.
"""
import numpy as np

from render_twin import pack_cams  # noqa: F401  (the camera rows are those of ovg_render_points)

F = np.float32
D = np.float64
I = np.int64
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BAND = F(16384.0)
SHADE_COLOR, SHADE_HEADLIGHT, SHADE_NORMAL = 0, 1, 2
CULL_NONE, CULL_BACK, CULL_FRONT = 0, 1, 2
CHUNK = 1 << 22                        # (face, pixel) candidates held at once


def project_vertices(points, cam, near):
    """Rule 2 for one camera row, elementwise over points [..., 3]: (usable bool, X int64, Y int64, zc float32); X, Y are 0 where the
    vertex is not usable."""
    p = np.asarray(points, F)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    c = np.asarray(cam, F)
    with np.errstate(all="ignore"):
        xc, yc, zc = (((c[3 * i] * x + c[3 * i + 1] * y) + c[3 * i + 2] * z) + c[9 + i] for i in range(3))
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(near))
        sx = c[12] * (xc / zc) + c[14]
        sy = c[13] * (yc / zc) + c[15]
        ok &= (sx >= -BAND) & (sx <= BAND) & (sy >= -BAND) & (sy <= BAND)
        fx = np.floor(sx * F(256.0) + F(0.5))
        fy = np.floor(sy * F(256.0) + F(0.5))
    for a in (xc, zc, sx, fx):
        assert a.dtype == F
    X = np.where(ok, fx, F(0)).astype(I)
    Y = np.where(ok, fy, F(0)).astype(I)
    return ok, X, Y, zc


def face_setup(X, Y, ok, cull, H, W):
    """Rule 3 on per-face arrays X, Y int64 [n, 3], ok bool [n, 3]: (drawn bool [n], area int64 [n], x0, x1, y0, y1 int64 [n]); the box is
    empty (x0 > x1 or y0 > y1) when the face misses the frame."""
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    drawn = ok.all(1) & (area != 0)
    if cull == CULL_BACK:
        drawn &= ~(area > 0)
    elif cull == CULL_FRONT:
        drawn &= ~(area < 0)
    x0 = np.maximum(-((-X.min(1)) // 256), 0)                              # ceil(min / 256)
    x1 = np.minimum(X.max(1) // 256, W - 1)
    y0 = np.maximum(-((-Y.min(1)) // 256), 0)
    y1 = np.minimum(Y.max(1) // 256, H - 1)
    drawn &= (x0 <= x1) & (y0 <= y1)
    return drawn, area, x0, x1, y0, y1


def edge_functions(X, Y, area, px, py):
    """Rule 4: (w0, w1, w2) int64 at the pixel centres (256 px, 256 py), negated where area < 0."""
    qx, qy = 256 * px, 256 * py
    w0 = (X[:, 2] - X[:, 1]) * (qy - Y[:, 1]) - (Y[:, 2] - Y[:, 1]) * (qx - X[:, 1])
    w1 = (X[:, 0] - X[:, 2]) * (qy - Y[:, 2]) - (Y[:, 0] - Y[:, 2]) * (qx - X[:, 2])
    w2 = (X[:, 1] - X[:, 0]) * (qy - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (qx - X[:, 0])
    neg = area < 0
    return tuple(np.where(neg, -w, w) for w in (w0, w1, w2))


def depth_terms(w, area, zc):
    """Rule 5: (a0, a1, a2, zf) float64 from the edge functions, the area and the three camera depths [n, 3] float32."""
    ab = np.abs(area).astype(D)
    with np.errstate(all="ignore"):
        a = [(wi.astype(D) / ab) * (D(1.0) / zc[:, i].astype(D)) for i, wi in enumerate(w)]
        zf = D(1.0) / ((a[0] + a[1]) + a[2])
    return a[0], a[1], a[2], zf


def _valid_faces(faces, M):
    f = np.asarray(faces, np.int32).reshape(-1, 3).astype(I)
    return f, ((f >= 0) & (f < M)).all(1)


def candidates(vertices, faces, cam, H, W, cull, near):
    """Rules 1-4 for one view, in chunks: yields (face index, px, py, X, Y, area, zc, (w0, w1, w2)) for every pixel of every drawn
    face's box (covered or not), all arrays of one length."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    f, valid = _valid_faces(faces, len(vertices))
    ids = np.nonzero(valid)[0]
    if not len(ids):
        return
    ok, X, Y, zc = project_vertices(vertices, cam, near)
    fv = f[ids]
    drawn, area, x0, x1, y0, y1 = face_setup(X[fv], Y[fv], ok[fv], cull, H, W)
    ids, fv, area, x0, x1, y0, y1 = (a[drawn] for a in (ids, fv, area, x0, x1, y0, y1))
    bw = x1 - x0 + 1
    n = bw * (y1 - y0 + 1)
    start = 0
    while start < len(ids):
        stop = start + max(int(np.searchsorted(np.cumsum(n[start:]), CHUNK, side="right")), 1)
        s = slice(start, stop)
        rep = np.repeat(np.arange(start, min(stop, len(ids))), n[s])
        local = np.arange(len(rep)) - np.repeat(np.cumsum(n[s]) - n[s], n[s])
        px, py = x0[rep] + local % bw[rep], y0[rep] + local // bw[rep]
        Xf, Yf, ar = X[fv[rep]], Y[fv[rep]], area[rep]
        yield ids[rep], px, py, Xf, Yf, ar, zc[fv[rep]], edge_functions(Xf, Yf, ar, px, py)
        start = stop


def zbuffer(vertices, faces, cams, H, W, cull=CULL_NONE, near=1e-3, stats=None):
    """Rules 1-5: the u64 key buffer [V, H * W]. stats (a dict) receives `covered`, the (face, pixel) pairs that passed the coverage
    test per view, and `boxes`, the largest box in pixels."""
    cams = np.asarray(cams, F).reshape(-1, 16)
    zbuf = np.full((len(cams), H * W), EMPTY, np.uint64)
    covered, largest = [], 0
    for v, cam in enumerate(cams):
        count = 0
        for fi, px, py, X, Y, area, zc, w in candidates(vertices, faces, cam, H, W, cull, near):
            assert (w[0] + w[1] + w[2] == np.abs(area)).all()
            m = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
            *_, zf = depth_terms([wi[m] for wi in w], area[m], zc[m])
            z = zf.astype(F)
            assert np.isfinite(z).all() and (z > 0).all()
            key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | fi[m].astype(np.uint64)
            np.minimum.at(zbuf[v], py[m] * W + px[m], key)
            count += int(m.sum())
            largest = max(largest, int(np.bincount(fi - fi.min()).max()))
        covered.append(count)
    if stats is not None:
        stats["covered"], stats["boxes"] = covered, largest
    return zbuf


def _clamp_u8(x):
    return np.where(~(x >= 0), D(0), np.where(x > 255, D(255), x)).astype(np.uint8)


def resolve(zbuf, vertices, faces, normals, colors, cams, H, W, shading=SHADE_HEADLIGHT, near=1e-3, background=(255, 255, 255)):
    """Rule 6: (rgb u8 [V,H,W,3], depth f32 [V,H,W], index int64 [V,H,W])."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    f, _ = _valid_faces(faces, len(vertices))
    cams = np.asarray(cams, F).reshape(-1, 16)
    V = len(cams)
    hit = zbuf != EMPTY
    idx = (zbuf & np.uint64(0xFFFFFFFF)).astype(I)
    index = np.where(hit, idx, I(-1))
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0.0)).astype(F)
    rgb = np.empty((V, H * W, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    for v in range(V):
        q = np.nonzero(hit[v])[0]
        if not len(q):
            continue
        fv = f[idx[v][q]]                                                   # [n, 3] vertex indices of the winners
        P = vertices[fv]                                                    # [n, 3, 3]
        ok, X, Y, zc = project_vertices(P, cams[v], near)
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        assert ok.all() and (area != 0).all()
        w = edge_functions(X, Y, area, q % W, q // W)
        assert all((wi >= 0).all() for wi in w)
        a0, a1, a2, zf = depth_terms(w, area, zc)
        assert zf.astype(F).tobytes() == depth[v][q].tobytes()
        b = (a0 * zf, a1 * zf, a2 * zf)

        def lerp(attr):                                                     # attr [n, 3 vertices, k] float64
            return (b[0][:, None] * attr[:, 0] + b[1][:, None] * attr[:, 1]) + b[2][:, None] * attr[:, 2]

        col = lerp(np.asarray(colors, np.uint8).reshape(-1, 3)[fv].astype(D)) if colors is not None else np.full((len(q), 3), D(128))
        with np.errstate(all="ignore"):
            if normals is not None:
                n = lerp(np.asarray(normals, F).reshape(-1, 3)[fv].astype(D))
            else:
                e1, e2 = P[:, 1].astype(D) - P[:, 0].astype(D), P[:, 2].astype(D) - P[:, 0].astype(D)
                n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                              e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            good = np.isfinite(length) & (length > 0)
            c = cams[v].astype(D)
            s = np.where(good, np.abs((n[:, 0] * c[6] + n[:, 1] * c[7]) + n[:, 2] * c[8]) / length, D(1.0))
            if shading == SHADE_COLOR:
                out = np.floor(col + D(0.5))
            elif shading == SHADE_HEADLIGHT:
                out = np.floor((D(0.25) + D(0.75) * s)[:, None] * col + D(0.5))
            elif shading == SHADE_NORMAL:
                out = np.where(good[:, None], np.floor((D(0.5) * (n / length[:, None]) + D(0.5)) * D(255.0) + D(0.5)), D(128))
            else:
                raise ValueError(shading)
        rgb[v][q] = _clamp_u8(out)
    return rgb.reshape(V, H, W, 3), depth.reshape(V, H, W), index.reshape(V, H, W)


def render(vertices, faces, normals, colors, cams, H, W, shading=SHADE_HEADLIGHT, cull=CULL_NONE, near=1e-3, background=(255, 255, 255),
           zbuf=None):
    """Rules 1-6. zbuf: a key buffer zbuffer() made for the same mesh, cameras, size, cull and near (it does not depend on the rest)."""
    if zbuf is None:
        zbuf = zbuffer(vertices, faces, cams, H, W, cull, near)
    return resolve(zbuf, vertices, faces, normals, colors, cams, H, W, shading, near, background)
