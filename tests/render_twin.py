"""numpy float32 restatement of the point-cloud rendering rule (include/omnivggt_hip.h, ovg_render_points), the oracle of the device
kernels bit for bit. Elementwise float32 numpy operations round one at a time, which is what the kernel does (no fused multiply-add):

  1. xc = ((R00 x + R01 y) + R02 z) + tx, likewise yc, zc;
  2. a point is skipped for a view unless xc, yc, zc are finite and zc > near;
  3. u = floor((fx (xc / zc) + cx) + 0.5), w = floor((fy (yc / zc) + cy) + 0.5);
  4. skipped unless -r <= u <= W - 1 + r and -r <= w <= H - 1 + r (in float32, NaN fails);
  5. key = (bits(zc) << 32) | index, u64; ~0 means empty;
  6. every pixel (u + dx, w + dy), |dx|, |dy| <= r, inside the image takes the minimum of its keys;
  7. a hit pixel shows colors[index], depth zc and the index; an empty one the background, depth 0 and index -1.
"""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack_cams(extrinsic, intrinsic):
    """[V][16] float32 rows (rotation row-major, translation, fx, fy, cx, cy) from (V,3,4) extrinsics and (V,3,3) or (3,3) intrinsics,
    each rounded to float32 first, as postprocess.render_point_cloud packs them."""
    e = np.asarray(extrinsic).astype(F).reshape(-1, 3, 4)
    k = np.asarray(intrinsic).astype(F)
    k = np.broadcast_to(k, (len(e), 3, 3))
    return np.concatenate([e[:, :, :3].reshape(-1, 9), e[:, :, 3], k[:, 0, 0:1], k[:, 1, 1:2], k[:, 0, 2:3], k[:, 1, 2:3]], axis=1).astype(F)


def project(points, cam, H, W, r, near):
    """Rules 1-5 for one camera row: (indices of the points that pass, px, py int64, keys u64)."""
    p = np.asarray(points, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.asarray(cam, F)
    with np.errstate(all="ignore"):
        xc, yc, zc = (((c[3 * i] * x + c[3 * i + 1] * y) + c[3 * i + 2] * z) + c[9 + i] for i in range(3))
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(near))
        u = np.floor((c[12] * (xc / zc) + c[14]) + F(0.5))
        w = np.floor((c[13] * (yc / zc) + c[15]) + F(0.5))
        ok &= (u >= F(-r)) & (u <= F(W - 1 + r)) & (w >= F(-r)) & (w <= F(H - 1 + r))
    sel = np.nonzero(ok)[0]
    for a in (xc, yc, zc, u, w):
        assert a.dtype == F
    key = (np.ascontiguousarray(zc[sel]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64)
    return sel, u[sel].astype(np.int64), w[sel].astype(np.int64), key


def zbuffer(points, cams, H, W, r, near):
    """Rules 1-6: the u64 key buffer [V, H * W]."""
    cams = np.asarray(cams, F).reshape(-1, 16)
    zbuf = np.full((len(cams), H * W), EMPTY, np.uint64)
    for v, cam in enumerate(cams):
        _, px, py, key = project(points, cam, H, W, r, near)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qx, qy = px + dx, py + dy
                m = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                np.minimum.at(zbuf[v], qy[m] * W + qx[m], key[m])
    return zbuf


def resolve(zbuf, colors, H, W, background):
    """Rule 7: (rgb u8 [V,H,W,3], depth f32 [V,H,W], index int64 [V,H,W])."""
    V = len(zbuf)
    hit = zbuf != EMPTY
    idx = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    index = np.where(hit, idx, np.int64(-1))
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0.0)).astype(F)
    rgb = np.empty((V, H * W, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    rgb[hit] = col[idx[hit]]
    return rgb.reshape(V, H, W, 3), depth.reshape(V, H, W), index.reshape(V, H, W)


def render(points, colors, cams, H, W, r=1, near=1e-3, background=(255, 255, 255)):
    return resolve(zbuffer(points, cams, H, W, r, near), colors, H, W, background)
