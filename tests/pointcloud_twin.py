"""CPU twin of the point-cloud selection (reference: visual_util.py:113-236 predictions_to_glb, :320-358 the scene alignment).

The rules are restated with explicit numpy operations in the data's own dtype -- `np.partition` for the order statistics, never
`np.percentile` -- so the GPU tests compare against the same arithmetic whatever numpy version the test machine has. They are what
numpy 2's `percentile(..., method="linear")` does (checked against it in tests/test_pointcloud_host.py):

  q  = p / 100                 in the data dtype (f32 for f32 keys: the python float is a weak scalar)
  vi = dtype(n - 1) * q        in the data dtype; vi >= dtype(n - 1) takes the maximum (numpy's index -1)
  lo = floor(vi), hi = dtype(lo + 1) clamped to n - 1 (numpy raises there), NaN sorts last
  t  = dtype(float64(vi) - lo_index)    (lo_index is -1 for the maximum)
  r  = a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t)    evaluated literally: inf order statistics give numpy's NaN
  any NaN key -> NaN
"""
import numpy as np


def index_rule(n, p, dtype=np.float32):
    """(lo, hi, gamma) of percentile p over n keys: lo / hi are 0-based ranks in ascending order, gamma in `dtype`."""
    dt = np.dtype(dtype).type
    q = dt(p) / dt(100)
    nm1 = dt(n - 1)
    vi = nm1 * q
    if vi >= nm1:
        return n - 1, n - 1, dt(np.float64(vi) + 1.0)
    flo = np.floor(vi)
    lo = int(flo)
    hi = min(int(flo + dt(1)), n - 1)
    return lo, hi, dt(np.float64(vi) - lo)


def lerp(a, b, t):
    """numpy's two-branch _lerp, literally, in the dtype of a / b / t."""
    dt = type(t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = dt(b) - dt(a)
        if t >= dt(0.5):
            return dt(dt(b) - d * (dt(1) - t))
        return dt(dt(a) + d * t)


def percentile(x, ps):
    """Percentiles `ps` (iterable) of the 1-D array x (f32 or f64) -> array of x.dtype."""
    x = np.asarray(x).reshape(-1)
    dt = x.dtype.type
    n = x.size
    rules = [index_rule(n, p, x.dtype) for p in ps]
    kth = sorted({k for lo, hi, _ in rules for k in (lo, hi)})
    part = np.partition(x, kth)
    has_nan = bool(np.isnan(x).any())
    out = []
    for lo, hi, g in rules:
        out.append(dt(np.nan) if has_nan else lerp(part[lo], part[hi], g))
    return np.array(out, dtype=x.dtype)


def colors_u8(images):
    """(S, 3, H, W) float images -> (S*H*W, 3) uint8: trunc(x * 255) in f32, clamped to [0, 255] (NaN -> 0)."""
    c = np.transpose(np.asarray(images, np.float32), (0, 2, 3, 1)).reshape(-1, 3) * np.float32(255)
    c = np.nan_to_num(c, nan=0.0)
    return np.trunc(np.clip(c, 0, 255)).astype(np.uint8)


def norm3(d):
    """np.linalg.norm of a 3-vector as numpy computes it (sqrt of the BLAS dot, x86-64 OpenBLAS): for f32 the products are rounded to
    f32 and summed in f64 left to right, the sum rounded to f32; for f64 the dot is fma(d2, d2, fma(d1, d1, d0 * d0)). The square root
    is correctly rounded in both."""
    from fractions import Fraction
    d = np.asarray(d)
    with np.errstate(invalid="ignore", over="ignore"):
        if d.dtype == np.float32:
            p = [np.float64(np.float32(d[i] * d[i])) for i in range(3)]
            return np.sqrt(np.float32((p[0] + p[1]) + p[2]))
        if not np.all(np.isfinite(d)):
            return np.sqrt(np.float64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        fr = [Fraction(float(v)) for v in d]
        acc = np.float64(float(fr[0] * fr[0]))
        acc = np.float64(float(fr[1] * fr[1] + Fraction(float(acc))))
        acc = np.float64(float(fr[2] * fr[2] + Fraction(float(acc))))
        return np.sqrt(acc)


def scene_scale(points):
    """||P95 - P5|| over the columns of the kept (M, 3) vertices (visual_util.py:231-236); 1 for M = 0."""
    pts = np.asarray(points)
    dt = pts.dtype.type
    if pts.shape[0] == 0:
        return dt(1)
    lo = np.array([percentile(pts[:, c], [5.0])[0] for c in range(3)], dtype=pts.dtype)
    hi = np.array([percentile(pts[:, c], [95.0])[0] for c in range(3)], dtype=pts.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return dt(norm3(hi - lo))


def alignment(extrinsic0):
    """inv(E0) @ diag(1, -1, -1, 1) @ R_y(180 deg) in float64 (visual_util.py:320-358), E0 the (3, 4) camera-from-world matrix."""
    e = np.eye(4)
    e[:3, :4] = np.asarray(extrinsic0, np.float64)
    gl = np.diag([1.0, -1.0, -1.0, 1.0])
    ry = np.diag([-1.0, 1.0, -1.0, 1.0])
    return np.linalg.inv(e) @ gl @ ry


def parse_frame(filter_by_frames):
    """`"k: ..."` -> k; "all" / "All" / anything unparsable -> None (visual_util.py:116-122)."""
    if filter_by_frames in ("all", "All"):
        return None
    try:
        return int(filter_by_frames.split(":")[0])
    except (ValueError, IndexError, AttributeError):
        return None


def select(points, conf, images, extrinsic, conf_thres=50.0, frame=None, mask_black_bg=False, mask_white_bg=False, sky_mask=None,
           min_conf=1e-5):
    """The selection core on one batch element: points (S, H, W, 3), conf (S, H, W), images (S, 3, H, W), extrinsic (S, 3, 4).
    -> dict(indices (flat pixel index into the S x H x W maps), points, colors, conf_threshold, scene_scale, transform)."""
    points = np.asarray(points)
    conf = np.asarray(conf, np.float32)
    S, H, W = conf.shape
    if sky_mask is not None:
        with np.errstate(invalid="ignore"):
            conf = conf * (np.asarray(sky_mask, np.float32) > np.float32(0.1)).astype(np.float32)
    base = 0
    frames = slice(None)
    if frame is not None:
        frames = slice(frame, frame + 1)
        base = frame * H * W
    pts = points[frames].reshape(-1, 3)
    cf = conf[frames].reshape(-1)
    col = colors_u8(np.asarray(images)[frames])
    if conf_thres is None:
        conf_thres = 10.0
    thr = np.float32(0.0) if conf_thres == 0.0 else percentile(cf, [conf_thres])[0]
    with np.errstate(invalid="ignore"):
        keep = (cf >= thr) & (cf > np.float32(min_conf))
    if mask_black_bg:
        keep &= col.astype(np.int64).sum(axis=1) >= 16
    if mask_white_bg:
        keep &= ~((col[:, 0] > 240) & (col[:, 1] > 240) & (col[:, 2] > 240))
    idx = np.nonzero(keep)[0]
    kept = pts[idx]
    ext = np.asarray(extrinsic)[frames]
    return {"indices": idx.astype(np.int64) + base, "points": kept, "colors": col[idx], "conf_threshold": np.float32(thr),
            "scene_scale": scene_scale(kept), "transform": alignment(ext[0])}
