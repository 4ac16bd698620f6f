"""The depth-evaluation rules of include/omnivggt_hip.h (ovg_deptheval_median, ovg_deptheval_sums, ovg_deptheval_solve) restated in
numpy, and the pose figures of postprocess.relative_pose_errors / pose_auc.

  used      the one predicate of all three entries
  median    the lower and upper middle order statistics of the used values by sorting (the device selects by radix: same bytes)
  sums      the five float64 sums of a group in the device's order, operation for operation: vectorised over the tiles, with a short
            Python loop over the rounds of a thread and the levels of the trees -- compared byte for byte (the log term: to a bound)
  solve     the coefficients and status bits, operation for operation
  pose      relative rotation / translation-direction errors of all camera pairs and the accuracy / AUC figures, in float64
"""
import numpy as np

F = np.float32
THREADS, TILE, SUMS, COUNTS = 256, 1024, 5, 4
ROUNDS = TILE // THREADS
MOMENTS, METRICS = 0, 1
NONE, MEDIAN, SCALE, SCALE_SHIFT = 0, 1, 2, 3
FEW, NOT_FINITE, NO_SPREAD, BAD_FIT = 1, 2, 4, 8
SPREAD_EPS = 2.0 ** -40
DELTAS = (1.25, 1.5625, 1.953125)


def used(pred, gt, valid=None, min_depth=0.0, max_depth=np.inf):
    """-> bool, shaped like pred: which pixels enter every figure."""
    p, g = np.asarray(pred, F), np.asarray(gt, F)
    with np.errstate(invalid="ignore"):
        use = np.isfinite(p) & np.isfinite(g) & (p > F(0)) & (g > F(min_depth)) & (g <= F(max_depth))
    if valid is not None:
        use &= np.asarray(valid).reshape(p.shape) != 0
    return use


def median(pred, gt, valid=None, min_depth=0.0, max_depth=np.inf):
    """pred, gt [G, n] -> (count int64 [G], med float32 [G, 2, 2]): [g, map, 0 / 1] the values of rank (N - 1) // 2 and N // 2."""
    p, g = np.asarray(pred, F), np.asarray(gt, F)
    use = used(p, g, valid, min_depth, max_depth)
    G = p.shape[0]
    count, med = np.zeros(G, np.int64), np.zeros((G, 2, 2), F)
    for k in range(G):
        n = int(use[k].sum())
        count[k] = n
        if n:
            for m, x in enumerate((p, g)):
                s = np.sort(x[k][use[k]])
                med[k, m] = s[(n - 1) // 2], s[n // 2]
    return count, med


def aligned(p, coeff, clip_min=1e-3, clip_max=np.inf):
    """q = clip(s p + t) in float64 for float32 p [n] of ONE group; a NaN becomes clip_min."""
    p = np.asarray(p, F).astype(np.float64)
    with np.errstate(all="ignore"):
        q = float(coeff[0]) * p + float(coeff[1])
        q = np.where(q > clip_min, q, clip_min)
        return np.where(q < clip_max, q, clip_max)


def terms(p, g, mode, coeff=None, clip_min=1e-3, clip_max=np.inf):
    """p, g float32 [n] of ONE group -> (terms float64 [n, 5], below [n, 3] bool), one rounding per operation."""
    p, g = np.asarray(p, F).astype(np.float64), np.asarray(g, F).astype(np.float64)
    out, below = np.empty((len(p), SUMS)), np.zeros((len(p), 3), bool)
    with np.errstate(all="ignore"):
        if mode == MOMENTS:
            out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = p, g, p * p, p * g, g * g
            return out, below
        q = aligned(p, coeff, clip_min, clip_max)
        e = q - g
        ae, ee = np.abs(e), e * e
        d = np.log(q) - np.log(g)
        out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = ae / g, ee / g, ee, ae, d * d
        r1, r2 = q / g, g / q
        ratio = np.where(r1 > r2, r1, r2)
        for k, thr in enumerate(DELTAS):
            below[:, k] = ratio < thr
    return out, below


def _fold(v):
    """[..., 256, 5]: v[l] += v[l + s] inside every wave of 64 for s = 32 .. 1, then (w0 + w1) + (w2 + w3). -> [..., 5]"""
    v = v.reshape(v.shape[:-2] + (THREADS // 64, 64, SUMS)).copy()
    s = 32
    while s:
        v[..., :s, :] = v[..., :s, :] + v[..., s:2 * s, :]
        s >>= 1
    w = v[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def _ordered(t):
    """The fixed-order sum of the rows of t [n, 5] (rows that are not used already zeroed). -> [5]"""
    n = len(t)
    tiles = (n + TILE - 1) // TILE
    x = np.zeros((tiles * TILE, SUMS))
    x[:n] = t
    x = x.reshape(tiles, ROUNDS, THREADS, SUMS)
    with np.errstate(all="ignore"):
        acc = np.zeros((tiles, THREADS, SUMS))
        for r in range(ROUNDS):                                # thread t: pixels t, t + 256, t + 512, t + 768 of its tile, in that order
            acc = acc + x[:, r]
        part = _fold(acc)
        rows = (tiles + THREADS - 1) // THREADS
        y = np.zeros((rows * THREADS, SUMS))
        y[:tiles] = part
        y = y.reshape(rows, THREADS, SUMS)
        acc = np.zeros((THREADS, SUMS))
        for k in range(rows):                                  # thread t: tiles t, t + 256, ... in that order
            acc = acc + y[k]
        return _fold(acc)


def sums(pred, gt, valid=None, min_depth=0.0, max_depth=np.inf, mode=MOMENTS, coeff=None, clip_min=1e-3, clip_max=np.inf):
    """pred, gt [G, n] -> (counts int64 [G, 4], sums float64 [G, 5]) exactly as ovg_deptheval_sums writes them."""
    p, g = np.asarray(pred, F), np.asarray(gt, F)
    use = used(p, g, valid, min_depth, max_depth)
    G = p.shape[0]
    counts, out = np.zeros((G, COUNTS), np.int64), np.zeros((G, SUMS))
    for k in range(G):
        t, below = terms(p[k], g[k], mode, None if coeff is None else np.asarray(coeff, np.float64)[k], clip_min, clip_max)
        t[~use[k]] = 0.0                                       # a skipped pixel: adding +0.0 changes no sum that started at +0.0
        counts[k, 0] = use[k].sum()
        counts[k, 1:] = (below & use[k][:, None]).sum(0)
        out[k] = _ordered(t)
    return counts, out


def solve(mode, count, sums=None, med=None):
    """-> (coeff float64 [G, 2], status int32 [G]) exactly as ovg_deptheval_solve writes them. count [G] or [G, 4]."""
    count = np.asarray(count, np.int64)
    count = count[:, 0] if count.ndim == 2 else count
    G = len(count)
    coeff, status = np.tile(np.array([1.0, 0.0]), (G, 1)), np.zeros(G, np.int32)
    for k in range(G):
        n, st = int(count[k]), 0
        if n < (2 if mode == SCALE_SHIFT else 1):
            st |= FEW
        if mode in (SCALE, SCALE_SHIFT):
            m = np.asarray(sums, np.float64)[k]
            if not np.isfinite(m).all():
                st |= NOT_FINITE
        elif mode == MEDIAN:
            md = np.asarray(med, F)[k].astype(np.float64).reshape(4)
            if not np.isfinite(md).all():
                st |= NOT_FINITE
        s, t = 1.0, 0.0
        if st == 0 and mode != NONE:
            dn = float(n)
            with np.errstate(all="ignore"):
                if mode == MEDIAN:
                    mp, mg = 0.5 * (md[0] + md[1]), 0.5 * (md[2] + md[3])
                    s = np.float64(mg) / np.float64(mp)
                elif mode == SCALE:
                    s = m[3] / m[2]
                else:
                    nspp = dn * m[2]
                    det = nspp - m[0] * m[0]
                    if not det > SPREAD_EPS * nspp:
                        st |= NO_SPREAD
                    else:
                        s = (dn * m[3] - m[0] * m[1]) / det
                        t = (m[1] - s * m[0]) / dn
            if st == 0 and not (np.isfinite(s) and np.isfinite(t) and s > 0.0):
                st |= BAD_FIT
        if st:
            s, t = 1.0, 0.0
        coeff[k], status[k] = (s, t), st
    return coeff, status


def figures(counts, sums):
    """The per-group figures depth_metrics derives: -> dict of float64 [G] (nan where a group has no used pixel)."""
    n = counts[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = sums / n[:, None]
        out = dict(abs_rel=mean[:, 0], sq_rel=mean[:, 1], rmse=np.sqrt(mean[:, 2]), mae=mean[:, 3], rmse_log=np.sqrt(mean[:, 4]))
        for k in range(3):
            out["delta%d" % (k + 1)] = counts[:, 1 + k].astype(np.float64) / n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------------------------------------------
def _to44(E):
    E = np.asarray(E, np.float64)
    out = np.tile(np.eye(4), (len(E), 1, 1))
    out[:, :3, :4] = E[:, :3, :4]
    return out


def relative_pose_errors(pred, gt):
    """All pairs i < j (i major) of world-to-camera matrices (S, 3, 4) / (S, 4, 4) -> (rot_err, trans_err) in degrees, float64."""
    P, Gt = _to44(pred), _to44(gt)
    S = len(P)
    i, j = np.triu_indices(S, 1)
    rp, rg = P[j] @ np.linalg.inv(P[i]), Gt[j] @ np.linalg.inv(Gt[i])
    dR = rp[:, :3, :3] @ rg[:, :3, :3].transpose(0, 2, 1)
    w = np.stack([dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]], 1)
    rot = np.degrees(np.arctan2(0.5 * np.linalg.norm(w, axis=1), (np.trace(dR, axis1=1, axis2=2) - 1.0) / 2.0))
    a, b = rp[:, :3, 3], rg[:, :3, 3]
    theta = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1)))
    trans = np.minimum(theta, 180.0 - theta)
    short = (np.linalg.norm(a, axis=1) < 1e-12) | (np.linalg.norm(b, axis=1) < 1e-12)
    return rot, np.where(short, 0.0, trans)


def pose_auc(rot_err, trans_err, thresholds=(5, 15, 30)):
    """-> dict: RRA@t, RTA@t, Acc@t (both below t), AUC@t (mean over the integer degrees 1 .. t of the share of pairs whose larger
    error lies below that degree)."""
    r, t = np.asarray(rot_err, np.float64), np.asarray(trans_err, np.float64)
    worst = np.maximum(r, t)
    P, out = len(r), {}
    for thr in thresholds:                                     # integer counts, one division each: exact in any order
        out["RRA@%d" % thr] = int((r < thr).sum()) / P
        out["RTA@%d" % thr] = int((t < thr).sum()) / P
        out["Acc@%d" % thr] = int(((r < thr) & (t < thr)).sum()) / P
        out["AUC@%d" % thr] = sum(int((worst < d).sum()) for d in range(1, int(thr) + 1)) / (P * int(thr))
    return out
