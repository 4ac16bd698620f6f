"""The weighted registration and chunk-stitching rules of include/omnivggt_hip.h (ovg_align_wmoments, ovg_align_wsolve,
ovg_align_move_maps, ovg_align_move_cameras) and of postprocess.fit_similarity_robust / chunk_plan / stitch_predictions restated in
numpy float64.

  wmoments      the 20 weighted sums in the device's order, operation for operation, folded as align_twin.moments folds its 18: the
                device result is compared byte for byte
  wsolve        ovg_align_wsolve's rule with numpy.linalg.eigh where the device runs Jacobi sweeps (compared within a bound), and
  wsolve_svd    a weighted Umeyama fit from the points themselves, which shares no code with it
  fit_robust    the refit loop of postprocess.fit_similarity_robust
  move_maps, move_cameras   byte for byte
  chunk_plan, stitch        the plan and the merge of stitch_predictions, given the transforms
"""
import numpy as np

import align_twin

F = np.float32
THREADS, TILE, SUMS = align_twin.THREADS, align_twin.TILE, 20
ROUNDS = TILE // THREADS
FEW_PAIRS, NO_SPREAD, NOT_FINITE = align_twin.FEW_PAIRS, align_twin.NO_SPREAD, align_twin.NOT_FINITE
SPREAD_EPS = align_twin.SPREAD_EPS


def moved64(T, P):
    """((T0 x + T1 y) + T2 z) + T3 in float64, NOT rounded to float32."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def pair_weights(p, q, weight=None, source_valid=None, target_valid=None, transform=None, delta=None, delta_scale=1.0, cauchy=False):
    """-> (use bool [n], W float64 [n], r2 float64 [n]) of every pair; W and r2 are meaningless where use is False."""
    p, q = np.asarray(p, F).reshape(-1, 3), np.asarray(q, F).reshape(-1, 3)
    P, Q = p.astype(np.float64), q.astype(np.float64)
    use = np.isfinite(p).all(1) & np.isfinite(q).all(1)
    if source_valid is not None:
        use &= np.asarray(source_valid).reshape(-1) != 0
    if target_valid is not None:
        use &= np.asarray(target_valid).reshape(-1) != 0
    w = np.ones(len(p))
    if weight is not None:
        wf = np.asarray(weight, F).reshape(-1)
        with np.errstate(invalid="ignore"):
            use &= np.isfinite(wf) & (wf > 0)
        w = wf.astype(np.float64)
    m = P
    if transform is not None:
        m = moved64(np.asarray(transform, np.float64), P)
        use &= np.isfinite(m).all(1)
    with np.errstate(all="ignore"):
        e = Q - m
        r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        h = np.ones(len(p))
        if cauchy:
            d = float(delta_scale) * (1.0 if delta is None else float(np.asarray(delta).reshape(-1)[0]))
            if np.isfinite(d) and d > 0 and d * d > 0:
                h = 1.0 / (1.0 + r2 / (d * d))
        W = w * h
    return use, W, r2


def wterms(p, q, W, r2, centre=None):
    """The 20 float64 terms of every pair, one rounding per operation. -> [n, 20]"""
    P, Q = np.asarray(p, F).reshape(-1, 3).astype(np.float64), np.asarray(q, F).reshape(-1, 3).astype(np.float64)
    c = np.zeros(6) if centre is None else np.asarray(centre, np.float64)
    with np.errstate(all="ignore"):
        a, b = P - c[:3], Q - c[3:]
        out = np.empty((len(P), SUMS))
        for k in range(3):
            out[:, k], out[:, 3 + k] = W * a[:, k], W * b[:, k]
        for r in range(3):
            for k in range(3):
                out[:, 6 + 3 * r + k] = (W * a[:, r]) * b[:, k]
        for k, v in ((15, a), (16, b)):
            out[:, k] = W * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        out[:, 17], out[:, 18], out[:, 19] = W * r2, W, W * W
    return out


def _fold(v):
    """[..., 256, k]: v[l] += v[l + s] inside every wave of 64 for s = 32 .. 1, then (w0 + w1) + (w2 + w3). -> [..., k]"""
    k = v.shape[-1]
    v = v.reshape(v.shape[:-2] + (THREADS // 64, 64, k)).copy()
    s = 32
    while s:
        v[..., :s, :] = v[..., :s, :] + v[..., s:2 * s, :]
        s >>= 1
    w = v[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def fold_terms(t):
    """The sums of [n, k] terms (unused rows already +0.0) in the order of ovg_align_moments, steps 1 .. 4. -> [k]"""
    n, k = t.shape
    tiles = (n + TILE - 1) // TILE
    x = np.zeros((tiles * TILE, k))
    x[:n] = t
    x = x.reshape(tiles, ROUNDS, THREADS, k)
    acc = np.zeros((tiles, THREADS, k))
    for r in range(ROUNDS):
        acc = acc + x[:, r]
    part = _fold(acc)
    rows = (tiles + THREADS - 1) // THREADS
    y = np.zeros((rows * THREADS, k))
    y[:tiles] = part
    y = y.reshape(rows, THREADS, k)
    acc = np.zeros((THREADS, k))
    for r in range(rows):
        acc = acc + y[r]
    return _fold(acc)


def wmoments(p, q, weight=None, source_valid=None, target_valid=None, transform=None, delta=None, delta_scale=1.0, cauchy=False, centre=None):
    """-> (count int64 [1], sums float64 [20]) exactly as ovg_align_wmoments writes them."""
    use, W, r2 = pair_weights(p, q, weight, source_valid, target_valid, transform, delta, delta_scale, cauchy)
    t = wterms(p, q, W, r2, centre)
    t[~use] = 0.0
    return np.array([int(use.sum())], np.int64), fold_terms(t)


def rotation_of(S):
    """Horn's rotation for the cross-covariance S through eigh."""
    w, V = np.linalg.eigh(align_twin.horn_matrix(S))
    qw, qx, qy, qz = V[:, -1] / np.linalg.norm(V[:, -1])
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])


def wsolve(count, sums, centre=None, with_scale=True, keep=False, previous=None):
    """ovg_align_wsolve's rule. previous: (transform, scale) that keep=True leaves in place on a degenerate solve.
    -> dict(transform [4, 4], scale, rms, fit_rms, weight, count, status, E, vb): E, vb the residual sum and the target's spread
    fit_rms came from (the cancellation bound of a test)."""
    n, m = int(np.asarray(count).reshape(-1)[0]), np.asarray(sums, np.float64)
    c = np.zeros(6) if centre is None else np.asarray(centre, np.float64)
    W = m[18]
    weighs = bool(W > 0)
    status = (FEW_PAIRS if n < 3 or not weighs else 0) | (0 if np.isfinite(m).all() and np.isfinite(c).all() else NOT_FINITE)
    dn = W if weighs else 1.0
    T, scale, E, vb = np.eye(4), 1.0, 0.0, 0.0
    with np.errstate(all="ignore"):
        if status == 0:
            var = m[15] - ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) / dn
            if not var > SPREAD_EPS * m[15]:
                status |= NO_SPREAD
        if status == 0:
            S = m[6:15].reshape(3, 3) - np.outer(m[0:3], m[3:6]) / dn
            R = rotation_of(S)
            tr = float((R * S.T).sum())
            scale = tr / var if with_scale else 1.0
            vb = m[16] - ((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]) / dn
            E = vb - (tr * tr) / var if with_scale else (var + vb) - 2.0 * tr
            T[:3, :3] = scale * R
            T[:3, 3] = (m[3:6] / dn + c[3:]) - T[:3, :3] @ (m[0:3] / dn + c[:3])
            if not np.isfinite(T).all():
                status, T, scale, E = status | NOT_FINITE, np.eye(4), 1.0, 0.0
        rms = float(np.sqrt(m[17] / W)) if weighs and np.isfinite(W) and np.isfinite(m[17]) else 0.0
        fit_rms = float(np.sqrt(max(E, 0.0) / W)) if status == 0 and np.isfinite(E) else 0.0
    if status != 0 and keep and previous is not None:
        T, scale = np.array(previous[0], np.float64), float(previous[1])
    return dict(transform=T, scale=scale, rms=rms, fit_rms=fit_rms, weight=float(W), count=n, status=status, E=float(E), vb=float(vb))


def wsolve_svd(P, Q, w=None, with_scale=True):
    """Weighted Umeyama from the points: the SVD of the weighted cross-covariance with the reflection correction.
    -> (transform [4, 4], scale)"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    w = np.ones(len(P)) if w is None else np.asarray(w, np.float64)
    sw = w.sum()
    mp, mq = (w[:, None] * P).sum(0) / sw, (w[:, None] * Q).sum(0) / sw
    A, B = P - mp, Q - mq
    U, D, Vt = np.linalg.svd((w[:, None] * B).T @ A / sw)
    Es = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        Es[2] = -1.0
    R = U @ np.diag(Es) @ Vt
    scale = float((D * Es).sum() / ((w[:, None] * A * A).sum() / sw)) if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mq - scale * R @ mp
    return T, scale


def weighted_residual(T, P, Q, W):
    """(sum of W |Q - T P|^2, sqrt of it over the sum of W) in float64, summed directly."""
    e = np.asarray(Q, np.float64) - (np.asarray(P, np.float64) @ T[:3, :3].T + T[:3, 3])
    s = float((W * (e * e).sum(1)).sum())
    return s, float(np.sqrt(s / W.sum()))


def fit_step(p, q, with_scale=True, keep=False, previous=None, **kw):
    """One iteration of the loop: moments about the origin, then about their weighted means, then the solve.
    -> (wsolve's dict, (count, sums, centre) of the second pass)"""
    n0, s0 = wmoments(p, q, **kw)
    centre = s0[:6] / (s0[18] if s0[18] > 0 else 1.0)
    n1, s1 = wmoments(p, q, centre=centre, **kw)
    return wsolve(n1, s1, centre, with_scale, keep, previous), (n1, s1, centre)


def fit_robust(p, q, weight=None, source_valid=None, target_valid=None, with_scale=True, iterations=6, rel_delta=0.5, delta=None):
    """postprocess.fit_similarity_robust -> [wsolve's dict per iteration 0 .. iterations] (each with the transform in force after it)."""
    kw = dict(weight=weight, source_valid=source_valid, target_valid=target_valid)
    out, prev = [], None
    for k in range(iterations + 1):
        if k:
            kw.update(transform=prev["transform"], cauchy=True)
            kw.update(dict(delta=np.array([prev["fit_rms"]]), delta_scale=rel_delta) if delta is None else dict(delta=None, delta_scale=delta))
        r, _ = fit_step(p, q, with_scale, keep=k > 0, previous=None if prev is None else (prev["transform"], prev["scale"]), **kw)
        out.append(r)
        prev = r
    return out


def robust_fixture(n=4096, seed=1, sigma=1e-3, outliers=0.3):
    """The robust case of the tests: a planted Sim(3) (s = 1.7, 40 degrees about (1, 2, 3)) on a uniform cloud of extent 1, Gaussian
    noise sigma on the targets, `outliers` of them displaced by uniform(0, 1)^3 -- one-sided. -> (source f32, target f32, T_true)"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.5, 0.5, (n, 3))
    ang, ax = np.deg2rad(40.0), np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 1.7 * R, np.array([0.3, -0.2, 0.5])
    P32 = P.astype(F)
    Q = P32.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(size=(n, 3)) * sigma
    bad = rng.uniform(size=n) < outliers
    Q[bad] += rng.uniform(0.0, 1.0, (int(bad.sum()), 3))
    return P32, Q.astype(F), T


def move_maps(T, s, points=None, depth=None, points_conf=None, depth_conf=None):
    """ovg_align_move_maps -> (points, depth, points_conf, depth_conf) in the inputs' shapes, None for an absent map."""
    out = [None, None, None, None]
    if points is not None:
        out[0] = align_twin.apply(T, points).reshape(np.shape(points))
    if depth is not None:
        with np.errstate(all="ignore"):
            out[1] = (np.asarray(depth, F).astype(np.float64) * float(s)).astype(F)
    if points_conf is not None:
        out[2] = np.array(points_conf, F)
    if depth_conf is not None:
        out[3] = np.array(depth_conf, F)
    return tuple(out)


def move_cameras(extrinsic, M, s):
    """ovg_align_move_cameras: [V, 3, 4] float32 -> [V, 3, 4] float32."""
    E, M, s = np.asarray(extrinsic, F).astype(np.float64), np.asarray(M, np.float64), float(s)
    with np.errstate(all="ignore"):
        Rg, tM = M[:3, :3] / s, M[:3, 3]
        out = np.empty(E.shape)
        for i in range(3):
            A = [(E[:, i, 0] * Rg[j, 0] + E[:, i, 1] * Rg[j, 1]) + E[:, i, 2] * Rg[j, 2] for j in range(3)]
            for j in range(3):
                out[:, i, j] = A[j]
            out[:, i, 3] = s * E[:, i, 3] - ((A[0] * tM[0] + A[1] * tM[1]) + A[2] * tM[2])
    return out.astype(F)


def chunk_plan(S, chunk_size, overlap):
    if not (0 < overlap < chunk_size and S >= 1):
        raise ValueError("0 < overlap < chunk_size and S >= 1")
    step, plan, c = chunk_size - overlap, [], 0
    while True:
        plan.append((c * step, min(c * step + chunk_size, S)))
        if plan[-1][1] == S:
            return plan
        c += 1


def chunk_indices(index, start, end):
    return [i - start for i in index if start <= i < end]


def stitch(chunks, plan, transforms, scales, select="first"):
    """The merge of stitch_predictions given every chunk's transform [4, 4] and scale (entry 0 is ignored: chunk 0 is the frame).
    chunks: dicts of numpy arrays WITHOUT the batch dimension -- any of world_points [S, H, W, 3], world_points_conf [S, H, W], depth
    [S, H, W, 1], depth_conf [S, H, W], and extrinsic [S, 3, 4]. -> the merged dict of the same keys for all views."""
    S = plan[-1][1]
    out = {k: np.zeros((S,) + v.shape[1:], F) for k, v in chunks[0].items()}
    for c, (chunk, (a, b)) in enumerate(zip(chunks, plan)):
        if c == 0:
            for k, v in chunk.items():
                out[k][a:b] = v
            continue
        lo = plan[c - 1][1] - a if select == "first" else 0
        T, s = transforms[c], scales[c]
        moved = move_maps(T, s, *(chunk[k][lo:] if k in chunk else None for k in ("world_points", "depth", "world_points_conf", "depth_conf")))
        for k, v in zip(("world_points", "depth", "world_points_conf", "depth_conf"), moved):
            if v is not None:
                out[k][a + lo:b] = v
        if "extrinsic" in chunk:
            out["extrinsic"][a + lo:b] = move_cameras(chunk["extrinsic"][lo:], T, s)
    return out
