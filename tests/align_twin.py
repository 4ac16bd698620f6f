"""The registration rules of include/omnivggt_hip.h (ovg_align_moments, ovg_align_solve, ovg_align_apply) restated in numpy float64.

  moments   the 18 sums of a pair's terms in the device's order, operation for operation: vectorised over the tiles, with a short
            Python loop over the rounds of a thread and the levels of the trees -- the device result is compared byte for byte
  apply     ((T0 x + T1 y) + T2 z) + T3 in float64, one rounding to float32: byte for byte as well
  solve     Horn's quaternion method through numpy.linalg.eigh where the device runs Jacobi sweeps (compared within a bound), and
            solve_svd: Umeyama's reflection-corrected SVD solution from the points themselves, which shares no code with it
  icp       the loop of postprocess.icp on nn_twin's exhaustive search
"""
import numpy as np

import nn_twin

F = np.float32
THREADS, TILE, SUMS = 256, 1024, 18
ROUNDS = TILE // THREADS
FEW_PAIRS, NO_SPREAD, NOT_FINITE = 1, 2, 4
SPREAD_EPS = 2.0 ** -40


def used(p, q, index=None, source_valid=None, target_valid=None, sqdist=None, max_sqdist=None):
    """-> (use bool [n], j int64 [n] clamped into the target): which pairs enter the sums."""
    p, q = np.asarray(p, F).reshape(-1, 3), np.asarray(q, F).reshape(-1, 3)
    n, m = len(p), len(q)
    if index is None:
        assert n == m
        j = np.arange(n, dtype=np.int64)
    else:
        j = np.asarray(index, np.int32).astype(np.int64)
    use = (j >= 0) & (j < m)
    j = np.where(use, j, 0)
    use &= np.isfinite(p).all(1) & np.isfinite(q[j]).all(1)
    if source_valid is not None:
        use &= np.asarray(source_valid).reshape(-1) != 0
    if target_valid is not None:
        use &= np.asarray(target_valid).reshape(-1)[j] != 0
    if sqdist is not None:
        with np.errstate(invalid="ignore"):
            use &= np.asarray(sqdist, F) <= F(max_sqdist)                         # inclusive; a NaN compares false
    return use, j


def terms(p, q, centre=None):
    """The 18 float64 terms of every pair (p[i], q[i]), one rounding per operation. -> [n, 18]"""
    P, Q = np.asarray(p, F).astype(np.float64), np.asarray(q, F).astype(np.float64)
    c = np.zeros(6) if centre is None else np.asarray(centre, np.float64)
    with np.errstate(all="ignore"):
        a, b, d = P - c[:3], Q - c[3:], Q - P
        out = np.empty((len(P), SUMS))
        out[:, 0:3], out[:, 3:6] = a, b
        for r in range(3):
            for k in range(3):
                out[:, 6 + 3 * r + k] = a[:, r] * b[:, k]
        for k, v in ((15, a), (16, b), (17, d)):
            out[:, k] = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return out


def _fold(v):
    """[..., 256, 18]: v[l] += v[l + s] inside every wave of 64 for s = 32 .. 1, then (w0 + w1) + (w2 + w3). -> [..., 18]"""
    v = v.reshape(v.shape[:-2] + (THREADS // 64, 64, SUMS)).copy()
    s = 32
    while s:
        v[..., :s, :] = v[..., :s, :] + v[..., s:2 * s, :]
        s >>= 1
    w = v[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def moments(p, q, index=None, source_valid=None, target_valid=None, sqdist=None, max_sqdist=None, centre=None):
    """-> (count int64 [1], sums float64 [18]) exactly as ovg_align_moments writes them."""
    p, q = np.asarray(p, F).reshape(-1, 3), np.asarray(q, F).reshape(-1, 3)
    use, j = used(p, q, index, source_valid, target_valid, sqdist, max_sqdist)
    n = len(p)
    t = terms(p, q[j], centre)
    t[~use] = 0.0                                              # a skipped pair: adding +0.0 changes no sum that started at +0.0
    tiles = (n + TILE - 1) // TILE
    x = np.zeros((tiles * TILE, SUMS))
    x[:n] = t
    x = x.reshape(tiles, ROUNDS, THREADS, SUMS)
    acc = np.zeros((tiles, THREADS, SUMS))
    for r in range(ROUNDS):                                    # thread t: pairs t, t + 256, t + 512, t + 768 of its tile, in that order
        acc = acc + x[:, r]
    part = _fold(acc)                                          # [tiles, 18]
    rows = (tiles + THREADS - 1) // THREADS
    y = np.zeros((rows * THREADS, SUMS))
    y[:tiles] = part
    y = y.reshape(rows, THREADS, SUMS)
    acc = np.zeros((THREADS, SUMS))
    for k in range(rows):                                      # thread t: tiles t, t + 256, ... in that order
        acc = acc + y[k]
    return np.array([int(use.sum())], np.int64), _fold(acc)


def apply(T, p):
    T, P = np.asarray(T, np.float64), np.asarray(p, F).reshape(-1, 3).astype(np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(F)


def horn_matrix(S):
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                     [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                     [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])


def cross_covariance(count, sums):
    n = float(np.asarray(count).reshape(-1)[0])
    return sums[6:15].reshape(3, 3) - np.outer(sums[0:3], sums[3:6]) / n


def gap(count, sums):
    """(largest - second largest eigenvalue) / largest magnitude of Horn's 4 x 4 matrix: what conditions the rotation."""
    w = np.linalg.eigvalsh(horn_matrix(cross_covariance(count, sums)))
    return (w[-1] - w[-2]) / np.abs(w).max()


def solve(count, sums, centre=None, with_scale=True):
    """ovg_align_solve's rule with eigh in the place of the Jacobi sweeps. -> (step [4, 4], scale, rms, status)"""
    n, m = int(np.asarray(count).reshape(-1)[0]), np.asarray(sums, np.float64)
    c = np.zeros(6) if centre is None else np.asarray(centre, np.float64)
    status = (FEW_PAIRS if n < 3 else 0) | (0 if np.isfinite(m).all() and np.isfinite(c).all() else NOT_FINITE)
    rms = float(np.sqrt(m[17] / n)) if n >= 1 and np.isfinite(m[17]) else 0.0
    step, scale = np.eye(4), 1.0
    if status == 0:
        var = m[15] - (m[0:3] ** 2).sum() / n
        if not var > SPREAD_EPS * m[15]:
            status |= NO_SPREAD
    if status == 0:
        S = cross_covariance(n, m)
        w, V = np.linalg.eigh(horn_matrix(S))
        qw, qx, qy, qz = V[:, -1] / np.linalg.norm(V[:, -1])
        R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                      [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                      [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
        scale = float((R * S.T).sum() / var) if with_scale else 1.0
        step[:3, :3] = scale * R
        step[:3, 3] = (m[3:6] / n + c[3:]) - step[:3, :3] @ (m[0:3] / n + c[:3])
        if not np.isfinite(step).all():
            status, step, scale = status | NOT_FINITE, np.eye(4), 1.0
    return step, scale, rms, status


def solve_svd(P, Q, with_scale=True):
    """Umeyama 1991 from the points: the SVD of the cross-covariance with the reflection correction. -> (step [4, 4], scale)"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    mp, mq = P.mean(0), Q.mean(0)
    A, B = P - mp, Q - mq
    U, D, Vt = np.linalg.svd(B.T @ A / len(P))
    E = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        E[2] = -1.0
    R = U @ np.diag(E) @ Vt
    scale = float((D * E).sum() / ((A * A).sum() / len(P))) if with_scale else 1.0
    step = np.eye(4)
    step[:3, :3] = scale * R
    step[:3, 3] = mq - scale * R @ mp
    return step, scale


def fit(p, q, with_scale=True, **kw):
    """postprocess.fit_similarity's two passes: moments about the origin, then about the means of the first pass, then solve."""
    n0, s0 = moments(p, q, **kw)
    centre = s0[:6] / max(int(n0[0]), 1)
    n1, s1 = moments(p, q, centre=centre, **kw)
    return solve(n1, s1, centre, with_scale) + (int(n1[0]),)


def residual(step, P, Q):
    """Root mean square of |Q - step P| in float64."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    return float(np.sqrt((((P @ step[:3, :3].T + step[:3, 3]) - Q) ** 2).sum(1).mean()))


def icp(source, target, iterations=20, max_distance=None, with_scale=False, init=None):
    """-> (T [4, 4], rms [iterations], count [iterations], status [iterations])"""
    src, tgt = np.asarray(source, F).reshape(-1, 3), np.asarray(target, F).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    max_sq = None if max_distance is None else F(F(max_distance) * F(max_distance))
    rms, count, status = np.zeros(iterations), np.zeros(iterations, np.int64), np.zeros(iterations, np.int32)
    for it in range(iterations):
        moved = apply(T, src)
        index, sqdist = nn_twin.nearest(moved, tgt)
        kw = dict(index=index) if max_sq is None else dict(index=index, sqdist=sqdist, max_sqdist=max_sq)
        step, _, rms[it], status[it], count[it] = fit(moved, tgt, with_scale, **kw)
        T = step @ T
    return T, rms, count, status


def icp_fixture():
    """The ICP case of the tests: a 45 x 45 grid on [-1, 1]^2 jittered by N(0, 0.01) (seed 0), z = 0.3 sin 3u cos 2v + 0.2 u v + 2.5, as
    the float32 target; the source is the target rotated by 3 degrees about (1, 2, 3) / sqrt 14 through the centroid and shifted by
    (0.02, -0.02, 0.01), rounded to float32. -> (source, target, T0): T0 the float64 4 x 4 that made the source from the target."""
    rng = np.random.default_rng(0)
    u, v = np.meshgrid(np.linspace(-1, 1, 45), np.linspace(-1, 1, 45))
    u = u.ravel() + rng.normal(size=2025) * 0.01
    v = v.ravel() + rng.normal(size=2025) * 0.01
    target = np.stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * u * v + 2.5], 1).astype(F)
    ang, ax = np.deg2rad(3.0), np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R0 = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    c = target.astype(np.float64).mean(0)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, c - R0 @ c + np.array([0.02, -0.02, 0.01])
    source = (target.astype(np.float64) @ R0.T + T0[:3, 3]).astype(F)
    return source, target, T0
