"""The plane-segmentation rules of include/omnivggt_hip.h (ovg_plane_hypotheses, ovg_plane_score, ovg_plane_select, ovg_plane_mask,
ovg_plane_fit) restated in numpy by BRUTE FORCE: the twin the device results are compared with. Nothing here knows a schedule.

  residual    e = ((nx x + ny y) + nz z) + w in float32, one rounding per operation; inlier iff usable and |e| <= t (a NaN never)
  draws       pos_j = ((mix(seed + 3 h + j) >> 32) * m) >> 32 in wrapping uint64, mix = splitmix64; the point candidates[pos_j] or pos_j
  hypotheses  the plane through three points in float64, one rounding per operation, void (four NaNs) by the header's list
  select      most inliers, ties to the lowest h; below min_inliers: -1, zeros, NONE
  fit         the smallest eigenvector of the inliers' scatter matrix from align_twin.moments' sums: `fit` restates the device's
              Jacobi sweeps operation for operation, `fit_eigh` uses numpy.linalg.eigh (an independent solver)
  segment_plane / segment_planes   postprocess' compositions of those
"""
import numpy as np

import align_twin
from nn_twin import usable

F = np.float32
U = np.uint64
NONE, FEW, NO_SPREAD, NOT_FINITE = 1, 2, 4, 8
COLLINEAR_EPS, SPREAD_EPS = 2.0 ** -20, 2.0 ** -40
SWEEPS = 8
MASK64 = (1 << 64) - 1


def mix(z):
    """splitmix64 of a Python int (or an array of uint64), wrapping."""
    if isinstance(z, np.ndarray):
        with np.errstate(over="ignore"):
            z = z.astype(U) + U(0x9E3779B97F4A7C15)
            z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
            return z ^ (z >> U(31))
    z = (int(z) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draws(seed, m, H):
    """-> positions int64 [H, 3] in [0, m), in exact Python integer arithmetic."""
    out = np.empty((H, 3), np.int64)
    for h in range(H):
        for j in range(3):
            out[h, j] = (((mix((seed + 3 * h + j) & MASK64) >> 32) * m) & MASK64) >> 32
    return out


def _orient(e, d=None):
    """The header's orientation of one unit normal e (float64 [3]): with d (n.axis) != 0 so that d > 0, else the component of
    largest magnitude positive, the lowest on ties."""
    if d is not None and d != 0.0:
        return -e if d < 0.0 else e
    big = e[0]
    if abs(e[1]) > abs(big):
        big = e[1]
    if abs(e[2]) > abs(big):
        big = e[2]
    return -e if big < 0.0 else e


def plane_of(a, b, c, axis=None, min_abs_cos=0.0):
    """The plane through three usable points (float32 [3] each) -> float32 [4], four NaNs when the triple is void."""
    void = np.full(4, np.nan, F)
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        uu, vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if not l2 > (COLLINEAR_EPS * uu) * vv:
            return void
        e = n / np.sqrt(l2)
        d = None
        if axis is not None:
            ax = np.asarray(axis, F).astype(np.float64)
            d = (e[0] * ax[0] + e[1] * ax[1]) + e[2] * ax[2]
            if not abs(d) >= np.float64(F(min_abs_cos)):
                return void
        e = _orient(e, d)
        w = -((e[0] * a[0] + e[1] * a[1]) + e[2] * a[2])
        return np.array([e[0], e[1], e[2], w]).astype(F)


def hypotheses(points, H, seed=0, valid=None, candidates=None, axis=None, min_abs_cos=0.0):
    """-> (planes float32 [H, 4], index int32 [H, 3]) as ovg_plane_hypotheses writes them."""
    p = np.asarray(points, F).reshape(-1, 3)
    n = len(p)
    ok = usable(p, valid)
    m = n if candidates is None else len(candidates)
    pos = draws(seed, m, H)
    index = (pos if candidates is None else np.asarray(candidates, np.int32)[pos]).astype(np.int32)
    planes = np.full((H, 4), np.nan, F)
    for h in range(H):
        i = index[h].astype(np.int64)
        if ((i < 0) | (i >= n)).any() or i[0] == i[1] or i[0] == i[2] or i[1] == i[2] or not ok[i].all():
            continue
        planes[h] = plane_of(p[i[0]], p[i[1]], p[i[2]], axis, min_abs_cos)
    return planes, index


def residual(points, plane):
    """float32 [n]: ((nx x + ny y) + nz z) + w, one rounding per operation (NaN / inf as the arithmetic gives them)."""
    p, q = np.asarray(points, F).reshape(-1, 3), np.asarray(plane, F)
    with np.errstate(all="ignore"):
        e = ((q[0] * p[:, 0] + q[1] * p[:, 1]) + q[2] * p[:, 2]) + q[3]
    assert e.dtype == F
    return e


def mask(points, plane, t, valid=None, gate=0):
    """-> (inlier uint8 [n], distance float32 [n] with NaN at unusable points, count int64 [1]) as ovg_plane_mask writes them."""
    p = np.asarray(points, F).reshape(-1, 3)
    ok = usable(p, valid) & (not (gate & NONE))
    e = np.where(ok, residual(p, plane), F(np.nan)).astype(F)
    with np.errstate(invalid="ignore"):
        inl = (np.abs(e) <= F(t)).astype(np.uint8)
    return inl, e, np.array([int(inl.sum())], np.int64)


def score(points, planes, t, valid=None, budget=1 << 23):
    """-> count int32 [H]: the inliers of every plane, chunked over the planes."""
    p, q = np.asarray(points, F).reshape(-1, 3), np.asarray(planes, F).reshape(-1, 4)
    ok = usable(p, valid)
    x, y, z = p[ok, 0][None], p[ok, 1][None], p[ok, 2][None]
    count = np.zeros(len(q), np.int32)
    step = max(1, budget // max(1, x.shape[1]))
    for a in range(0, len(q), step):
        b = q[a:a + step]
        with np.errstate(all="ignore"):
            e = ((b[:, 0:1] * x + b[:, 1:2] * y) + b[:, 2:3] * z) + b[:, 3:4]
            assert e.dtype == F
            count[a:a + step] = (np.abs(e) <= F(t)).sum(1)
    return count


def select(count, planes, min_inliers=3):
    """-> (best, plane float32 [4], best_count, status)"""
    count, planes = np.asarray(count, np.int32), np.asarray(planes, F).reshape(-1, 4)
    c = np.maximum(count, 0)
    h = int(c.argmax())                                                       # the FIRST maximum: lowest h on ties
    if c[h] >= min_inliers and np.isfinite(planes[h]).all():
        return h, planes[h].copy(), int(c[h]), 0
    return -1, np.zeros(4, F), int(c[h]), NONE


def inlier_moments(points, inlier):
    """The two passes of postprocess' refit: ovg_align_moments with source == target == points and source_valid = the inlier mask,
    about the origin and then about the means of the first pass. -> (count int64 [1], sums float64 [18], centre float64 [6])"""
    p = np.asarray(points, F).reshape(-1, 3)
    n0, s0 = align_twin.moments(p, p, source_valid=inlier)
    centre = s0[:6] / max(int(n0[0]), 1)
    n1, s1 = align_twin.moments(p, p, source_valid=inlier, centre=centre)
    return n1, s1, centre


def _scatter(N, m, c):
    dn = float(N)
    C = np.empty((3, 3))
    for r in range(3):
        for k in range(r, 3):
            C[r, k] = C[k, r] = m[6 + 3 * r + k] - (m[r] * m[k]) / dn
    return C, m[0:3] / dn + c[0:3]


def _finish(plane, N, lam_min, mid, top, e, g, axis):
    """Steps 4 and 5 of ovg_plane_fit, shared by the two solvers. -> (plane, rms, eigen, status)"""
    if not mid > SPREAD_EPS * top:
        return plane, 0.0, np.zeros(3), NO_SPREAD
    with np.errstate(all="ignore"):
        e = e / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        d = None
        if axis is not None:
            ax = np.asarray(axis, F).astype(np.float64)
            d = (e[0] * ax[0] + e[1] * ax[1]) + e[2] * ax[2]
        e = _orient(e, d)
        w = -((e[0] * g[0] + e[1] * g[1]) + e[2] * g[2])
        q = np.array([e[0], e[1], e[2], w]).astype(F)
    if not (np.isfinite(q).all() and np.isfinite(lam_min) and np.isfinite(top)):
        return plane, 0.0, np.zeros(3), NOT_FINITE
    return q, float(np.sqrt(max(lam_min, 0.0) / float(N))), np.array([lam_min, mid, top]), 0


def _degenerate(count, sums, centre):
    N, m = int(np.asarray(count).reshape(-1)[0]), np.asarray(sums, np.float64)
    c = np.zeros(6) if centre is None else np.asarray(centre, np.float64)
    return N, m, c, (FEW if N < 3 else 0) | (0 if np.isfinite(m).all() and np.isfinite(c).all() else NOT_FINITE)


def _rotate(A, V, p, q, r):
    """ovg_knn_normals' rotation in the (p, q) plane of the symmetric 3 x 3 A (r the third index), accumulated into V's columns."""
    apq = A[p, q]
    if apq == 0.0:
        return
    with np.errstate(all="ignore"):
        theta = (A[q, q] - A[p, p]) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        A[p, p], A[q, q] = A[p, p] - t * apq, A[q, q] + t * apq
        A[p, q] = A[q, p] = 0.0
        rp, rq = c * A[r, p] - s * A[r, q], s * A[r, p] + c * A[r, q]
        A[r, p] = A[p, r] = rp
        A[r, q] = A[q, r] = rq
        vp, vq = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
        V[:, p], V[:, q] = vp, vq


def fit(count, sums, centre, plane, axis=None):
    """ovg_plane_fit operation for operation (the Jacobi sweeps restated). -> (plane float32 [4], rms, eigen [3], status)"""
    plane = np.asarray(plane, F).copy()
    N, m, c, status = _degenerate(count, sums, centre)
    if status:
        return plane, 0.0, np.zeros(3), status
    with np.errstate(all="ignore"):
        A, g = _scatter(N, m, c)
    A = np.array(A, np.float64)
    V = np.eye(3)
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    lam = [A[0, 0], A[1, 1], A[2, 2]]
    kmin = 0
    if lam[1] < lam[kmin]:
        kmin = 1
    if lam[2] < lam[kmin]:
        kmin = 2
    ka, kb = (1 if kmin == 0 else 0), (1 if kmin == 2 else 2)
    mid, top = (lam[ka], lam[kb]) if lam[ka] < lam[kb] else (lam[kb], lam[ka])
    return _finish(plane, N, lam[kmin], mid, top, V[:, kmin].copy(), g, axis)


def fit_eigh(count, sums, centre, plane, axis=None):
    """The same rule with numpy.linalg.eigh in the place of the sweeps."""
    plane = np.asarray(plane, F).copy()
    N, m, c, status = _degenerate(count, sums, centre)
    if status:
        return plane, 0.0, np.zeros(3), status
    with np.errstate(all="ignore"):
        A, g = _scatter(N, m, c)
    w, V = np.linalg.eigh(A)
    return _finish(plane, N, w[0], w[1], w[2], V[:, 0].copy(), g, axis)


def eigen_gap(count, sums, centre):
    """(middle - smallest eigenvalue) / smallest: what conditions the refit normal (the rotation error is ~ eps * top / gap)."""
    N, m, c, _ = _degenerate(count, sums, centre)
    w = np.linalg.eigvalsh(_scatter(N, m, c)[0])
    return (w[1] - w[0]) / max(w[0], np.finfo(np.float64).tiny)


def segment_plane(points, t, H=1024, seed=0, refit=2, min_inliers=3, valid=None, axis=None, min_abs_cos=0.0, candidates=None,
                  fit_fn=fit, given_planes=None):
    """postprocess.segment_plane: hypotheses, score, select, mask, then `refit` rounds of moments, fit and mask.
    -> dict(plane, inlier uint8 [n], distance, count, hypothesis, rms, status, index [H, 3], counts [H])"""
    p = np.asarray(points, F).reshape(-1, 3)
    planes, index = hypotheses(p, H, seed, valid, candidates, axis, min_abs_cos)
    counts = score(p, planes, t, valid)
    best, plane, _, status = select(counts, planes, min_inliers)
    inl, dist, cnt = mask(p, plane, t, valid, status)
    rms = 0.0
    for _ in range(refit):
        N, s, c = inlier_moments(p, inl)
        plane, rms, _, st = fit_fn(N, s, c, plane, axis)
        status |= st
        inl, dist, cnt = mask(p, plane, t, valid, status)
    return dict(plane=plane, inlier=inl, distance=dist, count=int(cnt[0]), hypothesis=best, rms=rms, status=status, index=index, counts=counts)


def segment_planes(points, t, max_planes=4, min_inliers=3, H=1024, seed=0, refit=2, valid=None, axis=None, min_abs_cos=0.0, candidates=None,
                   fit_fn=fit):
    """postprocess.segment_planes: plane k draws from the candidates still unlabelled (all unlabelled points in ascending index
    when no list is given; k = 0 then draws from every point), with seed + k, scored over the unlabelled points only; stops at the
    first plane below min_inliers. -> (planes float32 [P, 4], labels int32 [n], the per-plane dicts)"""
    p = np.asarray(points, F).reshape(-1, 3)
    n = len(p)
    labels = np.full(n, -1, np.int32)
    v = np.ones(n, np.uint8) if valid is None else (np.asarray(valid).reshape(-1) != 0).astype(np.uint8)
    cand = None if candidates is None else np.asarray(candidates, np.int32)
    out, results = [], []
    for k in range(max_planes):
        if k > 0 or cand is not None:
            if cand is None:
                cand = np.nonzero(labels < 0)[0].astype(np.int32)
            else:
                inside = (cand >= 0) & (cand < n)
                cand = cand[inside & (labels[np.clip(cand, 0, n - 1)] < 0)]
            if len(cand) == 0:
                break
        r = segment_plane(p, t, H, (seed + k) & MASK64, refit, min_inliers, (v & (labels < 0)).astype(np.uint8), axis, min_abs_cos, cand, fit_fn)
        if r["status"] & NONE:
            break
        labels[r["inlier"] != 0] = k
        out.append(r["plane"])
        results.append(r)
        if candidates is None:
            cand = None
    return np.array(out, F).reshape(-1, 4), labels, results


def scene(n, seed=0):
    """The synthetic room of the tests: a floor of n // 2 points (uniform(-2, 2)^2 x normal(0, 0.003)), a wall of n // 4 points at the
    local y = 2 (the same noise, z in uniform(0, 2)), the rest uniform(-2, 2)^3; everything rotated by the Q of the QR of a normal
    3 x 3 matrix, shifted by (0.3, -0.2, 1.5), permuted, float32. -> (points, floor normal, wall normal, part uint8 [n]: 0 floor, 1
    wall, 2 clutter)"""
    rng = np.random.default_rng(seed)
    nf, nw = n // 2, n // 4
    floor = np.concatenate([rng.uniform(-2, 2, (nf, 2)), rng.normal(0, 0.003, (nf, 1))], 1)
    wall = np.stack([rng.uniform(-2, 2, nw), 2.0 + rng.normal(0, 0.003, nw), rng.uniform(0, 2, nw)], 1)
    rest = rng.uniform(-2, 2, (n - nf - nw, 3))
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    pts = np.concatenate([floor, wall, rest]) @ Q.T + np.array([0.3, -0.2, 1.5])
    part = np.concatenate([np.zeros(nf, np.uint8), np.ones(nw, np.uint8), np.full(n - nf - nw, 2, np.uint8)])
    perm = rng.permutation(n)
    return pts[perm].astype(F), Q[:, 2].copy(), Q[:, 1].copy(), part[perm]
