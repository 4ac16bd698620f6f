"""The rules of ovg_knn_search and ovg_knn_normals (include/omnivggt_hip.h) restated in numpy by BRUTE FORCE: the twin the device
results are compared with. Nothing here goes through a grid.

  search      the float32 d, the usable points and the candidates of radius_twin.search; every pair becomes the uint64 key
              (bits(d) << 32) | j, a pair that is no candidate all ones; a row's keys are sorted and the first k taken: nearest
              first, equal distances in ascending reference index, index -1 / sqdist +inf from rank min(k, count) on
  covariance  float64, one numpy operation per rounding, over the ranks of a neighbour table in ascending order: entries outside
              [0, nr) are skipped, mean = sum / m, entry ab = sum of (p - mean)_a (p - mean)_b / m (m = 0: zeros)
  normals     the eigenvector of the covariance's smallest eigenvalue by numpy.linalg.eigh (NOT the device's Jacobi sweeps: an
              independent solver), zero where m < 3 or the covariance is not finite, oriented by the header's rule
"""
import numpy as np

from nn_twin import usable

F = np.float32
NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def search(query, reference, radius_sq, k, query_valid=None, reference_valid=None, exclude_self=False, rows=None, budget=1 << 22):
    """-> (count int32 [n], index int32 [n, k], sqdist float32 [n, k]) for all queries, or for the query indices `rows` only."""
    q, r = np.asarray(query, F).reshape(-1, 3), np.asarray(reference, F).reshape(-1, 3)
    nq, nr, k = len(q), len(r), int(k)
    assert k >= 1 and (not exclude_self or nq == nr)
    rbits = np.asarray(radius_sq, F).reshape(1).view(np.uint32)[0]
    assert np.isfinite(F(radius_sq)) and F(radius_sq) >= F(2.0 ** -100)
    rows = np.arange(nq) if rows is None else np.asarray(rows, np.int64)
    q_ok, r_ok = usable(q, query_valid), usable(r, reference_valid)
    count = np.zeros(len(rows), np.int32)
    index, sqdist = np.full((len(rows), k), -1, np.int32), np.full((len(rows), k), np.inf, F)
    if nr == 0:
        return count, index, sqdist
    step = max(1, budget // nr)
    rx, ry, rz = r[None, :, 0], r[None, :, 1], r[None, :, 2]
    j = np.arange(nr, dtype=np.uint64)[None, :]
    for a in range(0, len(rows), step):
        i = rows[a:a + step]
        with np.errstate(all="ignore"):
            dx, dy, dz = q[i, 0:1] - rx, q[i, 1:2] - ry, q[i, 2:3] - rz          # float32 throughout
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        bits = np.ascontiguousarray(d).view(np.uint32)
        cand = (bits <= rbits) & r_ok[None, :] & q_ok[i][:, None]
        if exclude_self:
            cand[np.arange(len(i)), i] = False
        keys = (bits.astype(np.uint64) << np.uint64(32)) | j
        keys[~cand] = NONE_KEY
        keys = np.sort(keys, axis=1)[:, :k]                                      # keys of one row differ in j: the order is total
        hit = keys != NONE_KEY
        n = keys.shape[1]
        count[a:a + step] = cand.sum(1)
        index[a:a + step, :n] = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        sqdist[a:a + step, :n] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F), F(np.inf))
    assert ((index >= 0).sum(1) == np.minimum(count, k)).all()
    return count, index, sqdist


def covariance(query, reference, index):
    """-> (covariance float64 [n, 6] = xx xy xz yy yz zz, used int32 [n]). query only fixes the number of rows."""
    r = np.asarray(reference, F).reshape(-1, 3).astype(np.float64)
    index = np.asarray(index, np.int32)
    n, k = index.shape
    assert len(np.asarray(query).reshape(-1, 3)) == n
    ok = (index >= 0) & (index < len(r))
    p = r[np.where(ok, index, 0)]                                                # [n, k, 3]
    m = ok.sum(1).astype(np.int32)
    dm = np.maximum(m, 1).astype(np.float64)
    s = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for t in range(k):
            s = np.where(ok[:, t, None], s + p[:, t], s)
        mean = s / dm[:, None]
        c = np.zeros((n, 6))
        for t in range(k):
            d = p[:, t] - mean
            prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
            c = np.where(ok[:, t, None], c + prod, c)
        c = c / dm[:, None]
    return c, m


def matrices(c):
    """covariance [n, 6] -> symmetric matrices [n, 3, 3]."""
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def normals(query, reference, index, viewpoint=None):
    """-> (normal float64 [n, 3], eigenvalues float64 [n, 3] ascending, solved bool [n]): eigh's eigenvector of the smallest eigenvalue
    where m >= 3 and the covariance is finite (zeros and solved False elsewhere), oriented towards the viewpoint ([3] or [n, 3]) or,
    without one, so that the component of largest magnitude is positive (the lowest axis on ties)."""
    q = np.asarray(query, F).reshape(-1, 3).astype(np.float64)
    c, m = covariance(query, reference, index)
    solved = (m >= 3) & np.isfinite(c).all(1)
    n, lam = np.zeros((len(q), 3)), np.zeros((len(q), 3))
    if solved.any():
        w, v = np.linalg.eigh(matrices(c[solved]))
        n[solved], lam[solved] = v[:, :, 0], w
    if viewpoint is not None:
        d = np.asarray(viewpoint, F).astype(np.float64).reshape(-1, 3) - q
        with np.errstate(all="ignore"):
            flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] < 0
    else:
        flip = n[np.arange(len(n)), np.abs(n).argmax(1)] < 0
    n[flip] = -n[flip]
    return n, lam, solved
