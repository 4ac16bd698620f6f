"""The clustering rule of ovg_cluster (include/omnivggt_hip.h) restated in numpy by BRUTE FORCE: the twin the device result is compared
with byte for byte. Nothing here goes through a grid or a concurrent union-find.

  usable, d   as in radius_twin: float32, (dx dx + dy dy) + dz dz, one rounding per operation; d is symmetric bit for bit
  neighbours  usable i != j with bits(d) <= bits(radius_sq), inclusive
  degree      the number of neighbours (radius_twin.search(..., exclude_self=True)[0]); 0 for an unusable point
  core        usable and degree >= min_neighbours (min_neighbours = 0: every usable point, plain connected components)
  clusters    the connected components of the core points under the neighbour relation; root = the LOWEST index of the component
  border      usable, not core, with a core neighbour: root = root[j] of the core neighbour j that minimises (bits(d), j)
  noise       every other usable point; it and the unusable points have root -1
  kind        UNUSABLE 0, NOISE 1, BORDER 2, CORE 3

edges() lists the neighbour pairs by brute force; kdtree_edges() is a second source of them (scipy's cKDTree in float64), valid
only where every distance near the radius is exact in both precisions (the lattice case of the tests).
"""
import numpy as np

from nn_twin import usable as _usable

F = np.float32
UNUSABLE, NOISE, BORDER, CORE = 0, 1, 2, 3


def usable(points, valid=None):
    return _usable(points, valid)


def pair_bits(points, I, J):
    """bits(d) of the pairs (I, J) by the rule, float32 throughout."""
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[I, 0] - p[J, 0], p[I, 1] - p[J, 1], p[I, 2] - p[J, 2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F
    return np.ascontiguousarray(d).view(np.uint32)


def edges(points, valid, radius_sq, budget=1 << 23):
    """Every ordered neighbour pair, both directions, sorted by (I, J) -> (I int64, J int64, bits uint32). Chunked over i like
    radius_twin.search."""
    p = np.asarray(points, F).reshape(-1, 3)
    n = len(p)
    rbits = np.asarray(radius_sq, F).reshape(1).view(np.uint32)[0]
    assert np.isfinite(F(radius_sq)) and F(radius_sq) >= F(2.0 ** -100)
    ok = usable(p, valid)
    Is, Js, Bs = [], [], []
    step = max(1, budget // max(n, 1))
    px, py, pz = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    for a in range(0, n, step):
        i = np.arange(a, min(n, a + step))
        with np.errstate(all="ignore"):
            dx, dy, dz = p[i, 0:1] - px, p[i, 1:2] - py, p[i, 2:3] - pz
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        bits = np.ascontiguousarray(d).view(np.uint32)
        near = (bits <= rbits) & ok[None, :] & ok[i][:, None]
        near[np.arange(len(i)), i] = False
        ii, jj = np.nonzero(near)                                                # row-major: sorted by (i, j)
        Is.append(ii + a), Js.append(jj), Bs.append(bits[ii, jj])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(Is, np.int64), cat(Js, np.int64), cat(Bs, np.uint32)


def kdtree_edges(points, radius):
    """The same list from scipy's k-d tree over the float64 values of the points and the float64 radius. It agrees with edges() only
    where no pair's distance lies close enough to the radius for float32 and float64 to disagree: the caller has to know that."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, F).reshape(-1, 3)
    assert np.isfinite(p).all()
    pairs = cKDTree(p.astype(np.float64)).query_pairs(float(radius), output_type="ndarray").astype(np.int64)
    I, J = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((J, I))
    I, J = I[order], J[order]
    return I, J, pair_bits(p, I, J)


def cluster(n, usable, I, J, bits, min_neighbours):
    """-> (degree int32 [n], kind uint8 [n], root int32 [n]) from the neighbour pairs (both directions)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ok = np.asarray(usable, bool).reshape(-1)
    assert len(ok) == n and min_neighbours >= 0 and (I != J).all() and ok[I].all() and ok[J].all()
    degree = np.bincount(I, minlength=n).astype(np.int32)
    core = ok & (degree >= min_neighbours)
    root = np.full(n, -1, np.int32)
    kind = np.where(ok, NOISE, UNUSABLE).astype(np.uint8)
    kind[core] = CORE
    cc = core[I] & core[J]
    graph = coo_matrix((np.ones(int(cc.sum()), np.int8), (I[cc], J[cc])), shape=(n, n))
    ncomp, comp = connected_components(graph, directed=False)
    members = np.nonzero(core)[0]
    low = np.full(ncomp, n, np.int64)
    np.minimum.at(low, comp[members], members)
    root[members] = low[comp[members]]
    b = ~core[I] & core[J]                                                       # a usable non-core point next to a core point
    bi, key = I[b], (bits[b].astype(np.uint64) << np.uint64(32)) | J[b].astype(np.uint64)
    order = np.lexsort((key, bi))
    bi, key = bi[order], key[order]
    first = np.ones(len(bi), bool)
    first[1:] = bi[1:] != bi[:-1]                                                # the minimal (bits(d), j) of every border point
    root[bi[first]] = root[(key[first] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    kind[bi[first]] = BORDER
    return degree, kind, root


def run(points, valid, radius_sq, min_neighbours, budget=1 << 23):
    p = np.asarray(points, F).reshape(-1, 3)
    I, J, bits = edges(p, valid, radius_sq, budget)
    return cluster(len(p), usable(p, valid), I, J, bits, min_neighbours)


def labels(root, order="size"):
    """Dense labels of a root array -> (labels int32 like root, roots int32 [C], sizes int64 [C]). order "index": clusters by
    ascending root; "size": by descending size, equal sizes by ascending root."""
    root = np.asarray(root, np.int32)
    member = root >= 0
    roots, inverse, sizes = np.unique(root[member], return_inverse=True, return_counts=True)
    if order == "size":
        by_size = np.argsort(-sizes, kind="stable")
        rank = np.empty_like(by_size)
        rank[by_size] = np.arange(len(by_size))
        roots, sizes, inverse = roots[by_size], sizes[by_size], rank[inverse]
    else:
        assert order == "index"
    out = np.full(root.shape, -1, np.int32)
    out[member] = inverse.astype(np.int32)
    return out, roots.astype(np.int32), sizes.astype(np.int64)


def lattice_scene(n=262144, seed=7):
    """Two overlapping boxes of integer lattice points scaled by 1/64: every coordinate difference near the radius is an exact
    multiple of 2^-6 in float32 and float64, so squared distances are exact multiples of 2^-12 in both and, at radius sqrt(6.5) / 64,
    no pair lies between 6 and 7 units: brute force in float32 and the float64 k-d tree list the same pairs."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 112, (n // 2, 3))
    B = rng.integers(0, 200, (n // 2, 3)) + [128, 0, 0]
    pts = (np.concatenate([A, B]) / 64.0 - 2.0).astype(F)
    pts = pts[rng.permutation(n)]
    return pts, float(np.sqrt(6.5) / 64)
