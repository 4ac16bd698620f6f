"""The nearest-neighbour rule of ovg_nearest_neighbours (include/omnivggt_hip.h) restated in numpy float32, one rounding per operation,
chunked over the queries: the twin the device result is compared with byte for byte.

  usable      all three coordinates finite and the valid byte (if given) non-zero
  d           (dx dx + dy dy) + dz dz with dx = q.x - r.x ...; an overflow to +inf is still a candidate
  winner      the minimum of (bits(d), j) over the usable references j (j != i with exclude_self): lowest index on ties
  no winner   index -1, sqdist +inf (an unusable query, or no candidate)
"""
import numpy as np

F = np.float32
NONE_BITS = np.uint32(0xFFFFFFFF)           # what a pair that is no candidate sorts as: above bits(+inf) = 0x7F800000
INF_BITS = np.uint32(0x7F800000)


def usable(points, valid=None):
    points = np.asarray(points, F).reshape(-1, 3)
    ok = np.isfinite(points).all(1)
    return ok if valid is None else ok & (np.asarray(valid).reshape(-1) != 0)


def nearest(query, reference, query_valid=None, reference_valid=None, exclude_self=False, rows=None, budget=1 << 23):
    """-> (index int32 [n], sqdist float32 [n]) for all queries, or for the query indices `rows` only. budget: pairs per chunk."""
    q, r = np.asarray(query, F).reshape(-1, 3), np.asarray(reference, F).reshape(-1, 3)
    nq, nr = len(q), len(r)
    assert not exclude_self or nq == nr
    rows = np.arange(nq) if rows is None else np.asarray(rows, np.int64)
    q_ok, r_ok = usable(q, query_valid), usable(r, reference_valid)
    index, sqdist = np.full(len(rows), -1, np.int32), np.full(len(rows), np.inf, F)
    if nr == 0:
        return index, sqdist
    step = max(1, budget // nr)
    rx, ry, rz = r[None, :, 0], r[None, :, 1], r[None, :, 2]
    for a in range(0, len(rows), step):
        i = rows[a:a + step]
        with np.errstate(all="ignore"):
            dx, dy, dz = q[i, 0:1] - rx, q[i, 1:2] - ry, q[i, 2:3] - rz          # float32 throughout
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        bits = np.ascontiguousarray(d).view(np.uint32).copy()
        bits[:, ~r_ok] = NONE_BITS
        bits[~q_ok[i]] = NONE_BITS
        if exclude_self:
            bits[np.arange(len(i)), i] = NONE_BITS
        assert (bits[bits != NONE_BITS] <= INF_BITS).all()                       # +0, positive or +inf: the bits order like the value
        j = bits.argmin(1)                                                       # the FIRST minimum: lowest index on ties
        b = bits[np.arange(len(i)), j]
        hit = b != NONE_BITS
        index[a:a + step] = np.where(hit, j, -1)
        sqdist[a:a + step] = np.where(hit, b.view(F), F(np.inf))
    return index, sqdist


def reciprocal(P1, P2, valid1=None, valid2=None):
    """The contract of the reference's find_reciprocal_matches on the rule above: (reciprocal_in_P2 bool [n2], nn2_in_P1 int32 [n2],
    count). A -1 neighbour is never reciprocal."""
    nn1_in_P2, _ = nearest(P1, P2, valid1, valid2)
    nn2_in_P1, _ = nearest(P2, P1, valid2, valid1)
    rec = np.zeros(len(nn2_in_P1), bool)
    has = nn2_in_P1 >= 0
    rec[has] = nn1_in_P2[nn2_in_P1[has]] == np.nonzero(has)[0]
    return rec, nn2_in_P1, int(rec.sum())


def scene(nq, nr, seed=0, same=False):
    """Seeded clouds with everything the rule speaks of: points on a few blobs plus a coarse lattice (exact ties: multiples of 1/4),
    duplicated points, NaN / +-inf coordinates, coordinates of +-(1 .. 9)e20 (d overflows to +inf) and valid masks with holes.
    same=True: one cloud of nq points for the search inside a cloud. -> (query, reference, query_valid u8, reference_valid u8)."""
    rng = np.random.default_rng(seed)

    def cloud(n):
        centres = rng.normal(0.0, 2.0, (5, 3))
        p = (centres[rng.integers(0, 5, n)] + rng.normal(0.0, 0.3, (n, 3))).astype(F)
        lattice = rng.random(n) < 0.25
        p[lattice] = (rng.integers(-8, 9, (int(lattice.sum()), 3)) / 4.0).astype(F)
        dup = rng.random(n) < 0.05
        p[dup] = p[rng.integers(0, n, int(dup.sum()))]
        for share, value in ((0.01, np.nan), (0.005, np.inf), (0.005, -np.inf)):
            bad = np.nonzero(rng.random(n) < share)[0]
            p[bad, rng.integers(0, 3, len(bad))] = value
        far = np.nonzero(rng.random(n) < 0.02)[0]
        p[far, rng.integers(0, 3, len(far))] = (rng.choice([-1.0, 1.0], len(far)) * rng.uniform(1e20, 9e20, len(far))).astype(F)
        return p, (rng.random(n) >= 0.03).astype(np.uint8)

    q, qv = cloud(nq)
    if same:
        return q, q, qv, qv
    r, rv = cloud(nr)
    take = rng.random(min(nq, nr)) < 0.1                                         # points shared by both clouds: d = 0
    r[:len(take)][take] = q[:len(take)][take]
    return q, r, qv, rv
