"""The radius-search rule of ovg_radius_search (include/omnivggt_hip.h) restated in numpy float32 by BRUTE FORCE, one rounding per
operation, chunked over the queries: the twin the device result is compared with byte for byte. Nothing here goes through a grid.

  usable      as in nn_twin: all three coordinates finite and the valid byte (if given) non-zero
  d           (dx dx + dy dy) + dz dz with dx = q.x - r.x ...
  candidate   a usable reference j of a usable query i with bits(d) <= bits(radius_sq) (inclusive; j != i with exclude_self); a d that
              overflows to +inf is never one
  count       the number of candidates
  winner      the minimum of (bits(d), j) over the candidates: lowest index on ties; none: index -1, sqdist +inf

For the host tests and the device's statistics the grid's two formulas are restated as well: reach() (REACH of the header) and
cells() (the cell function C), with box_stats() = what ovg_radius_search reports in out_stats for them.
"""
import numpy as np

from nn_twin import usable

F = np.float32
NONE_BITS = np.uint32(0xFFFFFFFF)
CELL_LO, CELL_HI = F(-2.0 ** 20), F(2.0 ** 20 - 1)


def radius_sq(radius):
    """f32(f32(radius)^2): one float32 multiply."""
    r = F(radius)
    return F(r * r)


def search(query, reference, radius_sq, query_valid=None, reference_valid=None, exclude_self=False, rows=None, budget=1 << 23):
    """-> (count int32 [n], index int32 [n], sqdist float32 [n]) for all queries, or for the query indices `rows` only."""
    q, r = np.asarray(query, F).reshape(-1, 3), np.asarray(reference, F).reshape(-1, 3)
    nq, nr = len(q), len(r)
    assert not exclude_self or nq == nr
    rbits = np.asarray(radius_sq, F).reshape(1).view(np.uint32)[0]
    assert np.isfinite(F(radius_sq)) and F(radius_sq) >= F(2.0 ** -100)
    rows = np.arange(nq) if rows is None else np.asarray(rows, np.int64)
    q_ok, r_ok = usable(q, query_valid), usable(r, reference_valid)
    count, index, sqdist = np.zeros(len(rows), np.int32), np.full(len(rows), -1, np.int32), np.full(len(rows), np.inf, F)
    if nr == 0:
        return count, index, sqdist
    step = max(1, budget // nr)
    rx, ry, rz = r[None, :, 0], r[None, :, 1], r[None, :, 2]
    for a in range(0, len(rows), step):
        i = rows[a:a + step]
        with np.errstate(all="ignore"):
            dx, dy, dz = q[i, 0:1] - rx, q[i, 1:2] - ry, q[i, 2:3] - rz          # float32 throughout
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        bits = np.ascontiguousarray(d).view(np.uint32).copy()
        cand = (bits <= rbits) & r_ok[None, :] & q_ok[i][:, None]                # usable pairs give +0, positive or +inf: bits order like d
        if exclude_self:
            cand[np.arange(len(i)), i] = False
        bits[~cand] = NONE_BITS
        j = bits.argmin(1)                                                       # the FIRST minimum: lowest index on ties
        b = bits[np.arange(len(i)), j]
        hit = b != NONE_BITS
        count[a:a + step] = cand.sum(1)
        index[a:a + step] = np.where(hit, j, -1)
        sqdist[a:a + step] = np.where(hit, b.view(F), F(np.inf))
    assert ((count > 0) == (index >= 0)).all()
    return count, index, sqdist


def reach(radius_sq):
    """REACH: the float32 just above sqrt((double)radius_sq) (1 + 2^-20)."""
    v = np.sqrt(np.float64(F(radius_sq))) * (1.0 + 2.0 ** -20)
    r = F(v)
    return r if np.float64(r) > v else np.nextafter(r, F(np.inf))


def cells(x, origin, cell):
    """C(x) = clamp(floor(fl(fl(x - origin) / cell)), -2^20, 2^20 - 1) per coordinate, float32 throughout, clamped as a float and
    then converted. x [..., 3] float32 (+-inf allowed: a query's box corner may overflow) -> int64 [..., 3]."""
    x, o, cell = np.asarray(x, F), np.asarray(origin, F).reshape(3), F(cell)
    with np.errstate(all="ignore"):
        c = np.floor((x - o) / cell)
    assert c.dtype == F and not np.isnan(c).any()
    c = np.where(c >= CELL_LO, np.where(c <= CELL_HI, c, CELL_HI), CELL_LO)
    return c.astype(np.int64)


def pack(c):
    """The 63-bit key of a cell [..., 3] -> int64."""
    c = c + (1 << 20)
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def boxes(query, radius_sq, cell, origin=(0.0, 0.0, 0.0)):
    """The box of cells of every query: (lo, hi) int64 [n, 3] = C(fl(q - REACH)), C(fl(q + REACH)); q must be finite."""
    q, R = np.asarray(query, F).reshape(-1, 3), reach(radius_sq)
    with np.errstate(all="ignore"):
        return cells(q - R, origin, cell), cells(q + R, origin, cell)


def box_stats(query, reference, radius_sq, cell, origin=(0.0, 0.0, 0.0), query_valid=None, reference_valid=None):
    """-> (occupied cells, most references in one cell, candidate pairs, largest box in cells): the usable references binned by
    cells(), and for every usable query the references in the cells of its box, summed."""
    q, r = np.asarray(query, F).reshape(-1, 3), np.asarray(reference, F).reshape(-1, 3)
    q, r = q[usable(q, query_valid)], r[usable(r, reference_valid)]
    if len(r) == 0:
        return 0, 0, 0, 0
    uniq, counts = np.unique(pack(cells(r, origin, cell)), return_counts=True)
    pairs, largest = 0, 0
    if len(q):
        lo, hi = boxes(q, radius_sq, cell, origin)
        assert (lo <= hi).all()
        span = (hi - lo).max(0) + 1
        largest = int((hi - lo + 1).prod(1).max())
        for ox in range(span[0]):
            for oy in range(span[1]):
                for oz in range(span[2]):
                    c = lo + np.array([ox, oy, oz])
                    k = pack(c[(c <= hi).all(1)])
                    pos = np.minimum(np.searchsorted(uniq, k), len(uniq) - 1)
                    pairs += int(counts[pos][uniq[pos] == k].sum())
    return len(uniq), int(counts.max()), pairs, largest
