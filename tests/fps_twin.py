"""The farthest-point-sampling rule of ovg_farthest_point_sample (include/omnivggt_hip.h) restated in numpy float32, one rounding per
operation: the twin the device result is compared with byte for byte.

  usable      all three coordinates finite and the valid byte (if given) non-zero
  state       mind[j] = float32(1e10) for every j: squared distances saturate there, and points that far from every sample tie
  centre      step 0: first; step 1 with include_last: N - 1 (both forced, usable or not); otherwise the usable j that maximises
              bits(mind[j]), the lowest j on ties; -1 when no point is usable
  outputs     index[i] = c; sqdist[i] = mind[c] before the step's update (1e10 for the first sample and for an unusable forced centre),
              +inf when c = -1
  update      c >= 0 and usable: for every usable j, d = (dx dx + dy dy) + dz dz with dx = p[j].x - p[c].x ...; mind[j] = d if d < mind[j]
  distance    mind after the last step, +inf for unusable points
"""
import numpy as np

F = np.float32
FAR = F(1e10)


def usable(points, valid=None):
    points = np.asarray(points, F)
    ok = np.isfinite(points).all(-1)
    return ok if valid is None else ok & (np.asarray(valid).reshape(ok.shape) != 0)


def sample(points, npoint, valid=None, first=0, include_last=False):
    """points [B, N, 3] (or [N, 3]: one cloud) -> (index int32 [B, npoint], sqdist float32 [B, npoint], distance float32 [B, N])."""
    p = np.asarray(points, F)
    single = p.ndim == 2
    p = p.reshape((-1,) + p.shape[-2:])
    B, N, _ = p.shape
    assert N >= 1 and 0 <= first < N
    ok = usable(p, None if valid is None else np.asarray(valid).reshape(B, N))
    index, sqdist = np.zeros((B, npoint), np.int32), np.zeros((B, npoint), F)
    distance = np.zeros((B, N), F)
    for b in range(B):
        cand = np.nonzero(ok[b])[0]                                          # the usable points, ascending; unusable ones never change
        where = np.full(N, -1, np.int64)
        where[cand] = np.arange(len(cand))
        x, y, z = (np.ascontiguousarray(p[b, cand, k]) for k in range(3))
        mind = np.full(len(cand), FAR, F)                                    # mind of the usable points (1e10 for every other, for good)
        for i in range(npoint):
            if i == 0:
                c = first
            elif i == 1 and include_last:
                c = N - 1
            elif len(cand):
                c = int(cand[mind.view(np.uint32).argmax()])                 # the FIRST maximum: lowest index on ties
            else:
                c = -1
            index[b, i] = c
            sqdist[b, i] = F(np.inf) if c < 0 else mind[where[c]] if ok[b, c] else FAR
            if c >= 0 and ok[b, c]:
                with np.errstate(all="ignore"):
                    dx, dy, dz = x - p[b, c, 0], y - p[b, c, 1], z - p[b, c, 2]
                    d = (dx * dx + dy * dy) + dz * dz                        # float32 throughout
                assert d.dtype == F and not np.isnan(d).any()
                mind = np.where(d < mind, d, mind)
        distance[b] = np.inf
        distance[b, cand] = mind
    if single:
        return index[0], sqdist[0], distance[0]
    return index, sqdist, distance


def scene(B, N, seed=0):
    """Seeded clouds with everything the rule speaks of: points on a few blobs plus a coarse lattice (exact ties: multiples of 1/4),
    duplicated points, NaN / +-inf coordinates, coordinates of +-(1 .. 9)e20 (d overflows to +inf), coordinates of +-(1 .. 3)e5 (d
    finite above 1e10: saturated) and valid masks with holes. -> (points f32 [B, N, 3], valid u8 [B, N])."""
    rng = np.random.default_rng(seed)
    pts, val = np.zeros((B, N, 3), F), np.zeros((B, N), np.uint8)
    for b in range(B):
        centres = rng.normal(0.0, 2.0, (5, 3))
        p = (centres[rng.integers(0, 5, N)] + rng.normal(0.0, 0.3, (N, 3))).astype(F)
        lattice = rng.random(N) < 0.25
        p[lattice] = (rng.integers(-8, 9, (int(lattice.sum()), 3)) / 4.0).astype(F)
        dup = rng.random(N) < 0.05
        p[dup] = p[rng.integers(0, N, int(dup.sum()))]
        for share, value in ((0.01, np.nan), (0.005, np.inf), (0.005, -np.inf)):
            bad = np.nonzero(rng.random(N) < share)[0]
            p[bad, rng.integers(0, 3, len(bad))] = value
        far = np.nonzero(rng.random(N) < 0.004)[0]
        p[far, rng.integers(0, 3, len(far))] = (rng.choice([-1.0, 1.0], len(far)) * rng.uniform(1e20, 9e20, len(far))).astype(F)
        mid = np.nonzero(rng.random(N) < 0.004)[0]
        p[mid, rng.integers(0, 3, len(mid))] = (rng.choice([-1.0, 1.0], len(mid)) * rng.uniform(1e5, 3e5, len(mid))).astype(F)
        pts[b], val[b] = p, (rng.random(N) >= 0.03).astype(np.uint8)
    return pts, val
