"""numpy float32 restatement of the voxel-grid decimation rule (include/omnivggt_hip.h, ovg_voxel_downsample), the oracle of the
device kernel bit for bit:

  1. a point is valid when its three coordinates are finite;
  2. origin = component-wise minimum of the valid points;
  3. cell = np.floor((p - origin) / v) in float32; a valid point with a cell index above 2^21 - 1 is an overflow: nothing is kept;
     the key is the three 21-bit indices packed into 63 bits;
  4. inside a cell the largest conf wins (order-preserving u32 map of the f32 bits, -0 as +0, NaN lowest), ties go to the smallest
     index; without conf the smallest index wins;
  5. the winners in input order.
"""
import numpy as np

MAX_CELL = (1 << 21) - 1


class Overflow(ValueError):
    pass


def conf_order(conf):
    """u32 keys that order like the f32 values: NaN -> 0 (lowest), -0 counts as +0."""
    c = np.asarray(conf, np.float32) + np.float32(0.0)                    # -0 + 0 = +0
    u = c.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(c), np.uint32(0), k)


def cells(points, v):
    """(valid mask, origin f32 [3], int64 cell indices [n, 3] (rows of invalid points are 0)) of rule 1-3."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.float32(v)
    valid = np.isfinite(p).all(axis=1)
    if not valid.any():
        return valid, np.zeros(3, np.float32), np.zeros((len(p), 3), np.int64)
    origin = p[valid].min(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor((p[valid] - origin) / v)
    assert c.dtype == np.float32
    if not (c <= np.float32(MAX_CELL)).all():
        raise Overflow("%r cells at voxel %r: more than 2^21 along an axis" % (c.max(axis=0).tolist(), float(v)))
    out = np.zeros((len(p), 3), np.int64)
    out[valid] = c.astype(np.int64)
    return valid, origin, out


def downsample(points, v, conf=None):
    """Indices (int64, ascending) of the points rule 1-5 keeps. Raises Overflow where the device raises its flag."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int64)
    if not (np.float32(v) > 0 and np.isfinite(np.float32(v))):
        raise ValueError("voxel must be a positive finite float32")
    valid, _, c = cells(p, v)
    idx = np.nonzero(valid)[0].astype(np.int64)
    if idx.size == 0:
        return idx
    key = (c[idx, 0] << 42) | (c[idx, 1] << 21) | c[idx, 2]
    order = conf_order(conf)[idx].astype(np.int64) if conf is not None else np.zeros(idx.size, np.int64)
    s = np.lexsort((idx, -order, key))                                     # by key, then conf descending, then index
    first = np.ones(s.size, bool)
    first[1:] = key[s][1:] != key[s][:-1]
    return np.sort(idx[s[first]])


def voxel_from_rel(rel_size, scene_scale):
    """The one f32 multiply postprocess.voxel_downsample does on the device for rel_size."""
    return np.float32(rel_size) * np.float32(scene_scale)
