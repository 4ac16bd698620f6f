"""numpy restatement of the mesh simplification rule (include/omnivggt_hip.h, ovg_mesh_simplify), the oracle of the device kernels bit
for bit, and a second, deliberately naive form of the same rule (Python loops, dictionaries, fractions.Fraction) for small inputs.

  1. a vertex is valid when its three coordinates are finite;
  2. origin = component-wise minimum of the valid vertices; g = (p - origin) / v in float32, cell c = floor(g); a valid vertex with
     a cell index above 2^21 - 1 is an overflow, a v that is not positive and finite a bad voxel: nothing is kept;
  3. the leader of a cell is its lowest valid vertex index;
  4. a face is live when its indices lie in [0, M) and its vertices are valid; live with cells not pairwise different: degenerate;
  5. live, non-degenerate faces with the same unordered set of three cells are duplicates: the lowest face index survives as it is;
  6. one output vertex per cell a survivor names, in ascending leader index;
  7. the survivors in input order, corners as output vertex numbers, int32;
  8. position "first": the leader's bytes;
  9. position "mean": r = g - c (f32, exact), q = rint(float64(r) * 2^24), Q = sum q, n = count;
     f32(float64(origin) + float64(v) * (float64(c) + float64(Q) / (float64(n) * 16777216.0)));
 10. colours: (2 S + n) // (2 n) per channel;
 11. normals: those with finite components of magnitude <= 4 take part; per component the sum of rint(float64(x) * 2^20) in int64; the
     integer vector as float64 divided by sqrt((x x + y y) + z z), rounded to f32; (0, 0, 0) when the length is not finite and > 0;
 12. source_index = the leaders, vertex_count = n; counts = (M', F', flags, occupied cells, degenerate faces, duplicate faces).
"""
import math
from fractions import Fraction

import numpy as np

MAX_CELL = (1 << 21) - 1
OVERFLOW, BAD_VOXEL = 1, 2
F = np.float32


class Flagged(ValueError):
    """The device raises a flag here: .flags holds OVERFLOW or BAD_VOXEL."""

    def __init__(self, flags, msg):
        ValueError.__init__(self, msg)
        self.flags = flags


def grid(vertices, v):
    """(valid mask, origin f32 [3], g f32 [M, 3], cells int64 [M, 3]); rows of invalid vertices are 0. Rule 1-2."""
    p = np.asarray(vertices, F).reshape(-1, 3)
    v = F(v)
    if not (v > 0 and np.isfinite(v)):
        raise Flagged(BAD_VOXEL, "voxel %r is not a positive finite float32" % float(v))
    valid = np.isfinite(p).all(axis=1)
    g = np.zeros((len(p), 3), F)
    c = np.zeros((len(p), 3), np.int64)
    if not valid.any():
        return valid, np.zeros(3, F), g, c
    origin = p[valid].min(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        gv = (p[valid] - origin) / v
        cv = np.floor(gv)
    assert gv.dtype == np.float32 and cv.dtype == np.float32
    if not (cv <= F(MAX_CELL)).all():
        raise Flagged(OVERFLOW, "%r cells at voxel %r: more than 2^21 along an axis" % (cv.max(axis=0).tolist(), float(v)))
    g[valid] = gv
    c[valid] = cv.astype(np.int64)
    return valid, origin, g, c


def _empty(normals, colors, cells=0, degenerate=0):
    return dict(vertices=np.zeros((0, 3), F), faces=np.zeros((0, 3), np.int32), normals=None if normals is None else np.zeros((0, 3), F),
                colors=None if colors is None else np.zeros((0, 3), np.uint8), source_index=np.zeros(0, np.int64),
                vertex_count=np.zeros(0, np.int32), counts=np.array([0, 0, 0, cells, degenerate, 0], np.int64), face_index=np.zeros(0, np.int64))


def simplify(vertices, faces, v, normals=None, colors=None, position="mean"):
    """-> dict(vertices f32 [M', 3], faces int32 [F', 3], normals f32 [M', 3] or None, colors u8 [M', 3] or None, source_index int64
    [M'], vertex_count int32 [M'], counts int64 [6], face_index int64 [F'] (the survivors' input indices; not a device output)).
    Raises Flagged where the device raises a flag."""
    assert position in ("mean", "first")
    p = np.asarray(vertices, F).reshape(-1, 3)
    fc = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    M = len(p)
    valid, origin, g, c = grid(p, v)
    if not valid.any() or len(fc) == 0:
        return _empty(normals, colors)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    vidx = np.nonzero(valid)[0]
    _, first, inv = np.unique(key[vidx], return_index=True, return_inverse=True)
    ncell = len(first)
    leader = vidx[first]                                                   # vidx ascends: the first occurrence is the lowest index
    cell = np.full(M, -1, np.int64)
    cell[vidx] = inv.reshape(-1)
    n = np.bincount(cell[vidx], minlength=ncell).astype(np.int64)
    # rule 4
    inside = ((fc >= 0) & (fc < M)).all(axis=1)
    fcell = np.full((len(fc), 3), -1, np.int64)
    fcell[inside] = cell[fc[inside]]
    live = inside & (fcell >= 0).all(axis=1)
    a, b, d = fcell[:, 0], fcell[:, 1], fcell[:, 2]
    degenerate = live & ((a == b) | (b == d) | (a == d))
    cand = np.nonzero(live & ~degenerate)[0]
    # rule 5: the first occurrence of a sorted triple among the candidates (which ascend) is the lowest face index
    if len(cand) == 0:
        return _empty(normals, colors, ncell, int(degenerate.sum()))
    tri = np.sort(fcell[cand], axis=1)
    order = np.lexsort((cand, tri[:, 2], tri[:, 1], tri[:, 0]))            # by triple, then by face index
    ts = tri[order]
    head = np.ones(len(cand), bool)
    head[1:] = (ts[1:] != ts[:-1]).any(axis=1)
    surv = np.sort(cand[order[head]])
    # rule 6
    used = np.unique(fcell[surv])
    used = used[np.argsort(leader[used], kind="stable")]
    number = np.full(ncell, -1, np.int64)
    number[used] = np.arange(len(used))
    out_faces = number[fcell[surv]].astype(np.int32)
    src = leader[used].astype(np.int64)
    cnt = n[used]
    if position == "first":
        out_v = p[src].copy()
    else:
        r = g - c.astype(F)                                                # exact in f32
        assert r.dtype == np.float32 and (r[valid] >= 0).all() and (r[valid] < 1).all()
        q = np.rint(r.astype(np.float64) * 16777216.0).astype(np.int64)
        Q = np.zeros((ncell, 3), np.int64)
        np.add.at(Q, cell[vidx], q[vidx])
        frac = Q[used].astype(np.float64) / (cnt.astype(np.float64) * 16777216.0)[:, None]
        in_cells = c[src].astype(np.float64) + frac
        out_v = (origin.astype(np.float64) + np.float64(F(v)) * in_cells).astype(F)
    out_c = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).reshape(M, 3).astype(np.int64)
        S = np.zeros((ncell, 3), np.int64)
        np.add.at(S, cell[vidx], col[vidx])
        out_c = ((2 * S[used] + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)
    out_n = None
    if normals is not None:
        nr = np.asarray(normals, F).reshape(M, 3)
        with np.errstate(invalid="ignore"):
            part = valid & np.isfinite(nr).all(axis=1) & (np.abs(nr) <= F(4.0)).all(axis=1)
        qn = np.zeros((M, 3), np.int64)
        qn[part] = np.rint(nr[part].astype(np.float64) * 1048576.0).astype(np.int64)
        N = np.zeros((ncell, 3), np.int64)
        np.add.at(N, cell[vidx], qn[vidx])
        x, y, z = (N[used, k].astype(np.float64) for k in range(3))
        length = np.sqrt((x * x + y * y) + z * z)
        ok = (length > 0) & np.isfinite(length)
        safe = np.where(ok, length, 1.0)
        out_n = np.where(ok[:, None], np.stack([x / safe, y / safe, z / safe], axis=1), 0.0).astype(F)
    counts = np.array([len(used), len(surv), 0, ncell, int(degenerate.sum()), len(cand) - len(surv)], np.int64)
    return dict(vertices=out_v, faces=out_faces, normals=out_n, colors=out_c, source_index=src, vertex_count=cnt.astype(np.int32),
                counts=counts, face_index=surv.astype(np.int64))


def table_keys(vertices, faces, v):
    """(occupied cells, distinct triples of live non-degenerate faces): the keys the two device tables hold."""
    out = simplify(vertices, faces, v)
    return int(out["counts"][3]), int(out["counts"][1])


def simplify_naive(vertices, faces, v, normals=None, colors=None, position="mean"):
    """The same rule, one vertex and one face at a time. Same dict as simplify (without face_index)."""
    p = np.asarray(vertices, F).reshape(-1, 3)
    fc = [[int(x) for x in row] for row in np.asarray(faces).reshape(-1, 3)]
    M = len(p)
    v = F(v)
    if not (v > 0 and np.isfinite(v)):
        raise Flagged(BAD_VOXEL, "bad voxel")
    valid = [all(math.isfinite(float(x)) for x in p[i]) for i in range(M)]
    origin = [None, None, None]
    for i in range(M):
        if valid[i]:
            for k in range(3):
                if origin[k] is None or p[i, k] < origin[k]:
                    origin[k] = p[i, k]
    cells, cell_of = {}, [None] * M                                         # cell -> dict of accumulators
    for i in range(M):
        if not valid[i]:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            g = [F(F(p[i, k] - origin[k]) / v) for k in range(3)]
            c = [np.floor(x) for x in g]
        if not all(x <= F(MAX_CELL) for x in c):
            raise Flagged(OVERFLOW, "overflow")
        ck = tuple(int(x) for x in c)
        e = cells.setdefault(ck, dict(leader=i, n=0, Q=[0, 0, 0], S=[0, 0, 0], N=[0, 0, 0]))
        cell_of[i] = ck
        e["n"] += 1
        for k in range(3):
            r = Fraction(float(g[k])) - Fraction(float(c[k]))               # exact
            assert 0 <= r < 1 and Fraction(float(F(g[k] - c[k]))) == r
            e["Q"][k] += round(r * (1 << 24))                               # Python rounds halves to even
        if colors is not None:
            for k in range(3):
                e["S"][k] += int(colors[i][k])
        if normals is not None:
            x = [float(t) for t in np.asarray(normals, F)[i]]
            if all(math.isfinite(t) and abs(t) <= 4.0 for t in x):
                for k in range(3):
                    e["N"][k] += round(Fraction(x[k]) * (1 << 20))
    seen, surv, degenerate, cand = {}, [], 0, 0
    for f, row in enumerate(fc):
        if not all(0 <= i < M and valid[i] for i in row):
            continue
        cs = [cell_of[i] for i in row]
        if len(set(cs)) < 3:
            degenerate += 1
            continue
        cand += 1
        t = frozenset(cs)
        if t not in seen:
            seen[t] = f
            surv.append(f)
    used = sorted({cell_of[i] for f in surv for i in fc[f]}, key=lambda ck: cells[ck]["leader"])
    number = {ck: j for j, ck in enumerate(used)}
    out = _empty(normals, colors)
    out["faces"] = np.array([[number[cell_of[i]] for i in fc[f]] for f in surv], np.int32).reshape(-1, 3)
    out["source_index"] = np.array([cells[ck]["leader"] for ck in used], np.int64)
    out["vertex_count"] = np.array([cells[ck]["n"] for ck in used], np.int32)
    verts, cols, nrms = [], [], []
    for ck in used:
        e = cells[ck]
        if position == "first":
            verts.append(p[e["leader"]])
        else:
            row = []
            for k in range(3):
                frac = float(Fraction(e["Q"][k], e["n"] << 24))             # correctly rounded: the float64 quotient of two exact operands
                row.append(F(float(origin[k]) + float(v) * (float(ck[k]) + frac)))
            verts.append(row)
        cols.append([(2 * s + e["n"]) // (2 * e["n"]) for s in e["S"]])
        x, y, z = (float(t) for t in e["N"])
        length = math.sqrt((x * x + y * y) + z * z)
        nrms.append([F(x / length), F(y / length), F(z / length)] if length > 0 and math.isfinite(length) else [F(0), F(0), F(0)])
    out["vertices"] = np.array(verts, F).reshape(-1, 3)
    if colors is not None:
        out["colors"] = np.array(cols, np.uint8).reshape(-1, 3)
    if normals is not None:
        out["normals"] = np.array(nrms, F).reshape(-1, 3)
    out["counts"] = np.array([len(used), len(surv), 0, len(cells), degenerate, cand - len(surv)], np.int64)
    del out["face_index"]
    return out


# ---------------------------------------------------------------------------------------------
# scenes shared by the host and the device tests
# ---------------------------------------------------------------------------------------------
def grid_faces(n, base=0, reverse=False):
    """Two triangles per quad of an n x n vertex grid (row-major from `base`); reverse turns every winding round."""
    i = np.arange(n - 1)
    y, x = np.meshgrid(i, i, indexing="ij")
    a = (base + y * n + x).reshape(-1)
    b, c, d = a + 1, a + n, a + n + 1
    f = np.stack([np.stack([a, c, b], 1), np.stack([b, c, d], 1)], 1).reshape(-1, 3)
    return (f[:, ::-1] if reverse else f).astype(np.int32)


def double_sheet(n=33, gap=0.004, jitter=1e-4, seed=3):
    """Two n x n grid sheets over [0, 1]^2 with a gentle sine bulge, the second `gap` away with reversed winding; Gaussian jitter from a
    fixed seed. -> (vertices f32 [2 n n, 3], faces int32 [4 (n - 1)^2, 3], normals f32, colors u8)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)
    y, x = np.meshgrid(t, t, indexing="ij")
    z = 0.05 * np.sin(np.pi * x) * np.sin(np.pi * y)
    one = np.stack([x, y, z], -1).reshape(-1, 3)
    two = one + np.array([0.0, 0.0, gap])
    v = np.concatenate([one, two]) + rng.standard_normal((2 * n * n, 3)) * jitter
    faces = np.concatenate([grid_faces(n), grid_faces(n, n * n, reverse=True)])
    nrm = rng.standard_normal((2 * n * n, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])
    nrm[n * n:] *= -1.0
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = rng.integers(0, 256, (2 * n * n, 3)).astype(np.uint8)
    return v.astype(F), np.ascontiguousarray(faces), nrm.astype(F), col


def bad_input_sheet():
    """The double sheet with a NaN vertex, an infinite vertex, a face index of -1 and a face index equal to M."""
    v, f, n, c = double_sheet()
    v, f = v.copy(), f.copy()
    v[40, 1] = np.nan
    v[700, 0] = np.inf
    v[1500, 2] = -np.inf
    f[10, 2] = -1
    f[2000, 0] = len(v)
    f[3000, 1] = len(v) + 7
    return v, f, n, c


def hot_cell_sheet(extra=4096, seed=5):
    """The double sheet plus `extra` vertices inside one cell of the 0.06 grid, referenced by faces that reach into neighbouring cells."""
    v, f, n, c = double_sheet()
    rng = np.random.default_rng(seed)
    M = len(v)
    lo = v.min(axis=0).astype(np.float64)
    centre = lo + 0.06 * (np.array([8.0, 8.0, 0.0]) + 0.5)
    hot = centre + (rng.random((extra, 3)) - 0.5) * 0.05
    hn = rng.standard_normal((extra, 3))
    hn /= np.linalg.norm(hn, axis=1, keepdims=True)
    hc = rng.integers(0, 256, (extra, 3)).astype(np.uint8)
    hi = M + np.arange(extra)
    reach = rng.integers(0, M, (extra, 2))
    hf = np.stack([hi, reach[:, 0], reach[:, 1]], 1).astype(np.int32)
    return (np.concatenate([v, hot.astype(F)]), np.concatenate([f, hf]), np.concatenate([n, hn.astype(F)]), np.concatenate([c, hc]))


def collision_cloud(m=20000, faces=30000, seed=7):
    """m random vertices in a 1 x 1 x 0.3 slab and random faces between near neighbours in index order: at edge 0.04 about 5000 cells."""
    rng = np.random.default_rng(seed)
    v = rng.random((m, 3)) * np.array([1.0, 1.0, 0.3])
    order = np.lexsort((v[:, 0], np.floor(v[:, 1] * 12)))                  # stripes: neighbours in index are near in space
    v = v[order]
    a = rng.integers(0, m, faces)
    f = np.stack([a, (a + rng.integers(1, 40, faces)) % m, (a + rng.integers(1, 40, faces)) % m], 1).astype(np.int32)
    nrm = rng.standard_normal((m, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = rng.integers(0, 256, (m, 3)).astype(np.uint8)
    return v.astype(F), f, nrm.astype(F), col


def odd_normals(vertices, normals, v, at=500):
    """A copy with a NaN, an infinite component and a component of 5.0 (none of the three takes part) and, in the cell of vertex `at`
    on the grid of edge v, an exactly cancelling pair next to members that do not take part: that cell's sum is zero."""
    n = normals.copy()
    n[5, 0] = np.nan
    n[6, 1] = 5.0
    n[7, 2] = -np.inf
    _, _, _, c = grid(vertices, v)
    members = np.nonzero((c == c[at]).all(axis=1) & np.isfinite(vertices).all(axis=1))[0]
    assert len(members) >= 3
    n[members] = (0.0, 0.0, -4.5)
    n[members[0]] = (0.25, -0.5, 0.75)
    n[members[1]] = (-0.25, 0.5, -0.75)
    return n
