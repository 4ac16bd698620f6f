"""numpy restatement of the mesh cleaning rules (include/omnivggt_hip.h: ovg_mesh_topology, ovg_mesh_select, ovg_mesh_smooth), the oracle of
the device kernels bit for bit; a second, deliberately naive form of the same rules (Python loops and integers, a dictionary of edges, a
plain breadth-first search) for small inputs; and the mesh builders of the tests.

  1. a vertex is VALID when its three coordinates are finite;
  2. a face is LIVE when its three indices lie in [0, M), are pairwise different and name valid vertices;
  3. a vertex is REFERENCED when a live face names it;
  4. the edges of a live face are its unordered index pairs, an edge's multiplicity the number of live faces that hold it: 1 is a
     BOUNDARY edge, >= 3 a NON-MANIFOLD edge, and both ends of such an edge carry the flag;
  5. referenced vertices that a live face names together are connected; a component is named by its lowest vertex index.
 topology: vertex_root (-1: unreferenced), face_root (-1: not live), vertex_flags, counts = (live faces, referenced vertices, edges,
     boundary edges, non-manifold edges, boundary vertices, non-manifold vertices, status flags).
 select: a face survives when it is live and kept (face_keep, and vertex_keep at its three corners); the vertices the survivors name in
     ascending index, the survivors in input order with corners renumbered.
 smooth: `iterations` times a step with f32(lam) and, when mu != 0, one with f32(mu). Movable: valid, referenced, not fixed, and not a
     BOUNDARY vertex under fix_boundary -- all decided on the input. One step with factor f, float64, one rounding per operation:
     o, mx = component-wise min, max of the valid current positions; ext = max over axes of (f64(mx) - f64(o)); _, e = frexp(ext), e = 0
     for ext = 0; u = 2^(e - 30); q = rint((f64(p) - f64(o)) / u); S = int64 sum of q over the neighbour multiset (b and c once for every
     live face naming a, b, c), n its size; m = f64(o) + u * (f64(S) / f64(n)); p' = f32(f64(p) + f64(f) * (m - f64(p))).
     normals from the final positions: per live face d1 = pb - pa, d2 = pc - pa (float64), c = d1 x d2, l = sqrt((cx cx + cy cy) + cz cz);
     l finite and > 0: rint(c_k / l * 2^20) to the int64 sums of the three corners; normalised as rule 11 of ovg_mesh_simplify.
"""
from collections import deque

import numpy as np

F = np.float32
REFERENCED, BOUNDARY, NONMANIFOLD = 1, 2, 4
INTERNAL, NONFINITE = 1, 1


class NonFinite(ValueError):
    """The device raises OVG_MSM_NONFINITE here: the outputs are unspecified."""


# ---------------------------------------------------------------------------------------------
# the rules, vectorised
# ---------------------------------------------------------------------------------------------
def live_faces(vertices, faces):
    """-> (p f32 [M, 3], fc int64 [F, 3], valid bool [M], live bool [F]). Rules 1-2."""
    p = np.asarray(vertices, F).reshape(-1, 3)
    fc = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    M = len(p)
    valid = np.isfinite(p).all(axis=1)
    inside = ((fc >= 0) & (fc < M)).all(axis=1)
    a, b, c = fc[:, 0], fc[:, 1], fc[:, 2]
    live = inside & (a != b) & (b != c) & (a != c)
    live[live] = valid[fc[live]].all(axis=1)
    return p, fc, valid, live


def edge_table(fc, live):
    """-> (keys int64 [E] ascending, lo << 32 | hi; multiplicities int64 [E]). Rule 4."""
    lf = fc[live]
    pairs = np.concatenate([lf[:, [0, 1]], lf[:, [1, 2]], lf[:, [2, 0]]])
    keys = (pairs.min(axis=1) << 32) | pairs.max(axis=1)
    return np.unique(keys, return_counts=True)


def vertex_flags(M, fc, live):
    flags = np.zeros(M, np.uint8)
    flags[np.unique(fc[live])] |= REFERENCED
    keys, mult = edge_table(fc, live) if live.any() else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    for bit, sel in ((BOUNDARY, mult == 1), (NONMANIFOLD, mult >= 3)):
        flags[np.unique(np.concatenate([keys[sel] >> 32, keys[sel] & 0xFFFFFFFF]))] |= bit
    return flags, keys, mult


def topology(vertices, faces):
    """-> dict(vertex_root int32 [M], face_root int32 [F], vertex_flags u8 [M], counts int64 [8])."""
    p, fc, valid, live = live_faces(vertices, faces)
    M = len(p)
    flags, keys, mult = vertex_flags(M, fc, live)
    label = np.arange(M, dtype=np.int64)
    lf = fc[live]
    ea, eb = np.concatenate([lf[:, 0], lf[:, 1]]), np.concatenate([lf[:, 1], lf[:, 2]])
    while True:                                                            # label[x] <= x throughout; between rounds every label is a root
        ra, rb = label[ea], label[eb]
        apart = ra != rb
        if not apart.any():
            break
        np.minimum.at(label, np.maximum(ra, rb)[apart], np.minimum(ra, rb)[apart])       # hook the higher root under the lower one
        while True:                                                        # ... and jump until every vertex points at its root again
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
    referenced = (flags & REFERENCED) != 0
    vroot = np.where(referenced, label, -1).astype(np.int32)
    froot = np.full(len(fc), -1, np.int32)
    froot[live] = vroot[lf[:, 0]]
    counts = np.array([live.sum(), referenced.sum(), len(keys), (mult == 1).sum(), (mult >= 3).sum(), ((flags & BOUNDARY) != 0).sum(),
                       ((flags & NONMANIFOLD) != 0).sum(), 0], np.int64)
    return dict(vertex_root=vroot, face_root=froot, vertex_flags=flags, counts=counts)


def labels(vertex_root, face_root, order="size"):
    """The dense numbering of postprocess.mesh_topology -> dict(vertex_labels int32 [M], face_labels int32 [F], roots int32 [C],
    face_sizes int64 [C], vertex_sizes int64 [C]): "size" by descending face count, equal counts by ascending root; "index" by root."""
    roots, fsize = np.unique(face_root[face_root >= 0], return_counts=True)
    vsize = np.array([(vertex_root == r).sum() for r in roots], np.int64)
    if order == "size":
        by = np.argsort(-fsize, kind="stable")
        roots, fsize, vsize = roots[by], fsize[by], vsize[by]
    number = {int(r): k for k, r in enumerate(roots)}
    number[-1] = -1
    return dict(vertex_labels=np.array([number[int(r)] for r in vertex_root], np.int32).reshape(-1),
                face_labels=np.array([number[int(r)] for r in face_root], np.int32).reshape(-1), roots=roots.astype(np.int32),
                face_sizes=fsize.astype(np.int64), vertex_sizes=vsize)


def select(vertices, faces, face_keep=None, vertex_keep=None):
    """-> dict(vertices f32 [M', 3], source_index int64 [M'], faces int32 [F', 3], face_index int64 [F'], counts int64 [2])."""
    p, fc, valid, live = live_faces(vertices, faces)
    surv = live.copy()
    if face_keep is not None:
        surv &= np.asarray(face_keep).reshape(-1) != 0
    if vertex_keep is not None:
        vk = np.asarray(vertex_keep).reshape(-1) != 0
        surv[surv] = vk[fc[surv]].all(axis=1)
    fidx = np.nonzero(surv)[0].astype(np.int64)
    src = np.unique(fc[surv]).astype(np.int64)
    number = np.full(len(p), -1, np.int64)
    number[src] = np.arange(len(src))
    return dict(vertices=p[src].copy(), source_index=src, faces=number[fc[surv]].astype(np.int32).reshape(-1, 3), face_index=fidx,
                counts=np.array([len(src), len(fidx)], np.int64))


def movable_mask(vertices, faces, fixed=None, fix_boundary=True):
    p, fc, valid, live = live_faces(vertices, faces)
    flags, _, _ = vertex_flags(len(p), fc, live)
    mov = valid & ((flags & REFERENCED) != 0)
    if fixed is not None:
        mov &= np.asarray(fixed).reshape(-1) == 0
    if fix_boundary:
        mov &= (flags & BOUNDARY) == 0
    return mov


def frame(P, valid):
    """Rule a -> (o float64 [3], u float64); raises NonFinite."""
    cur = P[valid]
    if not np.isfinite(cur).all():
        raise NonFinite("a valid vertex left the finite range")
    if not len(cur):
        return np.zeros(3), np.ldexp(1.0, -30)
    o, mx = cur.min(axis=0).astype(np.float64), cur.max(axis=0).astype(np.float64)
    ext = float((mx - o).max())
    e = int(np.frexp(ext)[1]) if ext > 0 else 0
    return o, np.ldexp(1.0, e - 30)


def vertex_normals(P, fc, live):
    """Normals of the positions P f32 [M, 3] over the live faces."""
    M = len(P)
    lf = fc[live]
    N = np.zeros((M, 3), np.int64)
    if len(lf):
        pa, pb, pc = (P[lf[:, k]].astype(np.float64) for k in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
            d1, d2 = pb - pa, pc - pa
            c = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2],
                          d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], axis=1)
            l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
            ok = (l > 0) & np.isfinite(l)
            q = np.rint(c[ok] / l[ok][:, None] * 1048576.0).astype(np.int64)
        for k in range(3):
            np.add.at(N, lf[ok][:, k], q)
    x, y, z = (N[:, k].astype(np.float64) for k in range(3))
    length = np.sqrt((x * x + y * y) + z * z)
    ok = (length > 0) & np.isfinite(length)
    safe = np.where(ok, length, 1.0)
    return np.where(ok[:, None], np.stack([x / safe, y / safe, z / safe], axis=1), 0.0).astype(F)


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, fix_boundary=True, normals=True):
    """-> dict(vertices f32 [M, 3], normals f32 [M, 3] or None). Raises NonFinite where the device raises OVG_MSM_NONFINITE."""
    p, fc, valid, live = live_faces(vertices, faces)
    M = len(p)
    P = p.copy()
    factors = [F(lam)] + ([F(mu)] if F(mu) != 0 else [])
    if iterations > 0:
        mov = movable_mask(p, fc, fixed, fix_boundary)
        lf = fc[live]
        own = np.concatenate([lf[:, 0], lf[:, 0], lf[:, 1], lf[:, 1], lf[:, 2], lf[:, 2]])
        other = np.concatenate([lf[:, 1], lf[:, 2], lf[:, 2], lf[:, 0], lf[:, 0], lf[:, 1]])
        n = np.bincount(own, minlength=M).astype(np.float64)
        for _ in range(iterations):
            for f in factors:
                o, u = frame(P, valid)
                q = np.zeros((M, 3), np.int64)
                q[valid] = np.rint((P[valid].astype(np.float64) - o) / u).astype(np.int64)
                assert q.min() >= 0 and q.max() <= 1 << 30
                S = np.zeros((M, 3), np.int64)
                np.add.at(S, own, q[other])
                mean = S[mov].astype(np.float64) / n[mov][:, None]
                target = o + u * mean
                cur = P[mov].astype(np.float64)
                with np.errstate(over="ignore"):
                    P[mov] = (cur + np.float64(f) * (target - cur)).astype(F)
        if not np.isfinite(P[valid]).all():
            raise NonFinite("a valid vertex left the finite range")
    return dict(vertices=P, normals=vertex_normals(P, fc, live) if normals else None)


# ---------------------------------------------------------------------------------------------
# the rules once more, naively
# ---------------------------------------------------------------------------------------------
def _naive_live(p, faces):
    M = len(p)
    ok = [all(np.isfinite(float(x)) for x in row) for row in p]
    out = []
    for j, (a, b, c) in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if min(a, b, c) < 0 or max(a, b, c) >= M or len({a, b, c}) < 3 or not (ok[a] and ok[b] and ok[c]):
            continue
        out.append((j, a, b, c))
    return ok, out


def _naive_flags(M, live):
    edges, flags = {}, [0] * M
    for _, a, b, c in live:
        for x, y in ((a, b), (b, c), (c, a)):
            edges[(min(x, y), max(x, y))] = edges.get((min(x, y), max(x, y)), 0) + 1
        for x in (a, b, c):
            flags[x] |= REFERENCED
    for (x, y), k in edges.items():
        bit = BOUNDARY if k == 1 else (NONMANIFOLD if k >= 3 else 0)
        flags[x] |= bit
        flags[y] |= bit
    return edges, flags


def topology_naive(vertices, faces):
    p = np.asarray(vertices, F).reshape(-1, 3)
    M, nf = len(p), len(np.asarray(faces).reshape(-1, 3))
    _, live = _naive_live(p, faces)
    edges, flags = _naive_flags(M, live)
    near = {}
    for _, a, b, c in live:
        for x in (a, b, c):
            near.setdefault(x, set()).update((a, b, c))
    root = [-1] * M
    for start in range(M):                                                 # ascending: the start of a search is its component's lowest index
        if start not in near or root[start] >= 0:
            continue
        root[start] = start
        todo = deque([start])
        while todo:
            for y in near[todo.popleft()]:
                if root[y] < 0:
                    root[y] = start
                    todo.append(y)
    froot = [-1] * nf
    for j, a, _, _ in live:
        froot[j] = root[a]
    counts = [len(live), sum(1 for x in flags if x & REFERENCED), len(edges), sum(1 for k in edges.values() if k == 1),
              sum(1 for k in edges.values() if k >= 3), sum(1 for x in flags if x & BOUNDARY), sum(1 for x in flags if x & NONMANIFOLD), 0]
    return dict(vertex_root=np.array(root, np.int32), face_root=np.array(froot, np.int32).reshape(-1), vertex_flags=np.array(flags, np.uint8),
                counts=np.array(counts, np.int64))


def smooth_naive(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, fix_boundary=True, normals=True):
    p = np.asarray(vertices, F).reshape(-1, 3)
    M = len(p)
    ok, live = _naive_live(p, faces)
    _, flags = _naive_flags(M, live)
    rows = [[] for _ in range(M)]
    for _, a, b, c in live:
        rows[a] += [b, c]
        rows[b] += [c, a]
        rows[c] += [a, b]
    mov = [ok[i] and bool(flags[i] & REFERENCED) and not (fixed is not None and fixed[i]) and not (fix_boundary and flags[i] & BOUNDARY)
           for i in range(M)]
    P = [[float(x) for x in row] for row in p]                              # the f32 values, held as Python floats
    for _ in range(iterations):
        for f in [float(F(lam))] + ([float(F(mu))] if F(mu) != 0 else []):
            cur = [P[i] for i in range(M) if ok[i]]
            if not all(np.isfinite(x) for row in cur for x in row):
                raise NonFinite("a valid vertex left the finite range")
            o = [min(row[k] for row in cur) for k in range(3)]
            ext = max(max(row[k] for row in cur) - o[k] for k in range(3))
            e = int(np.frexp(ext)[1]) if ext > 0 else 0
            u = 2.0 ** (e - 30)
            q = [[int(np.rint((P[i][k] - o[k]) / u)) if ok[i] else 0 for k in range(3)] for i in range(M)]
            new = [row[:] for row in P]
            for i in range(M):
                if not mov[i]:
                    continue
                for k in range(3):
                    S = sum(q[j][k] for j in rows[i])
                    m = o[k] + u * (float(S) / float(len(rows[i])))
                    with np.errstate(over="ignore"):
                        new[i][k] = float(F(P[i][k] + f * (m - P[i][k])))
            P = new
    out = np.array(P, np.float64).astype(F).reshape(M, 3)
    out[~np.array(ok, bool)] = p[~np.array(ok, bool)]                       # NaN payloads do not survive a Python float: the input bytes do
    if iterations > 0 and not np.isfinite(out[np.array(ok, bool)]).all():
        raise NonFinite("a valid vertex left the finite range")
    fc = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    lv = np.zeros(len(fc), bool)
    lv[[j for j, _, _, _ in live]] = True
    return dict(vertices=out, normals=vertex_normals(out, fc, lv) if normals else None)


# ---------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """-> (vertices f32 [10 * 4^s + 2, 3], faces int32 [20 * 4^s, 3]), outward facing."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.array(centre, np.float64)).astype(F), np.array(f, np.int32)


def noisy_icosphere(subdivisions, noise=0.02, seed=1):
    v, f = icosphere(subdivisions)
    scale = 1.0 + noise * np.random.default_rng(seed).standard_normal(len(v))
    return (v.astype(np.float64) * scale[:, None]).astype(F), f


def grid_sheet(nx, ny, spacing=0.125, origin=(0.0, 0.0, 0.0)):
    """An open sheet of nx x ny vertices (vertex y * nx + x), 2 (nx - 1) (ny - 1) faces."""
    y, x = np.mgrid[0:ny, 0:nx]
    v = np.stack([x.reshape(-1) * spacing, y.reshape(-1) * spacing, np.zeros(nx * ny)], axis=1) + np.array(origin, np.float64)
    cy, cx = np.mgrid[0:ny - 1, 0:nx - 1]
    a = (cy * nx + cx).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + nx + 1], axis=1), np.stack([a, a + nx + 1, a + nx], axis=1)])
    return v.astype(F), f.astype(np.int32)


def sheet_rim(nx, ny):
    y, x = np.mgrid[0:ny, 0:nx]
    return ((x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1)).reshape(-1)


def relabel(v, f, seed):
    """The same mesh with its vertex numbers randomly permuted and its faces shuffled -> (v, f, new number of every old vertex)."""
    rng = np.random.default_rng(seed)
    new = rng.permutation(len(v))
    out = np.empty_like(v)
    out[new] = v
    return out, np.ascontiguousarray(new[f][rng.permutation(len(f))].astype(np.int32)), new


def zoo(seed=0):
    """Two spheres, an open sheet, three faces on one edge, two faces meeting in one vertex, a duplicated face, five unreferenced vertices,
    a NaN vertex and junk faces, relabelled by `seed` -> dict(vertices, faces, parts: name -> the part's vertex numbers)."""
    pieces = [("sphere2", icosphere(2)), ("sphere1", icosphere(1, 0.5, (3.0, 0.0, 0.0))), ("sheet", grid_sheet(9, 9, 0.125, (0.0, 3.0, 0.0))),
              ("triple", (np.array([[0, 0, 5], [1, 0, 5], [0.5, 1, 5], [0.5, -1, 5], [0.5, 0, 6]], F), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32))),
              ("corner", (np.array([[5, 0, 0], [6, 1, 0], [6, -1, 0], [4, 1, 0], [4, -1, 0]], F), np.array([[0, 1, 2], [0, 4, 3]], np.int32))),
              ("double", (np.array([[8, 0, 0], [9, 0, 0], [8, 1, 0]], F), np.array([[0, 1, 2], [0, 1, 2]], np.int32))),
              ("loose", (np.array([[k, -4.0, 0.5 * k] for k in range(5)], F), np.zeros((0, 3), np.int32))),
              ("nan", (np.array([[np.nan, 0, 0]], F), np.zeros((0, 3), np.int32)))]
    vs, fs, span, base = [], [], {}, 0
    for name, (v, f) in pieces:
        vs.append(v)
        fs.append(f.astype(np.int64) + base)
        span[name] = np.arange(base, base + len(v))
        base += len(v)
    nan, s2 = int(span["nan"][0]), span["sphere2"]
    fs.append(np.array([[s2[0], s2[1], nan]], np.int64))                    # names the NaN vertex
    v, f, new = relabel(np.concatenate(vs), np.concatenate(fs), seed)
    M = len(v)
    junk = np.array([[-1, new[s2[0]], new[s2[1]]], [new[s2[2]], M, new[s2[3]]], [new[s2[4]], new[s2[4]], new[s2[5]]]], np.int32)
    rng = np.random.default_rng(seed + 1000)
    f = np.insert(f, rng.integers(0, len(f), len(junk)), junk, axis=0)
    return dict(vertices=v, faces=np.ascontiguousarray(f), parts={k: np.sort(new[idx]) for k, idx in span.items()})


def ribbon(n=35000, seed=11):
    """A 2 x n strip, 2 (n - 1) faces, relabelled: one component whose root is vertex 0."""
    v, f = grid_sheet(n, 2, 0.01)
    return relabel(v, f, seed)[:2]


def quads(k=3000, seed=12):
    """k disjoint quads of two faces each, relabelled -> (v, f, the four vertex numbers of every quad [k, 4])."""
    base = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    v = np.concatenate([base + np.array([3.0 * (i % 64), 3.0 * (i // 64), 0.0]) for i in range(k)]).astype(F)
    f = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]]) + 4 * i for i in range(k)]).astype(np.int32)
    v, f, new = relabel(v, f, seed)
    return v, f, new.reshape(k, 4)


def fan(n=5000):
    """A closed fan of n faces around vertex 0, which stands above the rim's plane: a row of 2 n neighbours, n boundary edges."""
    ang = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1)]).astype(F)
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)


def volume(v, f):
    a, b, c = (np.asarray(v, np.float64)[np.asarray(f)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def radius_spread(v):
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(r.std() / r.mean())
