"""Device time of the four map-geometry entries (ops.map_depth, map_normals, map_edges, map_triangulate) for 8 and 64 views of 518^2 of
a synthetic scene made on the device (a bumpy backdrop, a box in front of it, 2 % dead pixels), with every tile shape of the edge
kernel at every window radius, with and without normals: torch events round `inner` back-to-back calls, 2 warm-ups, median
(min .. max) of 9 samples, per call. Bytes are what the rule needs (each map read once, each output written once), so GB/s is a
lower bound on the traffic of the stencils.
Set against the same computations as torch operations on the same GPU, which are not the code under test and do not follow the exact
rules (no per-pixel tolerance in the differences, no one-sided fall-back, no ordered compaction): max_pool2d of +-z for the depth
edge, sliced central differences + torch.linalg.cross for the normals, boolean indexing of the two face tables for the mesh.

    python tools/probes/mapgeom_probe.py [--views 8 64] [--out profiles/mapgeom_probe.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from omnivggt_official_amd import lib as L, ops  # noqa: E402

H = W = 518
TOL, NEAR = 0.03, 1e-3
TILES = (("default", L.MAP_TILE_DEFAULT), ("256x1", L.MAP_TILE_256x1), ("16x16", L.MAP_TILE_16x16), ("32x8", L.MAP_TILE_32x8), ("64x4", L.MAP_TILE_64x4))


def timed(fn, inner=5, warm=2, reps=9):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%7.3f (%.3f .. %.3f)" % t


def scene(S):
    g = torch.Generator(device="cuda").manual_seed(S)
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    s = torch.arange(S, device="cuda", dtype=torch.float32)[:, None, None]
    z = 4.0 + 0.2 * torch.sin(x / 40.0 + s) * torch.cos(y / 55.0) + 0.0005 * torch.rand(S, H, W, device="cuda", generator=g)
    box = (x > 150 + 2 * s) & (x < 330 + 2 * s) & (y > 120) & (y < 360)
    z = torch.where(box, z - 1.8, z)
    pts = torch.stack([(x - W / 2) * z / 500.0, (y - H / 2) * z / 500.0, z], -1).contiguous()
    valid = (torch.rand(S, H, W, device="cuda", generator=g) > 0.02).to(torch.uint8)
    cams = torch.zeros(S, 16, device="cuda")
    cams[:, 0] = cams[:, 4] = cams[:, 8] = 1.0
    cams[:, 12] = cams[:, 13] = 500.0
    cams[:, 14], cams[:, 15] = W / 2, H / 2
    colors = (torch.rand(S, H, W, 3, device="cuda", generator=g) * 255).to(torch.uint8)
    return pts, cams, valid, colors


def torch_edges(z, r):
    zz = z[:, None]
    hi = torch.nn.functional.max_pool2d(torch.nan_to_num(zz, nan=-float("inf")), 2 * r + 1, 1, r)
    lo = -torch.nn.functional.max_pool2d(torch.nan_to_num(-zz, nan=-float("inf")), 2 * r + 1, 1, r)
    return ((hi - lo) > TOL * zz)[:, 0]


def torch_normals(pts):
    dh = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    dv = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    n = torch.linalg.cross(dv, dh)
    return torch.nn.functional.pad(n / n.norm(dim=-1, keepdim=True), (0, 0, 1, 1, 1, 1))


def torch_mesh(z, pts, S):
    ok = ~torch.isnan(z)
    idx = torch.arange(S * H * W, device="cuda").reshape(S, H, W)
    a, b, c, d = idx[:, :-1, :-1], idx[:, :-1, 1:], idx[:, 1:, :-1], idx[:, 1:, 1:]
    oa, ob, oc, od = ok[:, :-1, :-1], ok[:, :-1, 1:], ok[:, 1:, :-1], ok[:, 1:, 1:]
    f0 = torch.stack([a, c, b], -1)[oa & oc & ob]
    f1 = torch.stack([b, c, d], -1)[ob & oc & od]
    faces = torch.cat([f0, f1])
    used = torch.zeros(S * H * W, dtype=torch.bool, device="cuda")
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    return pts.reshape(-1, 3)[used], remap[faces]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapgeom_probe.txt"))
    a = ap.parse_args()
    L.require_gpu()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("map geometry of S views of %d x %d, rel_tol %.2f; device times per call: median (min .. max) of 9 samples of 5 calls after 2 warm-ups, ms" % (H, W, TOL))
    say("%s, torch %s" % (L.load().ovg_build_info().decode(), torch.__version__))
    for S in a.views:
        n = S * H * W
        pts, cams, valid, colors = scene(S)
        z = ops.map_depth(points=pts, cams=cams, valid=valid, near=NEAR)
        normals = ops.map_normals(pts, z, rel_tol=TOL)
        flags = ops.map_edges(z, normals, radius=1, rel_tol=TOL, min_cos=0.866)
        torch.cuda.synchronize()
        usable = int((flags != L.MAP_UNUSABLE).sum())
        say()
        say("S = %d: %d pixels, %d usable, depth edges at r = 1: %.3f of the usable, normal edges %.3f, no normal %.4f" % (
            S, n, usable, float(((flags & L.MAP_DEPTH_EDGE) != 0).sum()) / usable, float(((flags & L.MAP_NORMAL_EDGE) != 0).sum()) / usable,
            float(((flags & L.MAP_NO_NORMAL) != 0).sum()) / usable))
        zb, nb, fb = torch.empty_like(z), torch.empty_like(normals), torch.empty_like(flags)
        t = timed(lambda: ops.map_depth(points=pts, cams=cams, valid=valid, near=NEAR, out=zb))
        say("map_depth from points      %s  %7.1f GB/s (17 B / pixel)" % (fmt(t), 17 * n / t[0] / 1e6))
        t = timed(lambda: ops.map_normals(pts, z, rel_tol=TOL, out=nb))
        say("map_normals                %s  %7.1f GB/s (28 B / pixel)" % (fmt(t), 28 * n / t[0] / 1e6))
        t = timed(lambda: torch_normals(pts))
        say("  torch: sliced differences + linalg.cross + normalise   %s" % fmt(t))
        best = {}
        for wn, label in ((None, "z only"), (normals, "z + normals")):
            say("map_edges, %s (%d B / pixel)      r = 1                      r = 2                      r = 3" % (label, 17 if wn is not None else 5))
            for name, tile in TILES:
                row = []
                for r in (1, 2, 3):
                    t = timed(lambda: ops.map_edges(z, wn, radius=r, rel_tol=TOL, min_cos=0.866, tile=tile, out=fb))
                    row.append(t)
                    key = (label, r)
                    if key not in best or t[0] < best[key][1]:
                        best[key] = (name, t[0])
                say("  tile %-7s %s" % (name, "   ".join(fmt(t) for t in row)))
            say("  best: %s" % ", ".join("r = %d %s %.3f ms = %.0f GB/s" % (r, best[(label, r)][0], best[(label, r)][1],
                                                                           (17 if wn is not None else 5) * n / best[(label, r)][1] / 1e6) for r in (1, 2, 3)))
        say("  torch: max_pool2d of +z and -z, z only                  %s" % "   ".join(fmt(timed(lambda: torch_edges(z, r))) for r in (1, 2, 3)))
        keep = ((flags & L.MAP_DEPTH_EDGE) == 0).to(torch.uint8)
        ws = torch.empty(ops.map_triangulate_workspace_bytes(S, H, W), device="cuda", dtype=torch.uint8)
        count = torch.empty(2, device="cuda", dtype=torch.int64)
        args = dict(z=z, points=pts, ws=ws, rel_tol=TOL, keep=keep, normals=normals, colors=colors, out_count=count)
        ops.map_triangulate(L.MAP_COUNT, **args)
        M, F = (int(v) for v in count.cpu())
        v, vn = torch.empty(M, 3, device="cuda"), torch.empty(M, 3, device="cuda")
        vc, vi = torch.empty(M, 3, device="cuda", dtype=torch.uint8), torch.empty(M, device="cuda", dtype=torch.int64)
        f = torch.empty(F, 3, device="cuda", dtype=torch.int32)
        tc = timed(lambda: ops.map_triangulate(L.MAP_COUNT, **args))
        ts = timed(lambda: ops.map_triangulate(L.MAP_SCATTER, vertex_capacity=M, face_capacity=F, vertices=v, out_normals=vn, out_colors=vc,
                                               pixel_index=vi, faces=f, **args))
        say("map_triangulate: %d vertices, %d faces; COUNT %s   SCATTER %s" % (M, F, fmt(tc), fmt(ts)))
        say("  torch: boolean indexing of the two face tables + remap (no tear test, no keep, positions only)   %s" % fmt(timed(lambda: torch_mesh(z, pts, S), inner=1)))
        del pts, z, normals, flags, zb, nb, fb, ws, v, vn, vc, vi, f, keep, colors, valid
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
