"""Device time of the mesh simplification (ops.mesh_simplify / postprocess.simplify_mesh) on the grid meshes of 8 and 64 views of 518^2
(tools/probes/mapgeom_probe.py's scene through map_depth / map_normals / triangulate_maps) and on the surface-nets mesh of a 256^3
fusion (tools/probes/tsdf_probe.py's scene), for cell edges that keep about 1/4, 1/16 and 1/64 of the vertices: torch events, 3
warm-ups, median (min .. max) of 20, per stage and for the whole Python call (its one synchronisation and its allocations included).
Set against the same clustering as torch operations on the same GPU (torch.unique on the cell keys and on the sorted cell triples,
index_add_ for the sums; float32 means, not the exact rule, not the code under test) and against the numpy twin on the host
(tests/meshsimp_twin.py, the device -> host copy of the mesh included). Also the bytes and the wall-clock of write_mesh_glb before and
after.

    python tools/probes/meshsimp_probe.py [--views 8 64] [--fusion 256] [--no-host] [--no-torch] [--no-export] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from omnivggt_official_amd import lib as L, ops, postprocess  # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def f3(t):
    return "%.3f (%.3f .. %.3f)" % t


def grid_mesh(S):
    import mapgeom_probe as mp
    pts, cams, valid, colors = mp.scene(S)
    z = ops.map_depth(points=pts, cams=cams, valid=valid, near=mp.NEAR)
    normals = ops.map_normals(pts, z, rel_tol=mp.TOL)
    return postprocess.triangulate_maps(pts, z, images=colors, normals=normals, rel_tol=mp.TOL)


def fusion_mesh(n, S=8, HW=518):
    import consistency_twin as ctwin
    pts, ext, intr = ctwin.device_scene(S, HW, HW)
    cams = torch.from_numpy(ctwin.pack_cams(ext, intr)).cuda()
    R, t = torch.from_numpy(ext[:, :, :3]).cuda(), torch.from_numpy(ext[:, :, 3]).cuda()
    depth = (torch.einsum("sj,shwj->shw", R[:, 2], pts.double()) + t[:, 2, None, None]).float().contiguous()
    voxel = float(np.float32(3.0 / (n - 1)))
    vol = postprocess.tsdf_volume((-1.5, -1.5, -1.5), voxel, (n, n, n), trunc=float(np.float32(4.0 * voxel)), color=False)
    ops.tsdf_integrate(vol.tsdf, vol.weight, depth, cams, vol.origin, vol.voxel_size, vol.trunc)
    mesh = postprocess.tsdf_extract(vol)
    M = int(mesh.vertices.shape[0])
    mesh.scene_scale = ops.percentile(mesh.vertices, M, 3, 1, 3, [5.0, 95.0], norm=True)[1]
    return mesh


def rel_for(mesh, fraction):
    """rel_size that keeps about `fraction` of the vertices: bisection on log(rel_size)."""
    lo, hi = 1e-5, 1.0
    M = int(mesh.vertices.shape[0])
    for _ in range(16):
        mid = (lo * hi) ** 0.5
        if postprocess.simplify_mesh(mesh, rel_size=mid, position="first").vertices.shape[0] > fraction * M:
            lo = mid
        else:
            hi = mid
    return (lo * hi) ** 0.5


def stages(mesh, rel):
    """(count stage, scatter stage, workspace bytes) on preallocated buffers, as simplify_mesh issues them."""
    M, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    voxel = torch.full((), rel, device="cuda") * mesh.scene_scale.reshape(())
    ws = torch.empty(ops.mesh_simplify_workspace_bytes(M, F), device="cuda", dtype=torch.uint8)
    count = torch.empty(6, device="cuda", dtype=torch.int64)
    args = dict(vertices=mesh.vertices, faces=mesh.faces, voxel=voxel, ws=ws, normals=mesh.normals, colors=mesh.colors, out_count=count)
    ops.mesh_simplify(L.MS_COUNT, **args)
    Mo, Fo = (int(v) for v in count[:2].cpu())
    out = dict(out_vertices=torch.empty(Mo, 3, device="cuda"), out_normals=torch.empty(Mo, 3, device="cuda"),
               out_colors=torch.empty(Mo, 3, device="cuda", dtype=torch.uint8), source_index=torch.empty(Mo, device="cuda", dtype=torch.int64),
               vertex_count=torch.empty(Mo, device="cuda", dtype=torch.int32), out_faces=torch.empty(Fo, 3, device="cuda", dtype=torch.int32))
    return (lambda: ops.mesh_simplify(L.MS_COUNT, **args),
            lambda: ops.mesh_simplify(L.MS_SCATTER, vertex_capacity=Mo, face_capacity=Fo, **out, **args), ws.numel())


def torch_simplify(mesh, voxel):
    """The same clustering as torch operations: float32 means, no exact rule. -> (vertices, faces)."""
    v, f = mesh.vertices, mesh.faces.long()
    ok = torch.isfinite(v).all(dim=1)
    origin = v[ok].min(dim=0).values
    c = torch.floor((v - origin) / voxel).long()
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, cell = torch.unique(key, return_inverse=True)
    ncell = int(cell.max()) + 1
    fc = cell[f]
    live = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    fc = fc[live]
    tri = torch.sort(fc, dim=1).values
    packed = (tri[:, 0] * ncell + tri[:, 1]) * ncell + tri[:, 2] if ncell < (1 << 21) else None
    if packed is not None:
        _, inv = torch.unique(packed, return_inverse=True)
    else:
        _, inv = torch.unique(tri, dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), fc.shape[0], device=v.device, dtype=torch.long)
    first.scatter_reduce_(0, inv, torch.arange(fc.shape[0], device=v.device), "amin")
    faces = fc[torch.sort(first).values]
    used, renum = torch.unique(faces, return_inverse=True)
    sums = torch.zeros(ncell, 3, device=v.device).index_add_(0, cell, v)
    n = torch.zeros(ncell, device=v.device).index_add_(0, cell, torch.ones_like(v[:, 0]))
    return (sums / n[:, None])[used], renum


def probe(name, mesh, a):
    import meshsimp_twin as twin
    M, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    say("\n%s: M = %d vertices, F = %d faces, scene_scale %.4f" % (name, M, F, float(mesh.scene_scale)))
    say("%-6s %9s %10s %10s %10s %10s | %-26s %-26s %-26s | %-26s | %s" % ("keep", "rel_size", "M'", "F'", "degenerate", "duplicates", "count stage",
                                                                           "scatter stage", "whole call (sync + allocs)", "torch operations", "host numpy incl. copy"))
    rels = {}
    for frac in (1 / 4, 1 / 16, 1 / 64):
        rel = rels[frac] = rel_for(mesh, frac)
        out = postprocess.simplify_mesh(mesh, rel_size=rel)
        cnt, sct, ws_bytes = stages(mesh, rel)
        t_c, t_s = timed(cnt), timed(sct)
        t_w = timed(lambda: postprocess.simplify_mesh(mesh, rel_size=rel))
        voxel = torch.full((), rel, device="cuda") * mesh.scene_scale.reshape(())
        tch = "-"
        if not a.no_torch and M <= a.torch_max:
            tv, tf = torch_simplify(mesh, voxel)
            same = tv.shape[0] == out.vertices.shape[0] and tf.shape[0] == out.faces.shape[0]
            tch = f3(timed(lambda: torch_simplify(mesh, voxel), warm=1, reps=5)) + ("" if same else " [counts differ: %d, %d]" % (tv.shape[0], tf.shape[0]))
        host = "-"
        if not a.no_host and M <= a.host_max:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arrays = [t.cpu().numpy() for t in (mesh.vertices, mesh.faces, mesh.normals, mesh.colors)]
            want = twin.simplify(arrays[0], arrays[1], np.float32(voxel.cpu().numpy()), arrays[2], arrays[3])
            ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(want["vertices"].view(np.uint32), out.vertices.cpu().numpy().view(np.uint32))
            assert np.array_equal(want["faces"], out.faces.cpu().numpy())
            host = "%.0f ms (1 run, bytes equal) = %.0fx the device call" % (ms, ms / t_w[0])
        say("1/%-4d %9.6f %10d %10d %10d %10d | %-26s %-26s %-26s | %-26s | %s" % (round(1 / frac), rel, out.vertices.shape[0], out.faces.shape[0],
                                                                                 out.degenerate_faces, out.duplicate_faces, f3(t_c), f3(t_s), f3(t_w), tch, host))
        del out, cnt, sct
        torch.cuda.empty_cache()
    say("workspace %.1f MB for M = %d, F = %d" % (ws_bytes / 1e6, M, F))
    if not a.no_export:
        with tempfile.TemporaryDirectory() as d:
            rows = []
            for label, rel in (("as it is", None), ("keep 1/16", rels[1 / 16]), ("keep 1/64", rels[1 / 64])):
                path = os.path.join(d, "mesh.glb")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = mesh if rel is None else postprocess.simplify_mesh(mesh, rel_size=rel)
                postprocess.write_mesh_glb(path, m)
                rows.append((label, (time.perf_counter() - t0) * 1e3, os.path.getsize(path), int(m.vertices.shape[0]), int(m.faces.shape[0])))
            for label, ms, size, mv, mf in rows:
                say("export %swrite_mesh_glb: %-10s %9.1f ms wall, %11d bytes, %9d vertices, %9d faces (%.1fx faster, %.1fx smaller)"
                    % ("simplify_mesh + " if label != "as it is" else "", label, ms, size, mv, mf, rows[0][1] / ms, rows[0][2] / size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--fusion", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-export", action="store_true")
    ap.add_argument("--host-max", type=int, default=3000000, help="largest mesh (vertices) the numpy twin is run on")
    ap.add_argument("--torch-max", type=int, default=3000000, help="largest mesh (vertices) the torch form is run on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.require_gpu()
    say("mesh simplification by vertex clustering; device times: median (min .. max) of 20 after 3 warm-ups, ms; torch form: of 5 after 1")
    for S in a.views:
        probe("grid mesh of %d views of 518^2" % S, grid_mesh(S), a)
        torch.cuda.empty_cache()
    if a.fusion:
        probe("surface-nets mesh of a %d^3 fusion of 8 views" % a.fusion, fusion_mesh(a.fusion), a)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
