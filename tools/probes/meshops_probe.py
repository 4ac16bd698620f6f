"""Device time of the mesh cleaning entries (ops.mesh_topology, ops.mesh_select, ops.mesh_smooth and the postprocess calls around them) on
the grid meshes of 8 and 64 views of 518^2 and on the surface-nets mesh of a 256^3 fusion (the meshes of tools/probes/meshsimp_probe.py):
torch events, 3 warm-ups, median (min .. max) of 20. Set against the same smoothing as float64 index_add_ torch operations on the same GPU
(umbrella means by float atomics: not the exact rule, not the code under test) and against scipy.sparse.csgraph.connected_components on
the host (the device -> host copy of the faces included).

    python tools/probes/meshops_probe.py [--views 8 64] [--fusion 256] [--iterations 10] [--no-host] [--no-torch] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from omnivggt_official_amd import lib as L, ops, postprocess  # noqa: E402
from meshsimp_probe import LINES, f3, fusion_mesh, grid_mesh, say, timed  # noqa: E402


def torch_smooth(v, f, iterations, lam, mu, movable):
    """Taubin smoothing as torch operations in float64: per step two index_add_ per corner pair, a division, a blend."""
    f = f.long()
    own = torch.cat([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    other = torch.cat([f[:, 1], f[:, 2], f[:, 2], f[:, 0], f[:, 0], f[:, 1]])
    n = torch.zeros(v.shape[0], device=v.device, dtype=torch.float64).index_add_(0, own, torch.ones_like(own, dtype=torch.float64))
    n = n.clamp_min(1.0)[:, None]
    p = v.double()
    for _ in range(iterations):
        for factor in (lam, mu):
            mean = torch.zeros_like(p).index_add_(0, own, p[other]) / n
            p = torch.where(movable[:, None], p + factor * (mean - p), p)
    return p.float()


def probe(name, mesh, a):
    M, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    v, f = mesh.vertices, mesh.faces
    say("\n%s: M = %d vertices, F = %d faces" % (name, M, F))
    top = postprocess.mesh_topology(mesh)
    say("components %d (largest %d faces), live faces %d, edges %d, boundary edges %d, non-manifold edges %d, euler %d"
        % (top.num_components, int(top.face_sizes[0]) if top.num_components else 0, top.live_faces, top.edges, top.boundary_edges,
           top.nonmanifold_edges, top.euler))
    # ovg_mesh_topology
    ws = torch.empty(ops.mesh_topology_workspace_bytes(M, F), device="cuda", dtype=torch.uint8)
    vr, fr = torch.empty(M, device="cuda", dtype=torch.int32), torch.empty(F, device="cuda", dtype=torch.int32)
    fl, cnt = torch.empty(M, device="cuda", dtype=torch.uint8), torch.empty(8, device="cuda", dtype=torch.int64)
    t_top = timed(lambda: ops.mesh_topology(v, f, ws, vr, fr, fl, cnt))
    t_top_call = timed(lambda: postprocess.mesh_topology(mesh))
    say("topology: entry %s ms, postprocess.mesh_topology (labels, one read-back) %s ms, workspace %.1f MB" % (f3(t_top), f3(t_top_call), ws.numel() / 1e6))
    host = "-"
    if not a.no_host and F <= a.host_max:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fc = f.cpu().numpy().astype(np.int64)
        rows, cols = np.concatenate([fc[:, 0], fc[:, 1]]), np.concatenate([fc[:, 1], fc[:, 2]])
        ncomp, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(M, M)), directed=False)
        ms = (time.perf_counter() - t0) * 1e3
        ref = (top.vertex_root >= 0).cpu().numpy()
        same = len(np.unique(lab[ref])) == top.num_components
        host = "%.0f ms (1 run, %s) = %.0fx the entry" % (ms, "same number of components" if same else "COMPONENTS DIFFER", ms / t_top[0])
    say("topology: scipy connected_components on the host incl. copy: %s" % host)
    del ws
    # ovg_mesh_select with the mask of remove_small_components(keep_largest=True)
    keep = (top.face_labels == 0).to(torch.uint8)
    ws = torch.empty(ops.mesh_select_workspace_bytes(M, F), device="cuda", dtype=torch.uint8)
    c2 = torch.empty(2, device="cuda", dtype=torch.int64)
    args = dict(vertices=v, faces=f, ws=ws, face_keep=keep, out_count=c2)
    ops.mesh_select(L.MSEL_COUNT, **args)
    Mo, Fo = (int(x) for x in c2.cpu())
    out = dict(out_vertices=torch.empty(Mo, 3, device="cuda"), source_index=torch.empty(Mo, device="cuda", dtype=torch.int64),
               out_faces=torch.empty(Fo, 3, device="cuda", dtype=torch.int32), face_index=torch.empty(Fo, device="cuda", dtype=torch.int64))
    t_cnt = timed(lambda: ops.mesh_select(L.MSEL_COUNT, **args))
    t_sct = timed(lambda: ops.mesh_select(L.MSEL_SCATTER, vertex_capacity=Mo, face_capacity=Fo, **out, **args))
    t_rsc = timed(lambda: postprocess.remove_small_components(mesh, keep_largest=True))
    say("select (largest component: %d vertices, %d faces): COUNT %s ms, SCATTER %s ms, workspace %.1f MB; remove_small_components whole call %s ms"
        % (Mo, Fo, f3(t_cnt), f3(t_sct), ws.numel() / 1e6, f3(t_rsc)))
    del ws, out
    # ovg_mesh_smooth
    ws = torch.empty(ops.mesh_smooth_workspace_bytes(M, F), device="cuda", dtype=torch.uint8)
    ov, on, st = torch.empty(M, 3, device="cuda"), torch.empty(M, 3, device="cuda"), torch.empty(1, device="cuda", dtype=torch.int64)
    it = a.iterations
    t_0 = timed(lambda: ops.mesh_smooth(v, f, ws, 0, 0.5, -0.53, ov, st, out_normals=on))
    t_1 = timed(lambda: ops.mesh_smooth(v, f, ws, 1, 0.5, -0.53, ov, st, out_normals=on))
    t_n = timed(lambda: ops.mesh_smooth(v, f, ws, it, 0.5, -0.53, ov, st, out_normals=on))
    t_call = timed(lambda: postprocess.smooth_mesh(mesh, iterations=it))
    step = (t_n[0] - t_1[0]) / max(2 * (it - 1), 1)
    say("smooth: normals only %s ms, 1 iteration %s ms, %d Taubin iterations + normals %s ms = %.3f ms per step (%.0f GB/s of the 80 M + 24 F "
        "bytes a step streams, the gathered records not counted), adjacency and flags %.3f ms, workspace %.1f MB; smooth_mesh whole call %s ms"
        % (f3(t_0), f3(t_1), it, f3(t_n), step, (80.0 * M + 24.0 * F) / 1e6 / max(step, 1e-9), t_1[0] - t_0[0] - 2 * step, ws.numel() / 1e6, f3(t_call)))
    ops.mesh_smooth(v, f, ws, it, 0.5, -0.53, ov, st, out_normals=on)
    a_bytes = ov.clone()
    ops.mesh_smooth(v, f, ws, it, 0.5, -0.53, ov, st, out_normals=on)
    say("smooth: two runs give identical bytes: %s; status %d" % (bool(torch.equal(a_bytes.view(torch.int32), ov.view(torch.int32))), int(st.cpu())))
    if not a.no_torch and M <= a.torch_max:
        live = top.face_root >= 0
        movable = ((top.vertex_flags & L.MT_REFERENCED) != 0) & ((top.vertex_flags & L.MT_BOUNDARY) == 0)
        fl_ = f[live]
        ref = torch_smooth(v, fl_, it, 0.5, -0.53, movable)
        err = float((ref - ov)[torch.isfinite(ref).all(dim=1)].abs().max())
        t_t = timed(lambda: torch_smooth(v, fl_, it, 0.5, -0.53, movable), warm=1, reps=5)
        say("smooth: the same %d iterations as float64 index_add_ torch operations %s ms = %.1fx the entry; largest coordinate difference %.3g"
            % (it, f3(t_t), t_t[0] / t_n[0], err))
    del ws
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--fusion", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--host-max", type=int, default=5000000, help="largest mesh (faces) scipy is run on")
    ap.add_argument("--torch-max", type=int, default=20000000, help="largest mesh (vertices) the torch form is run on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L.require_gpu()
    say("mesh cleaning: components, selection, Taubin smoothing; device times: median (min .. max) of 20 after 3 warm-ups, ms; torch form: of 5 after 1")
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
