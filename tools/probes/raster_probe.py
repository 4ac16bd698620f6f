"""Device time of mesh rasterisation: ops.render_mesh (fill + draw + resolve) of the fused mesh of tsdf_probe.py's scene into 1 / 8 / 64
views of 518 x 518 for a sweep of coop_threshold (the box size up to which a face is walked by its own lane; larger boxes are walked
by the whole wave), against the best the point renderer can do with the same mesh: ops.render_points of its vertices at radius 1.
Worst case of the cooperative path: two triangles that fill every frame (one quad in front of a camera repeated V times), drawn by
one wave.

Scene: tests/consistency_twin.device_scene -- a unit sphere inside a backdrop sphere of radius 6, 8 cameras of 518 x 518 on a circle of
radius 3; their depth maps fused into n^3 lattice points over [-1.5, 1.5]^3 (truncation 4 voxels), n = 32, 64, 256 and 512; the mesh is
rendered from V cameras on the same circle (postprocess.orbit_cameras) with vertex normals, vertex colours and headlight shading.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 7 after 2 warm-ups.

    python tools/probes/raster_probe.py [--out profiles/raster_probe.txt]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from radius_probe import timed  # noqa: E402

LATTICES = (32, 64, 256, 512)       # 32 and 64: faces of tens to hundreds of pixels, where coop_threshold decides the path
VIEWS = (1, 8, 64)
COOP = (16, 64, 256, 1024, 0)       # 0: the library's default, measured last (the first figure of a step is the coldest)
FUSED_VIEWS = 8
HW = 518
STEP_TIMEOUT = 300                  # seconds per GPU step


def step(n):
    """The GPU step (child process): prints one RESULT line per number of views; n = 0 is the two-triangle worst case."""
    import torch
    import consistency_twin as ctwin
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    pts, ext, intr = ctwin.device_scene(FUSED_VIEWS, HW, HW)
    if n:
        R, t = torch.from_numpy(ext[:, :, :3]).cuda(), torch.from_numpy(ext[:, :, 3]).cuda()
        depth = (torch.einsum("sj,shwj->shw", R[:, 2], pts.double()) + t[:, 2, None, None]).float().contiguous()
        voxel = float(np.float32(3.0 / (n - 1)))
        vol = postprocess.tsdf_volume((-1.5, -1.5, -1.5), voxel, (n, n, n), trunc=float(np.float32(4.0 * voxel)), color=False)
        postprocess.tsdf_integrate(vol, depth, ext, intr)
        mesh = postprocess.tsdf_extract(vol)
        del vol, depth
        vert, faces, nrm = mesh.vertices, mesh.faces, mesh.normals
    else:
        # a tilted quad in front of camera 0 that overhangs its frame on every side, seen V times by that camera
        R, t = ext[0, :, :3], ext[0, :, 3]
        corners = np.array([[-2.0, -2.0, 2.0], [2.0, -2.0, 2.5], [2.0, 2.0, 3.0], [-2.0, 2.0, 2.5]])
        vert = torch.from_numpy(((corners - t) @ R).astype(np.float32)).cuda()
        faces = torch.tensor([[0, 2, 1], [0, 3, 2]], device="cuda", dtype=torch.int32)
        nrm = torch.from_numpy(np.tile(-R[2], (4, 1)).astype(np.float32)).cuda()
    del pts
    col = torch.randint(0, 256, (len(vert), 3), device="cuda", dtype=torch.uint8)
    for V in VIEWS:
        ring = postprocess.orbit_cameras(ext[0], (0.0, 0.0, 0.0), V) if n else np.tile(ext[0], (V, 1, 1))
        cams = postprocess._pack_cams(torch.from_numpy(ring), torch.from_numpy(intr), V, torch.device("cuda"))
        ws = torch.empty(ops.render_mesh_workspace_bytes(V, HW, HW), device="cuda", dtype=torch.uint8)
        out = (torch.empty(V, HW, HW, 3, device="cuda", dtype=torch.uint8), torch.empty(V, HW, HW, device="cuda"), None)
        times = [timed(lambda: ops.render_mesh(vert, faces, cams, HW, HW, normals=nrm, colors=col, coop_threshold=c, ws=ws, out=out), reps=7)
                 for c in (COOP if n else COOP[-1:])]
        hit = float((out[1] > 0).float().mean())
        points = timed(lambda: ops.render_points(vert, col, cams, HW, HW, radius=1, ws=ws), reps=7)
        rgb, dep, _ = ops.render_points(vert, col, cams, HW, HW, radius=1, ws=ws)
        phit = float((dep > 0).float().mean())
        print("RESULT %d %d %d %d %.4f %.4f %s" % (n, V, len(vert), len(faces), hit, phit, " ".join("%.4f %.4f %.4f" % v for v in times + [points])),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_probe.txt"))
    a = ap.parse_args()
    if a.step is not None:
        return step(a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("mesh rasterisation (ovg_render_mesh: fill + draw + resolve, headlight shading, vertex normals and colours); ms by events, median")
    say("(min .. max) of 7 after 2 warm-ups; V views of %d x %d. coop: the box size in pixels up to which a face is walked by its own lane" % (HW, HW))
    say("(larger boxes: by the 64 lanes of its wave). hit: the share of pixels a face covers. points: ovg_render_points of the mesh's")
    say("vertices at radius 1 on the same machine (no faces, no shading) and the share of pixels it reaches.")
    failed = None
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)
    for n in LATTICES + (0,):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(n)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            V, coops = int(r[2]), (COOP if n else COOP[-1:])
            t = [[float(v) for v in r[7 + 3 * k:10 + 3 * k]] for k in range(len(coops) + 1)]
            say(("lattice %d^3" % n if n else "two triangles over the frame") + "  V %2d  vertices %d  faces %d  hit %.3f" % (V, int(r[3]), int(r[4]), float(r[5])))
            for c, v in zip(coops, t):
                rate = "%.1f Mface-views/s" % (V * int(r[4]) / v[0] / 1e3) if n else "%.1f Mpixels/s per face" % (V * HW * HW / 2 / v[0] / 1e3)
                say("    render_mesh, coop %-8s %-28s  %s" % (c if c else "default", fmt(v), rate))
            say("    render_points, radius 1  %-28s  reaches %.3f of the pixels" % (fmt(t[-1]), float(r[6])))
        if p.returncode != 0 or len(res) != len(VIEWS):
            failed = "step %d: the GPU step ended with status %d; nothing is started after it\n%s" % (n, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
