"""Device time of volumetric fusion: ops.tsdf_integrate for every tile (the 256 lattice points of a workgroup as an x x y x z brick),
with and without colours, and the two stages of ops.tsdf_extract, against the same integration as chunked torch operations on the
same GPU:
  torch       per slab of lattice planes and per view: the projection, a gather of the depth, the running mean, all as elementwise
              torch operations (its arithmetic is not the rule's operation for operation: the largest |tsdf| difference to the HIP
              result on a fresh volume is reported, not asserted)
Scene: tests/consistency_twin.device_scene -- a unit sphere inside a backdrop sphere of radius 6, S cameras of 518 x 518 on a circle
of radius 3, 6 % floaters and 3 % unusable pixels; the depth maps are the camera depths of its points. Volume: n^3 lattice points
over [-1.5, 1.5]^3, truncation 4 voxels. S: 8 and 64 views; n: 128, 256 and 512.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 7 after 2 warm-ups (torch: 3 after 1).

    python tools/probes/tsdf_probe.py [--out profiles/tsdf_probe.txt]
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

VIEWS = (8, 64)
LATTICES = (128, 256, 512)
HW = 518
STEP_TIMEOUT = 300           # seconds per GPU step
TORCH_SLAB_POINTS = 1 << 24  # lattice points per slab of the torch form
TILES = ("default", "256x1x1", "8x8x4", "16x4x4", "32x8x1")


def torch_integrate(T, Wt, depth, cams, origin, voxel, trunc, max_weight, near):
    import torch
    nz, ny, nx = T.shape
    S, H, W = depth.shape
    dev = T.device
    ax = [origin[a] + voxel * torch.arange(n, device=dev, dtype=torch.float32) for a, n in enumerate((nx, ny, nz))]
    slab = max(1, TORCH_SLAB_POINTS // (nx * ny))
    flat = depth.reshape(S, H * W)
    for k0 in range(0, nz, slab):
        t, w = T[k0:k0 + slab], Wt[k0:k0 + slab]
        X, Y, Z = ax[0][None, None, :], ax[1][None, :, None], ax[2][k0:k0 + slab, None, None]
        for s in range(S):
            c = cams[s]
            zc = (c[6] * X + c[7] * Y + c[8] * Z) + c[11]
            u = torch.floor(c[12] * (((c[0] * X + c[1] * Y + c[2] * Z) + c[9]) / zc) + c[14] + 0.5)
            v = torch.floor(c[13] * (((c[3] * X + c[4] * Y + c[5] * Z) + c[10]) / zc) + c[15] + 0.5)
            ok = (zc > near) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            idx = v.clamp(0, H - 1).long() * W + u.clamp(0, W - 1).long()
            d = flat[s][idx]
            sdf = d - zc
            ok &= torch.isfinite(d) & (d > near) & (sdf >= -trunc)
            wn = w + 1.0
            t = torch.where(ok, (t * w + (sdf / trunc).clamp(max=1.0)) / wn, t)
            w = torch.where(ok, wn.clamp(max=max_weight), w)
        T[k0:k0 + slab], Wt[k0:k0 + slab] = t, w


def step(S, n):
    """The GPU step (child process): prints one RESULT line."""
    import torch
    import consistency_twin as ctwin
    from omnivggt_official_amd import lib as L, ops
    L.require_gpu()
    pts, ext, intr = ctwin.device_scene(S, HW, HW)
    cams = torch.from_numpy(ctwin.pack_cams(ext, intr)).cuda()
    R, t = torch.from_numpy(ext[:, :, :3]).cuda(), torch.from_numpy(ext[:, :, 3]).cuda()
    depth = (torch.einsum("sj,shwj->shw", R[:, 2], pts.double()) + t[:, 2, None, None]).float().contiguous()   # NaN rows stay NaN
    colors = torch.randint(0, 256, (S, HW, HW, 3), device="cuda", dtype=torch.uint8)
    voxel = float(np.float32(3.0 / (n - 1)))
    origin, trunc = (-1.5, -1.5, -1.5), float(np.float32(4.0 * voxel))

    def fresh(color):
        return (torch.ones(n, n, n, device="cuda"), torch.zeros(n, n, n, device="cuda"), torch.zeros(n, n, n, 4, device="cuda") if color else None)

    T, Wt, _ = fresh(False)
    times = [timed(lambda: ops.tsdf_integrate(T, Wt, depth, cams, origin, voxel, trunc, tile=tile), reps=7) for tile in range(len(TILES))]
    Tc, Wc, Cc = fresh(True)
    with_colors = timed(lambda: ops.tsdf_integrate(Tc, Wc, depth, cams, origin, voxel, trunc, color=Cc, colors=colors), reps=7)
    del Tc, Wc, Cc
    # the mesh of one integration of a fresh volume
    T, Wt, _ = fresh(False)
    ops.tsdf_integrate(T, Wt, depth, cams, origin, voxel, trunc)
    ws = torch.empty(ops.tsdf_extract_workspace_bytes(n, n, n), device="cuda", dtype=torch.uint8)
    cnt = torch.empty(2, device="cuda", dtype=torch.int64)
    args = dict(tsdf=T, weight=Wt, origin=origin, voxel=voxel, ws=ws, out_count=cnt)
    count = timed(lambda: ops.tsdf_extract(L.TSDF_COUNT, **args), reps=7)
    M, Q = (int(v) for v in cnt.cpu())
    out = dict(vertices=torch.empty(M, 3, device="cuda"), normals=torch.empty(M, 3, device="cuda"),
               colors=torch.empty(M, 3, device="cuda", dtype=torch.uint8), faces=torch.empty(2 * Q, 3, device="cuda", dtype=torch.int32))
    scatter = timed(lambda: ops.tsdf_extract(L.TSDF_SCATTER, vertex_capacity=M, quad_capacity=Q, **out, **args), reps=7)
    observed = float((Wt > 0).float().mean())
    # the torch form on a fresh volume: its difference to the HIP result, then its time
    T2, W2, _ = fresh(False)
    host_cams = [[float(v) for v in row] for row in cams.cpu().numpy()]
    targs = (depth, host_cams, origin, voxel, trunc, 64.0, 1e-3)
    torch_integrate(T2, W2, *targs)
    differ = float((T2 - T).abs().max())
    wdiffer = float((W2 != Wt).float().mean())
    tch = timed(lambda: torch_integrate(T2, W2, *targs), warm=1, reps=3)
    print("RESULT %d %d %d %d %.4f %s %.3e %.3e" % (S, n, M, Q, observed, " ".join("%.4f %.4f %.4f" % v for v in times + [with_colors, count, scatter, tch]),
                                                     differ, wdiffer), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("volumetric fusion (ovg_tsdf_integrate per tile, without and with colours; ovg_tsdf_extract COUNT and SCATTER); ms by events,")
    say("median (min .. max) of 7 after 2 warm-ups; S views of %d x %d into n^3 lattice points over [-1.5, 1.5]^3, truncation 4 voxels." % (HW, HW))
    say("Gproj/s: lattice points x views over the time of the default tile. torch: the same integration as elementwise torch operations in")
    say("slabs of %d M lattice points on the same GPU, median (min .. max) of 3 after 1 warm-up; |dT|: the largest tsdf difference and" % (TORCH_SLAB_POINTS >> 20))
    say("dW: the share of lattice points whose weight differs between the torch form and the HIP result on a fresh volume.")
    failed = None
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)
    for S in VIEWS:
        for n in LATTICES:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(S), str(n)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
            for r in res:
                t = [[float(v) for v in r[6 + 3 * k:9 + 3 * k]] for k in range(len(TILES) + 4)]
                say("S %2d  n %3d  observed %.2f  vertices %d  quads %d" % (int(r[1]), int(r[2]), float(r[5]), int(r[3]), int(r[4])))
                for name, v in zip(TILES, t):
                    say("    integrate, tile %-8s %-28s" % (name, fmt(v)) + ("  %.1f Gproj/s" % (S * n ** 3 / v[0] / 1e6) if name == "default" else ""))
                k = len(TILES)
                say("    integrate with colours  %-28s" % fmt(t[k]))
                say("    extract COUNT           %-28s" % fmt(t[k + 1]))
                say("    extract SCATTER         %-28s" % fmt(t[k + 2]))
                say("    torch integrate         %-28s  torch/hip %.1f  |dT| %s  dW %s" % (fmt(t[k + 3]), t[k + 3][0] / t[0][0], r[-2], r[-1]))
            if p.returncode != 0 or len(res) != 1:
                failed = "(%d, %d): the GPU step ended with status %d; nothing is started after it\n%s" % (S, n, p.returncode, (p.stdout + p.stderr)[-2000:])
                say(failed)
                break
        if failed:
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
