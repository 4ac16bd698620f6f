"""Device time of the point-cloud renderer (ops.render_points: fill + splat + resolve) on the cloud of tools/probes/pointcloud_probe.py's
inputs (64 views x 518^2 selected with conf_thres=0: 17.2 M points in no spatial order, the incoherent case for the atomics) and on the
same cloud after voxel_downsample to about 1 M points, into 1, 8 and 64 views of 518^2 on an orbit, for splat radii 0, 1, 2: torch events,
2 warm-ups, median (min .. max) of 7. Each row is taken with the plain pre-read of the pixel in front of the atomic on and off
(L.RENDER_NO_PREREAD), alternating. The splat's own time is the call minus the same call on an empty cloud (fill + resolve only).
Without the pre-read every depth test is one 8-byte atomic min, so tests / splat time is the achieved integer-atomic rate; the tests
are counted with torch on the device.
Next to it the numpy twin (tests/render_twin.py) on the same inputs, including the device -> host copy of the cloud it needs.

    python tools/probes/render_probe.py [--views 1 8 64] [--radii 0 1 2] [--no-host]
    python tools/probes/render_probe.py --trace        # a few calls only: the run rocprofv3 --kernel-trace --stats wraps
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from omnivggt_official_amd import lib as L, ops, postprocess  # noqa: E402

H = W = 518
NEAR = 1e-3
FLOAT_ATOMIC_TBS = 1.3     # MI355X, global_atomic_add_f32, 4 bytes per lane, 256-byte wave instructions: a DIFFERENT instruction


def timed_pair(fa, fb, warm=2, reps=7):
    """Two closures timed alternately (a, b, a, b, ...): median, min, max of each in ms."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return tuple((statistics.median(t), min(t), max(t)) for t in ts)


def inputs(S):
    g = torch.Generator(device="cuda").manual_seed(S)
    conf = 1.0 + torch.floor(torch.rand(S, H, W, device="cuda", generator=g) * 40) / 4
    pts = torch.randn(S, H, W, 3, device="cuda", generator=g)
    img = torch.rand(S, 3, H, W, device="cuda", generator=g)
    ext = torch.eye(4, device="cuda")[:3].repeat(S, 1, 1)
    return {"world_points": pts[None], "world_points_conf": conf[None], "images": img[None], "extrinsic": ext[None]}


def cameras(V):
    """V cameras on a circle of radius 4 around the cloud's centre (the origin), f = 400: a unit-variance cloud spreads ~100 pixels."""
    e0 = np.eye(4)[:3].copy()
    e0[2, 3] = 4.0
    ext = postprocess.orbit_cameras(e0, np.zeros(3), V)
    K = torch.tensor([[400.0, 0.0, (W - 1) / 2.0], [0.0, 400.0, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    e = torch.from_numpy(ext).float()
    cams = torch.cat([e[:, :, :3].reshape(V, 9), e[:, :, 3], K[0, 0].expand(V, 1), K[1, 1].expand(V, 1), K[0, 2].expand(V, 1), K[1, 2].expand(V, 1)], 1)
    return cams.contiguous().cuda()


def depth_tests(pts, cams, r):
    """Number of (point, pixel) pairs the splat visits = atomics issued without the pre-read (torch f32 on the device: a point whose
    projection lies within an ulp of a pixel boundary may count one column off, nothing else differs from the kernel)."""
    total = 0
    for c in cams:
        cam = pts @ c[:9].reshape(3, 3).t() + c[9:12]
        z = cam[:, 2]
        u = torch.floor(c[12] * (cam[:, 0] / z) + c[14] + 0.5)
        w = torch.floor(c[13] * (cam[:, 1] / z) + c[15] + 0.5)
        ok = torch.isfinite(cam).all(1) & (z > NEAR) & (u >= -r) & (u <= W - 1 + r) & (w >= -r) & (w <= H - 1 + r)
        u, w = u[ok], w[ok]
        nx = torch.clamp(u + r, max=W - 1) - torch.clamp(u - r, min=0) + 1
        ny = torch.clamp(w + r, max=H - 1) - torch.clamp(w - r, min=0) + 1
        total += int((nx * ny).sum().item())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--radii", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    L.require_gpu()
    full = postprocess.predictions_to_point_cloud(inputs(64), conf_thres=0.0)
    if a.trace:
        for V, r in ((1, 0), (8, 1), (64, 1)):
            cams = cameras(V)
            for flags in (0, L.RENDER_NO_PREREAD):
                torch.cuda.synchronize()
                print("TRACE %d view(s), r = %d, flags = %d: 3 calls follow" % (V, r, flags), flush=True)
                for _ in range(3):
                    ops.render_points(full.points, full.colors, cams, H, W, radius=r, near=NEAR, flags=flags)
        torch.cuda.synchronize()
        return
    import render_twin as twin
    lo, hi = 1e-4, 1.0
    for _ in range(14):                                   # rel_size that keeps about 1 M points: bisection on log(rel_size)
        mid = (lo * hi) ** 0.5
        if len(postprocess.voxel_downsample(full, rel_size=mid)) > 1_000_000:
            lo = mid
        else:
            hi = mid
    rel = (lo * hi) ** 0.5
    small = postprocess.voxel_downsample(full, rel_size=rel)
    print("point-cloud rendering into %d x %d views on an orbit; device times: median (min .. max) of 7 after 2 warm-ups, ms, pre-read on / off alternating" % (H, W))
    print("guide figure beside the atomic columns: float atomic adds (global_atomic_add_f32, a different instruction) run at ~%.1f TB/s of added bytes chip-wide" % FLOAT_ATOMIC_TBS)
    f3 = lambda t: "%.3f (%.3f .. %.3f)" % t
    for name, cloud in (("64 x 518^2 selection", full), ("voxel_downsample(rel_size=%.5f)" % rel, small)):
        M = len(cloud)
        print("\n%s: M = %d points" % (name, M))
        print("%5s %2s | %-26s %-26s | %-9s %-9s | %12s %11s %9s | %s" % ("views", "r", "call, pre-read on", "call, pre-read off", "fill+res", "winner", "depth tests",
                                                                         "G atomics/s", "TB/s", "(last three: pre-read off, splat alone)"))
        empty_pts, empty_col = cloud.points[:0], cloud.colors[:0]
        for V in a.views:
            cams = cameras(V)
            ws = torch.empty(ops.render_workspace_bytes(V, H, W), device="cuda", dtype=torch.uint8)
            for r in a.radii:
                kw = dict(H=H, W=W, radius=r, near=NEAR, ws=ws)
                on, off = timed_pair(lambda: ops.render_points(cloud.points, cloud.colors, cams, **kw),
                                     lambda: ops.render_points(cloud.points, cloud.colors, cams, flags=L.RENDER_NO_PREREAD, **kw))
                base, _ = timed_pair(lambda: ops.render_points(empty_pts, empty_col, cams, **kw), lambda: None)
                tests = depth_tests(cloud.points, cams, r)
                splat_off = max(off[0] - base[0], 1e-6)
                print("%5d %2d | %-26s %-26s | %-9.3f %-9s | %12d %11.2f %9.3f |" % (V, r, f3(on), f3(off), base[0], "on" if on[0] <= off[0] else "off", tests,
                                                                                  tests / splat_off / 1e6, tests * 8 / splat_off / 1e9), flush=True)
        if not a.no_host:
            for V, r in ((1, 0), (1, 1), (1, 2)) if M > 2_000_000 else ((1, 0), (1, 2), (8, 1)):
                cams = cameras(V)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p_h, c_h = cloud.points.cpu().numpy(), cloud.colors.cpu().numpy()
                want = twin.render(p_h, c_h, cams.cpu().numpy(), H, W, r, NEAR)
                ms = (time.perf_counter() - t0) * 1e3
                got = ops.render_points(cloud.points, cloud.colors, cams, H, W, radius=r, near=NEAR, index=True)
                same = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, want))
                print("host numpy twin incl. copy: %d view(s), r = %d: %.0f ms; device output %s" % (V, r, ms, "identical" if same else "DIFFERENT"), flush=True)


if __name__ == "__main__":
    main()
