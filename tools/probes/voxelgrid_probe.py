"""Device time of the voxel-grid decimation (postprocess.voxel_downsample) on the clouds of tools/probes/pointcloud_probe.py's inputs
(8 and 64 views x 518^2, selected with conf_thres=0), for voxel edges that keep about 1/4, 1/16 and 1/64 of the points: torch events,
3 warm-ups, median (min .. max) of 20. Next to it the same rule run with numpy on the host (tests/voxelgrid_twin.py, including the
device -> host copy of the cloud it needs) and the wall-clock of the export predictions_to_point_cloud + write_glb with and without
the decimation in between, with the file sizes.

    python tools/probes/voxelgrid_probe.py [--views 8 64] [--no-host] [--no-export]
    python tools/probes/voxelgrid_probe.py --trace        # a few 64-view calls only: the run rocprofv3 --kernel-trace --stats wraps
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from omnivggt_official_amd import lib as L, ops, postprocess  # noqa: E402


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


def inputs(S, H=518, W=518):
    g = torch.Generator(device="cuda").manual_seed(S)
    conf = 1.0 + torch.floor(torch.rand(S, H, W, device="cuda", generator=g) * 40) / 4
    pts = torch.randn(S, H, W, 3, device="cuda", generator=g)
    img = torch.rand(S, 3, H, W, device="cuda", generator=g)
    ext = torch.eye(4, device="cuda")[:3].repeat(S, 1, 1)
    return {"world_points": pts[None], "world_points_conf": conf[None], "images": img[None], "extrinsic": ext[None]}


def rel_for(cloud, fraction):
    """rel_size that keeps about `fraction` of the cloud: bisection on log(rel_size)."""
    lo, hi = 1e-4, 1.0
    for _ in range(18):
        mid = (lo * hi) ** 0.5
        if len(postprocess.voxel_downsample(cloud, rel_size=mid, conf=cloud.conf)) > fraction * len(cloud):
            lo = mid
        else:
            hi = mid
    return (lo * hi) ** 0.5


def stages(cloud, rel):
    """(count stage, scatter stage) closures on preallocated buffers, as voxel_downsample issues them."""
    M = len(cloud)
    voxel = torch.full((), rel, device="cuda") * cloud.scene_scale
    ws = torch.empty(ops.voxel_downsample_workspace_bytes(M), device="cuda", dtype=torch.uint8)
    count = torch.empty(2, device="cuda", dtype=torch.int64)
    args = dict(points=cloud.points, voxel=voxel, ws=ws, conf=cloud.conf, colors=cloud.colors)
    ops.voxel_downsample(L.VG_COUNT, out_count=count, **args)
    kept = int(count[0])
    op, oc, oi = (torch.empty(kept, 3, device="cuda"), torch.empty(kept, 3, device="cuda", dtype=torch.uint8),
                  torch.empty(kept, device="cuda", dtype=torch.int64))
    return (lambda: ops.voxel_downsample(L.VG_COUNT, out_count=count, **args),
            lambda: ops.voxel_downsample(L.VG_SCATTER, capacity=kept, out_points=op, out_colors=oc, out_index=oi, **args), ws.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-export", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    L.require_gpu()
    if a.trace:
        cloud = postprocess.predictions_to_point_cloud(inputs(64), conf_thres=0.0, return_conf=True)
        for frac in (1 / 4, 1 / 16, 1 / 64):
            rel = rel_for(cloud, frac)
            torch.cuda.synchronize()
            print("TRACE fraction 1/%d rel_size %.5f: 5 calls follow" % (round(1 / frac), rel), flush=True)
            for _ in range(5):
                postprocess.voxel_downsample(cloud, rel_size=rel, conf=cloud.conf)
        torch.cuda.synchronize()
        return
    import voxelgrid_twin as twin
    print("voxel-grid decimation of the conf_thres=0 cloud, 518 x 518 maps; device times: median (min .. max) of 20 after 3 warm-ups, ms")
    for S in a.views:
        pred = inputs(S)
        kw = dict(conf_thres=0.0, return_conf=True)
        cloud = postprocess.predictions_to_point_cloud(pred, **kw)
        M = len(cloud)
        sel = timed(lambda: postprocess.predictions_to_point_cloud(pred, conf_thres=0.0))
        print("\nS = %d views, M = %d points, scene_scale %.4f; selection (whole call, conf_thres=0) %.4f (%.4f .. %.4f)"
              % (S, M, float(cloud.scene_scale), *sel))
        print("%-9s %9s %9s %10s | %-27s %-27s %-27s | %s" % ("keep", "rel_size", "voxel", "M'", "count stage (hash + flags)", "scatter stage",
                                                               "whole call (sync + allocs)", "host numpy incl. copy"))
        rels = {}
        for frac in (1 / 4, 1 / 16, 1 / 64):
            rel = rels[frac] = rel_for(cloud, frac)
            out = postprocess.voxel_downsample(cloud, rel_size=rel, conf=cloud.conf)
            cnt, sct, ws_bytes = stages(cloud, rel)
            t_c, t_s = timed(cnt), timed(sct)
            t_w = timed(lambda: postprocess.voxel_downsample(cloud, rel_size=rel, conf=cloud.conf))
            host = ""
            if not a.no_host:
                hs = []
                for _ in range(3 if S <= 8 else 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    p_h, c_h, col_h = cloud.points.cpu().numpy(), cloud.conf.cpu().numpy(), cloud.colors.cpu().numpy()
                    keep = twin.downsample(p_h, twin.voxel_from_rel(rel, cloud.scene_scale.cpu().numpy()), c_h)
                    p_o, col_o = p_h[keep], col_h[keep]
                    hs.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(keep, out.indices.cpu().numpy())
                host = "%.0f ms (%d run%s) = %.0fx the device call" % (statistics.median(hs), len(hs), "s" if len(hs) > 1 else "",
                                                                       statistics.median(hs) / t_w[0])
            f3 = lambda t: "%.4f (%.4f .. %.4f)" % t
            print("1/%-7d %9.5f %9.5f %10d | %-27s %-27s %-27s | %s" % (round(1 / frac), rel, rel * float(cloud.scene_scale), len(out), f3(t_c),
                                                                       f3(t_s), f3(t_w), host), flush=True)
        print("workspace %.1f MB (table %.1f MB = 2 M slots of 16 bytes)" % (ws_bytes / 1e6, 32 * M / 1e6))
        if not a.no_export:
            with tempfile.TemporaryDirectory() as d:
                rows = []
                for name, rel in (("no decimation", None), ("keep 1/16", rels[1 / 16]), ("keep 1/64", rels[1 / 64])):
                    path = os.path.join(d, "scene.glb")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    c = postprocess.predictions_to_point_cloud(pred, conf_thres=0.0, return_conf=rel is not None)
                    if rel is not None:
                        c = postprocess.voxel_downsample(c, rel_size=rel, conf=c.conf)
                    postprocess.write_glb(path, c, cameras=True)
                    rows.append((name, (time.perf_counter() - t0) * 1e3, os.path.getsize(path), len(c)))
                for name, ms, size, m in rows:
                    print("export predictions_to_point_cloud%s + write_glb(cameras=True): %-14s %9.1f ms wall, %11d bytes, %9d vertices (%.1fx faster, %.1fx smaller)"
                          % (" + voxel_downsample" if name != "no decimation" else "", name, ms, size, m, rows[0][1] / ms, rows[0][2] / size), flush=True)


if __name__ == "__main__":
    main()
