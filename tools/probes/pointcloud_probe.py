"""Device time of the point-cloud extraction (postprocess.predictions_to_point_cloud) per stage and for the whole call, at 8 and 64
views x 518^2: torch events, 3 warm-ups, median of 20. Reports the bytes each stage moves against the measured 6.3 TB/s copy rate
of the MI355X, and, for context, the host numpy time of the same selection (tests/pointcloud_twin.py, one run).

    python tools/probes/pointcloud_probe.py [--views 8 64] [--no-host]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from omnivggt_official_amd import lib as L, ops, postprocess  # noqa: E402

COPY_RATE = 6.3e12


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
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    L.require_gpu()
    print("point-cloud extraction, 518 x 518 maps, conf_thres 50, black + white background tests; median of 20 after 3 warm-ups (ms)")
    for S in a.views:
        H = W = 518
        n = S * H * W
        g = torch.Generator(device="cuda").manual_seed(S)
        conf = 1.0 + torch.floor(torch.rand(S, H, W, device="cuda", generator=g) * 40) / 4
        pts = torch.randn(S, H, W, 3, device="cuda", generator=g)
        img = torch.rand(S, 3, H, W, device="cuda", generator=g)
        ext = torch.eye(4, device="cuda")[:3].repeat(S, 1, 1)
        pred = {"world_points": pts[None], "world_points_conf": conf[None], "images": img[None], "extrinsic": ext[None]}
        kw = dict(conf_thres=50.0, mask_black_bg=True, mask_white_bg=True)
        whole = timed(lambda: postprocess.predictions_to_point_cloud(pred, **kw))
        cloud = postprocess.predictions_to_point_cloud(pred, **kw)
        M = len(cloud)
        cf = conf.reshape(-1)
        ws_p = torch.empty(ops.percentile_workspace_bytes(n, 4), device="cuda", dtype=torch.uint8)
        ws_f = torch.empty(ops.point_filter_workspace_bytes(n), device="cuda", dtype=torch.uint8)
        count = torch.empty(1, device="cuda", dtype=torch.int64)
        thr = ops.percentile(cf, n, 1, 0, 1, [50.0], ws=ws_p).reshape(1)
        args = dict(conf=cf, images=img, points=pts, hw=H * W, ws=ws_f, threshold=thr, flags=L.PF_BLACK_BG | L.PF_WHITE_BG)
        out_p = torch.empty(M, 3, device="cuda")
        out_c = torch.empty(M, 3, device="cuda", dtype=torch.uint8)
        stages = [
            ("percentile of conf (3 passes)", lambda: ops.percentile(cf, n, 1, 0, 1, [50.0], ws=ws_p), 3 * 4 * n),
            ("mask + count + scan", lambda: ops.point_filter(L.PF_COUNT, out_count=count, **args), 4 * n + 12 * n + n),
            ("scatter", lambda: ops.point_filter(L.PF_SCATTER, capacity=M, out_points=out_p, out_colors=out_c, **args),
             n + M * (12 + 12 + 12 + 3)),
            ("scene-scale percentiles (3 columns)", lambda: ops.percentile(out_p, M, 3, 1, 3, [5.0, 95.0], norm=True, ws=ws_p), 3 * 12 * M),
        ]
        print("\nS = %d views, N = %d pixels, M = %d kept" % (S, n, M))
        print("%-40s %9s %10s %9s" % ("stage", "ms", "MB moved", "@6.3TB/s"))
        total_b = 0
        for name, fn, nbytes in stages:
            t = timed(fn)
            total_b += nbytes
            print("%-40s %9.4f %10.1f %9.4f" % (name, t, nbytes / 1e6, nbytes / COPY_RATE * 1e3))
        print("%-40s %9.4f %10.1f %9.4f" % ("whole call (incl. the one sync + allocs)", whole, total_b / 1e6, total_b / COPY_RATE * 1e3))
        if not a.no_host:
            import pointcloud_twin as twin
            c_h, p_h, i_h = conf.cpu().numpy(), pts.cpu().numpy(), img.cpu().numpy()
            t0 = time.perf_counter()
            twin.select(p_h, c_h, i_h, ext.cpu().numpy(), conf_thres=50.0, mask_black_bg=True, mask_white_bg=True)
            print("%-40s %9.1f" % ("host numpy, same selection (1 run)", (time.perf_counter() - t0) * 1e3))


if __name__ == "__main__":
    main()
