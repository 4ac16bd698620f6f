"""Device time of the multi-view consistency filter (ops.multiview_consistency: z-maps + pair kernel) for 8 / 16 / 64 views of 518^2 of
a consistent synthetic scene made on the device (a unit sphere inside a backdrop sphere seen from a circle of cameras, 6 % floaters,
3 % NaN rows: the scene of tests/test_gpu_consistency.py's full-size test), for every tile shape of the pair kernel and both target
orders, with and without the `occluded` output: torch events, 2 warm-ups, median (min .. max) of 7 launches. "pairs" is the pair
kernel alone (L.MVC_KEEP_MAP), "call" both launches. A projection is one (usable source pixel, other view) pair: the projection of
the render kernel plus one gathered 4-byte read.
Set against two things that are not the code under test: the numpy twin (tests/consistency_twin.py) on the same inputs on this host
(8 views in full; 64 views from one source view x 64, labelled extrapolated), and the render kernel's rate at radius 0 from
profiles/render_probe.txt (the same projection with an atomic where this has a read).

    python tools/probes/consistency_probe.py [--views 8 16 64] [--no-host] [--out profiles/consistency_probe.txt]
    python tools/probes/consistency_probe.py --trace       # a few calls only: the run rocprofv3 --kernel-trace --stats wraps
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
from omnivggt_official_amd import lib as L, ops  # noqa: E402

H = W = 518
TOL, NEAR = 0.02, 1e-3
RENDER_RATE = 6e10         # profiles/render_probe.txt: 17.2 M points into one view at radius 0 in 0.28 ms
TILES = (("256x1", L.MVC_TILE_256x1), ("32x8", L.MVC_TILE_32x8), ("16x16", L.MVC_TILE_16x16), ("8x32", L.MVC_TILE_8x32))


def timed(fn, warm=2, reps=7):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 16, 64])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_probe.txt"))
    a = ap.parse_args()
    L.require_gpu()
    import consistency_twin as twin
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.trace:
        pts, ext, intr = twin.device_scene(64, H, W)
        cams = torch.from_numpy(twin.pack_cams(ext, intr)).cuda()
        for name, tile in TILES:
            torch.cuda.synchronize()
            print("TRACE 64 views, tile %s: 3 calls follow" % name, flush=True)
            for _ in range(3):
                ops.multiview_consistency(pts, cams, TOL, near=NEAR, occluded=True, tile=tile)
        torch.cuda.synchronize()
        return
    say("multi-view consistency of S views of %d x %d, rel_tol %.2f; device times: median (min .. max) of 7 after 2 warm-ups, ms" % (H, W, TOL))
    say("reference rate: the render kernel at radius 0 does ~%.0e projections/s (profiles/render_probe.txt)" % RENDER_RATE)
    f3 = lambda t: "%.3f (%.3f .. %.3f)" % t
    for S in a.views:
        pts, ext, intr = twin.device_scene(S, H, W)
        cams = torch.from_numpy(twin.pack_cams(ext, intr)).cuda()
        ws = torch.empty(ops.consistency_workspace_bytes(S, H, W), device="cuda", dtype=torch.uint8)
        sup, vio, occ = ops.multiview_consistency(pts, cams, TOL, near=NEAR, occluded=True, ws=ws)
        usable = int((~torch.isnan(ws.view(torch.float32))).sum())
        proj = usable * (S - 1)
        counted = int(sup.sum(dtype=torch.int64) + vio.sum(dtype=torch.int64) + occ.sum(dtype=torch.int64))
        say("\nS = %d: %d usable source pixels, %d projections, %d of them counted (support %.3f, violations %.3f, occluded %.3f of the counted); z-maps %.1f MB"
            % (S, usable, proj, counted, float(sup.sum(dtype=torch.int64)) / counted, float(vio.sum(dtype=torch.int64)) / counted,
               float(occ.sum(dtype=torch.int64)) / counted, ws.numel() / 1e6))
        say("%-6s %-8s | %-26s %-26s %9s | %-26s %9s" % ("tile", "targets", "call, with occluded", "pairs, with occluded", "G proj/s", "pairs, no occluded", "G proj/s"))
        best = None
        for name, tile in TILES:
            for oname, flags in (("same", 0), ("rotated", L.MVC_ROTATE_TARGETS)):
                kw = dict(near=NEAR, ws=ws, tile=tile)
                call = timed(lambda: ops.multiview_consistency(pts, cams, TOL, occluded=True, flags=flags, **kw))
                pairs = timed(lambda: ops.multiview_consistency(pts, cams, TOL, occluded=True, flags=flags | L.MVC_KEEP_MAP, **kw))
                pairs0 = timed(lambda: ops.multiview_consistency(pts, cams, TOL, occluded=False, flags=flags | L.MVC_KEEP_MAP, **kw))
                say("%-6s %-8s | %-26s %-26s %9.2f | %-26s %9.2f" % (name, oname, f3(call), f3(pairs), proj / pairs[0] / 1e6, f3(pairs0), proj / pairs0[0] / 1e6))
                if best is None or pairs[0] < best[0]:
                    best = (pairs[0], name, oname)
        say("best: tile %s, targets %s: %.3f ms = %.2e projections/s = %.2f x the render rate" % (best[1], best[2], best[0], proj / best[0] * 1e3, proj / best[0] * 1e3 / RENDER_RATE))
        if not a.no_host and S in (8, 64):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hp, hc = pts.cpu().numpy(), cams.cpu().numpy()
            if S == 8:
                want = twin.consistency(hp, hc, TOL, near=NEAR)
                ms = (time.perf_counter() - t0) * 1e3
                same = all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((sup, vio, occ), want))
                say("host numpy twin incl. copy, all 8 source views: %.0f ms; device output %s" % (ms, "identical" if same else "DIFFERENT"))
            else:
                zm = twin.zmap(hp, hc, NEAR)
                t1 = time.perf_counter()
                want = twin.count_pixels(hp[37].reshape(-1, 3), ~np.isnan(zm[37].reshape(-1)), 37, zm, hc, TOL, NEAR)
                one = (time.perf_counter() - t1) * 1e3
                same = all(g[37].reshape(-1).cpu().numpy().tobytes() == w.tobytes() for g, w in zip((sup, vio, occ), want))
                say("host numpy twin: copy + z-maps %.0f ms, source view 37 alone %.0f ms -> x 64 = %.0f ms (extrapolated); device row 37 %s"
                    % ((t1 - t0) * 1e3, one, (t1 - t0) * 1e3 + 64 * one, "identical" if same else "DIFFERENT"))
        del pts, ws, sup, vio, occ
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
