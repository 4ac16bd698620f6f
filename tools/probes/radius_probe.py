"""Device time of the radius neighbour search (ops.radius_search: BUILD and SEARCH timed apart) against the exhaustive search
(ops.nearest_neighbours) on the same inputs, and the pair rate the default work budget (postprocess.RADIUS_MAX_PAIRS) rests on.
  1 x 1 views    268 324 x 268 324, radii giving about 8 and about 64 neighbours per query
  4 x 4 views    1 073 296 x 1 073 296, likewise
  64 views       17 172 736 points inside one cloud (exclude-self), likewise; no exhaustive search at this size
The clouds are synthetic prediction maps in PIXEL ORDER, as a model's are: every view is a 518 x 518 pinhole camera inside a sphere
of radius 3, looking within 15 degrees of a common direction, each pixel's ray cut with the sphere, 0.1 % noise. The radius of a
case is found on the device by bisection on the mean count of 16 384 sampled queries.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups. A step also checks the search
against the exhaustive one where both ran: index and sqdist must be equal wherever the exhaustive sqdist is within the radius.

    python tools/probes/radius_probe.py [--out profiles/radius_probe.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HW = 518
CASES = ((1, 1, 1), (4, 4, 1), (64, 0, 0))      # (query views, reference views, run the exhaustive search); 0 reference views: inside one cloud
TARGETS = (8, 64)
STEP_TIMEOUT = 360           # seconds per GPU step


def views(first, n, seed=0):
    """n views from view number `first` on -> float32 [n * 518 * 518, 3] in pixel order."""
    out = np.empty((n, HW * HW, 3), np.float32)
    v, u = np.meshgrid(np.arange(HW), np.arange(HW), indexing="ij")
    f = (HW / 2) / np.tan(np.radians(30.0))
    rays = np.stack([(u - HW / 2 + 0.5) / f, (v - HW / 2 + 0.5) / f, np.ones_like(u, float)], -1).reshape(-1, 3)
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    for k in range(n):
        rng = np.random.default_rng(seed * 1000 + first + k)
        c = rng.normal(size=3)
        c *= rng.random() ** (1 / 3) / np.linalg.norm(c)                         # uniform in the unit ball
        w = rng.normal(size=3)
        w *= np.radians(15.0) * rng.random() / np.linalg.norm(w)                 # a rotation vector of at most 15 degrees
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        d = rays @ R.T
        b = d @ c
        t = -b + np.sqrt(b * b - (c @ c - 9.0))
        out[k] = (c + t[:, None] * d) * (1.0 + rng.normal(0.0, 1e-3, (len(d), 1)))
    return out.reshape(-1, 3)


def timed(run, warm=2, reps=5):
    import torch
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def step(nqv, nrv, exhaustive):
    """The GPU step (child process): prints one RESULT line per target."""
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    same = nrv == 0
    q = torch.from_numpy(views(0, nqv)).cuda()
    r = q if same else torch.from_numpy(views(nqv, nrv)).cuda()
    nq, nr = q.shape[0], r.shape[0]
    ws = torch.empty(ops.radius_workspace_bytes(nq, nr), device="cuda", dtype=torch.uint8)
    pick = torch.from_numpy(np.random.default_rng(1).choice(nq, 16384, replace=False)).cuda()

    def mean_count(radius):
        """Mean neighbours of the sampled queries; None when the guard refuses."""
        r2 = postprocess._radius_sq(radius)
        args = dict(query=q[pick].contiguous(), reference=r, radius_sq=r2, cell=ops.radius_reach(r2), ws=ws)
        stats = ops.radius_search(L.RS_BUILD, **args)[0].tolist()
        if stats[3] > 4000 * pick.numel():
            return None
        cnt = ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, **args)[1]
        return float(cnt.double().mean()) - (1.0 if same else 0.0)               # inside one cloud a sampled point finds itself

    nn = None
    if exhaustive:
        nn_time = timed(lambda: ops.nearest_neighbours(q, r, exclude_self=same))
        nn = ops.nearest_neighbours(q, r, exclude_self=same)
    for target in TARGETS:
        lo, hi = 1e-4, 1.0
        for _ in range(14):
            mid = (lo * hi) ** 0.5
            m = mean_count(mid)
            lo, hi = (lo, mid) if m is None or m > target else (mid, hi)
        radius = lo
        r2 = postprocess._radius_sq(radius)
        args = dict(query=q, reference=r, radius_sq=r2, cell=ops.radius_reach(r2), ws=ws, exclude_self=same)
        stats = torch.empty(4, device="cuda", dtype=torch.int64)
        cnt, idx, sq = (torch.empty(nq, device="cuda", dtype=dt) for dt in (torch.int32, torch.int32, torch.float32))
        build = timed(lambda: ops.radius_search(L.RS_BUILD, out_stats=stats, **args))
        flags, cells, largest, pairs = stats.tolist()
        search = timed(lambda: ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, count=cnt, index=idx, sqdist=sq, **args))
        wrong = -1
        if nn is not None:
            inside = (nn[0] >= 0) & (nn[1] <= r2)
            wrong = int((idx[inside] != nn[0][inside]).sum() + (sq[inside].view(torch.int32) != nn[1][inside].view(torch.int32)).sum()
                        + (idx[~inside] != -1).sum())
        print("RESULT %d %d %d %.6g %.3f %.4f %.4f %.4f %.4f %.4f %.4f %d %d %d %d %s" % (
            nq, nr, target, radius, float(cnt.double().mean()), *build, *search, cells, largest, pairs, wrong,
            "%.4f %.4f %.4f" % nn_time if exhaustive else "- - -"), flush=True)
        if wrong > 0:
            sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("radius neighbour search on the hash grid; ms by events, median (min .. max) of 5 after 2 warm-ups; clouds: synthetic views in pixel order.")
    say("pairs: candidate pairs = distances the search evaluates (out_stats[3]); rate = pairs / search time; exhaustive: ops.nearest_neighbours.")
    say("%21s %9s %7s | %-27s %-30s | %8s %8s %14s %9s | %-26s %8s" % ("nq x nr", "radius", "mean k", "build ms", "search ms", "cells", "largest",
                                                                 "pairs", "Gpairs/s", "exhaustive ms", "speed-up"))
    failed, rates = None, []
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step"] + [str(v) for v in case]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            build, search = [float(v) for v in r[6:9]], [float(v) for v in r[9:12]]
            pairs, wrong = int(r[14]), int(r[15])
            rate = pairs / (search[0] * 1e-3) / 1e9
            rates.append(rate)
            ex, speed = "-", "-"
            if r[16] != "-":
                ex = "%.3f (%.3f .. %.3f)" % tuple(float(v) for v in r[16:19])
                speed = "%.1f" % (float(r[16]) / (build[0] + search[0]))
            say("%21s %9.4g %7.2f | %-27s %-30s | %8d %8d %14d %9.2f | %-26s %8s%s" % (
                "%s x %s" % (r[1], r[2]), float(r[4]), float(r[5]), "%.3f (%.3f .. %.3f)" % tuple(build), "%.3f (%.3f .. %.3f)" % tuple(search),
                int(r[12]), int(r[13]), pairs, rate, ex, speed, "" if wrong <= 0 else "   %d MISMATCHES against the exhaustive search" % wrong))
        if p.returncode != 0 or len(res) != len(TARGETS):
            failed = "%r: the GPU step ended with status %d; nothing is started after it\n%s" % (case, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    if rates:
        from omnivggt_official_amd import postprocess
        say("lowest pair rate %.2f Gpairs/s: the default budget of 2^%d pairs is %.1f s of search at that rate" % (
            min(rates), postprocess.RADIUS_MAX_PAIRS.bit_length() - 1, postprocess.RADIUS_MAX_PAIRS / (min(rates) * 1e9)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
