"""Device time of the exact nearest-neighbour search (ops.nearest_neighbours) against scipy's k-d tree on the host, on the same inputs:
9.5 k x 9.5 k (two views at every 4th pixel), 268 k x 268 k (two full 518^2 views) and 1 M x 1 M (decimated clouds at evaluation
size). The clouds are seeded surface samples: points on a unit sphere and a ground plane with 1 % noise, the reference cloud a
second sampling of the same surfaces.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. The device figure is torch events around the call (median (min .. max) of 5 after 2 warm-ups, auto splits), set against
  * cKDTree build + query(workers=8) on the host, the reference's find_reciprocal_matches recipe (wall clock, one run), and
  * the vector-ALU bound: 11 operations per pair (3 subtractions, 3 products, 2 sums, compare, two selects; no FMA by the rule) at
    256 CUs x 64 lanes x 2.4 GHz = 3.9e13 lane-operations/s.

    python tools/nn_probe.py [--sizes 9500 268324 1000000] [--no-host] [--out profiles/nn_probe.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OPS_PER_PAIR = 11
VALU_RATE = 256 * 64 * 2.4e9
STEP_TIMEOUT = 240           # seconds per GPU step: the largest takes a few seconds of device time plus start-up


def clouds(n, seed=0):
    rng = np.random.default_rng(seed + n)

    def one():
        v = rng.normal(size=(n, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True)
        ground = rng.random(n) < 0.4
        p[ground] = np.stack([rng.uniform(-3, 3, int(ground.sum())), np.full(int(ground.sum()), -1.0), rng.uniform(-3, 3, int(ground.sum()))], 1)
        return (p + rng.normal(0.0, 0.01, (n, 3))).astype(np.float32)
    return one(), one()


def step(n):
    """The GPU step (child process): prints one RESULT line."""
    import torch
    from omnivggt_official_amd import lib as L, ops
    L.require_gpu()
    q, r = (torch.from_numpy(a).cuda() for a in clouds(n))
    ws = torch.empty(ops.nn_workspace_bytes(n, n), device="cuda", dtype=torch.uint8)
    idx, sq = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.float32)
    run = lambda: ops.nearest_neighbours(q, r, ws=ws, index=idx, sqdist=sq)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    print("RESULT %d %.4f %.4f %.4f %d %.9g" % (n, statistics.median(ts), min(ts), max(ts), int(idx.to(torch.int64).sum()),
                                               float(sq.double().sum())), flush=True)


def host(n):
    from scipy.spatial import cKDTree
    q, r = clouds(n)
    t0 = time.perf_counter()
    d, j = cKDTree(r).query(q, workers=8)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, int(j.sum()), float((d * d).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[9500, 518 * 518, 1000000])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("exact nearest neighbours, n x n points; device: ms median (min .. max) of 5 after 2 warm-ups; host: cKDTree build + query, 8 workers, one run")
    say("bound: %d vector operations per pair at %.2e lane-operations/s" % (OPS_PER_PAIR, VALU_RATE))
    say("%9s | %-28s %11s %8s | %10s %8s | %s" % ("n", "device ms", "G pairs/s", "of bound", "host ms", "host/dev", "index sums (device, tree)"))
    failed = None
    for n in a.sizes:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(n)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        if p.returncode != 0 or len(res) != 1:
            failed = "n = %d: the GPU step ended with status %d; nothing is started after it\n%s" % (n, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
        med, lo, hi, isum, dsum = float(res[0][2]), float(res[0][3]), float(res[0][4]), int(res[0][5]), float(res[0][6])
        rate = n * n / (med * 1e-3)
        hs = ("%10s %8s | %d" % ("-", "-", isum))
        if not a.no_host:
            hms, hsum, hd = host(n)
            hs = "%10.0f %8.1f | %d, %d; sum of d^2 %.9g, %.9g" % (hms, hms / med, isum, hsum, dsum, hd)
        say("%9d | %-28s %11.1f %7.1f%% | %s" % (n, "%.3f (%.3f .. %.3f)" % (med, lo, hi), rate / 1e9, 100 * rate * OPS_PER_PAIR / VALU_RATE, hs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
