"""Device time of the k-nearest-neighbour search (ops.knn_search at k = 8 / 16 / 32 on an already-built grid) next to the search stage
of the radius search (ops.radius_search, L.RS_SEARCH) on the same grid, and of postprocess.estimate_normals (grid, search and the
PCA kernel, k = 16) on the same clouds:
  1 x 1 views    268 324 x 268 324
  4 x 4 views    1 073 296 x 1 073 296
at the radii of radius_probe.py (about 8 and about 64 neighbours per query, found by bisection as there; the clouds are its synthetic
prediction maps in pixel order). If scipy imports, cKDTree.query(k, distance_upper_bound=radius, workers=8) on the same inputs is
printed as well (build + query, host, one run).

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups. A step also checks
composition: count equals the radius search's, rank 0 its index and sqdist, and k = 8 is the first eight columns of k = 32.

    python tools/probes/knn_probe.py [--out profiles/knn_probe.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe import timed, views  # noqa: E402

CASES = ((1, 1), (4, 4))          # (query views, reference views)
TARGETS = (8, 64)
KS = (8, 16, 32)
STEP_TIMEOUT = 360                # seconds per GPU step


def step(nqv, nrv):
    """The GPU step (child process): prints one RESULT line per target radius."""
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    qh, rh = views(0, nqv), views(nqv, nrv)
    q, r = torch.from_numpy(qh).cuda(), torch.from_numpy(rh).cuda()
    nq, nr = q.shape[0], r.shape[0]
    ws = torch.empty(ops.radius_workspace_bytes(nq, nr), device="cuda", dtype=torch.uint8)
    pick = torch.from_numpy(np.random.default_rng(1).choice(nq, 16384, replace=False)).cuda()

    def mean_count(radius):
        r2 = postprocess._radius_sq(radius)
        args = dict(query=q[pick].contiguous(), reference=r, radius_sq=r2, cell=ops.radius_reach(r2), ws=ws)
        stats = ops.radius_search(L.RS_BUILD, **args)[0].tolist()
        if stats[3] > 4000 * pick.numel():
            return None
        return float(ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, **args)[1].double().mean())

    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    for target in TARGETS:
        lo, hi = 1e-4, 1.0
        for _ in range(14):
            mid = (lo * hi) ** 0.5
            m = mean_count(mid)
            lo, hi = (lo, mid) if m is None or m > target else (mid, hi)
        radius = lo
        r2 = postprocess._radius_sq(radius)
        args = dict(query=q, reference=r, radius_sq=r2, cell=ops.radius_reach(r2), ws=ws)
        stats = ops.radius_search(L.RS_BUILD, **args)[0].tolist()
        cnt, idx, sq = (torch.empty(nq, device="cuda", dtype=dt) for dt in (torch.int32, torch.int32, torch.float32))
        search = timed(lambda: ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, count=cnt, index=idx, sqdist=sq, **args))
        out, times = {}, []
        for k in KS:
            kc = torch.empty(nq, device="cuda", dtype=torch.int32)
            ki, kd = torch.empty(nq, k, device="cuda", dtype=torch.int32), torch.empty(nq, k, device="cuda", dtype=torch.float32)
            times.append(timed(lambda: ops.knn_search(k=k, max_pairs=1 << 40, count=kc, index=ki, sqdist=kd, **args)))
            out[k] = (kc, ki, kd)
        wrong = 0
        for k in KS:
            kc, ki, kd = out[k]
            wrong += int((kc != cnt).sum() + (ki[:, 0] != idx).sum() + (kd[:, 0].view(torch.int32) != sq.view(torch.int32)).sum())
            wrong += int((ki != out[KS[-1]][1][:, :k]).sum() + (kd.view(torch.int32) != out[KS[-1]][2][:, :k].view(torch.int32)).sum())
        normals = timed(lambda: postprocess.estimate_normals(q, k=16, radius=radius), warm=1, reps=3)
        tree = "- -"
        if cKDTree is not None:
            a = time.perf_counter()
            t = cKDTree(rh)
            b = time.perf_counter()
            t.query(qh, k=16, distance_upper_bound=radius, workers=8)
            tree = "%.1f %.1f" % ((b - a) * 1e3, (time.perf_counter() - b) * 1e3)
        print("RESULT %d %d %d %.6g %.3f %d %s %s %s %d %s" % (
            nq, nr, target, radius, float(cnt.double().mean()), stats[3], "%.4f %.4f %.4f" % search,
            " ".join("%.4f %.4f %.4f" % t for t in times), "%.4f %.4f %.4f" % normals, wrong, tree), flush=True)
        if wrong:
            sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("k nearest neighbours within a radius on the built hash grid; ms by events, median (min .. max) of 5 after 2 warm-ups; clouds: synthetic views in pixel order.")
    say("radius search: the SEARCH stage of ops.radius_search on the same grid; normals: postprocess.estimate_normals(k = 16), grid and search included (3 runs);")
    say("cKDTree: scipy build / query(k = 16, distance_upper_bound = radius, workers = 8) on the host, ms, one run.")
    say("%21s %9s %7s %12s | %-24s | %-24s %-24s %-24s | %-26s | %s" % ("nq x nr", "radius", "mean n", "pairs", "radius search ms", "k = 8 ms", "k = 16 ms",
                                                                       "k = 32 ms", "normals ms", "cKDTree build / query ms"))
    failed = None
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(float(x) for x in v)
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step"] + [str(v) for v in case]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            say("%21s %9.4g %7.2f %12d | %-24s | %-24s %-24s %-24s | %-26s | %s" % (
                "%s x %s" % (r[1], r[2]), float(r[4]), float(r[5]), int(r[6]), fmt(r[7:10]), fmt(r[10:13]), fmt(r[13:16]), fmt(r[16:19]), fmt(r[19:22]),
                "%s / %s" % (r[23], r[24])))
        if p.returncode != 0 or len(res) != len(TARGETS):
            failed = "%r: the GPU step ended with status %d; nothing is started after it\n%s" % (case, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
