"""Device time of clustering a point cloud (ops.radius_search BUILD + ops.cluster, timed apart) and, where scipy imports, the host
path on the same inputs (scipy.spatial.cKDTree.query_pairs + scipy.sparse.csgraph.connected_components, wall clock, one run).
  1 view      268 324 points, radii giving about 8 and about 64 neighbours per point
  4 views     1 073 296 points, likewise
  64 views    17 172 736 points, likewise; no host path at this size (the pair list alone is 0.5e9 pairs at 64 neighbours)
The clouds are radius_probe's: synthetic prediction maps in pixel order. The radius of a case is found on the device by bisection
on the mean count of 16 384 sampled points. ovg_cluster runs as connected components (min_neighbours 0) and as DBSCAN
(min_neighbours 4); the host path computes the connected components only.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups. A step also checks the
device's components with the host's where both ran and reports the points whose root (the lowest index of the cluster) differs.

    python tools/probes/cluster_probe.py [--out profiles/cluster_probe.txt]
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

CASES = ((1, 1), (4, 1), (64, 0))               # (views, run the host path)
TARGETS = (8, 64)
MIN_NEIGHBOURS = (0, 4)
STEP_TIMEOUT = 420           # seconds per GPU step


def host_components(points, radius):
    """-> (seconds for the pairs, seconds for the components, root int32 [n]: the lowest index of every point's component)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(points)
    t0 = time.perf_counter()
    pairs = cKDTree(points).query_pairs(radius, output_type="ndarray")
    t1 = time.perf_counter()
    graph = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    t2 = time.perf_counter()
    low = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(low, comp, np.arange(n))
    return t1 - t0, t2 - t1, low[comp].astype(np.int32)


def step(nviews, host):
    """The GPU step (child process): prints one RESULT line per target."""
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    cloud = views(0, nviews)
    p = torch.from_numpy(cloud).cuda()
    n = p.shape[0]
    ws = torch.empty(ops.radius_workspace_bytes(n, n), device="cuda", dtype=torch.uint8)
    pick = torch.from_numpy(np.random.default_rng(1).choice(n, 16384, replace=False)).cuda()

    def mean_count(radius):
        """Mean neighbours of the sampled points; None when the guard refuses."""
        r2 = postprocess._radius_sq(radius)
        args = dict(query=p[pick].contiguous(), reference=p, radius_sq=r2, cell=ops.radius_reach(r2), ws=ws)
        stats = ops.radius_search(L.RS_BUILD, **args)[0].tolist()
        if stats[3] > 4000 * pick.numel():
            return None
        cnt = ops.radius_search(L.RS_SEARCH, max_pairs=1 << 40, **args)[1]
        return float(cnt.double().mean()) - 1.0                                  # a sampled point finds itself

    try:
        import scipy  # noqa: F401
    except ImportError:
        host = 0
    for target in TARGETS:
        lo, hi = 1e-4, 1.0
        for _ in range(14):
            mid = (lo * hi) ** 0.5
            m = mean_count(mid)
            lo, hi = (lo, mid) if m is None or m > target else (mid, hi)
        radius = lo
        r2 = postprocess._radius_sq(radius)
        cell = ops.radius_reach(r2)
        stats = torch.empty(4, device="cuda", dtype=torch.int64)
        build = timed(lambda: ops.radius_search(L.RS_BUILD, p, p, r2, cell, ws, exclude_self=True, out_stats=stats))
        pairs = int(stats[3])
        root, kind, degree = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.uint8), torch.empty(n, device="cuda", dtype=torch.int32)
        out = []
        for mn in MIN_NEIGHBOURS:
            ms = timed(lambda: ops.cluster(p, r2, cell, ws, mn, max_pairs=1 << 40, out_stats=stats, root=root, kind=kind, degree=degree))
            if int(stats[0]):
                print("flags %d" % int(stats[0]), flush=True)
                sys.exit(4)
            member = root[root >= 0]
            sizes = torch.unique(member, return_counts=True)[1]
            out.append((ms, int(sizes.numel()), int(sizes.max()) if sizes.numel() else 0, int((kind == L.CL_BORDER).sum()), int((kind == L.CL_NOISE).sum())))
        mean_k = float(degree.double().mean())
        wrong, ht = -1, "- -"
        if host:
            ops.cluster(p, r2, cell, ws, 0, max_pairs=1 << 40, root=root, kind=kind, degree=False)
            t_pairs, t_cc, want = host_components(cloud, float(np.float32(radius)))
            # float64 against float32 at the radius: a pair within rounding of it may connect on one side only, so the differing
            # points are reported, not asserted
            wrong = int((root.cpu().numpy() != want).sum())
            ht = "%.3f %.3f" % (t_pairs, t_cc)
        print("RESULT %d %d %.6g %.3f %d %.4f %.4f %.4f %s %d %s" % (
            n, target, radius, mean_k, pairs, *build,
            " ".join("%.4f %.4f %.4f %d %d %d %d" % (*ms, c, big, border, noise) for ms, c, big, border, noise in out), wrong, ht), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("clustering on the hash grid (ovg_radius_search BUILD + ovg_cluster); ms by events, median (min .. max) of 5 after 2 warm-ups;")
    say("clouds: synthetic views in pixel order. cc: min_neighbours 0 (connected components); dbscan: min_neighbours %d." % MIN_NEIGHBOURS[1])
    say("host: cKDTree.query_pairs + csgraph.connected_components in float64, seconds of wall clock, one run; differ: points whose root")
    say("differs from the host's (pairs within float rounding of the radius may connect on one side only).")
    say("%10s %9s %7s %12s | %-24s %-27s %9s %9s | %-27s %8s %8s %8s | %-19s %9s %7s" % (
        "points", "radius", "mean k", "pairs", "build ms", "cc ms", "clusters", "largest", "dbscan ms", "clusters", "border", "noise",
        "host pairs + cc s", "speed-up", "differ"))
    failed = None
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step"] + [str(v) for v in case]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            build, cc, db = [float(v) for v in r[6:9]], [float(v) for v in r[9:12]], [float(v) for v in r[16:19]]
            host, speed = "-", "-"
            if r[24] != "-":
                host = "%.2f + %.2f" % (float(r[24]), float(r[25]))
                speed = "%.0f" % ((float(r[24]) + float(r[25])) * 1e3 / (build[0] + cc[0]))
            say("%10d %9.4g %7.2f %12d | %-24s %-27s %9d %9d | %-27s %8d %8d %8d | %-19s %9s %7s" % (
                int(r[1]), float(r[3]), float(r[4]), int(r[5]), "%.3f (%.3f .. %.3f)" % tuple(build), "%.3f (%.3f .. %.3f)" % tuple(cc),
                int(r[12]), int(r[13]), "%.3f (%.3f .. %.3f)" % tuple(db), int(r[19]), int(r[21]), int(r[22]), host, speed,
                r[23] if r[23] != "-1" else "-"))
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
