"""Device time of farthest-point sampling (ops.farthest_point_sample) at B x N x npoint = 8 x 8192 x 1024 (the one-workgroup form),
1 x 268 324 x 2048 and 1 x 1 048 576 x 4096 (the per-step form) against
  (a) the same rule written as a loop of torch operations on the same GPU (gather the centre, squared distances, minimum, arg-max:
      what a user of the reference's Python sampler has today), and
  (b) the numpy twin (tests/fps_twin.py) on the host.
The clouds are seeded surface samples: points on a unit sphere and a ground plane with 1 % noise.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups for the device function, of 3
after 1 warm-up for the torch loop. The step also reports how many of the torch loop's indices equal the device function's (its
sum of squares is rounded differently, so a near-tie may go the other way) and both coverage radii.

    python tools/probes/fps_probe.py [--no-host] [--out profiles/fps_probe.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((8, 8192, 1024), (1, 518 * 518, 2048), (1, 1 << 20, 4096))
STEP_TIMEOUT = 300           # seconds per GPU step: the largest takes a few seconds of device time plus start-up


def clouds(B, N, seed=0):
    rng = np.random.default_rng(seed + N)
    v = rng.normal(size=(B, N, 3))
    p = v / np.linalg.norm(v, axis=-1, keepdims=True)
    ground = rng.random((B, N)) < 0.4
    k = int(ground.sum())
    p[ground] = np.stack([rng.uniform(-3, 3, k), np.full(k, -1.0), rng.uniform(-3, 3, k)], 1)
    return (p + rng.normal(0.0, 0.01, (B, N, 3))).astype(np.float32)


def torch_loop(xyz, npoint):
    """The rule for clean clouds as torch operations, one sample per iteration. -> (index int64 [B, npoint], distance f32 [B, N])."""
    import torch
    B, N, _ = xyz.shape
    index = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    mind = torch.full((B, N), 1e10, device=xyz.device)
    rows = torch.arange(B, device=xyz.device)
    c = torch.zeros(B, dtype=torch.long, device=xyz.device)
    for i in range(npoint):
        index[:, i] = c
        d = ((xyz - xyz[rows, c].view(B, 1, 3)) ** 2).sum(-1)
        mind = torch.minimum(mind, d)
        c = mind.max(-1)[1]
    return index, mind


def timed(run, warm, reps):
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


def step(B, N, npoint):
    """The GPU step (child process): prints one RESULT line."""
    import torch
    from omnivggt_official_amd import lib as L, ops
    L.require_gpu()
    xyz = torch.from_numpy(clouds(B, N)).cuda()
    ws = torch.empty(ops.fps_workspace_bytes(B, N, npoint), device="cuda", dtype=torch.uint8)
    idx, sq = torch.empty(B, npoint, device="cuda", dtype=torch.int32), torch.empty(B, npoint, device="cuda", dtype=torch.float32)
    dist = torch.empty(B, N, device="cuda", dtype=torch.float32)
    dev = timed(lambda: ops.farthest_point_sample(xyz, npoint, ws=ws, index=idx, sqdist=sq, distance=dist), 2, 5)
    out = []
    loop = timed(lambda: out.append(torch_loop(xyz, npoint)), 1, 3)
    tidx, tdist = out[-1]
    same = int((tidx == idx.long()).sum())
    print("RESULT %d %d %d %.4f %.4f %.4f %.4f %.4f %.4f %d %d %.9g %.9g" % (
        B, N, npoint, *dev, *loop, same, int(idx.to(torch.int64).sum()), float(dist.max().sqrt()), float(tdist.max().sqrt())), flush=True)


def host(B, N, npoint):
    import fps_twin as twin
    xyz = clouds(B, N)
    t0 = time.perf_counter()
    idx, _, dist = twin.sample(xyz, npoint)
    return (time.perf_counter() - t0) * 1e3, int(idx.astype(np.int64).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    from omnivggt_official_amd import lib as L
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("farthest-point sampling, B x N x npoint; device and torch loop: ms by events, median (min .. max) of 5 after 2 warm-ups / of 3 after 1;")
    say("host: tests/fps_twin.py in numpy, one run. One workgroup per cloud up to N = %d, one launch per sample above." % L.FPS_SMALL_MAX)
    say("%22s | %-30s %9s | %-32s %8s | %10s %8s | %s" % ("B x N x npoint", "device ms", "us/sample", "torch loop ms (same GPU)", "loop/dev", "host ms",
                                                        "host/dev", "indices equal to the loop's; index sums (device, host); coverage radius (device, loop)"))
    failed = None
    for B, N, npoint in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(B), str(N), str(npoint)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        if p.returncode != 0 or len(res) != 1:
            failed = "%d x %d x %d: the GPU step ended with status %d; nothing is started after it\n%s" % (B, N, npoint, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
        r = res[0]
        dev, loop = [float(v) for v in r[4:7]], [float(v) for v in r[7:10]]
        same, isum, rad, lrad = int(r[10]), int(r[11]), float(r[12]), float(r[13])
        hs, tail = "%10s %8s" % ("-", "-"), "%d" % isum
        if not a.no_host:
            hms, hsum = host(B, N, npoint)
            hs, tail = "%10.0f %8.1f" % (hms, hms / dev[0]), "%d, %d" % (isum, hsum)
        say("%22s | %-30s %9.2f | %-32s %8.1f | %s | %d of %d; %s; %.6g, %.6g" % (
            "%d x %d x %d" % (B, N, npoint), "%.3f (%.3f .. %.3f)" % tuple(dev), 1e3 * dev[0] / npoint, "%.1f (%.1f .. %.1f)" % tuple(loop),
            loop[0] / dev[0], hs, same, B * npoint, tail, rad, lrad))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
