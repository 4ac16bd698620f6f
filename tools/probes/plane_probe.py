"""Device time of plane segmentation, stage by stage (ops.plane_hypotheses, plane_score, plane_select, plane_mask and the fit of one
refit round: two ops.align_moments passes and ops.plane_fit; the round's mask is the mask stage again), against two other ways to
score the same planes:
  torch       the same scoring as chunked torch operations on the same GPU: points @ planes[:, :3].T + w, abs() <= t, sum(0)
              (a matrix product rounds differently from the rule's residual, so its counts may differ near the threshold: the
              number of planes whose count differs is reported, not asserted)
  twin        tests/plane_twin.py's numpy score on the host, wall clock, one run, at the smallest size only; its counts must equal
              the device's
Points: 268 324 (one view), 1 048 576 and the 17 172 736-point cloud of 64 views; H: 256, 1024 and 4096 hypotheses. The clouds are
radius_probe's synthetic views in pixel order; the threshold is 0.01.

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups (torch: 3 after 1).

    python tools/probes/plane_probe.py [--out profiles/plane_probe.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from radius_probe import timed, views  # noqa: E402

CASES = ((1, 268324, 1), (4, 1048576, 0), (64, 17172736, 0))      # (views generated, points used, run the host twin)
HYPOTHESES = (256, 1024, 4096)
THRESHOLD = 0.01
STEP_TIMEOUT = 420           # seconds per GPU step
TORCH_CHUNK_BYTES = 1 << 29  # the [chunk, H] float32 residuals of the torch form


def torch_score(p, planes, t):
    import torch
    H = planes.shape[0]
    chunk = max(1, TORCH_CHUNK_BYTES // (4 * H))
    normal_t, w = planes[:, :3].t().contiguous(), planes[:, 3]
    count = torch.zeros(H, device=p.device, dtype=torch.int64)
    for a in range(0, p.shape[0], chunk):
        count += ((p[a:a + chunk] @ normal_t + w).abs() <= t).sum(0)
    return count


def step(nviews, n, host):
    """The GPU step (child process): prints one RESULT line per H."""
    import torch
    from omnivggt_official_amd import lib as L, ops
    L.require_gpu()
    cloud = np.ascontiguousarray(views(0, nviews)[:n])
    p = torch.from_numpy(cloud).cuda()
    assert p.shape[0] == n
    for H in HYPOTHESES:
        planes, index = ops.plane_hypotheses(p, H, 0)
        hyp = timed(lambda: ops.plane_hypotheses(p, H, 0, planes=planes, index=index))
        count = torch.empty(H, device="cuda", dtype=torch.int32)
        score = timed(lambda: ops.plane_score(p, planes, THRESHOLD, count=count))
        sel = ops.plane_select(count, planes, 3)
        select = timed(lambda: ops.plane_select(count, planes, 3, *sel))
        best, plane, best_count, status = sel
        inlier, _, total = ops.plane_mask(p, plane, THRESHOLD, gate=status)
        mask = timed(lambda: ops.plane_mask(p, plane, THRESHOLD, gate=status, inlier=inlier, out_count=total))
        ws = torch.empty(ops.align_workspace_bytes(n), device="cuda", dtype=torch.uint8)
        fitted = plane.clone()

        def refit():
            n0, s0 = ops.align_moments(p, p, source_valid=inlier, ws=ws)
            centre = s0[:6] / n0.clamp_min(1).to(torch.float64)
            n1, s1 = ops.align_moments(p, p, source_valid=inlier, centre=centre, ws=ws)
            ops.plane_fit(n1, s1, fitted, centre=centre)
        fit = timed(refit)
        live = ~torch.isnan(planes).any(1)
        ref = torch_score(p, planes, THRESHOLD)
        differ = int(((ref != count.long()) & live).sum())
        tch = timed(lambda: torch_score(p, planes, THRESHOLD), warm=1, reps=3)
        twin_s, twin_ok = -1.0, -1
        if host and H == HYPOTHESES[0]:
            import plane_twin
            t0 = time.perf_counter()
            want = plane_twin.score(cloud, planes.cpu().numpy(), THRESHOLD)
            twin_s = time.perf_counter() - t0
            twin_ok = int((want == count.cpu().numpy()).all())
        print("RESULT %d %d %d %d %d %s %d %.4f %d" % (
            n, H, int(live.sum()), int(best_count), int(total),
            " ".join("%.4f %.4f %.4f" % v for v in (hyp, score, select, mask, fit, tch)), differ, twin_s, twin_ok), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("plane segmentation stage by stage (ovg_plane_hypotheses / _score / _select / _mask; refit: 2 x ovg_align_moments + ovg_plane_fit);")
    say("ms by events, median (min .. max) of 5 after 2 warm-ups; clouds: synthetic views in pixel order; threshold %g; seed 0." % THRESHOLD)
    say("Gpairs/s: points x hypotheses over the score time. torch: points @ normals^T + w, abs() <= t, sum(0) in chunks of %d MiB on the" % (TORCH_CHUNK_BYTES >> 20))
    say("same GPU, median (min .. max) of 3 after 1 warm-up; differ: live planes whose torch count is not the rule's (a matrix product")
    say("rounds differently). twin: tests/plane_twin.py's numpy score on the host, seconds of wall clock, one run; its counts equal the device's.")
    say("%10s %5s %5s %9s | %-22s %-27s %8s %-22s %-22s %-24s | %-30s %6s %8s | %s" % (
        "points", "H", "live", "winner", "hypotheses ms", "score ms", "Gpairs/s", "select ms", "mask ms", "refit ms", "torch score ms", "differ",
        "torch/hip", "twin s"))
    failed = None
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step"] + [str(v) for v in case]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            n, H = int(r[1]), int(r[2])
            t = [[float(v) for v in r[6 + 3 * k:9 + 3 * k]] for k in range(6)]
            fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)
            twin = "-" if float(r[25]) < 0 else "%.2f (%s)" % (float(r[25]), "equal" if r[26] == "1" else "DIFFERENT")
            say("%10d %5d %5d %9d | %-22s %-27s %8.1f %-22s %-22s %-24s | %-30s %6d %8.2f | %s" % (
                n, H, int(r[3]), int(r[4]), fmt(t[0]), fmt(t[1]), n * H / t[1][0] / 1e6, fmt(t[2]), fmt(t[3]), fmt(t[4]), fmt(t[5]), int(r[24]),
                t[5][0] / t[1][0], twin))
        if p.returncode != 0 or len(res) != len(HYPOTHESES):
            failed = "%r: the GPU step ended with status %d; nothing is started after it\n%s" % (case, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
