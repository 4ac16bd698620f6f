"""Device time of the registration entries (ops.align_moments, ops.align_solve, ops.align_apply) and of one ICP iteration
(postprocess.icp(iterations=1) with each search), next to the same steps written as torch operations on the same GPU:
  268 324 pairs      one 518 x 518 view of radius_probe.py's synthetic prediction maps against itself, moved a little
  1 048 576 pairs    the first 2^20 points of four views
torch moments: the 18 sums as float64 tensor operations (subtract, outer products, sum); torch solve: Umeyama by torch.linalg.svd of
the 3 x 3 cross-covariance; torch apply: (p.double() @ R^T + t).float(); torch search: torch.cdist in chunks of 1024 queries and min
(only at 268 324: the 2^20 case would evaluate 1.1e12 distances through a [1024, 2^20] buffer).

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups (ICP iterations: 3 after 1).
A step also checks itself: two moment calls give the same bytes, and the fitted transform recovers the applied one.

    python tools/probes/align_probe.py [--out profiles/align_probe.txt]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe import HW, timed, views  # noqa: E402

CASES = (HW * HW, 1 << 20)
MAX_DISTANCE = 0.02               # about three pixel spacings of the synthetic views: the gate and the grid's radius
STEP_TIMEOUT = 300                # seconds per GPU step


def torch_moments(p, q, c):
    import torch
    a, b, d = p.double() - c[:3], q.double() - c[3:], q.double() - p.double()
    return torch.cat([a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1),
                      torch.stack([(a * a).sum(), (b * b).sum(), (d * d).sum()])])


def torch_solve(n, s, c):
    import torch
    S = s[6:15].reshape(3, 3) - torch.outer(s[0:3], s[3:6]) / n
    U, D, Vt = torch.linalg.svd(S.T / n)
    E = torch.ones(3, device=s.device, dtype=torch.float64)
    E[2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    R = U @ torch.diag(E) @ Vt
    scale = (D * E).sum() / ((s[15] - (s[0:3] ** 2).sum() / n) / n)
    T = torch.eye(4, device=s.device, dtype=torch.float64)
    T[:3, :3] = scale * R
    T[:3, 3] = (s[3:6] / n + c[3:]) - T[:3, :3] @ (s[0:3] / n + c[:3])
    return T


def torch_apply(p, T):
    return (p.double() @ T[:3, :3].T + T[:3, 3]).float()


def torch_nearest(q, r, chunk=1024):
    import torch
    idx = torch.empty(q.shape[0], device=q.device, dtype=torch.int64)
    for a in range(0, q.shape[0], chunk):
        idx[a:a + chunk] = torch.cdist(q[a:a + chunk], r).argmin(1)
    return idx


def step(n):
    """The GPU step (child process): prints one RESULT line."""
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    tgt_h = views(0, (n + HW * HW - 1) // (HW * HW))[:n]
    ang = np.radians(0.05)
    M = np.eye(4)
    M[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    M[:3, 3] = [0.002, -0.001, 0.0015]
    src_h = (tgt_h.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)          # source = M target: the fit must return inv(M)
    src, tgt = torch.from_numpy(src_h).cuda(), torch.from_numpy(tgt_h).cuda()
    ws = torch.empty(ops.align_workspace_bytes(n), device="cuda", dtype=torch.uint8)
    count, sums = torch.empty(1, device="cuda", dtype=torch.int64), torch.empty(18, device="cuda", dtype=torch.float64)
    ops.align_moments(src, tgt, ws=ws, count=count, sums=sums)
    centre = (sums[:6] / count.double()).contiguous()
    first = sums.clone()
    t_plain = timed(lambda: ops.align_moments(src, tgt, ws=ws, count=count, sums=sums))
    same = bool((first.view(torch.int64) == sums.view(torch.int64)).all())
    t_centred = timed(lambda: ops.align_moments(src, tgt, centre=centre, ws=ws, count=count, sums=sums))
    T = torch.empty(4, 4, device="cuda", dtype=torch.float64)
    t_solve = timed(lambda: ops.align_solve(count, sums, T, centre=centre))
    out = torch.empty_like(src)
    t_apply = timed(lambda: ops.align_apply(src, T, out=out))
    t_fit = timed(lambda: postprocess.fit_similarity(src, tgt))
    err = float((T @ torch.from_numpy(M).cuda() - torch.eye(4, device="cuda", dtype=torch.float64)).abs().max())
    tt_moments = timed(lambda: torch_moments(src, tgt, centre))
    ts = torch_moments(src, tgt, centre)
    tt_solve = timed(lambda: torch_solve(float(n), ts, centre))
    Tt = torch_solve(float(n), ts, centre)
    tt_apply = timed(lambda: torch_apply(src, Tt))
    terr = float((Tt - T).abs().max())
    icp_ex = timed(lambda: postprocess.icp(src, tgt, iterations=1, max_distance=MAX_DISTANCE), warm=1, reps=3)
    icp_grid = timed(lambda: postprocess.icp(src, tgt, iterations=1, max_distance=MAX_DISTANCE, search="grid"), warm=1, reps=3)
    used = int(postprocess.icp(src, tgt, iterations=1, max_distance=MAX_DISTANCE, search="grid").count[0])

    def torch_iteration():
        eye = torch.eye(4, device="cuda", dtype=torch.float64)
        moved = torch_apply(src, eye)
        j = torch_nearest(moved, tgt)
        q = tgt[j]
        keep = ((q - moved) ** 2).sum(1) <= MAX_DISTANCE ** 2
        p2, q2 = moved[keep], q[keep]
        c = torch.cat([p2.double().mean(0), q2.double().mean(0)])
        return torch_solve(float(p2.shape[0]), torch_moments(p2, q2, c), c) @ eye

    icp_torch = timed(torch_iteration, warm=1, reps=3) if n <= HW * HW else (float("nan"),) * 3
    f = lambda t: "%.4f %.4f %.4f" % t
    print("RESULT %d %s %s %s %s %s %s %s %s %s %s %s %d %d %.3g %.3g" % (
        n, f(t_plain), f(t_centred), f(t_solve), f(t_apply), f(t_fit), f(tt_moments), f(tt_solve), f(tt_apply), f(icp_ex), f(icp_grid),
        f(icp_torch), used, same, err, terr), flush=True)
    if not same or not err <= 1e-6:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("registration of n pairs (a synthetic view against itself moved by 0.05 degrees and 2.7e-3); ms by events, median (min .. max) of 5 after 2 warm-ups")
    say("(ICP iterations: 3 after 1); torch: the same step as float64 tensor operations / torch.linalg.svd / chunked torch.cdist on the same GPU.")
    say("fit: postprocess.fit_similarity (two moment passes, the centre, the solve); icp: postprocess.icp(iterations=1, max_distance=%g), apply + search +" % MAX_DISTANCE)
    say("two gated moment passes + solve. GB/s: 24 bytes per pair (moments: two float32 points, no index, masks or gate; apply: a point read and written).")
    names = ("moments", "moments, centred", "solve", "apply", "fit", "torch moments", "torch solve", "torch apply", "icp exhaustive", "icp grid", "torch icp exhaustive")
    failed = None
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(float(x) for x in v)
    for n in CASES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(n)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            say("n = %d pairs; ICP pairs used %d; two calls identical: %s; |T M - I| %s; |T_torch - T| %s" % (int(r[1]), int(r[35]), bool(int(r[36])), r[37], r[38]))
            for k, name in enumerate(names):
                t = r[2 + 3 * k:5 + 3 * k]
                extra = "   %.0f GB/s" % (24.0 * int(r[1]) / float(t[0]) * 1e-6) if name.startswith("moments") or name == "apply" else ""
                say("  %-22s %s%s" % (name, "-" if t[0] == "nan" else fmt(t), extra))
        if p.returncode != 0 or len(res) != 1:
            failed = "n = %d: the GPU step ended with status %d; nothing is started after it\n%s" % (n, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
