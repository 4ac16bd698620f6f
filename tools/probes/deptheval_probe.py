"""Device time of the depth-evaluation entries (ops.deptheval_median, ops.deptheval_sums in both modes, ops.deptheval_solve) and of
the whole postprocess.depth_metrics call, next to the same figures written as masked float64 torch operations on the same GPU
(boolean compaction of the used pixels, torch.median on the compacted values, sums and ratios as tensor operations):
  8 and 64 views of 518 x 518; per-view and sequence scope; all four alignments
gt is uniform in [0.5, 8], pred = gt (1 + 0.1 noise) 1.7 + 0.3, 80 % of the pixels valid (seeded, generated on the device).

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing
after it. Device figures are torch events around the call: median (min .. max) of 7 after 2 warm-ups. A step also checks itself:
two calls give the same bytes, and the entries' figures agree with the torch ones to 1e-9.

    python tools/probes/deptheval_probe.py [--out profiles/deptheval_probe.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe import HW, timed  # noqa: E402

VIEWS = (8, 64)
ALIGNS = ("none", "median", "scale", "scale_shift")
SCOPES = ("view", "sequence")
STEP_TIMEOUT = 300                # seconds per GPU step
FIGURES = ("abs_rel", "rmse", "rmse_log", "delta1")


def torch_metrics(pred, gt, valid, align, scope):
    """The yardstick: the same figures per group as masked float64 torch operations. -> float64 [G, 4] (abs_rel, rmse, rmse_log, delta1)"""
    import torch
    S = pred.shape[0]
    groups = [(pred[k], gt[k], valid[k]) for k in range(S)] if scope == "view" else [(pred, gt, valid)]
    out = []
    for p, g, v in groups:
        use = v & torch.isfinite(p) & torch.isfinite(g) & (p > 0) & (g > 0)
        p, g = p[use].double(), g[use].double()
        s, t = 1.0, 0.0
        if align == "median":                                                 # the mean of the two middles, as numpy.median has it
            s = (g.median() + (-(-g).median())) / (p.median() + (-(-p).median()))
        elif align == "scale":
            s = (p * g).sum() / (p * p).sum()
        elif align == "scale_shift":
            n, sp, sg = p.numel(), p.sum(), g.sum()
            s = (n * (p * g).sum() - sp * sg) / (n * (p * p).sum() - sp * sp)
            t = (sg - s * sp) / n
        q = (s * p + t).clamp_min(1e-3)
        e = q - g
        ratio = torch.maximum(q / g, g / q)
        out.append(torch.stack([(e.abs() / g).mean(), (e * e).mean().sqrt(), ((q.log() - g.log()) ** 2).mean().sqrt(), (ratio < 1.25).double().mean()]))
    return torch.stack(out)


def step(S):
    """The GPU step (child process): prints RESULT lines."""
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(S)
    gt = torch.rand(S, HW, HW, device="cuda", generator=gen) * 7.5 + 0.5
    pred = gt * (1 + 0.1 * torch.randn(S, HW, HW, device="cuda", generator=gen)) * 1.7 + 0.3
    valid = torch.rand(S, HW, HW, device="cuda", generator=gen) < 0.8
    ok = True
    for scope in SCOPES:
        shape = (S, HW * HW) if scope == "view" else (1, S * HW * HW)
        G, n = shape
        p, g, v = pred.reshape(shape), gt.reshape(shape), valid.view(torch.uint8).reshape(shape)
        mws = torch.empty(ops.deptheval_median_workspace_bytes(G, n), device="cuda", dtype=torch.uint8)
        sws = torch.empty(ops.deptheval_sums_workspace_bytes(G, n), device="cuda", dtype=torch.uint8)
        count, med = torch.empty(G, device="cuda", dtype=torch.int64), torch.empty(G, 2, 2, device="cuda", dtype=torch.float32)
        counts, sums = torch.empty(G, 4, device="cuda", dtype=torch.int64), torch.empty(G, 5, device="cuda", dtype=torch.float64)
        coeff, status = torch.empty(G, 2, device="cuda", dtype=torch.float64), torch.empty(G, device="cuda", dtype=torch.int32)
        t_med = timed(lambda: ops.deptheval_median(p, g, v, ws=mws, count=count, median=med), reps=7)
        first = med.clone()
        t_mom = timed(lambda: ops.deptheval_sums(p, g, v, ws=sws, counts=counts, sums=sums), reps=7)
        moments = sums.clone()
        t_solve = timed(lambda: ops.deptheval_solve(L.DEPTHEVAL_SCALE_SHIFT, counts, sums=moments, coeff=coeff, status=status), reps=7)
        t_met = timed(lambda: ops.deptheval_sums(p, g, v, coeff=coeff, ws=sws, counts=counts, sums=sums), reps=7)
        ops.deptheval_median(p, g, v, ws=mws, count=count, median=med)
        same = bool((first.view(torch.int32) == med.view(torch.int32)).all())
        f = lambda t: "%.4f %.4f %.4f" % t
        print("RESULT entries %d %s %d %d %s %s %s %s %d" % (S, scope, G, n, f(t_med), f(t_mom), f(t_solve), f(t_met), same), flush=True)
        ok = ok and same
        for align in ALIGNS:
            t_all = timed(lambda: postprocess.depth_metrics(pred, gt, valid, align, scope), reps=7)
            t_torch = timed(lambda: torch_metrics(pred, gt, valid, align, scope), reps=7)
            res, ref = postprocess.depth_metrics(pred, gt, valid, align, scope), torch_metrics(pred, gt, valid, align, scope)
            got = torch.stack([getattr(res, k) for k in FIGURES], 1)
            dev = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
            print("RESULT whole %d %s %s %s %s %.3g %.6f %.6f" % (S, scope, align, f(t_all), f(t_torch), dev, res.mean["abs_rel"], res.mean["delta1"]), flush=True)
            ok = ok and dev <= 1e-9
    if not ok:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deptheval_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("depth evaluation of S views of %d x %d (gt uniform in [0.5, 8], pred = gt (1 + 0.1 noise) 1.7 + 0.3, 80 %% valid); ms by events," % (HW, HW))
    say("median (min .. max) of 7 after 2 warm-ups. Entries alone: median (the radix select: four histogram passes), moments and metrics (one pass")
    say("and a fold each), solve. GB/s: 9 bytes per pixel and pass (two float32 maps and the mask). whole: postprocess.depth_metrics, the alignment,")
    say("the metric pass, the float64 ratios and the one read-back; torch: the same figures as masked float64 tensor operations on the same GPU")
    say("(boolean compaction per group, torch.median on the compacted values).")
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(float(x) for x in v)
    failed = None
    for S in VIEWS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(S)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            if r[1] == "entries":
                px = int(r[4]) * int(r[5])
                say("S = %d, scope %s: %d group(s) of %d pixels; two median calls identical: %s" % (int(r[2]), r[3], int(r[4]), int(r[5]), bool(int(r[18]))))
                for k, (name, passes) in enumerate((("median", 4), ("moments", 1), ("solve", 0), ("metrics", 1))):
                    t = r[6 + 3 * k:9 + 3 * k]
                    say("  %-22s %s%s" % (name, fmt(t), "   %.0f GB/s" % (9.0 * passes * px / float(t[0]) * 1e-6) if passes else ""))
            else:
                say("  whole, %-12s %s   torch %s   x %.1f   largest relative difference of abs_rel / rmse / rmse_log / delta1 %s; abs_rel %s delta1 %s"
                    % (r[4], fmt(r[5:8]), fmt(r[8:11]), float(r[8]) / float(r[5]), r[11], r[12], r[13]))
        if p.returncode != 0 or len(res) != 2 * (1 + len(ALIGNS)):
            failed = "S = %d: the GPU step ended with status %d; nothing is started after it\n%s" % (S, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
