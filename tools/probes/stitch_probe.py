"""Device time of stitching overlapping chunks (postprocess.stitch_predictions, fit_similarity_robust, ops.align_move_maps) and of a
long sequence run in chunks (OmniVGGT.forward_chunked):
  stitch     two synthetic chunks of 8 views at 518 x 518 (radius_probe.py's views; the second chunk is the scene under a Sim(3), with 1e-3
             noise and a fifth of its pixels displaced), overlap 4: the whole stitch, the robust fit over the 4 x 518 x 518 overlap pairs
             alone, and the move of the 4 owned views alone -- next to the same reweighted fit (weights, Cauchy reweighting by the previous
             fit's weighted rms, two passes and a solve per iteration, nothing read back) written as float64 torch operations with
             torch.linalg.svd on the same GPU
  chunked    128 views at 518 x 518 in float16 (seeded synthetic weights: no checkpoint offline) as chunks of 32 with overlap 4
             (5 chunks) against the single 128-view forward of the same build; both return the prediction dict for all 128 views

Every GPU step is a child process of its own under `timeout`; the driver stops at the first step that fails and starts nothing after
it. Device figures are torch events around the call: median (min .. max) of 5 after 2 warm-ups (forwards: 2 after 1). There is no gate
on either time; a step that could not be measured is reported as NOT measured.

    python tools/probes/stitch_probe.py [--out profiles/stitch_probe.txt] [--only stitch|chunked]
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

STEP_TIMEOUT = {"stitch": 300, "chunked": 900}
VIEWS, OVERLAP = 8, 4
ITERATIONS, REL_DELTA = 6, 0.5


def torch_robust_fit(p, q, w, valid, iterations=ITERATIONS, rel_delta=REL_DELTA):
    """fit_similarity_robust's loop as float64 torch operations; delta stays on the device."""
    import torch
    P, Q = p.double(), q.double()
    w0 = torch.where(valid, w.double(), torch.zeros((), device=p.device, dtype=torch.float64))
    T = torch.eye(4, device=p.device, dtype=torch.float64)
    fit_rms = None
    for k in range(iterations + 1):
        W = w0
        if k:
            r2 = ((Q - (P @ T[:3, :3].T + T[:3, 3])) ** 2).sum(1)
            d = rel_delta * fit_rms
            W = w0 / (1.0 + r2 / (d * d))
        sw = W.sum()
        mp, mq = (W[:, None] * P).sum(0) / sw, (W[:, None] * Q).sum(0) / sw
        A, B = P - mp, Q - mq
        S = (W[:, None] * A).T @ B / sw
        var, vb = (W * (A * A).sum(1)).sum() / sw, (W * (B * B).sum(1)).sum() / sw
        U, D, Vt = torch.linalg.svd(S.T)
        E = torch.ones(3, device=p.device, dtype=torch.float64)
        E[2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
        R = U @ torch.diag(E) @ Vt
        tr = (D * E).sum()
        scale = tr / var
        T = torch.eye(4, device=p.device, dtype=torch.float64)
        T[:3, :3] = scale * R
        T[:3, 3] = mq - T[:3, :3] @ mp
        fit_rms = (vb - tr * tr / var).clamp_min(0).sqrt()
    return T


def _chunks():
    """-> ([chunk 0, chunk 1] of device tensors, plan, the Sim(3) that takes chunk 1's frame to chunk 0's)"""
    import torch
    plan = [(0, VIEWS), (VIEWS - OVERLAP, 2 * VIEWS - OVERLAP)]
    rng = np.random.default_rng(7)
    a = np.radians(25.0)
    G = np.eye(4)
    G[:3, :3] = 1.3 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    G[:3, 3] = [0.4, -0.3, 0.2]
    Gi = np.linalg.inv(G)
    chunks = []
    for c, (s, e) in enumerate(plan):
        n = e - s
        pts = views(s, n).astype(np.float64)
        if c:
            pts = pts @ Gi[:3, :3].T + Gi[:3, 3] + rng.normal(size=pts.shape) * 1e-3
        conf = rng.uniform(1, 3, n * HW * HW)
        if c:
            bad = rng.random(n * HW * HW) < 0.2
            pts[bad] += rng.uniform(0, 0.5, (int(bad.sum()), 3))
            conf[bad] = rng.uniform(1, 3, int(bad.sum())) * 0.9                 # displaced pixels keep a usual confidence: the fit has to cope
        enc = np.zeros((1, n, 9), np.float32)
        enc[..., 6], enc[..., 7:] = 1.0, 1.0
        f32 = lambda x, *shape: torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(shape)).cuda()
        chunks.append({"world_points": f32(pts, 1, n, HW, HW, 3), "world_points_conf": f32(conf, 1, n, HW, HW),
                       "depth": f32(np.linalg.norm(pts, axis=1), 1, n, HW, HW, 1), "depth_conf": f32(conf, 1, n, HW, HW),
                       "pose_enc": torch.from_numpy(enc).cuda(), "pose_enc_list": [torch.from_numpy(enc).cuda()] * 4,
                       "images": torch.zeros(1, n, 3, HW, HW, device="cuda")})
    return chunks, plan, G


def step_stitch():
    import torch
    from omnivggt_official_amd import lib as L, ops, postprocess
    L.require_gpu()
    chunks, plan, G = _chunks()
    out = postprocess.stitch_predictions(chunks, plan)
    T = out["chunk_transforms"][1].transform.matrix
    err = float((T - torch.from_numpy(G).cuda()).abs().max())
    again = postprocess.stitch_predictions(chunks, plan)
    same = bool(torch.equal(out["world_points"], again["world_points"]) and torch.equal(T, again["chunk_transforms"][1].transform.matrix))
    t_stitch = timed(lambda: postprocess.stitch_predictions(chunks, plan))
    n = OVERLAP * HW * HW
    src = chunks[1]["world_points"][0, :OVERLAP].reshape(n, 3)
    tgt = chunks[0]["world_points"][0, VIEWS - OVERLAP:].reshape(n, 3)
    cs, ct = chunks[1]["world_points_conf"][0, :OVERLAP].reshape(n), chunks[0]["world_points_conf"][0, VIEWS - OVERLAP:].reshape(n)
    sv, tv = cs >= postprocess.percentile(cs, 50.0), ct >= postprocess.percentile(ct, 50.0)
    w = torch.minimum(cs, ct)
    t_fit = timed(lambda: postprocess.fit_similarity_robust(src, tgt, weights=w, source_valid=sv, target_valid=tv))
    t_plain = timed(lambda: postprocess.fit_similarity(src, tgt, source_valid=sv, target_valid=tv))
    m = (VIEWS - OVERLAP) * HW * HW
    own = {k: chunks[1][k][0, OVERLAP:].contiguous() for k in ("world_points", "depth", "world_points_conf", "depth_conf")}
    dst = {k: torch.empty_like(v) for k, v in own.items()}
    s = out["chunk_transforms"][1].transform.scale.reshape(1)
    t_move = timed(lambda: ops.align_move_maps(m, T, s, own["world_points"], own["depth"], own["world_points_conf"], own["depth_conf"],
                                               dst["world_points"], dst["depth"], dst["world_points_conf"], dst["depth_conf"]))
    valid = sv & tv
    t_torch = timed(lambda: torch_robust_fit(src, tgt, w, valid))
    terr = float((torch_robust_fit(src, tgt, w, valid) - T).abs().max())
    f = lambda t: "%.4f %.4f %.4f" % t
    print("RESULT stitch %s %s %s %s %s %d %d %.3g %.3g %d" % (f(t_stitch), f(t_fit), f(t_plain), f(t_move), f(t_torch), n, m, err, terr, same), flush=True)
    if not same or not err <= 1e-2:
        sys.exit(3)


def step_chunked():
    import torch
    from omnivggt_official_amd import lib as L, weights
    from omnivggt_official_amd.model import OmniVGGT
    L.require_gpu()
    S, chunk, overlap = 128, 32, 4
    with torch.device("meta"):
        model = OmniVGGT(compute_dtype=torch.float16)
    sd = weights.synthetic_state_dict(weights.manifest_of(model), seed=2)
    model = model.to_empty(device="cpu")
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    images = torch.rand(1, S, 3, HW, HW, generator=torch.Generator().manual_seed(1234)).cuda()
    with torch.no_grad():
        t_chunked = timed(lambda: model.forward_chunked(images, chunk_size=chunk, overlap=overlap), warm=1, reps=2)
        out = model.forward_chunked(images, chunk_size=chunk, overlap=overlap)
        status = [int(v) for f in out["chunk_transforms"] for v in f.status.tolist()]
        finite = bool(torch.isfinite(out["world_points"]).all())
        n_chunks = len(out["chunks"])
        del out
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model.forward_chunked(images, chunk_size=chunk, overlap=overlap)
        peak_chunked = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t_single = timed(lambda: model(images), warm=1, reps=2)
        peak_single = torch.cuda.max_memory_allocated()
    f = lambda t: "%.2f %.2f %.2f" % t
    print("RESULT chunked %s %s %d %d %d %.2f %.2f" % (f(t_chunked), f(t_single), n_chunks, finite, sum(1 for v in status if v), peak_chunked / 2 ** 30,
                                                     peak_single / 2 ** 30), flush=True)
    if not finite:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, choices=("stitch", "chunked"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stitch_probe.txt"))
    a = ap.parse_args()
    if a.step:
        return {"stitch": step_stitch, "chunked": step_chunked}[a.step]()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(float(x) for x in v)
    say("stitching overlapping chunks; ms by events, median (min .. max) of 5 after 2 warm-ups (forwards: 2 after 1). No gate on any time.")
    failed = None
    for name in ("stitch", "chunked"):
        if a.only and a.only != name:
            say("%s: NOT measured (not asked for in this run)" % name)
            continue
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[name]), sys.executable, os.path.abspath(__file__), "--step", name]
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [line.split() for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        for r in res:
            if name == "stitch":
                say("stitch: two chunks of %d views at %d x %d, overlap %d: %s overlap pairs, %s owned pixels; |T - planted| %s; two calls identical: %s" % (
                    VIEWS, HW, HW, OVERLAP, r[17], r[18], r[19], bool(int(r[21]))))
                for k, label in enumerate(("stitch_predictions (percentiles, fit, move, cameras)", "fit_similarity_robust, %d refits (21 launches + centres)" % ITERATIONS,
                                           "fit_similarity (the plain fit, for scale)", "align_move_maps, four maps of the owned views",
                                           "torch: the same reweighted fit in float64 operations")):
                    say("  %-62s %s" % (label, fmt(r[2 + 3 * k:5 + 3 * k])))
                say("  |T_torch - T| %s (another summation order and an SVD in the place of Horn's method)" % r[20])
            else:
                say("chunked: 128 views at %d x %d, float16, seeded synthetic weights; %s chunks of 32 with overlap 4; outputs finite: %s; degenerate refits: %s" % (
                    HW, HW, r[8], bool(int(r[9])), r[10]))
                say("  %-62s %s   peak %s GiB allocated" % ("forward_chunked (5 forwards of <= 32 views + 4 stitches)", fmt(r[2:5]), r[11]))
                say("  %-62s %s   peak %s GiB allocated" % ("forward, all 128 views at once", fmt(r[5:8]), r[12]))
        if p.returncode != 0 or len(res) != 1:
            failed = "%s: NOT measured: the GPU step ended with status %d; nothing is started after it\n%s" % (name, p.returncode, (p.stdout + p.stderr)[-2000:])
            say(failed)
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
