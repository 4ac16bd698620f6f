#!/usr/bin/env python
"""Benchmark of the OmniVGGT aggregator hot path on MI355X (contract: see the task prompt).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--views S] [--dtype bf16|f16|f32] [--dump-outputs DIR] [--full]
        (N > 1 without a launcher around it: the script starts its own N ranks -- self_launch -- and returns their exit code)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is ONE forward of the aggregator (DINOv2 embed + modality fusion + 24 x [frame block,
camera injection, global block]) over one synthetic multi-view batch already resident in HBM.
Default workload at every N: 64 views, 518^2, images-only, bf16 -- BASELINE.json configs[3] and the
north star's scaling statement ("frames/sec at 1/2/4/8 GPUs ... on 64-view 518^2 synthetic input";
SURVEY.md section 8d: "Config 4 ... also run G=1,2,4 for the scaling curve"), so `python bench.py --gpus N`
for N=1,2,4,8 IS that strong-scaling curve ("scaling": "strong": total work fixed, views sharded over the
ranks).  N > 1: the timed exchange form is the head-parallel all-to-all (sharding.py; `--shard-mode` picks it).

A plain run does only what the headline needs: it sets up, warms up, times the K steps, writes the outputs of
the last one (--dump-outputs), and prints the JSON line: `value`, `ms_per_step`, `config`, `roofline` (the live
per-launch timing of the global attention inside the timed steps, plus the committed profiles/traffic.json
figure when it matches the attention sources).  Everything else the benchmark measures or checks runs only with
--full, after the headline measurement, and adds its own fields to the same line.

With --full at N > 1 the JSON line also carries `preflight` (before anything is timed: both exchange forms on
the bench's own input, compared, and the attention launch against several CU budgets), `comm`: the
un-overlapped cost of the exchange per layer (collectives issued alone), the compute-only step (same kernels,
no collective) and exposed_comm_ms = step - compute-only, plus `second_form`: the same measurement with the
north star's K/V all-gather form.

With --full at N=1 the same JSON line carries
  `secondary`    the 8-view configs[1] measurement (frames/s + roofline of the same kernel on that shape);
  `parity`       the timed 16-bit forward cross-checked against the parity-proven f32 mode of the SAME library on
                 the SAME inputs, per sampled layer, at 8 and at 64 views (max-rel and rms-rel) -- the headline
                 number rests on verified outputs; the f32 mode's own throughput at 8 views rides along, and so does
                 the split-f16 mode (`f32x_mode`: the <= 1e-4 mode with throughput -- its distance from the f32 mode per
                 sampled layer and its frames/s at 8 and at 64 views);
  `cpu_baseline` the oracle (CPU restatement of the reference) timed on the host: one frame block + one global
                 block + one DINO block at the REAL 64-view shapes, extrapolated x24, plus a complete
                 2-view forward.
  `e2e`          the whole OmniVGGT.forward (aggregator + camera head + both DPT heads) at the timed view count, and at
                 8 views next to `secondary`.
The --no-* options drop single items of --full.
--views S overrides the view count; --aux adds depth + camera tokens on every view (configs[2]).
--dump-outputs DIR writes what the last timed step returned (a fixed, seeded sample of every layer's tokens, and
patch_start_idx) as DIR/<name>.npy; the inputs and weights are seeded, so two builds can be compared output for output.

N > 1 robustness: every rank runs a watchdog thread (--watchdog-s): a rank that makes no progress for that long dumps the
stacks of all its threads to stderr, tagged with its rank and the stage it was in, rank 0 prints the JSON line with what has
been measured so far plus a `watchdog` record, and the process exits -- a hung collective yields a diagnosable record instead
of a silent timeout. With --full, a form that disagrees with the other in the pre-flight by more than 5e-2 is not used as the
primary.

Prints ONE JSON line on rank 0.
"""
import argparse
import faulthandler
import json
import os
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from omnivggt_official_amd import lib as L, weights  # noqa: E402
from omnivggt_official_amd.model import OmniVGGT  # noqa: E402

P_TOK, C = 1374, 1024
# MI355X_MICROARCH.md, dense MFMA. f32x (split-f16, three f16 MFMAs per product): a third of the f16 peak per ALGORITHMIC flop
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "f32x": 2500.0 / 3.0}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x": L.F32X}
KERNEL_NAME = {"bf16": "attn16_kernel<bf16,QB=%d,WAVES=%d,MODE=0> (speculative anchored softmax + verified fallback; K/V^T tiles by LDS-DMA; %d-row q tiles)",
               "f16": "attn16_kernel<f16,QB=%d,WAVES=%d,MODE=1> (lazy-rescale online softmax; K/V^T tiles by LDS-DMA; %d-row q tiles)",
               "f32": "attn_kernel<float,QB=1> (exact-f32 MFMA 16x16x4, classic online softmax)",
               "f32x": "attn16_kernel<f16,QB=2,WAVES=8,MODE=1,X3> (split-f16: q / K / V^T / P as (hi, lo) f16 planes, three f16 MFMAs per product, "
                       "lazy-rescale online softmax, exact f32 row sums; K / V^T tiles by LDS-DMA; 256-row q tiles)"}


def kernel_name(dtype_name, n_q, n_k):
    """Name of the global-attention kernel the library's launch plan picks for this shape (ovg_attn_plan)."""
    if dtype_name in ("f32", "f32x"):
        return KERNEL_NAME[dtype_name]
    from omnivggt_official_amd import ops
    plan = ops.attn_plan(16, n_q, [n_k], DT[dtype_name])
    qb, waves = {128: (2, 4), 256: (4, 4), 512: (4, 8)}[plan["q_tile"]]          # q tile = 16 x QB x WAVES rows (dispatch16 in ovg_attn.hip)
    name = KERNEL_NAME[dtype_name] % (qb, waves, plan["q_tile"])
    if plan["tail_q_tile"] and plan["splits"] > 1:                                    # key-split tail (ABI 9)
        return name + "; rows %d.. of every head in a second launch cut into %d key ranges + merge" % (plan["main_rows"], plan["splits"])
    if plan["tail_q_tile"]:
        name += "; rows %d.. of every head in a second launch of %d-row tiles" % (plan["main_rows"], plan["tail_q_tile"])
    return name + (", split-KV x%d" % plan["splits"] if plan["splits"] > 1 else "")
PARITY_LAYERS = (0, 4, 11, 17, 23)


class Watchdog:
    """Progress monitor of one rank. `stage(name)` is the heartbeat; a stage older than `timeout` seconds means a hang
    (in practice: a collective some rank never joined): dump every thread's stack to stderr, let rank 0 print the JSON
    line with what exists, and exit the process so the launcher tears the job down."""

    def __init__(self, rank, world, timeout, partial_result):
        self.rank, self.world, self.timeout, self.partial = rank, world, float(timeout), partial_result
        self.name, self.t0, self.done = "start", time.time(), False
        if timeout > 0:
            threading.Thread(target=self._run, daemon=True).start()

    def stage(self, name, quiet=False):
        self.name, self.t0 = name, time.time()
        if self.world > 1 and not quiet:
            sys.stderr.write("[rank %d/%d %s] %s\n" % (self.rank, self.world, time.strftime("%H:%M:%S"), name))
            sys.stderr.flush()

    def _run(self):
        while not self.done:
            time.sleep(1.0)
            if time.time() - self.t0 > self.timeout:
                sys.stderr.write("[rank %d/%d] WATCHDOG: no progress for %.0f s in stage '%s'; thread stacks follow\n"
                                 % (self.rank, self.world, self.timeout, self.name))
                faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
                sys.stderr.flush()
                if self.rank == 0:
                    out = dict(self.partial)
                    out["watchdog"] = {"stage": self.name, "timeout_s": self.timeout, "rank": self.rank}
                    print(json.dumps(out), flush=True)
                os._exit(3)


def attention_source_digest():
    """sha256 over the sources that define the attention kernels and their launch plan (what profiles/traffic.json is tied to)."""
    import hashlib
    h = hashlib.sha256()
    for f in ("ovg_attn.hip", "ovg_attn16.h", "ovg_attn16_body_q4.inc", "ovg_attn16_body_q2.inc", "ovg_common.h"):
        with open(os.path.join(ROOT, "omnivggt-official_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def agg_flops(S):
    """F(S) and F_ga(S) for B=1 (FLOP)."""
    f_ga = 96.0 * (S * P_TOK) ** 2 * 1024
    return S * (72 * 34.58e9 + 48 * 7.73e9 + 1.65e9) + f_ga, f_ga


def synthetic_inputs(S, device, seed=1234, aux=False):
    """SURVEY.md section 8d inputs: images U[0,1); with aux also random-rotation cameras, depth 0.5+5U,
    mask Bernoulli(0.8).  Images-only runs carry the loader's zero placeholders (visual_util.py:793-824)."""
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(1, S, 3, 518, 518, generator=g)
    z = lambda *s: torch.zeros(*s)
    if not aux:
        return dict(images=images.to(device), extrinsics=z(1, S, 3, 4).to(device), intrinsics=z(1, S, 3, 3).to(device),
                    depth=z(1, S, 518, 518, 1).to(device), mask=z(1, S, 518, 518).to(device))
    from omnivggt_official_amd.camera_math import quaternion_to_rotation
    q = torch.randn(S, 4, generator=g)
    R = quaternion_to_rotation(q / q.norm(dim=-1, keepdim=True))
    ext = torch.cat([R, torch.randn(S, 3, 1, generator=g)], dim=-1).unsqueeze(0)
    f = 400 + 300 * torch.rand(S, generator=g)
    K = torch.zeros(1, S, 3, 3)
    K[0, :, 0, 0], K[0, :, 1, 1], K[0, :, 0, 2], K[0, :, 1, 2], K[0, :, 2, 2] = f, f, 259.0, 259.0, 1.0
    depth = 0.5 + 5 * torch.rand(1, S, 518, 518, 1, generator=g)
    mask = (torch.rand(1, S, 518, 518, generator=g) > 0.2).float()
    return dict(images=images.to(device), extrinsics=ext.to(device), intrinsics=K.to(device), depth=depth.to(device), mask=mask.to(device))


def launch_command(n, argv, port, script=None):
    """The command line `python bench.py --gpus N` re-executes itself under: torch's elastic launcher, one rank per GPU on this
    node, rendezvous on 127.0.0.1 (the container hostname may not resolve) at `port`; argv is forwarded verbatim."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(n)), "--master-addr", "127.0.0.1",
            "--master-port", str(int(port)), script or os.path.abspath(__file__)] + list(argv)


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n, argv, script=None, timeout=None):
    """Run N ranks of this script (launch_command) and return the job's exit code. The ranks inherit stdout / stderr: rank 0's ONE
    JSON line is the only thing on stdout (the launcher's own chatter goes to stderr), so `python bench.py --gpus N` behaves
    like the N = 1 call. A rank that dies makes the launcher tear the others down and return non-zero; a rank that hangs is
    the per-rank watchdog's business (it prints a partial line and exits 3)."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL / cross-process device memory on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, int(n)))))
    cmd = launch_command(n, argv, free_port(), script)
    sys.stderr.write("[bench launcher] %s\n" % " ".join(cmd))
    sys.stderr.flush()
    try:
        return subprocess.run(cmd, env=env, timeout=timeout).returncode
    except subprocess.TimeoutExpired:
        sys.stderr.write("[bench launcher] timed out after %s s\n" % timeout)
        return 124


RCCL_LOG = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ovg_bench_rccl_rank%d.log")


def rccl_channels_observed(rank):
    """Channel counts RCCL reported while it set up its communicators (NCCL_DEBUG=INFO lines "N coll channels, ... M p2p channels, K p2p
    channels per peer", written to RCCL_LOG by this run): what sharding.available_cus() should have subtracted. None + reason when the
    job configured NCCL_DEBUG itself or the lines are absent."""
    import re
    path = RCCL_LOG % rank
    if os.environ.get("NCCL_DEBUG_FILE") != path:
        return {"unavailable": "NCCL_DEBUG was set by the job: its own log has the channel lines"}
    try:
        text = open(path, errors="replace").read()
    except OSError as e:
        return {"unavailable": repr(e)[:120]}
    out = {}
    m = re.findall(r"(\d+) coll channels", text)
    if m:
        out["coll_channels"] = max(int(v) for v in m)
    m = re.findall(r"(\d+) p2p channels(?:, (\d+) p2p channels per peer)?", text)
    if m:
        out["p2p_channels"] = max(int(a) for a, _ in m)
        per = [int(b) for _, b in m if b]
        if per:
            out["p2p_channels_per_peer"] = max(per)
    m = re.search(r"(?:RCCL|NCCL) version ([^\s]+)", text)
    if m:
        out["version"] = m.group(1)
    return out or {"unavailable": "no channel lines in %s (%d bytes)" % (path, len(text))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=0, help="total views S (default 64 at every N)")
    ap.add_argument("--dtype", default="bf16", choices=list(DT))
    ap.add_argument("--full", action="store_true", help="after the headline measurement also run everything else the benchmark measures or "
                    "checks: N=1 secondary, parity, e2e, cpu_baseline; N>1 preflight, comm, second_form (the --no-* options drop single items)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline (N=1)")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the f32-mode cross-check of the timed outputs (N=1)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the 8-view secondary measurement (N=1)")
    ap.add_argument("--torch-heads", action="store_true", help="with --full: run the DPT heads of the end-to-end measurement as f32 PyTorch modules instead of the HIP kernels")
    ap.add_argument("--e2e-views", type=int, default=0, help="view count of the end-to-end measurement (default: the timed view count, and 8 views next to the secondary)")
    ap.add_argument("--e2e", action="store_true", help="(kept for old command lines) the end-to-end measurement is part of --full")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the end-to-end measurement (aggregator + camera head + both DPT heads; N = 1)")
    ap.add_argument("--attn-variant", type=int, default=0)
    ap.add_argument("--gemm-tile", type=int, default=0, help="force OVG_TILE_* on the block GEMMs (A/B runs)")
    ap.add_argument("--aux", action="store_true", help="depth + camera tokens on every view (BASELINE configs[2] with --views 16)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="N > 1: torch.distributed backend (nccl = RCCL; gloo only for debugging, e.g. several ranks on one GPU)")
    ap.add_argument("--shard-mode", default="auto", choices=["auto", "heads", "allgather"],
                    help="N > 1: exchange form of the global attention that `value` is measured with (sharding.ViewSharding)")
    ap.add_argument("--no-second-form", action="store_true", help="N > 1, with --full: do not also measure the other exchange form")
    ap.add_argument("--watchdog-s", type=float, default=float(os.environ.get("OVG_BENCH_WATCHDOG_S", "420")),
                    help="abort (with thread stacks, rank-tagged, and a partial JSON line) after this many seconds without progress; 0 = off")
    ap.add_argument("--partial-aux", action="store_true", help="cameras on the even views, depth on the second half of the views "
                    "(BASELINE configs[4] with --views 128 --dtype f16)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step returned as DIR/<name>.npy "
                    "(every layer's tokens at a fixed, seeded sample of token rows, and patch_start_idx)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: become the launcher of N ranks (one process per GPU) and hand back their verdict
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    result = {"metric": "frames/sec (518^2, S views) aggregator hot path", "value": None, "unit": "frames/s", "n_gpus": world,
              "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "strong",
              "vs_baseline": None, "dtype": args.dtype, "data": "synthetic"}
    wd = Watchdog(rank, world, args.watchdog_s, result)
    wd.stage("library load (a stale in-tree .so is rebuilt under a file lock: one rank compiles, the others wait)")
    wd.timeout = max(wd.timeout, 900.0) if args.watchdog_s > 0 else wd.timeout
    L.require_gpu()
    L.load()
    wd.timeout = float(args.watchdog_s)
    if os.environ.get("OVG_FORCE_DEVICE"):      # debugging aid: several ranks on one GPU (only if the RCCL build accepts it)
        local = int(os.environ["OVG_FORCE_DEVICE"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            # with --full, what RCCL actually sets up (channel counts) goes to a per-rank file that rank 0 parses into
            # comm.rccl_channels_observed; a job that configured NCCL_DEBUG itself keeps its own settings (and the field reports that)
            if args.full and "NCCL_DEBUG" not in os.environ:
                os.environ["NCCL_DEBUG"] = "INFO"
                os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,ENV")
                os.environ["NCCL_DEBUG_FILE"] = RCCL_LOG % rank
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:                                     # host backend: ViewSharding stages its collectives through the host
            dist.init_process_group(args.backend, rank=rank, world_size=world)
        wd.stage("process group up (%s)" % args.backend)

    dtype = DT[args.dtype]
    with torch.device("meta"):
        model = OmniVGGT(compute_dtype=dtype)
    manifest = weights.manifest_of(model)
    sd = weights.synthetic_state_dict(manifest, seed=2)
    model = model.to_empty(device="cpu")
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    wd.stage("model on device")
    agg = model.aggregator
    agg.attn_variant = args.attn_variant
    agg.gemm_tile = args.gemm_tile
    shard = None
    if world > 1:
        from omnivggt_official_amd.sharding import ViewSharding, resolve_mode
        shard = agg.shard = ViewSharding(gather_output=False, mode=args.shard_mode)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_max(vals):
        if dist is None:
            return vals
        t = torch.tensor(vals, device=dev if args.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def make_step(S):
        inp = synthetic_inputs(S, dev, aux=args.aux or args.partial_aux)
        idx = list(range(S)) if args.aux else []
        didx, cidx = (list(range(S // 2, S)), list(range(0, S, 2))) if args.partial_aux else (idx, idx)
        return lambda: agg(inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], didx, cidx)

    def timed_steps(step, steps, warmup):
        """EXACTLY `steps` timed forwards between barrier + synchronize on both sides; MAX over ranks."""
        agg.enable_attention_events(steps * agg.depth * 4)   # live HIP-event timing of every global-attention launch
        if agg.fallback_counter is None:
            agg.enable_fallback_counter(dev)                 # speculative-softmax telemetry: workgroups that re-ran (one atomic each)
        for i in range(warmup):
            wd.stage("warm-up step %d/%d" % (i + 1, warmup))
            step()
            if world > 1:
                torch.cuda.synchronize()                     # warm-up only: a hang shows up in THIS stage, not three stages later
        agg.reset_attention_events()
        agg.read_fallback_counter()                          # zero it for the timed region (synchronises; outside the timing)
        wd.stage("barrier before the timed region")
        barrier()
        wd.stage("timed region: %d steps" % steps)
        t0 = time.perf_counter()
        for i in range(steps):
            if i + 1 < steps:
                step()                                       # result dropped at once: the next step reuses its memory
            else:
                last = step()                                # what the last timed step returned (--dump-outputs)
            wd.stage("timed step queued", quiet=True)        # heartbeat only (no I/O inside the timed region)
        barrier()
        dt = time.perf_counter() - t0
        ms, fl = agg.attention_event_times(), agg.attention_event_flops()
        agg.disable_attention_events()
        fb = agg.read_fallback_counter() or 0
        dt, attn_ms, fb = reduce_max([dt, sum(ms), float(fb)])
        return dt, attn_ms, sum(fl), len(ms), int(fb), last

    def reduce_sum(t):
        if dist is None:
            return t
        t = t.to(dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def measure(S, steps, warmup, dump_dir=None):
        """Time `steps` aggregator forwards on S views; returns the result dict (rank-reduced). With dump_dir, the outputs of the
        last timed step are written there (dump_outputs) before anything else runs."""
        step = make_step(S)
        n_local = S // world + (1 if rank < S % world else 0)
        dt, attn_ms, attn_flop, launches, fallbacks, last = timed_steps(step, steps, warmup)
        if dump_dir is not None:
            wd.stage("dump of the last timed step's outputs")
            view0 = shard.last_partition[rank][0] if shard is not None else 0
            result["dump_outputs"] = dump_outputs(dump_dir, last, S, view0, reduce_sum, rank == 0)
        del last
        f_total, _ = agg_flops(S)
        achieved = attn_flop / (attn_ms * 1e-3) / 1e12 if attn_ms > 0 else 0.0
        peak = PEAK_TFLOPS[args.dtype]
        cfg = "2" if (args.aux and S == 16) else ("4" if (args.partial_aux and S == 128) else ("-" if (args.aux or args.partial_aux) else {8: "1", 64: "3"}.get(S, "-")))
        form = ""
        if shard is not None:
            from omnivggt_official_amd.sharding import head_groups
            ex_now = next(iter(shard._executors.values()), None)
            ng = len(head_groups(16 // world, world, n_local * P_TOK, cus=int(getattr(ex_now, "cus", 0)) or 256)) if 16 % world == 0 else 1
            form = ", " + {"heads": "head-parallel all-to-all, %s" % ("2 pipelined head groups" if ng == 2 else "1 head group per rank"),
                           "allgather": "K/V all-gather, local keys first + log-sum-exp merge"}[shard.last_mode]
        res = {
            "value": round(S * steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 3),
            "config": {"workload": "OmniVGGT aggregator forward, %d views 518x518 %s (BASELINE configs[%s]), view-sharded over %d GPU(s)"
                                   % (S, "+ depth + camera tokens" if args.aux else ("+ partial aux (cameras on even views, depth on the second half)" if args.partial_aux else "images-only"), cfg, world),
                       "views": S, "views_per_gpu": n_local, "tokens": S * P_TOK, "weights": "seeded synthetic (no checkpoint offline)",
                       "parallelism": "view-shard x%d%s" % (world, form)},
            "algorithmic_tflop_per_step": round(f_total / 1e12, 2),
            "tflops_per_gpu": round(f_total / 1e12 / (dt / steps) / world, 1),
            "roofline": {"bound": "mfma", "kernel": kernel_name(args.dtype, n_local * P_TOK, S * P_TOK) + " (global cross-view attention, D=64)",
                         "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": None,
                         "flop_per_launch": attn_flop / max(launches, 1), "avg_launch_ms": round(attn_ms / max(launches, 1), 4),
                         "launches_timed": launches,
                         # bf16: workgroups of ALL attention launches of the timed steps (DINOv2 + frame + global) whose speculative
                         # softmax pass failed its check and re-ran with the lazy-rescale body (max over ranks); 0 = the fast path always paid
                         "fallback_workgroups": fallbacks if args.dtype == "bf16" else None},
        }
        if shard is not None and args.full:
            res["comm"] = comm_report(step, S, steps, dt / steps * 1e3)
        torch.cuda.empty_cache()
        return res

    def comm_report(step, S, steps, step_ms):
        """N > 1: (i) the exchange of one layer issued alone (nothing to hide behind), (ii) the sharded step with every
        collective skipped (same kernels on the stale exchange buffers) -> exposed = step - compute-only."""
        wd.stage("comm report: exchange-only loop (%s)" % shard.last_mode)
        for _ in range(2):
            shard.exchange_only(agg, S, dev, mode=shard.last_mode, layers=agg.depth)
        barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            shard.exchange_only(agg, S, dev, mode=shard.last_mode, layers=agg.depth)
        barrier()
        ex_ms = (time.perf_counter() - t0) / 3 * 1e3
        wd.stage("comm report: compute-only steps")
        shard.skip_comm = True
        step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        barrier()
        comp_ms = (time.perf_counter() - t0) / steps * 1e3
        shard.skip_comm = False
        ex_ms, comp_ms = reduce_max([ex_ms, comp_ms])
        rep = {"exchange_form": shard.last_mode, "comm_ms_per_layer": round(ex_ms / agg.depth, 4), "comm_ms_per_step_unoverlapped": round(ex_ms, 3),
               "compute_only_ms_per_step": round(comp_ms, 3), "exposed_comm_ms": round(step_ms - comp_ms, 3),
               "hidden_fraction": round(1.0 - max(step_ms - comp_ms, 0.0) / max(ex_ms, 1e-9), 3)}
        # what the launch plans of the global attention were told about the chip they share with RCCL (sharding.available_cus):
        # backend, rccl_channels / NCCL_MAX_NCHANNELS, attention_plan_cus of device_cus
        rep.update(shard.comm_report(torch.cuda.get_device_properties(dev).multi_processor_count))
        rep["rccl_channels_observed"] = rccl_channels_observed(rank) if args.backend == "nccl" else None
        if result.get("preflight", {}).get("attention_cus_table") is not None:
            rep["attention_cus_table"] = result["preflight"]["attention_cus_table"]
        return rep

    S = args.views or 64
    if shard is not None and args.full:
        # PRE-FLIGHT, before anything is timed (round-2 review: the exchange code had never met RCCL at N > 1): one forward
        # in each exchange form the shapes admit, on the bench's own input, compared across forms (MAX over ranks). Under the
        # watchdog, with rank-tagged stage lines on stderr. If the forms disagree the all-gather form -- two plain
        # all_gather_into_tensor calls per layer -- becomes the primary and the report says so.
        wd.stage("pre-flight: both exchange forms, one forward each")
        step = make_step(S)
        pre = shard.compare_modes(lambda: step()[0][-1], S, args.dtype in ("f32", "f32x"), on_stage=wd.stage)
        torch.cuda.synchronize()
        pre["tolerance"] = 5e-2
        pre["agree"] = pre.get("max_rel_heads_vs_allgather", 0.0) <= pre["tolerance"]
        # first-run insurance (round-5 review item 7): this rank's global-attention launch planned for 256 / 240 / 224 / 192 CUs, alone and
        # with one layer's inbound exchange in flight -- does the reservation behind sharding.available_cus() pay on this node?
        wd.stage("pre-flight: attention launch against the CU budgets")
        try:
            pre["attention_cus_table"] = shard.attention_cus_probe(agg, S, dev, [256, 240, 224, 192])
        except RuntimeError as e:                  # host-side failure only; a hung collective is the watchdog's business
            pre["attention_cus_table"] = {"error": repr(e)[:200]}
        result["preflight"] = pre
        if not pre["agree"] and args.shard_mode != "allgather":
            shard.mode = "allgather"
            pre["primary_forced_to"] = "allgather"
        del step
    wd.stage("primary measurement: %d views" % S)
    primary = measure(S, args.steps, args.warmup, dump_dir=args.dump_outputs)
    result.update({"value": primary["value"], "ms_per_step": primary["ms_per_step"]})
    result.update({k: primary[k] for k in ("config", "algorithmic_tflop_per_step", "tflops_per_gpu", "roofline")})
    if "comm" in primary:
        result["comm"] = primary["comm"]

    if shard is not None and args.full and not args.no_second_form:
        # the other exchange form on the same workload (never part of `value`): the north star names the K/V all-gather.
        # Host-side failures of this block are recorded, not raised -- the primary number above must reach the JSON line;
        # a HUNG collective is the watchdog's business (it prints the partial line and exits).
        first = shard.last_mode
        other = "allgather" if first == "heads" else "heads"
        try:
            resolve_mode(other, S, world, args.dtype in ("f32", "f32x"))       # same answer on every rank, no communication
            possible = result.get("preflight", {}).get("agree", True) or other == "allgather"
        except ValueError:
            possible = False
        if possible:
            saved_mode = shard.mode
            shard.mode = other
            wd.stage("second form: %s" % other)
            sec = measure(S, max(2, args.steps // 2), 1)
            result["second_form"] = {"frames_per_s": sec["value"], "ms_per_step": sec["ms_per_step"], "parallelism": sec["config"]["parallelism"],
                                     "roofline": sec["roofline"], "comm": sec["comm"],
                                     "forms_agree": {k: v for k, v in result.get("preflight", {}).items() if k in ("modes", "max_rel_heads_vs_allgather", "agree")}}
            shard.mode = saved_mode
        else:
            result["second_form"] = {"skipped": "the %s form is not available for S=%d, world=%d, dtype=%s (or failed the pre-flight)" % (other, S, world, args.dtype)}

    if args.full and world == 1 and S != 8 and not args.views and not args.no_secondary:
        wd.stage("secondary: 8 views")
        sec = measure(8, 10, 3)                                      # BASELINE configs[1] on the same process
        result["secondary"] = {"frames_per_s": sec["value"], "ms_per_step": sec["ms_per_step"], "config": sec["config"],
                               "tflops_per_gpu": sec["tflops_per_gpu"], "roofline": sec["roofline"]}

    if rank == 0 and world == 1:
        tr = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tr):
            # HBM / fabric bytes per global-attention launch from the committed rocprofv3 --pmc passes. They describe the
            # attention kernels they were taken on: the file carries the digest of the attention sources of that tree
            # (tools/pmc_summary.py --traffic-json writes it) and a stale record is NOT printed as if it were current.
            try:
                traffic = json.load(open(tr))
                current = attention_source_digest()
                if traffic.get("attention_source_digest") == current:
                    result["roofline"]["traffic"] = traffic.get("global_attn_S%d_bytes_per_launch" % S)
                    result["roofline"]["traffic_source"] = traffic.get("source", "profiles/traffic.json (rocprofv3 --pmc passes of this kernel, not re-measured in this run)")
                    if "secondary" in result:
                        result["secondary"]["roofline"]["traffic"] = traffic.get("global_attn_S8_bytes_per_launch")
                else:
                    result["roofline"]["traffic_source"] = ("profiles/traffic.json is STALE (taken on attention sources %s, this tree is %s): "
                                                            "traffic not reported" % (str(traffic.get("attention_source_digest"))[:12], current[:12]))
            except Exception as e:
                result["roofline"]["traffic_source"] = "profiles/traffic.json unreadable: %r" % (e,)
        if args.full and args.dtype != "f32" and not args.no_parity:
            wd.stage("parity block (f32 mode of the same library on the same inputs)")
            result["parity"] = parity_block(agg, dev, args, sorted({8, S}) if not (args.views or args.aux or args.partial_aux) else [S])
        if args.full and not args.no_e2e:
            # SURVEY 8d "report aggregator-only and end-to-end separately": the whole OmniVGGT.forward (aggregator + camera head + the two DPT
            # heads, all on the HIP kernels; `--torch-heads` forces PyTorch's) with the step protocol of the headline -- 2 warm-ups, then
            # timed forwards between synchronisations -- at the timed view count and, next to the secondary, at 8 views
            def e2e_measure(Se, reps):
                hd = "f32" if args.dtype in ("f32", "f32x") else args.dtype       # the split-f16 aggregator keeps the heads on the exact-f32 kernels
                inp = synthetic_inputs(Se, dev, aux=args.aux)
                idx = list(range(Se)) if args.aux else []
                model.hip_heads = not args.torch_heads
                full = lambda: model(inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], idx, idx)
                full()
                full()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(reps):
                    full()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t1) / reps * 1e3
                torch_heads = args.torch_heads or (hd == "f32" and not model.hip_heads_f32)
                return {"views": Se, "frames_per_s": round(Se / ms * 1e3, 3), "ms_per_forward": round(ms, 3), "forwards_timed": reps,
                        "dpt_heads": "pytorch-f32" if torch_heads else "hip-" + hd, "camera_head": "pytorch-f32" if torch_heads else "hip-" + hd,
                        "heads": ("three side streams, <= %d frames per DPT pass, one-launch output stage, pyramid levels of layers 4 / 11 / 17 started under the aggregator"
                                  % model.dpt_frames_chunk) if not torch_heads else "sequential"}
            try:
                wd.stage("end-to-end forward (aggregator + three heads)")
                Se = args.e2e_views or S
                result["e2e"] = e2e_measure(Se, 3 if Se > 16 else 5)
                if "secondary" in result and not args.e2e_views and Se != 8:
                    result["secondary"]["e2e"] = e2e_measure(8, 5)
            except Exception as e:  # never let the heads hide the hot-path number
                result["e2e_error"] = repr(e)[:200]
        if args.full and not args.no_cpu_baseline:
            wd.stage("cpu baseline (host cores)")
            wd.timeout = max(wd.timeout, 1800.0)       # CPU work: minutes on a loaded host are not a hang
            result["cpu_baseline"] = cpu_baseline(sd)
    wd.done = True
    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.destroy_process_group()


DUMP_ROWS, DUMP_SEED, DUMP_MAX_BYTES = 256, 0, 64 << 20


def dump_outputs(out_dir, last, S, view0, reduce_sum, write):
    """Write what one aggregator forward returned, (tokens of every layer (1, S, 1374, 2048) f32, patch_start_idx), as .npy files that
    two builds can compare output for output: tokens_layerNN.npy = the same DUMP_ROWS token rows of every layer (all 2048 channels),
    rows drawn once by a seeded permutation of the S * 1374 (view, token) rows, so the files depend on S alone; patch_start_idx.npy
    (float64 scalar). The forward may hold only views view0.. of the S (view sharding): each rank fills the sampled rows it holds,
    the others stay 0, and reduce_sum (a sum over the ranks) assembles the full sample exactly. Returns the record for the JSON line."""
    import numpy as np
    outs, start = last
    rows = S * P_TOK
    pick = torch.randperm(rows, generator=torch.Generator().manual_seed(DUMP_SEED))[:DUMP_ROWS].sort().values
    width = outs[0].shape[-1]
    assert len(outs) * len(pick) * width * 4 <= DUMP_MAX_BYTES
    arrays = {"patch_start_idx": np.array(start, dtype=np.float64)}
    lo = view0 * P_TOK
    for i, o in enumerate(outs):
        flat = o.reshape(-1, width)
        mine = (pick >= lo) & (pick < lo + flat.shape[0])
        sample = torch.zeros(len(pick), width, dtype=torch.float32, device=o.device)
        sample[mine.to(o.device)] = flat[(pick[mine] - lo).to(o.device)].float()
        arrays["tokens_layer%02d" % i] = reduce_sum(sample).cpu().numpy()
    if write:
        os.makedirs(out_dir, exist_ok=True)
        for name, a in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "files": sorted(n + ".npy" for n in arrays), "bytes": int(sum(a.nbytes for a in arrays.values())),
            "sample": "tokens_layerNN = rows torch.randperm(%d, seed %d)[:%d] (sorted) of layer NN's tokens viewed as (S * 1374, 2048)"
                      % (rows, DUMP_SEED, len(pick))}


def parity_block(agg, dev, args, view_counts):
    """Cross-check of the TIMED 16-bit path against the f32 parity mode of the same library (itself <= 1e-4 of the
    reference CPU path: tests/test_gpu_aggregator.py) on the bench's own inputs and sizes. Per sampled layer:
    max-rel = max|a-b| / max|b| and rms-rel = rms(a-b) / rms(b) over a strided sample of the (S,1374,2048) tokens."""
    dt16 = agg.compute_dtype
    out = {"mode_checked": repr(dt16).replace("torch.", ""),
           "reference": "same library in compute_dtype=float32 (exact-f32 MFMA; <= 1e-4 of the reference CPU path at S <= 3, tests/test_gpu_aggregator.py)",
           "layers": list(PARITY_LAYERS), "sample": "tokens[:, :, ::7, ::8] of each sampled layer"}

    def sample(outs):
        return [outs[i][0, :, ::7, ::8].float().cpu() for i in PARITY_LAYERS if i < len(outs)]

    for S in view_counts:
        inp = synthetic_inputs(S, dev, aux=args.aux or args.partial_aux)
        idx = list(range(S)) if args.aux else []
        didx, cidx = (list(range(S // 2, S)), list(range(0, S, 2))) if args.partial_aux else (idx, idx)
        run = lambda: agg(inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], didx, cidx)[0]
        agg.set_compute_dtype(dt16)
        low = sample(run())
        agg.set_compute_dtype(torch.float32)
        outs = run()
        ref = sample(outs)
        entry = {"max_rel": [], "rms_rel": [], "finite": True}
        for a, b in zip(low, ref):
            d = (a - b).double()
            entry["max_rel"].append(float("%.3e" % float(d.abs().max() / b.abs().max())))        # 4 significant digits: the split-f16 mode sits at 1e-6
            entry["rms_rel"].append(float("%.3e" % float(d.pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt())))
            entry["finite"] = entry["finite"] and bool(torch.isfinite(a).all())
        outs = None
        if S == 8:                                 # the 1e-4-compliant mode's own throughput on configs[1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 3 * 1e3
            f_total, _ = agg_flops(S)
            entry["f32_mode"] = {"frames_per_s": round(S / ms * 1e3, 3), "ms_per_step": round(ms, 3),
                                 "tflops": round(f_total / 1e12 / (ms * 1e-3), 1), "frac_of_f32_mfma_peak": round(f_total / 1e12 / (ms * 1e-3) / PEAK_TFLOPS["f32"], 4)}
        # the <= 1e-4 mode WITH throughput (split-f16, lib.F32X) on the same inputs: its distance from the exact-f32 mode and its own rate
        agg.set_compute_dtype(L.F32X)
        xs = sample(run())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 2 * 1e3
        entry["f32x_mode"] = {"max_rel_vs_f32_mode": [float("%.3e" % float((a - b).double().abs().max() / b.abs().max())) for a, b in zip(xs, ref)],
                              "frames_per_s": round(S / ms * 1e3, 3), "ms_per_step": round(ms, 3),
                              "what": "compute_dtype='f32x': (hi, lo) f16 planes, three f16 MFMAs per product; <= 1e-4 of the reference like the f32 mode (tests)"}
        # the opt-in faster form of that mode (round 6): attention's PV contraction without its P_lo x V_hi product (aggregator.f32x_fast_pv).
        # Reported next to the mode, never as the mode: it keeps 3e-5 here but reaches 1.0e-4 on single rows of the depth-1 64-view parity case
        agg.f32x_fast_pv = True
        try:
            xs = sample(run())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 2 * 1e3
        finally:
            agg.f32x_fast_pv = False
        entry["f32x_fast_pv"] = {"max_rel_vs_f32_mode": [float("%.3e" % float((a - b).double().abs().max() / b.abs().max())) for a, b in zip(xs, ref)],
                                 "frames_per_s": round(S / ms * 1e3, 3), "ms_per_step": round(ms, 3),
                                 "what": "opt-in: split-f16 attention with two of the three PV products (P_hi V_lo + P_hi V_hi); outside the mode's 1e-4 contract"}
        out["S%d" % S] = entry
        del inp
        torch.cuda.empty_cache()
    agg.set_compute_dtype(dt16)
    return out


def _cpu_block_runners(sd):
    """(kind, {name: callable(x, pos) -> tensor}) for one frame / global / DINOv2 block on the host: kind "port", the oracle
    restatement of the upstream modules (bit-exact against them, tests/golden/oracle_vs_reference_report.json)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import aggregator_oracle as orc
    rope = orc.rope_tables(38)
    return "port", {"frame": lambda x, pos: orc.block(x, sd, "aggregator.frame_blocks.0", pos, rope, True),
                    "global": lambda x, pos: orc.block(x, sd, "aggregator.global_blocks.0", pos, rope, True),
                    "dino": lambda x, pos: orc.block(x, sd, "aggregator.patch_embed.blocks.0", None, None, False, eps=orc.DINO_LN_EPS)}


def cpu_baseline(sd):
    """The reference CPU path (the bit-exact oracle restatement of its modules) on the
    host cores, one warm-up + one timed run of each piece:
    (1) headline config: ONE frame block, ONE global block and ONE DINOv2 block at the real 64-view shapes
        ((64,1374,1024) / (1,87936,1024)), extrapolated x24 each ("time ONE frame block + ONE global block
        ... and extrapolate x24 (state that it is extrapolated)"); patch embed / token assembly are < 1 % and left out.
        The warm-up of the global block runs on an eighth of the sequence (its cost is quadratic: a full-size warm-up would
        double the 25 s this leg takes) -- it warms the thread pool, the allocator and the GEMM / SDPA primitives.
    (2) a COMPLETE 24-layer aggregator forward on 2 views (nothing extrapolated; the blocks above are its warm-up)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import aggregator_oracle as orc
    ncpu = os.cpu_count() or 1
    cores = min(ncpu, 64)         # measured on the 256-core GPU host: 256 intra-op threads are slower than 64
    torch.set_num_threads(cores)
    kind, run = _cpu_block_runners(sd)
    S, P = 64, P_TOK
    g = torch.Generator().manual_seed(0)
    x = torch.randn(S, P, 1024, generator=g)
    pos_yx = torch.cartesian_prod(torch.arange(37), torch.arange(37)) + 1
    pos = torch.cat([torch.zeros(5, 2, dtype=pos_yx.dtype), pos_yx]).unsqueeze(0).expand(S, -1, -1).contiguous()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    with torch.no_grad():
        run["frame"](x[:8], pos[:8])                                                   # warm-ups (untimed)
        run["dino"](x[:8], None)
        run["global"](x[:8].reshape(1, 8 * P, 1024), pos[:8].reshape(1, 8 * P, 2))
        t_frame = timed(lambda: run["frame"](x, pos))
        t_dino = timed(lambda: run["dino"](x, None))
        t_global = timed(lambda: run["global"](x.reshape(1, S * P, 1024), pos.reshape(1, S * P, 2)))
        total = 24 * (t_frame + t_global + t_dino)
        inp = orc.synthetic_inputs(2)
        t2 = timed(lambda: orc.aggregator_forward(sd, inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], [], []))
    what = "oracle restatement of the reference (bit-exact against it)"
    return {"value": round(S / total, 5), "unit": "frames/s", "cores": cores, "host_cores": ncpu, "kind": kind, "extrapolated": True, "warmup": 1,
            "sample": "%s, fp32, torch CPU, %d threads of %d host cores, at the headline shapes (64 views 518^2), after one warm-up: one frame block "
                      "%.2f s, one global block %.2f s, one DINOv2 block %.2f s, extrapolated x24 each = %.0f s per forward"
                      % (what, cores, ncpu, t_frame, t_global, t_dino, total),
            "full_forward_2_views": {"value": round(2 / t2, 4), "unit": "frames/s", "seconds": round(t2, 2), "kind": "port",
                                     "sample": "complete oracle aggregator forward, 2 views 518^2 images-only, 1 timed run after the block warm-ups (not extrapolated)"}}


if __name__ == "__main__":
    main()
