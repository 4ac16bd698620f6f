"""-m gpu: the layers above the C ABI on a caller's side stream (the sibling of test_gpu_stream_contract.py, same gated run).

The model forks three head streams from the caller's stream and joins them back, feeds aggregator layers to them while the trunk still
runs, and keeps workspaces across calls; the post-processing layer chains entries with torch operations and reads counts back. All of it
must follow the stream the CALLER made current -- not torch's default stream. These layers allocate and synchronise by design, so they
are exempt from `early` and from the allocation check; the check is bytes: behind the blocker on a side stream, on inputs that held decoys
until then, every result must equal the same call on the default stream.

 * OmniVGGT, the depth-2 reduced model, f32 and bf16, S = 2 and S = 3 with partial aux indices, concurrent heads and early DPT levels on:
   one gated forward; then two forwards with different inputs back to back on the side stream, no host synchronisation between them
   (the cached Aggregator workspaces, the EarlyLevels buffers and the shared head streams across calls)
 * predictions_to_point_cloud, voxel_downsample, fuse_predictions, render_mesh, icp, segment_plane, cluster_points: once each
 * two host threads, each with its own stream and buffers, run the GEMM, attention, convolution, dpt_tail, FPS and radius cases at the
   same time (ctypes releases the GIL), once: every result equals the single-thread bytes
"""
import threading

import numpy as np
import pytest
import torch

import aggregator_oracle as orc
import common
import stream_contract as sc
import test_gpu_stream_contract as tsc
from omnivggt_official_amd import lib as L, postprocess
from omnivggt_official_amd.model import OmniVGGT

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device fault is sticky: start nothing more on this GPU
        pytest.exit("the device reported %s; stopping the session" % e, returncode=3)
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# results -> bytes
# ---------------------------------------------------------------------------------------------
def flatten(x, path="result"):
    """Every tensor / array / number inside a result (dicts, lists, __slots__ objects) -> [(path, bytes-comparable value)]."""
    if x is None:
        return [(path, None)]
    if torch.is_tensor(x):
        t = x.detach().contiguous()
        return [(path, (str(t.dtype), tuple(t.shape), t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes()))]
    if isinstance(x, np.ndarray):
        return [(path, (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes()))]
    if isinstance(x, dict):
        return [kv for k in sorted(x) for kv in flatten(x[k], "%s[%r]" % (path, k))]
    if isinstance(x, (list, tuple)):
        return [kv for i, v in enumerate(x) for kv in flatten(v, "%s[%d]" % (path, i))]
    if hasattr(x, "__slots__"):
        return [kv for k in x.__slots__ for kv in flatten(getattr(x, k), "%s.%s" % (path, k))]
    return [(path, x)]


def differences(got, want):
    g, w = flatten(got), flatten(want)
    assert [p for p, _ in g] == [p for p, _ in w], ([p for p, _ in g], [p for p, _ in w])
    return [p for (p, a), (_, b) in zip(g, w) if a != b]


def gated_layer(name, run, live, real, decoy):
    """run(): the layer call on the tensors of `live` (a list), which `real` / `decoy` fill. Default stream: real -> want, decoy -> must
    differ. Then behind the blocker on the side stream: live <- real, run() -> must equal want in every byte. -> (want, decoy result)."""
    gate = sc.Gate.get()
    S = gate.require_stream()

    def load(src):
        for l, s in zip(live, src):
            l.copy_(s)
    load(real)
    run()                                               # warm-up: module loads, cached workspaces, the plans
    torch.cuda.synchronize()
    load(real)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    want = run()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    load(decoy)
    other = run()
    torch.cuda.synchronize()
    assert differences(other, want), "%s: the decoy inputs give the same bytes, the case cannot tell the two apart" % name
    scale = gate.scale_for(ms)
    with torch.cuda.stream(S):
        gate.block(scale)
        load(real)
        got = run()
    S.synchronize()
    torch.cuda.synchronize()
    bad = differences(got, want)
    print("[%s] gated %-52s default stream %.2f ms, blocker %.0f ms" % ("FAIL" if bad else "PASS", name, ms, scale * gate.block_ms), flush=True)
    assert not bad, "%s on a side stream differs from the default-stream call in %s" % (name, bad)
    return want, other


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        sd = common.reduced_state_dict(2, 2)
        with torch.device("meta"):
            m = OmniVGGT(depth=2, dino_depth=2, compute_dtype=dtype)
        m = m.to_empty(device="cpu")
        m.load_state_dict(sd, strict=True)
        _MODELS[dtype] = m.to(DEV).eval()
    return _MODELS[dtype]


KEYS = ("images", "extrinsics", "intrinsics", "depth", "mask")


@pytest.mark.parametrize("S,dgi,cgi", [(2, [1], []), (3, [1], [0, 2])])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_model_forward_on_a_side_stream_and_back_to_back(dtype, S, dgi, cgi):
    m = _model(dtype)
    assert m.concurrent_heads and m.early_dpt_levels
    a, b = orc.synthetic_inputs(S, seed=1234), orc.synthetic_inputs(S, seed=4321)
    real, decoy = [a[k].to(DEV) for k in KEYS], [b[k].to(DEV) for k in KEYS]
    live = [t.clone() for t in real]

    def forward(inputs):
        with torch.no_grad():
            out = m(*inputs, dgi, cgi)
        return {k: v for k, v in out.items() if k != "images"}
    want_a, want_b = gated_layer("OmniVGGT %s S=%d aux %s %s" % (dtype, S, dgi, cgi), lambda: forward(live), live, real, decoy)
    assert {"pose_enc", "depth", "depth_conf", "world_points", "world_points_conf"} <= set(want_a)

    # two forwards back to back on the side stream, nothing waits on the host in between
    gate = sc.Gate.get()
    Sd = gate.require_stream()
    other = [t.clone() for t in decoy]
    live_a = [t.clone() for t in decoy]                 # holds the wrong scene until the side stream gets there
    torch.cuda.synchronize()
    with torch.cuda.stream(Sd):
        gate.block()
        for l, s in zip(live_a, real):
            l.copy_(s)
        got_a = forward(live_a)
        got_b = forward(other)
    Sd.synchronize()
    torch.cuda.synchronize()
    bad_a, bad_b = differences(got_a, want_a), differences(got_b, want_b)
    assert not bad_a and not bad_b, "back to back on a side stream: first forward differs in %s, second in %s" % (bad_a, bad_b)


# ---------------------------------------------------------------------------------------------
# post-processing
# ---------------------------------------------------------------------------------------------
def _prediction_sets():
    import test_gpu_consistency as tc
    real, _ = tc._predictions(0)
    decoy = {k: v.clone() for k, v in real.items()}
    decoy["depth"] = decoy["depth"] * 1.03
    for k in ("world_points", "world_points_from_depth"):
        decoy[k] = decoy[k] * 1.03 + 0.01
    for k in ("depth_conf", "world_points_conf"):
        decoy[k] = decoy[k].flip(-1).contiguous()
    decoy["images"] = decoy["images"].flip(-1).contiguous()
    keys = sorted(real)
    return keys, [real[k].contiguous() for k in keys], [decoy[k].contiguous() for k in keys]


def test_postprocessing_pipeline_on_a_side_stream():
    keys, real, decoy = _prediction_sets()
    live = [t.clone() for t in real]
    pred = dict(zip(keys, live))

    def cloud_and_voxels():
        cloud = postprocess.predictions_to_point_cloud(pred, conf_thres=50.0, return_indices=True, return_conf=True)
        small = postprocess.voxel_downsample(cloud, rel_size=0.01, conf=cloud.conf)
        return cloud, small
    gated_layer("predictions_to_point_cloud -> voxel_downsample", cloud_and_voxels, live, real, decoy)

    def fuse_and_render():
        volume, mesh = postprocess.fuse_predictions(pred, resolution=48)
        H, W = pred["depth"].shape[2:4]
        img = postprocess.render_mesh(mesh, pred["extrinsic"][0], pred["intrinsic"][0], (H, W), return_index=True)
        return (volume.tsdf, volume.weight, volume.color), (mesh.vertices, mesh.faces, mesh.normals, mesh.colors), img
    gated_layer("fuse_predictions -> render_mesh", fuse_and_render, live, real, decoy)


def test_registration_planes_and_clusters_on_a_side_stream():
    g = torch.Generator().manual_seed(31)
    src = (torch.rand(3000, 3, generator=g) - 0.5)
    src[:1500, 1] = 0.2 + 0.004 * torch.randn(1500, generator=g)            # a slab: a plane to find, a dense cluster
    ang = 0.1
    R = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    tgt = src @ R.t() + torch.tensor([0.02, -0.01, 0.03])
    real = [src.to(DEV), tgt.to(DEV)]
    decoy = [(src.flip(0) * 0.9 + 0.05).to(DEV), (tgt.flip(0) * 1.1).to(DEV)]
    live = [t.clone() for t in real]

    gated_layer("icp exhaustive, 5 iterations", lambda: postprocess.icp(live[0], live[1], iterations=5), live, real, decoy)
    gated_layer("icp on the grid, gated at 0.2", lambda: postprocess.icp(live[0], live[1], iterations=3, search="grid", max_distance=0.2), live, real, decoy)
    gated_layer("segment_plane 256 hypotheses, 2 refits",
                lambda: postprocess.segment_plane(live[0], threshold=0.01, hypotheses=256, seed=3, refit=2, return_distance=True), live, real, decoy)
    gated_layer("cluster_points DBSCAN", lambda: postprocess.cluster_points(live[0], radius=0.06, min_neighbours=3), live, real, decoy)


# ---------------------------------------------------------------------------------------------
# two host threads, two streams
# ---------------------------------------------------------------------------------------------
def test_two_host_threads_on_their_own_streams_give_the_single_thread_bytes():
    builders = [tsc._linear_case(L.TILE_256, L.EPI_RES), tsc._attn_case("default plan bf16", torch.bfloat16, 65, [7, 129]),
                tsc._conv_case(128, 128, 64), tsc._dpt_tail_case(torch.bfloat16), tsc._fps_case(1, 500, 33), tsc._fps_case(2, 2500, 17),
                tsc._radius_case(False)]
    sets = [[sc.setup_case(b()) for b in builders] for _ in range(2)]       # each thread its own buffers; `want` from the default stream
    for cases in sets:
        for c in cases:
            c._load(c.real)
            c._refill()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    start = threading.Barrier(2)
    errors = [None, None]

    def worker(i):
        try:
            start.wait(timeout=30)
            with torch.cuda.stream(streams[i]):
                for c in sets[i]:
                    c.call()
            streams[i].synchronize()
        except Exception as e:                          # noqa: BLE001 -- reported by the main thread
            errors[i] = e
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    assert errors == [None, None], errors
    torch.cuda.synchronize()
    bad = []
    for i, cases in enumerate(sets):
        for c in cases:
            c._check_guards("thread %d" % i)
            if not all(torch.equal(g, w) for g, w in zip(c._bytes(), c.want)):
                bad.append("thread %d: %s" % (i, c.name))
    print("two threads x %d cases: %s" % (len(builders), "all equal the single-thread bytes" if not bad else bad), flush=True)
    assert not bad, bad
