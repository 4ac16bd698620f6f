"""-m gpu: the result of a forward does not depend on what the process did before it.

The model is written for a long-lived process, and state survives a call: ZeroAggregator's LRU of workspaces (a new shape with
the same M shares xn / attn / hid with a live one; each keeps its own q / k / v^T and split-KV buffers), the per-geometry
pos tables, the bias-table and camera-index caches (flushed at 16 entries), the DPT heads' position tables and packs, the camera
head's workspace (dropped when its key changes), the process-wide head streams shared by all models, and set_compute_dtype ->
invalidate().  The only history test so far ran the same 518^2 shape twice.

The calls are the menu of small_grids.py (m1 .. m11: 14 x 14 ... 1778 x 14, three items with M = 66) plus m12, the trained 518^2
grid.  The RESULT of a call is every aggregator layer, every entry of pose_enc_list and the four dense maps, copied to the host and
compared BYTE FOR BYTE: the project claims run-to-run identical bytes, so identity is the assertion, not a tolerance.  X's m1 and
Y's m12 are first calls of fresh instances, and X's f32 / f32x results are what test_gpu_small_grids.py holds to the oracle (same
weights, same order), so a corruption cannot hide by being the same everywhere.

Depth-2 models take all four DPT levels from the last layer, so the early pyramid levels never start here (C2 d toggles the flag
all the same); test_gpu_aggregator.py checks them at these grids on the full-depth model."""
import itertools
import os
import random

import pytest
import torch

import common
import small_grids as sg
from omnivggt_official_amd import lib as L

pytestmark = pytest.mark.gpu
ITEMS = tuple(sg.MENU)                                               # m1 .. m12
OTHER = {"bf16": "f16", "f16": "bf16", "f32x": "f32", "f32": "f32x"}
TAGS = ["bf16", "f16", "f32x", "f32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    L.require_gpu()
    torch.set_num_threads(min(32, os.cpu_count()))


def z_order(seed=20):
    """Seeded shuffle of the menu, every item twice, no item next to itself."""
    rng = random.Random(seed)
    order = list(ITEMS) * 2
    while True:
        rng.shuffle(order)
        if all(a != b for a, b in zip(order, order[1:])):
            return order


def workspace_keys(items):
    """The distinct (M, seq) workspace shapes the items ask for: DINOv2 / frame (K * P, P) and global (K * P, S * P)."""
    keys = set()
    for it in items:
        B, S, hw, _, _ = sg.MENU[it]
        P = (hw[0] // 14) * (hw[1] // 14) + 5
        keys |= {(B * S * P, P), (B * S * P, S * P)}
    return keys


class History:
    """Three instances of one mode and what they returned: X ran m1 .. m12 and keeps every result on the host; Y (m12 .. m1) and Z
    (the shuffle, max_workspaces = 2) are compared with X call by call."""

    def __init__(self, sd, tag):
        self.tag = tag
        self.X, self.Y, self.Z = (sg.build(sd, sg.mode_dtype(tag)) for _ in range(3))
        self.Z.aggregator.max_workspaces = 2
        self.ref, self.diff, self.live = {}, [], {}
        for it in ITEMS:
            self.ref[it] = sg.to_host(sg.run_item(self.X, it))
        self.live["X"] = len(self.X.aggregator._ws)
        for name, m, order in (("Y", self.Y, ITEMS[::-1]), ("Z", self.Z, z_order())):
            for n, it in enumerate(order):
                bad = sg.same_bytes(sg.to_host(sg.run_item(m, it)), self.ref[it])
                if bad:
                    self.diff.append((name, n, it, bad))
            self.live[name] = len(m.aggregator._ws)

    def assert_reproduces(self, m, items, what):
        for it in items:
            bad = sg.same_bytes(sg.to_host(sg.run_item(m, it)), self.ref[it])
            assert bad == [], "%s: %s after %s differs from its first bytes in %s" % (self.tag, it, what, bad)


@pytest.fixture(scope="module")
def histories():
    sd = common.reduced_state_dict(2, 2)
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = History(sd, tag)
        return cache[tag]
    return get


# ---- C1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_three_instances_three_orders_same_bytes(histories, tag):
    h = histories(tag)
    order = z_order()
    assert sorted(order) == sorted(ITEMS * 2) and all(a != b for a, b in zip(order, order[1:]))
    assert h.diff == [], "(instance, call number, item, tensors that differ from X's): %s" % h.diff[:8]
    # evictions really happened: 19 distinct shapes were asked for, 4 (X, Y) / 2 (Z) are alive
    assert len(workspace_keys(ITEMS)) > 4
    assert h.live["X"] <= 4 and h.live["Y"] <= 4 and h.live["Z"] <= 2
    assert h.live["X"] == 4 and h.live["Z"] == 2
    for it in ITEMS:
        assert all(torch.isfinite(v).all() for v in h.ref[it].values()), it
    # m6 / m8 share M = 66 and nothing else: different calls, not one buffer read twice
    assert h.ref["m6"]["tok_L1"].shape != h.ref["m8"]["tok_L1"].shape


# ---- C2: events between two good calls, all on X; after each, m5 and m8 give their bytes again ---------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_refused_calls_between_good_calls(histories, tag):
    h = histories(tag)
    m = h.X
    ok = sg.device_inputs(1, 3, (28, 42))
    h.assert_reproduces(m, ("m5", "m8"), "nothing")
    with pytest.raises(AssertionError):                                   # height not a multiple of 14
        sg.forward(m, dict(ok, images=torch.zeros(1, 3, 3, 30, 42, device=sg.DEV)), [], [])
    h.assert_reproduces(m, ("m5", "m8"), "a refused 30-px height")
    for hw in ((14, 1792), (1792, 14)):                                   # a 1792-px side
        with pytest.raises(ValueError):
            sg.forward(m, sg.device_inputs(1, 2, hw), [], [])
    h.assert_reproduces(m, ("m5", "m8"), "a refused 1792-px side")
    # camera_gt_index out of range -- also when the same list was legal, and cached, for a call with more views
    four = sg.device_inputs(1, 4, (28, 42))
    sg.forward(m, four, [], [0, 3])
    for cgi in ([0, 3], [3], [0, -1]):
        with pytest.raises(IndexError):
            sg.forward(m, ok, [1], cgi)
    h.assert_reproduces(m, ("m5", "m8"), "a refused camera_gt_index")
    with pytest.raises(ValueError):                                       # depth_gt_index without depth
        with torch.no_grad():
            m(ok["images"], ok["extrinsics"], ok["intrinsics"], None, None, [1], [0])
    assert m.aggregator.layer_hook is None
    h.assert_reproduces(m, ("m5", "m8"), "a refused depth_gt_index without depth")


@pytest.mark.parametrize("tag", TAGS)
def test_compute_dtype_there_and_back(histories, tag):
    h = histories(tag)
    m = h.X
    other = histories(OTHER[tag])
    m.set_compute_dtype(sg.mode_dtype(OTHER[tag]))
    try:
        there = sg.to_host(sg.run_item(m, "m5"))
    finally:
        m.set_compute_dtype(sg.mode_dtype(tag))
    assert sg.same_bytes(there, other.ref["m5"]) == []                    # in the other mode it IS the other mode's model
    h.assert_reproduces(m, ("m5", "m8"), "set_compute_dtype there and back")


@pytest.mark.parametrize("tag", TAGS)
def test_kv_splits_off_and_back(histories, tag):
    h = histories(tag)
    m = h.X
    m.aggregator.attn_kv_splits = 1
    try:
        one = {it: sg.to_host(sg.run_item(m, it)) for it in ("m5", "m8", "m12")}
        again = {it: sg.to_host(sg.run_item(m, it)) for it in ("m5", "m8", "m12")}
    finally:
        m.aggregator.attn_kv_splits = 0
    for it in one:                                                        # 1 may differ from 0, but reproduces itself
        assert sg.same_bytes(one[it], again[it]) == [], it
    h.assert_reproduces(m, ("m5", "m8", "m12"), "attn_kv_splits = 1 and back to 0")


@pytest.mark.parametrize("tag", TAGS)
def test_head_scheduling_flags_do_not_change_bytes(histories, tag):
    h = histories(tag)
    m = h.X
    try:
        for early, conc in itertools.product((False, True), (False, True)):
            m.early_dpt_levels, m.concurrent_heads = early, conc
            h.assert_reproduces(m, ("m5", "m8"), "early_dpt_levels=%s concurrent_heads=%s" % (early, conc))
    finally:
        m.early_dpt_levels, m.concurrent_heads = True, True
    h.assert_reproduces(m, ("m5", "m8"), "the head flags back at their defaults")


@pytest.mark.parametrize("tag", TAGS)
def test_dpt_frames_chunk_does_not_change_bytes(histories, tag):
    """dpt_frames_chunk = 8: m6 is one pass of six views, nine views are two passes (8 + 1); 64 takes both in one."""
    h = histories(tag)
    m = h.X
    nine = sg.device_inputs(1, 9, (28, 42))
    whole = sg.to_host(sg.forward(m, nine, [1, 8], [0, 2]))
    m.dpt_frames_chunk = 8
    try:
        h.assert_reproduces(m, ("m6",), "dpt_frames_chunk = 8")
        assert sg.same_bytes(sg.to_host(sg.forward(m, nine, [1, 8], [0, 2])), whole) == []
    finally:
        m.dpt_frames_chunk = 64
    h.assert_reproduces(m, ("m5", "m8"), "dpt_frames_chunk = 8 and back to 64")


@pytest.mark.parametrize("tag", TAGS)
def test_camera_caches_past_their_flush(histories, tag):
    """17 view counts without cameras and 17 index lists at S = 4: both caches of camera_tables are flushed at 16 entries."""
    h = histories(tag)
    m = h.X
    pk = m.aggregator._packed
    for S in range(1, 18):
        sg.forward(m, sg.device_inputs(1, S, (14, 14)), [], [])
    lists = [list(c) for r in range(1, 5) for c in itertools.combinations(range(4), r)] + [[1, 0], [2, 0]]
    assert len({tuple(c) for c in lists}) == 17
    four = sg.device_inputs(1, 4, (28, 42))
    for cgi in lists:
        sg.forward(m, four, [], cgi)
    assert pk is m.aggregator._packed
    assert 0 < len([k for k in pk if isinstance(k, tuple) and k[0] == "bias_tables"]) <= 16
    assert 0 < len([k for k in pk if isinstance(k, tuple) and k[0] == "cam_index"]) <= 16
    h.assert_reproduces(m, ("m9", "m5", "m8"), "17 view counts and 17 camera index lists")


# ---- C3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_two_models_of_different_dtype_alternate(histories, tag):
    """Two live models share the process-wide head streams; they alternate call by call, nothing is synchronised in between."""
    a, b = histories(tag), histories(OTHER[tag])
    got = []
    for rnd in range(2):
        for it in ("m5", "m8", "m2"):
            got.append((a, it, sg.run_item(a.X, it)))
            got.append((b, it, sg.run_item(b.X, it)))
    torch.cuda.synchronize()
    for h, it, res in got:
        assert sg.same_bytes(sg.to_host(res), h.ref[it]) == [], (h.tag, it)


# ---- C4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_shuffled_order_on_a_side_stream_without_host_sync(histories, tag):
    h = histories(tag)
    order = z_order()
    for it in ITEMS:
        sg.device_inputs(*sg.MENU[it][:3])                                 # the inputs exist before the side stream starts
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = [(it, sg.run_item(h.Z, it)) for it in order]
    side.synchronize()
    assert torch.cuda.current_stream() != side
    for n, (it, res) in enumerate(got):
        assert sg.same_bytes(sg.to_host(res), h.ref[it]) == [], (n, it)
    assert len(h.Z.aggregator._ws) <= 2
