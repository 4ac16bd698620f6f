"""ovg_attn_plan against the recorded sweep tests/golden/attn_plan_sweep.npz (tools/gen_attn_plan_golden.py: 57 426 calls over dtype x BH x
nq x key segments x variant x kv_splits x cus x nq_pad, recorded before the launch plan was rewritten into one function per rule): the
return code and all six output fields of every row are equal. Host only: the plan assumes 256 CUs where no device is visible, and cus = 999
(more than any device has) falls back to that count, so the test pins itself to a run without a visible GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_attn_plan_golden as G  # noqa: E402


def test_attention_plan_sweep_equals_the_recorded_plans():
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.fail("the sweep was recorded for 256 CUs; run it on the CPU host or on a 256-CU device")
    z = np.load(G.OUT)
    inputs = np.stack([z[n].astype(np.int64) for n in G.INPUTS], axis=1)
    want = np.stack([z[n].astype(np.int64) for n in G.OUTPUTS], axis=1)
    assert len(inputs) >= 50000 and np.array_equal(inputs, G.grid()), "the committed sweep is not the generator's grid"
    # the axes' extremes and the dense block are all there
    for i, axis in enumerate((G.DTYPES, G.BHS, G.NQS, G.KEYS, G.VARIANTS, G.KV_SPLITS, G.CUS, G.NQ_PADS)):
        assert set(inputs[:, i].tolist()) == set(axis), G.INPUTS[i]
    dense = inputs[(inputs[:, 0] == 0) & (inputs[:, 1] == 16) & (inputs[:, 3] == 0) & (inputs[:, 7] == 0) & (inputs[:, 2] % G.P == 0)]
    assert len(np.unique(dense, axis=0)) >= 72 * len(G.VARIANTS) * len(G.KV_SPLITS) * len(G.CUS)
    got = G.query(inputs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d plans differ; first: %s -> %s, recorded %s" % (
        len(bad), len(inputs), dict(zip(G.INPUTS, inputs[bad[0]].tolist())), dict(zip(G.OUTPUTS, got[bad[0]].tolist())),
        dict(zip(G.OUTPUTS, want[bad[0]].tolist())))
