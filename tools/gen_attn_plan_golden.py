"""Record ovg_attn_plan over a grid of shapes and knobs -> tests/golden/attn_plan_sweep.npz (tests/test_attn_plan_host.py compares the
current library with it row by row).

The committed file was recorded from the PARENT of the commit "Attention launch plan: named kernels, one function per rule" -- the
150-line plan16() -- so that the rewrite of the plan could be held to it decision for decision. It is a record of behaviour, not of an
implementation: a regeneration that changes the file IS a behaviour change of the launch plan (a threshold, a cost-model constant, a
workspace size) and belongs in a commit that says so and shows the measurement behind it.

Run without a visible GPU (the plan then assumes 256 CUs, as the CPU tests do):  python tools/gen_attn_plan_golden.py

Grid: dtype bf16 / f16; BH 16, 32, 48, 128, 1024; nq = S * 1374 for S in 1..72 and the tile edges 1, 63, 64, 65,
127, 128, 129, 4095, 4096, 4097, 8192; keys [nq], [nq] * 8 and the ragged [nq, 1, 65]; every shipped variant, the plan knobs 71-74 and one
retired number; kv_splits 0, 1, 2, 5, 8 (1 = the plan of a launch without a workspace); cus 0, 224, 64, 999; nq_pad = nq padded to 64 and
a larger buffer. Unknown variant numbers are not recorded: ovg_flash_attn refuses them, and the plan's answer for them is unspecified.
Dense: every S x variant x kv_splits x cus at BH = 16 (bf16, one key segment, default nq_pad; f16 with cus 0 / 64). The rest of the
product is sampled with a fixed seed."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "attn_plan_sweep.npz")

P = 1374
DTYPES = (0, 1)                                                    # OVG_BF16, OVG_F16
BHS = (16, 32, 48, 128, 1024)
NQS = tuple(S * P for S in range(1, 73)) + (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8192)
KEYS = (0, 1, 2)                                                   # [nq], [nq] * 8, [nq, 1, 65]
VARIANTS = (0, 1, 50, 52, 53, 54, 55, 57, 71, 72, 73, 74, 51)      # 51: retired
KV_SPLITS = (0, 1, 2, 5, 8)
CUS = (0, 224, 64, 999)
NQ_PADS = (0, 1)                                                   # nq padded to 64; that + 192 rows
INPUTS = ("dtype", "BH", "nq", "keys", "variant", "kv_splits", "cus", "nq_pad")
OUTPUTS = ("rc", "splits", "q_tile", "part_bytes", "lse_bytes", "main_rows", "tail_q_tile")
SAMPLED = 30000


def key_counts(kind, nq):
    return ([nq], [nq] * 8, [nq, 1, 65])[kind]


def nq_pad_of(kind, nq):
    return (nq + 63) // 64 * 64 + 192 * kind


def grid():
    """-> int64 [rows, len(INPUTS)]: the dense blocks, then the seeded sample of the whole product (duplicates of a dense row dropped)."""
    S72 = NQS[:72]
    dense = list(itertools.product((0,), (16,), S72, (0,), VARIANTS, KV_SPLITS, CUS, (0,)))
    dense += list(itertools.product((1,), (16,), S72, (0,), VARIANTS, KV_SPLITS, (0, 64), (0,)))
    axes = (DTYPES, BHS, NQS, KEYS, VARIANTS, KV_SPLITS, CUS, NQ_PADS)
    total = int(np.prod([len(a) for a in axes]))
    picks = np.sort(np.random.default_rng(20261018).choice(total, SAMPLED, replace=False))
    seen, rows = set(dense), list(dense)
    for flat in picks:
        idx = np.unravel_index(int(flat), [len(a) for a in axes])
        row = tuple(a[i] for a, i in zip(axes, idx))
        if row not in seen:
            seen.add(row)
            rows.append(row)
    return np.asarray(rows, dtype=np.int64)


def query(inputs):
    """ovg_attn_plan of the loaded library for every row of `inputs` -> int64 [rows, len(OUTPUTS)] (the output fields of a refused row
    are recorded as the call left them: zeroed here before the call)."""
    from omnivggt_official_amd import lib as L
    fn = L.load().ovg_attn_plan
    got = np.zeros((len(inputs), len(OUTPUTS)), dtype=np.int64)
    for r, (dtype, BH, nq, keys, variant, kv_splits, cus, pad) in enumerate(inputs.tolist()):
        p, out = L.AttnParams(), L.AttnPlanOut()
        nks = key_counts(keys, nq)
        p.nq, p.nq_pad, p.BH, p.nseg = nq, nq_pad_of(pad, nq), BH, len(nks)
        for i, nk in enumerate(nks):
            p.seg[i].nk = nk
        p.dtype, p.variant, p.kv_splits, p.cus = dtype, variant, kv_splits, cus
        rc = fn(C.byref(p), C.byref(out))
        got[r] = (rc, out.splits, out.q_tile, out.part_bytes, out.lse_bytes, out.main_rows, out.tail_q_tile)
    return got


def main():
    inputs = grid()
    got = query(inputs)
    small = lambda a: a.astype(np.int32) if np.abs(a).max() < 2 ** 31 else a
    cols = {n: small(inputs[:, i]) for i, n in enumerate(INPUTS)}
    cols.update({n: small(got[:, i]) for i, n in enumerate(OUTPUTS)})
    np.savez_compressed(OUT, **cols)
    print("%s: %d rows, %d bytes; rc counts %s; %d rows with a split workspace, %d with a tail" % (
        OUT, len(inputs), os.path.getsize(OUT), dict(zip(*np.unique(got[:, 0], return_counts=True))),
        int((got[:, 3] > 0).sum()), int((got[:, 5] < inputs[:, 2]).sum())))


if __name__ == "__main__":
    main()
