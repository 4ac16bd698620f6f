"""tests/golden/fps_reference.npz from the REAL reference farthest_point_sample (reference tree only; no test runs this).

    python tools/gen_fps_golden.py /path/to/reference/checkout [--out tests/golden/fps_reference.npz]

Loads omnivggt/utils/po_utils/misc.py of the checkout (its `prettytable` import, which the sampler does not use, is stubbed), runs
farthest_point_sample(xyz, npoint, include_ends, deterministic=True) on torch CPU tensors for two seeded batches of three clouds each
(random, quarter-lattice with exact ties, duplicated points), asserts tests/fps_twin.py reproduces every index and writes the
inputs with the recorded indices: small_xyz [3, 300, 3] with npoint 300, large_xyz [3, 2000, 3] with npoint 500,
*_index / *_index_ends int16 (the reference's int64 values).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def batch(n, seed):
    rng = np.random.default_rng(seed)
    rand = rng.normal(0.0, 1.0, (n, 3)).astype(F)
    lattice = (rng.integers(-8, 9, (n, 3)) / 4.0).astype(F)
    dup = rng.normal(0.0, 1.0, (n, 3)).astype(F)
    dup[n // 3:] = dup[rng.integers(0, n // 3, n - n // 3)]                   # a third of the points are distinct
    return np.stack([rand, lattice, dup])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fps_reference.npz"))
    a = ap.parse_args()
    import torch
    import fps_twin as twin
    stub = types.ModuleType("prettytable")
    stub.PrettyTable = object
    sys.modules.setdefault("prettytable", stub)
    path = os.path.join(a.reference, "omnivggt", "utils", "po_utils", "misc.py")
    spec = importlib.util.spec_from_file_location("reference_po_misc", path)
    misc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(misc)
    out = {}
    for name, n, npoint, seed in (("small", 300, 300, 11), ("large", 2000, 500, 12)):
        xyz = batch(n, seed)
        out[name + "_xyz"], out[name + "_npoint"] = xyz, np.int32(npoint)
        for key, ends in (("_index", False), ("_index_ends", True)):
            idx = misc.farthest_point_sample(torch.from_numpy(xyz), npoint, include_ends=ends, deterministic=True).numpy()
            assert idx.dtype == np.int64 and idx.shape == (3, npoint) and idx.min() >= 0 and idx.max() < n
            mine = twin.sample(xyz, npoint, include_last=ends)[0]
            assert (mine == idx).all(), (name, key, int((mine != idx).sum()))
            out[name + key] = idx.astype(np.int16)
    np.savez_compressed(a.out, **out)
    print("%s: %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
