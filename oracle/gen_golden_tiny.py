"""Reference fixtures for the smallest and longest patch grids (build container only; sibling of gen_golden.py and
gen_golden_bf16twin.py, same seeded synthetic weights and inputs, same REAL reference through oracle/ref_shim.py).

For every case of TINY_CASES (the twin of tests/common.py::TINY_CASES; a host test holds the two tables equal):

  * run the reference and the oracle restatement in f32, assert they agree below 2e-5 on all 24 token layers and the
    predictions, and store tests/golden/<name>.npz;
  * run the reference under `torch.autocast('cpu', dtype=torch.bfloat16)` and store <name>_bf16twin.npz -- except on
    the one-column case, where the CPU autocast reference itself is not finite -- asserting that every stored twin
    tensor is finite and within 5e-2 (max-rel) of the f32 run;
  * write tests/golden/oracle_vs_reference_tiny.json, and the twin's own errors into bf16twin_report.json under the
    new names (the entries of the 518-class cases are left as they are).

Unlike the 518-class goldens these keep ALL token rows (every 8th channel) of TOK_LAYERS and the four dense maps
WHOLE: a ::37 stride would leave one pixel of a 14-pixel side.  One exception keeps every file under the 1 MiB limit
of a committed file: along a side longer than the trained 518 px (the 1778-px case) the maps keep every 4th pixel and
the last one, and the tokens every 32nd channel -- still all 132 rows, the last RoPE position among them.  Neither
report records wall times and the archives carry no time stamps, so a second run on the same torch build reproduces
every file byte for byte.

    python oracle/gen_golden_tiny.py [case ...]          # all five: under a minute on 8 cores
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import aggregator_oracle as orc  # noqa: E402
import gen_golden as gg  # noqa: E402
import gen_golden_bf16twin as twin  # noqa: E402
import ref_shim  # noqa: E402
from omnivggt_official_amd import weights  # noqa: E402

TINY_CASES = {
    # name: (S, depth_gt_index, camera_gt_index, (H, W))
    "t1_14x14": (1, [], [], (14, 14)),                  # one patch, 6 tokens, one view
    "t2_14x14_aux": (2, [1], [0], (14, 14)),
    "t3_28x42_aux": (3, [1], [0, 2], (28, 42)),         # 2 x 3 patches
    "t2_70x14_cam": (2, [], [0, 1], (70, 14)),          # one column; no twin
    "t2_14x1778_aux": (2, [1], [0], (14, 1778)),        # one row of 127 patches: the last RoPE position
}
NO_TWIN = ("t2_70x14_cam",)
DENSE = ("depth", "depth_conf", "world_points", "world_points_conf")
REPORT = "oracle_vs_reference_tiny.json"


def thin(n):
    """Pixel indices kept along one image side: all of them up to the trained 518, every 4th and the last beyond."""
    return list(range(n)) if n <= 518 else sorted(set(range(0, n, 4)) | {n - 1})


def chan_step(hw):
    """Token channels are stored every 8th; every 32nd where a side is longer than the trained 518 px."""
    return 8 if max(hw) <= 518 else 32


def sample(toks, pred, hw, with_list):
    """ALL token rows of TOK_LAYERS, every chan_step-th channel; pose_enc(_list); the four dense maps on thin(H) x thin(W)
    (whole up to 518 px per side).  Also what the tests apply to a device result before they compare it with a fixture."""
    rows, cols = torch.tensor(thin(hw[0])), torch.tensor(thin(hw[1]))
    g = {"tok_L%d" % l: toks[l][0][..., ::chan_step(hw)].float().contiguous().numpy() for l in gg.TOK_LAYERS}
    g["pose_enc"] = pred["pose_enc"].float().numpy()
    if with_list:
        g["pose_enc_list"] = torch.stack([p.float() for p in pred["pose_enc_list"]]).numpy()
    for k in DENSE:
        m = pred[k][0, ..., 0] if k == "depth" else pred[k][0]                 # [S, H, W(, 3)]
        g[k] = m.float().index_select(1, rows).index_select(2, cols).contiguous().numpy()
    return g


def save_npz(path, arrays):
    """np.savez_compressed with the archive's time stamps pinned, so that a regeneration gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def run_reference(model, inp, dgi, cgi, autocast):
    captured = {}

    def hook(mod, args, out):
        captured["toks"] = [t.float() for t in out[0]]
    h = model.aggregator.register_forward_hook(hook)
    try:
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            pred = model(inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"], list(dgi), list(cgi))
    finally:
        h.remove()
    return captured["toks"], pred


def main():
    torch.set_num_threads(os.cpu_count())
    manifest = json.load(open(os.path.join(gg.GOLD, "state_dict_manifest.json")))
    sd = weights.synthetic_state_dict(manifest, seed=2)
    model = ref_shim.build_reference_model()
    model.load_state_dict(sd, strict=True)
    only = sys.argv[1:]
    rep_path, twin_path = os.path.join(gg.GOLD, REPORT), os.path.join(gg.GOLD, "bf16twin_report.json")
    report = json.load(open(rep_path)) if (only and os.path.exists(rep_path)) else {}
    twin_report = json.load(open(twin_path))
    for name, (S, dgi, cgi, hw) in TINY_CASES.items():
        if only and name not in only:
            continue
        inp = orc.synthetic_inputs(S, hw=hw)
        toks, ref = run_reference(model, inp, dgi, cgi, autocast=False)
        with torch.no_grad():
            mine = orc.model_forward(sd, inp["images"], inp["extrinsics"], inp["intrinsics"], inp["depth"], inp["mask"],
                                     list(dgi), list(cgi))
        errs = {"tokens_L%d" % l: gg.rel_err(mine["_tokens"][l], toks[l]) for l in range(24)}
        for k in ("pose_enc",) + DENSE:
            errs[k] = gg.rel_err(mine[k], ref[k])
        worst = max(errs.values())
        print("%s: worst rel err oracle-vs-reference %.3e" % (name, worst), flush=True)
        assert worst < 2e-5, errs
        report[name] = {"oracle_vs_reference_max_rel": errs}
        gold = sample(toks, ref, hw, with_list=True)
        gold["tok_absmean"] = np.array([float(toks[l].abs().mean()) for l in range(24)], dtype=np.float64)
        save_npz(os.path.join(gg.GOLD, name + ".npz"), gold)
        if name in NO_TWIN:
            continue
        ttoks, tref = run_reference(model, inp, dgi, cgi, autocast=True)
        tw = sample(ttoks, tref, hw, with_list=False)
        errs = {k: {"max_rel": twin.max_rel(tw[k], gold[k]), "rms_rel": twin.rms_rel(tw[k], gold[k])} for k in tw}
        print(name, "twin", {k: "%.2e" % v["max_rel"] for k, v in errs.items()}, flush=True)
        for k, v in tw.items():
            assert np.isfinite(v).all(), (name, k)
            assert errs[k]["max_rel"] < 5e-2, (name, k, errs[k])
        save_npz(os.path.join(gg.GOLD, name + "_bf16twin.npz"), tw)
        twin_report[name] = {"twin_vs_f32_reference": errs, "torch": torch.__version__}
    json.dump(report, open(rep_path, "w"), indent=1)
    json.dump(twin_report, open(twin_path, "w"), indent=1)
    print("done")


if __name__ == "__main__":
    main()
