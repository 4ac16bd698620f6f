"""Write tests/golden/pointcloud.npz from the REAL reference point-cloud export (visual_util.predictions_to_glb, :77-267).

    python tools/gen_golden_pointcloud.py

Runs only where the reference tree exists (oracle/ref_shim.py, read-only). The modules the export imports but this selection never
needs (trimesh, cv2, onnxruntime, viser, imageio, and torchvision where it is absent) are stubs that RECORD what the reference hands them: the trimesh.PointCloud vertices /
colours, the matrix given to Scene.apply_transform, and the scene_scale passed to integrate_camera_into_scene (show_cam=True). The
reference's own np.percentile calls are observed through a forwarding proxy of its `np` module, which records the confidence threshold.
Each case runs twice: once on its real points and once with world points that encode the flat pixel index (exact in f32 below 2^24),
which pins the selection ORDER, not just the set. The sky-mask case goes through the reference's mask_sky branch with a throw-away
target_dir whose mask files the cv2 stub serves from memory.
"""
import json
import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
import pointcloud_twin as twin  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pointcloud.npz")
REC = {}
SKY = {}


def _stub_modules():
    tm = types.ModuleType("trimesh")

    class Scene:
        def add_geometry(self, g):
            pass

        def apply_transform(self, m):
            REC["transform"] = np.array(m, dtype=np.float64)

    class PointCloud:
        def __init__(self, vertices=None, colors=None):
            REC["vertices"], REC["colors"] = np.asarray(vertices), np.asarray(colors)

    tm.Scene, tm.PointCloud, tm.Trimesh = Scene, PointCloud, mock.MagicMock(name="trimesh.Trimesh")
    tm.creation = mock.MagicMock(name="trimesh.creation")
    sys.modules["trimesh"] = tm
    cv2 = mock.MagicMock(name="cv2")
    cv2.imread = lambda path, flag=None: SKY[os.path.basename(path)]
    cv2.resize = mock.Mock(side_effect=AssertionError("sky masks are stored at the map size"))
    sys.modules["cv2"] = cv2
    # requests: the reference's mask_sky branch downloads its ONNX model when the file is missing; nothing here may reach a network
    for name in ("onnxruntime", "viser", "viser.transforms", "imageio", "requests", "torchvision", "torchvision.transforms"):
        if name.startswith("torchvision") and name in sys.modules:
            continue
        sys.modules[name] = mock.MagicMock(name=name)


class _RecordingNumpy(types.ModuleType):
    """Forwards every attribute to numpy; np.percentile calls are recorded (the first one of a run is the confidence threshold)."""
    def __init__(self):
        super().__init__("numpy")

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def percentile(a, q, *args, **kw):
        r = np.percentile(a, q, *args, **kw)
        REC.setdefault("percentiles", []).append((q, kw.get("axis"), np.array(r)))
        return r


def _maps(rng, S, H, W, conf_kind="smooth"):
    conf = (1.0 + 19.0 * rng.random((S, H, W))).astype(np.float32)
    if conf_kind == "ties":
        conf = np.float32(1.0) + np.floor(conf / np.float32(5.0))          # 4 levels
    pts = (rng.standard_normal((S, H, W, 3)) * np.array([2.0, 1.0, 3.0]) + np.array([0.0, 0.0, 5.0])).astype(np.float32)
    img = rng.random((S, 3, H, W)).astype(np.float32)
    return conf, pts, img


def _extrinsics(rng, S):
    from scipy.spatial.transform import Rotation
    e = np.zeros((S, 3, 4), np.float32)
    e[:, :, :3] = Rotation.from_rotvec(rng.standard_normal((S, 3)) * 0.3).as_matrix()
    e[:, :, 3] = rng.standard_normal((S, 3))
    return e


def _boundary_images(rng, S, H, W):
    """Channel values whose f32 x * 255 lands one ulp either side of the black (sum 16) and white (240) boundaries."""
    cands = []
    for k in (0, 5, 6, 10, 240, 241, 255):
        x = np.float32(k) / np.float32(255)
        for v in (np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))):
            cands.append(np.float32(min(max(v, 0), 1)))
    cands = np.array(cands, np.float32)
    img = cands[rng.integers(0, len(cands), (S, 3, H, W))]
    white = rng.random((S, H, W)) < 0.25                                   # whole-white / near-white pixels
    img[:, :, :][np.broadcast_to(white[:, None], img.shape)] = cands[rng.integers(12, len(cands), int(white.sum()) * 3)]
    return img


def _run(vu, pred, opts, mode):
    REC.clear()
    kw = dict(conf_thres=opts["conf_thres"], filter_by_frames=opts["filter_by_frames"], mask_black_bg=opts["mask_black_bg"],
              mask_white_bg=opts["mask_white_bg"], show_cam=True, prediction_mode=mode)
    scales = []
    with mock.patch.object(vu, "integrate_camera_into_scene", lambda scene, tf, col, scale: scales.append(scale)), \
            mock.patch.object(vu, "np", _RecordingNumpy()), \
            mock.patch.object(vu, "download_file_from_url", mock.Mock(side_effect=AssertionError("no downloads"))), \
            mock.patch.object(vu.os.path, "exists", lambda path, _e=os.path.exists: path == "skyseg.onnx" or _e(path)):
        if opts.get("sky"):
            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, "images"))
                for i in range(len(pred["images"])):
                    open(os.path.join(d, "images", "%03d.png" % i), "w").close()
                    SKY["%03d.png" % i] = opts["sky"][i]
                os.makedirs(os.path.join(d, "sky_masks"))
                for name in SKY:
                    open(os.path.join(d, "sky_masks", name), "w").close()
                vu.predictions_to_glb(dict(pred), mask_sky=True, target_dir=d, **kw)
        else:
            vu.predictions_to_glb(dict(pred), **kw)
    rec = dict(REC)
    rec["scene_scale"] = scales[0]
    return rec


def main():
    _stub_modules()
    ref_shim.install()
    import visual_util as vu
    rng = np.random.default_rng(20261015)
    cases, arrays = [], {}
    base = dict(conf_thres=50.0, filter_by_frames="all", mask_black_bg=False, mask_white_bg=False)

    def add(name, pred, mode="Predicted Pointmap", **opts):
        o = dict(base, **opts)
        o["sky"] = None
        sky = opts.get("sky")
        key_pts, key_conf = ("world_points", "world_points_conf") if "Pointmap" in mode and "world_points" in pred else \
            ("world_points_from_depth", "depth_conf")
        S, H, W = pred[key_conf].shape
        ref = _run(vu, pred, dict(o, sky=None if sky is None else list(sky)), mode)
        enc = dict(pred)
        flat = np.arange(S * H * W, dtype=np.float32)
        enc[key_pts] = np.repeat(flat[:, None], 3, axis=1).reshape(S, H, W, 3)
        ref_idx = _run(vu, enc, dict(o, sky=None if sky is None else list(sky)), mode)
        empty = np.issubdtype(ref["vertices"].dtype, np.integer)          # the reference's (1, 0, 0) stand-in for an empty cloud
        idx = np.zeros(0, np.int64) if empty else ref_idx["vertices"][:, 0].astype(np.int64)
        thr = [r for q, ax, r in ref["percentiles"] if ax is None]
        tw = twin.select(pred[key_pts], pred[key_conf], pred["images"], pred["extrinsic"], conf_thres=o["conf_thres"],
                         frame=twin.parse_frame(o["filter_by_frames"]), mask_black_bg=o["mask_black_bg"], mask_white_bg=o["mask_white_bg"],
                         sky_mask=sky)
        # the twin must reproduce the reference bit for bit before anything is written
        assert np.array_equal(tw["indices"], idx), name
        if not empty:
            pts = np.asarray(pred[key_pts]).reshape(-1, 3)
            assert ref["vertices"].dtype == pts.dtype and np.array_equal(ref["vertices"], pts[idx]), name
            assert np.array_equal(ref["colors"], tw["colors"]), name
            assert np.asarray(ref["scene_scale"]).dtype == tw["scene_scale"].dtype, name
            assert np.array_equal(np.asarray(ref["scene_scale"]), tw["scene_scale"]), (name, ref["scene_scale"], tw["scene_scale"])
        else:
            assert ref["scene_scale"] == 1 and tw["points"].shape[0] == 0, name
        if thr:
            assert thr[0].dtype == np.float32 and np.array_equal(thr[0], tw["conf_threshold"], equal_nan=True), name
        assert np.abs(ref["transform"] - tw["transform"]).max() <= 1e-12, name
        p = "c%d_" % len(cases)
        arrays[p + "indices"] = idx.astype(np.int32)
        arrays[p + "colors"] = np.zeros((0, 3), np.uint8) if empty else ref["colors"].astype(np.uint8)
        arrays[p + "threshold"] = np.array(thr[0] if thr else np.float32(0.0), np.float32)
        arrays[p + "scene_scale"] = np.array(ref["scene_scale"])
        arrays[p + "transform"] = ref["transform"]
        if sky is not None:
            arrays[p + "sky"] = np.asarray(sky)
        cases.append({"name": name, "map": pred["_map"], "mode": mode, "empty": bool(empty), "n_kept": int(idx.size),
                      **{k: o[k] for k in base}})

    def register(mapname, pred):
        for k, v in pred.items():
            if isinstance(v, np.ndarray):
                arrays["%s_%s" % (mapname, k)] = v
        pred["_map"] = mapname
        return pred

    def pointmap(mapname, S, H, W, conf=None, img=None, kind="smooth"):
        c, pts, im = _maps(rng, S, H, W, kind)
        pred = {"world_points": pts, "world_points_conf": c if conf is None else conf, "images": im if img is None else img,
                "extrinsic": _extrinsics(rng, S)}
        return register(mapname, pred)

    m = pointmap("smooth", 3, 28, 42)
    for t in (0.0, 10.0, 25.0, 37.3, 50.0, 100.0, None):
        add("conf_thres=%s" % t, m, conf_thres=t)
    add("frame 1", m, filter_by_frames="1: 001.png")
    add("frame unparsable", m, filter_by_frames="x: y")
    m = pointmap("ties", 2, 28, 56, kind="ties")
    for t in (25.0, 50.0, 75.0):
        add("ties %s" % t, m, conf_thres=t)
    c = np.where(rng.random((2, 28, 42)) < 0.5, np.float32(1e-5), np.float32(2.0)).astype(np.float32)
    c[rng.random(c.shape) < 0.2] = np.nextafter(np.float32(1e-5), np.float32(1))
    c[rng.random(c.shape) < 0.2] = np.nextafter(np.float32(1e-5), np.float32(0))
    c[rng.random(c.shape) < 0.05] = 0
    m = pointmap("min_conf", 2, 28, 42, conf=c)
    for t in (0.0, 10.0, 60.0):
        add("min_conf %s" % t, m, conf_thres=t)
    c = (1.0 + rng.random((2, 28, 42))).astype(np.float32)
    c[rng.random(c.shape) < 0.3] = np.inf
    m = pointmap("inf30", 2, 28, 42, conf=c)
    for t in (50.0, 69.0, 75.0, 100.0):                                   # 75 / 100: both order statistics inf
        add("inf %s" % t, m, conf_thres=t)
    c = (1.0 + rng.random((2, 28, 42))).astype(np.float32)
    c[0, 3, 5] = np.nan
    m = pointmap("nan", 2, 28, 42, conf=c)
    for t in (0.0, 50.0):
        add("nan %s" % t, m, conf_thres=t)
    img = _boundary_images(rng, 2, 28, 42)
    m = pointmap("colours", 2, 28, 42, img=img)
    add("black bg", m, conf_thres=0.0, mask_black_bg=True)
    add("white bg", m, conf_thres=0.0, mask_white_bg=True)
    add("both bg 30", m, conf_thres=30.0, mask_black_bg=True, mask_white_bg=True)
    m = pointmap("sky", 2, 28, 42)
    sky = rng.choice(np.array([0, 1, 255], np.uint8), (2, 28, 42), p=[0.3, 0.2, 0.5])
    add("sky 50", m, conf_thres=50.0, sky=sky)
    add("sky 0 frame 1", m, conf_thres=0.0, sky=sky, filter_by_frames="1")

    # "Predicted Depth": pose encodings + depth through the reference's own get_world_points_from_depth
    S, H, W = 3, 28, 42
    enc = torch.zeros(1, S, 9)
    enc[..., :3] = torch.from_numpy(rng.standard_normal((1, S, 3)).astype(np.float32)) * 0.5
    q = torch.from_numpy(rng.standard_normal((1, S, 4)).astype(np.float32))
    enc[..., 3:7] = q / q.norm(dim=-1, keepdim=True)
    enc[..., 7:] = torch.from_numpy((0.7 + 0.5 * rng.random((1, S, 2))).astype(np.float32))
    depth = torch.from_numpy((1.0 + 4.0 * rng.random((1, S, H, W, 1))).astype(np.float32))
    dconf = torch.from_numpy((1.0 + 9.0 * rng.random((1, S, H, W))).astype(np.float32))
    images = torch.from_numpy(rng.random((1, S, 3, H, W)).astype(np.float32))
    pred = {"pose_enc": enc, "depth": depth, "depth_conf": dconf, "images": images}
    vu.get_world_points_from_depth(pred)                                   # numpy from here on, batch squeezed, f64 world points
    pred = register("depthmode", {k: pred[k] for k in ("pose_enc", "depth", "depth_conf", "images", "extrinsic", "world_points_from_depth")})
    for t in (0.0, 50.0):
        add("depth %s" % t, pred, mode="Predicted Depth", conf_thres=t)
    add("depth frame 2", pred, mode="Predicted Depth", conf_thres=25.0, filter_by_frames="2: c.png")

    arrays["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(OUT, **arrays)
    print("%d cases; twin == reference on every one; wrote %s (%d bytes)" % (len(cases), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
