"""Device loaders on the MI355X (omnivggt_official_amd/preprocess.py, csrc/ovg_preprocess.hip): bit-identical to PIL's bicubic resize and
to the reference loaders as oracle/loader_oracle.py restates them, on generated files of every decode path, on the reference's own
example frames (some views of them in tests/golden/real/loader_originals.npz, written by tools/gen_loader_originals.py) and at the 64-view headline size."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import common
import loader_oracle as lo
import resample_twin as twin
from omnivggt_official_amd import preprocess

pytestmark = pytest.mark.gpu

REAL = os.path.join(common.GOLD, "real")


def pil_resize(a, size):
    return np.asarray(Image.fromarray(a, "RGB").resize(size, Image.Resampling.BICUBIC))


def test_resize_bicubic_equals_pil_in_one_call():
    frames = [twin.test_image(*src, seed=src[0] * 7 + src[1]) for src, _ in twin.GEOMETRIES]
    sizes = [size for _, size in twin.GEOMETRIES]
    got = preprocess.resize_bicubic(frames, sizes)
    for a, size, g in zip(frames, sizes, got):
        assert g.dtype == torch.uint8 and g.is_cuda
        assert np.array_equal(g.cpu().numpy(), pil_resize(a, size)), (a.shape, size)


def crop_reference(paths):
    """omnivggt/utils/load_fn.py mode="crop" with PIL + ToTensor: width 518, centre crop to 518, mixed heights padded white."""
    imgs = []
    for p in sorted(paths):
        img = lo.open_rgb(p)
        w, h = img.size
        nh = round(h * (518 / w) / 14) * 14
        t = lo.to_tensor(img.resize((518, nh), Image.Resampling.BICUBIC))
        if nh > 518:
            t = t[:, (nh - 518) // 2:(nh - 518) // 2 + 518, :]
        imgs.append(t)
    H = max(t.shape[1] for t in imgs)
    return torch.stack([torch.nn.functional.pad(t, (0, 0, (H - t.shape[1]) // 2, H - t.shape[1] - (H - t.shape[1]) // 2), value=1.0)
                        for t in imgs])


def _write_frames(folder, rng, specs):
    """specs: (name, (h, w), kind) with kind in rgb-png / rgb-jpg / rgba / L -> list of paths."""
    folder.mkdir(parents=True, exist_ok=True)
    paths = []
    for name, (h, w), kind in specs:
        a = twin.test_image(h, w, int(rng.integers(1 << 30)))
        p = folder / name
        if kind == "rgba":
            alpha = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
            alpha[h // 4:h // 2, w // 4:w // 2] = 0
            Image.fromarray(np.concatenate([a, alpha], -1), "RGBA").save(p)
        elif kind == "L":
            Image.fromarray(a[..., 0], "L").save(p)
        else:
            Image.fromarray(a, "RGB").save(p, **({"quality": 90} if kind == "rgb-jpg" else {}))
        paths.append(str(p))
    return paths


def test_load_and_preprocess_images_both_modes(tmp_path):
    rng = np.random.default_rng(3)
    same = _write_frames(tmp_path / "same", rng, [("b.png", (480, 640), "rgb-png"), ("a.jpg", (480, 640), "rgb-jpg"),
                                                  ("c.png", (480, 640), "rgba"), ("d.png", (480, 640), "L")])
    mixed = _write_frames(tmp_path / "mixed", rng, [("m0.jpg", (720, 1280), "rgb-jpg"), ("m1.png", (640, 480), "rgba"),
                                                    ("m2.png", (301, 517), "L"), ("m3.jpeg", (999, 333), "rgb-jpg"),
                                                    ("m4.png", (288, 512), "rgb-png")])
    for paths in (same, mixed):
        got = preprocess.load_and_preprocess_images(paths, mode="pad")
        assert got.is_cuda and got.shape == (len(paths), 3, 518, 518)
        assert torch.equal(got.cpu(), lo.load_and_preprocess_images_pad(paths))
        got = preprocess.load_and_preprocess_images(paths)
        want = crop_reference(paths)
        assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert preprocess.load_and_preprocess_images(mixed).shape == (5, 3, 518, 518)       # portraits set the height, the rest is white
    one = preprocess.load_and_preprocess_images(mixed[:1], mode="crop", workers=1)
    assert one.shape == (1, 3, 294, 518) and torch.equal(one.cpu(), crop_reference(mixed[:1]))


def _depth_map(rng, h, w):
    d = (0.5 + 60 * rng.random((h, w))).astype(np.float32)
    d[:5] = 1e10
    d[10:14, 10:20] = np.nan
    d[20:22] = np.inf
    d[23, :7] = -np.inf
    d[30:33, 5:40] = -1.0
    d[40:45, 40:45] = 150.0
    d[50, 50] = 100.0
    d[51, 51] = np.float32(1e-5)
    d[52, 52] = -0.0
    return d


def test_load_images_and_cameras_matches_the_oracle(tmp_path):
    rng = np.random.default_rng(9)
    cams = {}

    def scene(root, specs, depth_views, cam_views):
        _write_frames(root / "images", rng, specs)
        (root / "depths").mkdir()
        (root / "cameras").mkdir()
        (root / "images" / "readme.txt").write_text("not an image\n")
        for name, (h, w), _ in specs:
            stem = os.path.splitext(name)[0]
            if stem in depth_views:
                np.save(root / "depths" / (stem + ".npy"), _depth_map(rng, 97 + h // 3, 131 + w // 5))
            if stem in cam_views:
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                with open(root / "cameras" / (stem + ".txt"), "w") as fh:
                    fh.write("# c2w\n")
                    for row in np.concatenate([q, rng.normal(size=(3, 1))], 1):
                        fh.write(" ".join("%.9g" % v for v in row) + "\n\n")
                    f = 500 + 100 * rng.random()
                    fh.write("%r 0 %r\n0 %r %r\n0 0 1\n" % (f, w / 2 + 0.3, f, h / 2 - 0.7))
                cams[stem] = True

    land, port = tmp_path / "land", tmp_path / "port"
    scene(land, [("v0.jpg", (480, 640), "rgb-jpg"), ("v1.png", (480, 640), "rgba"), ("v2.png", (480, 640), "L"),
                 ("v3.png", (479, 641), "rgb-png")], {"v0", "v1", "v3"}, {"v0", "v2", "v3"})
    scene(port, [("p0.png", (640, 480), "rgb-png"), ("p1.jpg", (1000, 700), "rgb-jpg"), ("p2.png", (700, 500), "rgba")],
          {"p1", "p2"}, {"p0", "p1"})
    for root in (land, port):
        args = (str(root / "images"), str(root / "cameras"), str(root / "depths"))
        got = preprocess.load_images_and_cameras(*args)
        want = lo.load_images_and_cameras(*args)
        for i in range(5):
            assert got[i].is_cuda and got[i].dtype == torch.float32 and got[i].shape == want[i].shape, i
            assert torch.equal(got[i].cpu(), want[i]), i
        assert got[5] == want[5] and got[6] == want[6]
        assert float(got[4].sum()) > 0 and float(got[3].max()) <= 100.0
    got = preprocess.load_images_and_cameras(str(land / "images"))
    want = lo.load_images_and_cameras(str(land / "images"))
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got[:5], want[:5])) and got[5:] == ([], [])
    mixed = tmp_path / "mixed"
    _write_frames(mixed, rng, [("a.png", (480, 640), "rgb-png"), ("b.png", (640, 480), "rgb-png")])
    with pytest.raises(RuntimeError):
        preprocess.load_images_and_cameras(str(mixed))
    np.save(land / "depths" / "v2.npy", np.ones((4, 4), np.float32))
    Image.fromarray(np.zeros((4, 4), np.uint16)).save(land / "depths" / "v2.png")
    with pytest.raises(NotImplementedError, match="v2.png"):
        preprocess.load_images_and_cameras(str(land / "images"), None, str(land / "depths"))


def _filtered_source_depth(resized, src_hw):
    """The filtered source map behind a depth fixture of an UPSAMPLED view: cv2's nearest rule reads every source row and column there,
    so the first output pixel of each source pixel holds its filtered value. Zeros go back as the 1e10 sky marker of the originals
    (the filter turns them into 0 again)."""
    sh, sw = src_hw
    h, w = resized.shape
    ys = np.minimum(np.floor(np.arange(h) * (sh / h)).astype(np.int64), sh - 1)
    xs = np.minimum(np.floor(np.arange(w) * (sw / w)).astype(np.int64), sw - 1)
    first_y, first_x = np.searchsorted(ys, np.arange(sh)), np.searchsorted(xs, np.arange(sw))
    assert np.array_equal(ys[first_y], np.arange(sh)) and np.array_equal(xs[first_x], np.arange(sw))
    src = resized[first_y][:, first_x].astype(np.float32)
    src[src == 0] = 1e10
    return src


def test_reference_example_frames_reproduce_the_fixtures(tmp_path):
    """The reference's own example frames and camera files (tests/golden/real/loader_originals.npz holds the original bytes of some of
    the fixtures' views; tools/gen_loader_originals.py) through the device loaders: they reproduce the stored views of
    office_*.png / infinigen_*.png and *_inputs.npz bit for bit."""
    files = np.load(os.path.join(REAL, "loader_originals.npz"))
    views = {scene: files[scene + "/views"].tolist() for scene in ("office", "infinigen")}
    for key in files.files:
        if not key.endswith("/views"):
            path = tmp_path / key
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(files[key].tobytes())

    def frames(scene):
        return torch.stack([lo.to_tensor(Image.open(os.path.join(REAL, "%s_%d.png" % (scene, i)))) for i in views[scene]])

    inf = tmp_path / "infinigen"
    want = np.load(os.path.join(REAL, "infinigen_294_aux_inputs.npz"))
    v = views["infinigen"]
    (inf / "depths").mkdir()
    for i, name in zip(v, sorted(os.listdir(inf / "images"))):
        w, h = Image.open(inf / "images" / name).size
        np.save(inf / "depths" / (os.path.splitext(name)[0] + ".npy"), _filtered_source_depth(want["depth"][i], (h, w)))
    images, ext, intr, depth, mask, dgi, cgi = preprocess.load_images_and_cameras(str(inf / "images"), str(inf / "cameras"),
                                                                                  str(inf / "depths"))
    assert images.shape[0] == len(v) >= 2 and torch.equal(images.cpu(), frames("infinigen"))
    assert torch.equal(ext.cpu(), torch.from_numpy(want["extrinsics"][:, v]))
    assert torch.equal(intr.cpu(), torch.from_numpy(want["intrinsics"][:, v]))
    assert torch.equal(depth.cpu(), torch.from_numpy(want["depth"][v])[None, ..., None])
    assert torch.equal(mask.cpu(), (torch.from_numpy(want["depth"][v]) > 1e-5).float()[None])
    assert float(mask.mean()) < 1.0 and dgi == cgi == list(range(len(v)))

    office = tmp_path / "office"
    images, ext, intr, depth, mask, dgi, cgi = preprocess.load_images_and_cameras(str(office / "images"), str(office / "cameras"))
    want = np.load(os.path.join(REAL, "office_392_cams_inputs.npz"))
    v = views["office"]
    assert torch.equal(images.cpu(), frames("office")) and tuple(images.shape[-2:]) == tuple(want["hw"].tolist())
    assert torch.equal(ext.cpu(), torch.from_numpy(want["extrinsics"][:, v]))
    assert torch.equal(intr.cpu(), torch.from_numpy(want["intrinsics"][:, v]))
    assert not depth.any() and not mask.any() and dgi == [] and cgi == list(range(len(v)))

    paths = [str(office / "images" / f) for f in os.listdir(office / "images")]
    pad = preprocess.load_and_preprocess_images(paths, mode="pad")
    assert torch.equal(pad.cpu(), lo.pad_to_square(frames("office")))


def test_64_mixed_frames_chunks_and_streams(monkeypatch):
    rng = np.random.default_rng(64)
    shapes = [(480, 640), (720, 1280), (1080, 1920), (640, 480), (301, 517), (288, 512), (999, 333), (77, 1400)]
    frames = [twin.test_image(*shapes[i % len(shapes)], seed=int(rng.integers(1 << 30))) for i in range(64)]
    sizes = [preprocess.crop_geometry(a.shape[1], a.shape[0])[:2] for a in frames]
    want = [pil_resize(a, s) for a, s in zip(frames, sizes)]
    first = preprocess.resize_bicubic(frames, sizes)
    for g, w in zip(first, want):
        assert np.array_equal(g.cpu().numpy(), w)
    second = preprocess.resize_bicubic(frames, sizes)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    monkeypatch.setattr(preprocess, "STAGING_BYTES", 4 << 20)                # several chunks, each with its own upload
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = preprocess.resize_bicubic(frames, sizes)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, third))
