"""Device loaders, host side: the numpy twin of Pillow's bicubic resize (tests/resample_twin.py) against PIL itself, the product's
fixed-point tables against the twin's, the loaders' geometry and camera code against oracle/loader_oracle.py, and the C ABI of the
preprocessing entries without a device."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import abi_layout
import loader_oracle as lo
import resample_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import preprocess


GEOMETRIES = twin.GEOMETRIES


def pil_resize(a, size):
    return np.asarray(Image.fromarray(a, "RGB").resize(size, Image.Resampling.BICUBIC))


@pytest.mark.parametrize("src,size", GEOMETRIES, ids=["%dx%d-%dx%d" % (s[1], s[0], o[0], o[1]) for s, o in GEOMETRIES])
def test_twin_is_pillow_and_product_tables_are_the_twins(src, size):
    a = twin.test_image(*src, seed=src[0] * 7 + src[1])
    got = twin.resize(a, size)
    want = pil_resize(a, size)
    assert got.shape == want.shape and int(np.abs(got.astype(np.int64) - want).max()) == 0
    for n_in, n_out in ((src[1], size[0]), (src[0], size[1])):
        bounds, k = preprocess.coefficients(n_in, n_out)
        if n_in == n_out:                                                   # Pillow skips the pass; the product uses the identity
            assert np.array_equal(bounds[:, 0], np.arange(n_out)) and (bounds[:, 1] == 1).all() and (k[:, 0] == 1 << 22).all()
            continue
        xmin, n, kt = twin.coeffs(n_in, n_out)
        assert np.array_equal(bounds[:, 0], xmin) and np.array_equal(bounds[:, 1], n)
        assert k.shape == kt.shape and np.array_equal(k.astype(np.int64), kt)


def test_geometry_rules_match_the_reference_loaders():
    for w in list(range(1, 80)) + list(range(500, 540)) + [640, 1280, 1920, 3024, 4032]:
        for h in list(range(1, 80, 3)) + list(range(380, 700, 7)) + [1080, 3024, 4032]:
            assert preprocess.crop_geometry(w, h) == lo.resized_geometry(w, h), (w, h)
            if w >= h:
                want = (518, round(h * (518 / w) / 14) * 14)
            else:
                want = (round(w * (518 / h) / 14) * 14, 518)
            assert preprocess.pad_geometry(w, h) == want, (w, h)
    assert preprocess.crop_geometry(480, 640) == (518, 686, 84, 518) and preprocess.pad_geometry(480, 640) == (392, 518)


def _write_camera(path, c2w, K, rng):
    with open(path, "w") as fh:
        fh.write("# camera-to-world, then intrinsics\n\n")
        for row in c2w:
            fh.write(" ".join("%.9g" % v for v in row) + "\n")
            if rng.random() < 0.5:
                fh.write("\n   \n")
        fh.write("# intrinsics\n")
        for row in K:
            fh.write("  " + "\t".join(repr(float(v)) for v in row) + "  \n")


def test_cameras_are_bit_equal_to_the_oracle(tmp_path):
    """read_camera_txt + view_camera (intrinsics scaled, cy shifted by the crop, camera-to-world inverted) against the oracle loader on
    seeded camera files with comments and blank lines, for landscape, portrait (cropped) and odd image sizes."""
    rng = np.random.default_rng(5)
    sizes = [(640, 480), (480, 640), (517, 333), (1920, 1080), (37, 23), (1000, 1400)]
    for i, (w, h) in enumerate(sizes):
        d = tmp_path / ("s%d" % i)
        (d / "images").mkdir(parents=True)
        (d / "cameras").mkdir()
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(d / "images" / "v.png")
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        c2w = np.concatenate([q, 10 * rng.normal(size=(3, 1))], axis=1)
        f = 300 + 900 * rng.random()
        K = np.array([[f, 0, w / 2 + rng.normal()], [0, f * (1 + 0.01 * rng.random()), h / 2 + rng.normal()], [0, 0, 1]])
        _write_camera(d / "cameras" / "v.txt", c2w, K, rng)
        _, ext, intr, *_ = lo.load_images_and_cameras(str(d / "images"), str(d / "cameras"))
        e, k = preprocess.view_camera(str(d / "cameras" / "v.txt"), w, h)
        assert e.dtype == np.float64 and k.dtype == np.float32
        assert torch.from_numpy(np.array([e]))[None].float().numpy().tobytes() == ext.numpy().tobytes(), (w, h)
        assert k[None, None].tobytes() == intr.numpy().tobytes(), (w, h)
        c2w_o, K_o = lo.load_camera_from_txt(str(d / "cameras" / "v.txt"))
        c2w_p, K_p = preprocess.read_camera_txt(str(d / "cameras" / "v.txt"))
        assert c2w_p.tobytes() == c2w_o.tobytes() and K_p.tobytes() == K_o.tobytes()
        assert preprocess.world_to_camera(c2w_p).tobytes() == lo.closed_form_inverse_se3(c2w_o[None])[0][:3].tobytes()
    bad = tmp_path / "bad.txt"
    bad.write_text("1 2 3 4\n1 2 3\n1 2 3 4\n1 0 0\n0 1 0\n0 0 1\n")
    assert preprocess.read_camera_txt(str(bad)) == (None, None) == lo.load_camera_from_txt(str(bad))
    bad.write_text("# only comments\n\n1 2 3 4\n")
    assert preprocess.read_camera_txt(str(bad)) == (None, None) == lo.load_camera_from_txt(str(bad))


def test_abi_version_and_struct_layout_match_c():
    lib = L.load()
    assert L.ABI_VERSION == 13 and lib.ovg_abi_version() == 13
    pairs = {"ovg_resample_frame": L.ResampleFrame, "ovg_resample_params": L.ResampleParams, "ovg_depth_frame": L.DepthFrame,
             "ovg_depth_params": L.DepthParams}
    fmt, _ = abi_layout.check(pairs, ["OVG_RS_F32_CHW", "OVG_RS_U8_HWC"])
    assert fmt == [L.RS_F32_CHW, L.RS_U8_HWC]


def _valid_resample():
    """Host descriptors / tables of one 8x6 -> 5x4 frame into a 3 x 6 x 7 f32 canvas, device pointers fake (never dereferenced)."""
    hb, hk = preprocess.coefficients(8, 5)
    vb, vk = preprocess.coefficients(6, 4)
    coef = np.concatenate([hb.ravel(), hk.ravel(), vb.ravel(), vk.ravel()]).astype(np.int32)
    f = L.ResampleFrame(src_off=0, src_w=8, src_h=6, res_w=5, res_h=4, crop_y=0, out_h=4, mid_row0=0, mid_rows=6, mid_off=0,
                        h_bounds_off=0, h_k_off=hb.size, h_ksize=hk.shape[1], v_bounds_off=hb.size + hk.size,
                        v_k_off=hb.size + hk.size + vb.size, v_ksize=vk.shape[1], canvas_w=7, canvas_h=6, pad_top=1, pad_left=1,
                        canvas_off=0)
    return f, coef


def test_preprocess_argument_validation_without_gpu():
    lib = L.load()
    big = 1 << 40
    f0, coef0 = _valid_resample()

    def rs(frame_kw=None, coef_patch=None, **kw):
        f = L.ResampleFrame.from_buffer_copy(f0)
        for k, v in (frame_kw or {}).items():
            setattr(f, k, v)
        coef = coef0.copy()
        if coef_patch:
            coef[coef_patch[0]] = coef_patch[1]
        frames = (L.ResampleFrame * 1)(f)
        p = L.ResampleParams(frames=big, frames_host=ctypes.addressof(frames), nframes=1, out_format=L.RS_F32_CHW, src=big,
                             src_bytes=3 * 8 * 6, coef=big, coef_host=coef.ctypes.data, coef_len=coef.size, lut=big, out=big,
                             out_elems=3 * 6 * 7, ws=big, ws_bytes=3 * 6 * 5)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_resample_frames(ctypes.byref(p), None)

    assert lib.ovg_resample_frames(None, None) == -1
    frames = (L.ResampleFrame * 1)(f0)
    assert lib.ovg_resample_workspace_bytes(ctypes.addressof(frames), 1) == 3 * 6 * 5
    assert lib.ovg_resample_workspace_bytes(None, 1) == -1 and lib.ovg_resample_workspace_bytes(ctypes.addressof(frames), 0) == -1
    hb, hk = preprocess.coefficients(8, 5)
    v0 = hb.size + hk.size                                                   # first entry of the vertical bounds
    bad_cases = [
        dict(frames=None), dict(frames_host=None), dict(src=None), dict(coef=None), dict(coef_host=None), dict(out=None), dict(lut=None),
        dict(nframes=0), dict(nframes=-1), dict(out_format=2), dict(src_bytes=3 * 8 * 6 - 1), dict(out_elems=3 * 6 * 7 - 1),
        dict(ws_bytes=3 * 6 * 5 - 1), dict(ws=None), dict(coef_len=int(coef0.size) - 1),
        dict(frame_kw=dict(src_w=0)), dict(frame_kw=dict(src_h=-3)), dict(frame_kw=dict(res_w=0)), dict(frame_kw=dict(src_off=1)),
        dict(frame_kw=dict(src_off=-1)), dict(frame_kw=dict(crop_y=1)), dict(frame_kw=dict(out_h=0)), dict(frame_kw=dict(out_h=5)),
        dict(frame_kw=dict(pad_top=3)), dict(frame_kw=dict(pad_left=3)), dict(frame_kw=dict(pad_top=-1)), dict(frame_kw=dict(canvas_off=1)),
        dict(frame_kw=dict(canvas_w=5, canvas_h=6)), dict(frame_kw=dict(mid_rows=7)), dict(frame_kw=dict(mid_row0=1)),
        dict(frame_kw=dict(mid_off=1)), dict(frame_kw=dict(h_ksize=0)), dict(frame_kw=dict(h_k_off=10 ** 6)),
        dict(frame_kw=dict(v_bounds_off=int(coef0.size) - 2)), dict(frame_kw=dict(v_k_off=-2)), dict(frame_kw=dict(h_k_off=-1)),
        dict(frame_kw=dict(canvas_w=1 << 21)),
        dict(coef_patch=(0, -1)), dict(coef_patch=(1, 0)), dict(coef_patch=(1, 100)), dict(coef_patch=(2 * 4, 7)),
        dict(coef_patch=(v0 + 2 * 3, 5)), dict(coef_patch=(v0 + 1, 0)),
    ]
    for bad in bad_cases:
        assert rs(**bad) == -1, bad

    def dp(frame_kw=None, idx_patch=None, **kw):
        idx = np.array([0, 1, 2, 0, 3, 4], np.int32)                         # rows (3 of a 3-row map), cols (3 of a 5-column map)
        if idx_patch:
            idx[idx_patch[0]] = idx_patch[1]
        f = L.DepthFrame(src_off=0, src_w=5, src_h=3, rows_off=0, cols_off=3, out_w=3, out_h=3, out_off=0)
        for k, v in (frame_kw or {}).items():
            setattr(f, k, v)
        frames = (L.DepthFrame * 1)(f)
        p = L.DepthParams(frames=big, frames_host=ctypes.addressof(frames), nframes=1, max_depth=100.0, src=big, src_elems=15, index=big,
                          index_host=idx.ctypes.data, index_len=6, depth=big, mask=big, out_elems=9)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_depth_frames(ctypes.byref(p), None)

    assert lib.ovg_depth_frames(None, None) == -1
    for bad in (dict(frames=None), dict(frames_host=None), dict(src=None), dict(index=None), dict(index_host=None), dict(depth=None),
                dict(mask=None), dict(nframes=0), dict(src_elems=14), dict(out_elems=8), dict(index_len=5),
                dict(frame_kw=dict(out_off=1)), dict(frame_kw=dict(src_off=1)), dict(frame_kw=dict(out_w=0)),
                dict(frame_kw=dict(rows_off=4)), dict(frame_kw=dict(cols_off=-1)),
                dict(idx_patch=(0, -1)), dict(idx_patch=(2, 3)), dict(idx_patch=(5, 5)), dict(idx_patch=(3, -2))):
        assert dp(**bad) == -1, bad


def test_loaders_reject_cpu_devices_and_bad_arguments(tmp_path):
    a = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(L.OvgError):
        preprocess.resize_bicubic([a], [(3, 2)], device="cpu")
    with pytest.raises(L.OvgError):
        preprocess.resize_bicubic([a], [(3, 2)], device=torch.device("cpu"))
    Image.fromarray(a).save(tmp_path / "x.png")
    with pytest.raises(L.OvgError):
        preprocess.load_and_preprocess_images([str(tmp_path / "x.png")], device="cpu")
    with pytest.raises(L.OvgError):
        preprocess.load_images_and_cameras(str(tmp_path), device="cpu")
    with pytest.raises(ValueError):
        preprocess.load_and_preprocess_images([])
    with pytest.raises(ValueError):
        preprocess.load_and_preprocess_images([str(tmp_path / "x.png")], mode="stretch")
    with pytest.raises(ValueError):
        preprocess.resize_bicubic([a], [])
    with pytest.raises(ValueError):
        preprocess.load_and_preprocess_images([str(tmp_path / "x.png")], workers=0)


def test_decoder_keeps_input_order_and_bounds_its_window(tmp_path, monkeypatch):
    paths = []
    for i in range(11):
        p = tmp_path / ("f%02d.png" % i)
        Image.fromarray(np.full((3 + i, 4, 3), i, np.uint8)).save(p)
        paths.append(str(p))
    frames = list(preprocess._decode_ordered(paths, 3))
    assert [int(f[0, 0, 0]) for f in frames] == list(range(11)) and [f.shape[0] for f in frames] == [3 + i for i in range(11)]
    rgba = np.zeros((5, 6, 4), np.uint8)
    rgba[..., 0] = 200
    rgba[2:, :, 3] = 255
    Image.fromarray(rgba, "RGBA").save(tmp_path / "a.png")
    got = preprocess.decode_rgb(str(tmp_path / "a.png"))
    assert np.array_equal(got, np.asarray(lo.open_rgb(str(tmp_path / "a.png"))))
    assert (got[:2] == 255).all() and (got[2:, :, 0] == 200).all()
    Image.fromarray(np.arange(30, dtype=np.uint8).reshape(5, 6), "L").save(tmp_path / "g.png")
    assert np.array_equal(preprocess.decode_rgb(str(tmp_path / "g.png")), np.asarray(lo.open_rgb(str(tmp_path / "g.png"))))
