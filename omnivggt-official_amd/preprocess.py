"""Input loaders on the device: the reference's `load_images_and_cameras` (visual_util.py:679-845, what inference.py:335 calls) and
`load_and_preprocess_images` (omnivggt/utils/load_fn.py:53-146), bit for bit.

The host decodes, as the reference does (PIL `Image.open`, RGBA composited onto white, `convert("RGB")`, no EXIF transpose), in a
thread pool that keeps input order. Everything after `convert("RGB")` runs in libomnivggt_hip.so: Pillow's 8-bit bicubic resize
(`ovg_resample_frames`, integer arithmetic on fixed-point weights computed here in float64 exactly as Pillow computes them), the
centre crop or the white pad, ToTensor and the stack; for depth maps the filter, the cv2 INTER_NEAREST resize, the crop and the mask
(`ovg_depth_frames`). Cameras are O(S) and stay on the host in numpy. Frames travel in chunks of at most STAGING_BYTES of pinned memory:
descriptors, weight tables and pixels of a chunk in one asynchronous copy on the current stream.
"""
import collections
import ctypes
import functools
import glob
import itertools
import math
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from . import lib as L

STAGING_BYTES = 512 << 20          # pinned (and device) staging per chunk of frames
PRECISION_BITS = 22                # Pillow's 8-bit resample: 32 - 8 - 2 fractional bits
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")


# ---------------------------------------------------------------------------------------------------------------------------------
# Pillow's bicubic weights (Resample.c: bicubic_filter, precompute_coeffs, normalize_coeffs_8bpc)
# ---------------------------------------------------------------------------------------------------------------------------------

def _bicubic_filter(x):
    a = -0.5
    x = np.abs(x)
    out = np.zeros_like(x)
    near, far = x < 1.0, (x >= 1.0) & (x < 2.0)
    xn, xf = x[near], x[far]
    out[near] = ((a + 2.0) * xn - (a + 3.0)) * xn * xn + 1
    out[far] = (((xf - 5) * xf + 8) * xf - 4) * a
    return out


@functools.lru_cache(maxsize=256)
def coefficients(in_size, out_size):
    """Fixed-point weights of one axis of Pillow's BICUBIC resize from `in_size` to `out_size` samples: (bounds int32 [out, 2] =
    (first input index, tap count), k int32 [out, ksize]). An axis that keeps its size gets the identity (one tap of 2^22): Pillow
    skips that pass, and the identity reproduces the copy exactly. Read-only arrays, cached per (in, out)."""
    if in_size < 1 or out_size < 1:
        raise ValueError("resize sizes must be positive (got %d -> %d)" % (in_size, out_size))
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32)
        k = np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
    else:
        scale = in_size / out_size
        filterscale = max(scale, 1.0)
        support = 2.0 * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)          # C (int) truncates
        count = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
        j = np.arange(ksize)
        w = _bicubic_filter(((j[None, :] + xmin[:, None]) - center[:, None] + 0.5) * ss)
        w[j[None, :] >= count[:, None]] = 0.0
        ww = np.cumsum(w, axis=1)[:, -1:]                       # summed left to right, as Pillow's loop does (np.sum is pairwise)
        w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
        scaled = w * (1 << PRECISION_BITS)
        k = np.where(w < 0, np.trunc(scaled - 0.5), np.trunc(scaled + 0.5)).astype(np.int32)
        bounds = np.stack([xmin, count], 1).astype(np.int32)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


# ---------------------------------------------------------------------------------------------------------------------------------
# Geometry (the reference's rules)
# ---------------------------------------------------------------------------------------------------------------------------------

def crop_geometry(width, height, target_size=518):
    """visual_util.py:731-747 / load_fn.py mode="crop": (new_width, new_height, crop_start_y, final_height)."""
    new_width = target_size
    new_height = round(height * (new_width / width) / 14) * 14
    if new_height > target_size:
        return new_width, new_height, (new_height - target_size) // 2, target_size
    return new_width, new_height, 0, new_height


def pad_geometry(width, height, target_size=518):
    """load_fn.py mode="pad": the largest side becomes target_size, the other a multiple of 14 -> (new_width, new_height)."""
    if width >= height:
        return target_size, round(height * (target_size / width) / 14) * 14
    return round(width * (target_size / height) / 14) * 14, target_size


# ---------------------------------------------------------------------------------------------------------------------------------
# Host I/O
# ---------------------------------------------------------------------------------------------------------------------------------

def decode_rgb(path):
    """The reference's decode: PIL open, RGBA onto white with alpha_composite, convert("RGB") -> (H, W, 3) uint8."""
    img = Image.open(path)
    if img.mode == "RGBA":
        background = Image.new("RGBA", img.size, (255, 255, 255, 255))
        img = Image.alpha_composite(background, img)
    return np.asarray(img.convert("RGB"))


def _image_size(path):
    with Image.open(path) as img:                # header only; compositing and convert() keep the size
        return img.size


def _decode_ordered(paths, workers):
    """decode_rgb over `paths` in a pool of `workers` threads, yielded in input order, at most 2 * workers frames ahead."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        it = iter(paths)
        pending = collections.deque(ex.submit(decode_rgb, p) for p in itertools.islice(it, 2 * workers))
        while pending:
            frame = pending.popleft().result()
            nxt = next(it, None)
            if nxt is not None:
                pending.append(ex.submit(decode_rgb, nxt))
            yield frame


def read_camera_txt(camera_path):
    """visual_util.py:847-893: three rows of the 3x4 camera-to-world matrix, then three rows of the 3x3 intrinsics, ignoring blank
    lines and `#` comments -> (c2w f32 (3, 4), K f32 (3, 3)), or (None, None) when the file does not hold them."""
    with open(camera_path, "r") as fh:
        rows = [s.strip() for s in fh.readlines()]
    rows = [s for s in rows if s and not s.startswith("#")]
    if len(rows) < 6:
        return None, None
    values = []
    for i, s in enumerate(rows[:6]):                 # row by row: a short row ends the parse before later rows are read
        v = [float(x) for x in s.split()]
        if len(v) != (4 if i < 3 else 3):
            return None, None
        values.append(v)
    return np.array(values[:3], dtype=np.float32), np.array(values[3:], dtype=np.float32)


def world_to_camera(c2w):
    """omnivggt/utils/geometry.py closed_form_inverse_se3 (numpy branch) of one (3, 4) f32 camera-to-world matrix -> (3, 4) float64:
    R^T and -R^T t formed in f32 and stored into a float64 identity, as the reference does."""
    se3 = c2w[None]
    rot_t = np.transpose(se3[:, :3, :3], (0, 2, 1))
    inv = np.tile(np.eye(4), (1, 1, 1))
    inv[:, :3, :3] = rot_t
    inv[:, :3, 3:] = -np.matmul(rot_t, se3[:, :3, 3:])
    return inv[0][:3]


def view_camera(camera_path, width, height, target_size=518):
    """One view's camera as visual_util.py:810-833 prepares it for a width x height image: (world-to-camera (3, 4) float64, intrinsics
    (3, 3) f32 scaled to the resized image and shifted by the centre crop), or (None, None) when the file holds no camera."""
    c2w, intr = read_camera_txt(camera_path)
    if c2w is None or intr is None:
        return None, None
    new_w, new_h, crop_y, _ = crop_geometry(width, height, target_size)
    scale_x, scale_y = new_w / width, new_h / height
    intr[0, 0] *= scale_x
    intr[1, 1] *= scale_y
    intr[0, 2] *= scale_x
    intr[1, 2] *= scale_y
    if new_h > target_size:
        intr[1, 2] -= crop_y
    return world_to_camera(c2w), intr


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else device
    dev = torch.device(dev) if dev is not None else torch.device("cpu")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise L.OvgError("the device loaders need a HIP device (got %s): there is no CPU fallback" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


# ---------------------------------------------------------------------------------------------------------------------------------
# Device passes
# ---------------------------------------------------------------------------------------------------------------------------------

def _align(n, a=16):
    return (n + a - 1) // a * a


class _Staging:
    """One pinned host buffer holding several regions (descriptors, tables, data), copied to the device in one asynchronous copy."""

    def __init__(self, sizes):
        self.offsets, total = [], 0
        for s in sizes:
            self.offsets.append(total)
            total = _align(total + s)
        self.host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
        self.np = self.host.numpy()

    def view(self, i, dtype, count):
        return self.np[self.offsets[i]:self.offsets[i] + count * np.dtype(dtype).itemsize].view(dtype)

    def upload(self, device):
        self.dev = torch.empty_like(self.host, device=device)
        self.dev.copy_(self.host, non_blocking=True)
        return self.dev

    def host_ptr(self, i):
        return self.host.data_ptr() + self.offsets[i]

    def dev_ptr(self, i):
        return self.dev.data_ptr() + self.offsets[i]


def _chunks(items, nbytes):
    """Group (item, array) pairs into lists whose arrays hold at most STAGING_BYTES (one oversized array goes alone)."""
    chunk, size = [], 0
    for item in items:
        b = nbytes(item)
        if chunk and size + b > STAGING_BYTES:
            yield chunk
            chunk, size = [], 0
        chunk.append(item)
        size += b
    if chunk:
        yield chunk


def _resample_chunk(chunk, out, fmt, device):
    """chunk: list of (geometry dict, (H, W, 3) uint8 array). Writes every frame's canvas into `out` (device, contiguous)."""
    lib = L.load()
    n = len(chunk)
    tables, table_off, coef_len = [], {}, 0

    def table(in_size, out_size):
        nonlocal coef_len
        key = (in_size, out_size)
        if key not in table_off:
            bounds, k = coefficients(in_size, out_size)
            table_off[key] = (coef_len, coef_len + bounds.size, k.shape[1])
            tables.extend([bounds.ravel(), k.ravel()])
            coef_len += bounds.size + k.size
        return table_off[key]

    descs = (L.ResampleFrame * n)()
    src_bytes, ws_bytes = 0, 0
    for i, (g, a) in enumerate(chunk):
        h, w = a.shape[:2]
        d = descs[i]
        d.src_off, d.src_w, d.src_h = src_bytes, w, h
        d.res_w, d.res_h, d.crop_y, d.out_h = g["res_w"], g["res_h"], g["crop_y"], g["out_h"]
        d.v_bounds_off, d.v_k_off, d.v_ksize = table(h, g["res_h"])
        if w != g["res_w"]:
            d.h_bounds_off, d.h_k_off, d.h_ksize = table(w, g["res_w"])
            vb = coefficients(h, g["res_h"])[0][g["crop_y"]:g["crop_y"] + g["out_h"]]
            row0, row1 = int(vb[:, 0].min()), int((vb[:, 0] + vb[:, 1]).max())
            d.mid_row0, d.mid_rows, d.mid_off = row0, row1 - row0, ws_bytes
            ws_bytes = _align(ws_bytes + 3 * (row1 - row0) * g["res_w"])
        else:
            d.h_bounds_off, d.h_k_off, d.h_ksize = -1, -1, 0
        d.canvas_w, d.canvas_h, d.pad_top, d.pad_left, d.canvas_off = g["canvas_w"], g["canvas_h"], g["pad_top"], g["pad_left"], g["canvas_off"]
        src_bytes += a.nbytes
    st = _Staging([ctypes.sizeof(descs), 4 * coef_len, 4 * 256, src_bytes])
    ctypes.memmove(st.host_ptr(0), descs, ctypes.sizeof(descs))
    st.view(1, np.int32, coef_len)[:] = np.concatenate(tables)
    st.view(2, np.float32, 256)[:] = (torch.arange(256, dtype=torch.float32) / 255).numpy()
    pix = st.view(3, np.uint8, src_bytes)
    for i, (_, a) in enumerate(chunk):
        pix[descs[i].src_off:descs[i].src_off + a.nbytes] = a.reshape(-1)
    st.upload(device)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
    p = L.ResampleParams(frames=st.dev_ptr(0), frames_host=st.host_ptr(0), nframes=n, out_format=fmt, src=st.dev_ptr(3),
                         src_bytes=src_bytes, coef=st.dev_ptr(1), coef_host=st.host_ptr(1), coef_len=coef_len, lut=st.dev_ptr(2),
                         out=out.data_ptr(), out_elems=out.numel(), ws=ws.data_ptr(), ws_bytes=ws.numel())
    assert lib.ovg_resample_workspace_bytes(ctypes.cast(descs, ctypes.c_void_p), n) <= ws.numel()
    L.call("ovg_resample_frames", p, torch.cuda.current_stream(device).cuda_stream)


def _resample(geoms, frames, out, fmt, device):
    with torch.cuda.device(device):
        for chunk in _chunks(zip(geoms, frames), lambda item: item[1].nbytes):
            _resample_chunk(chunk, out, fmt, device)


def _depth_chunk(chunk, depth, mask, max_depth, device):
    """chunk: list of (geometry dict, (h, w) f32 array); cv2 INTER_NEAREST index rule of the resize to (res_w, res_h), then the crop."""
    n = len(chunk)
    descs = (L.DepthFrame * n)()
    index, index_len, src_elems = [], 0, 0
    for i, (g, a) in enumerate(chunk):
        sh, sw = a.shape
        ys = np.minimum(np.floor(np.arange(g["res_h"]) * (sh / g["res_h"])).astype(np.int64), sh - 1)[g["crop_y"]:g["crop_y"] + g["out_h"]]
        xs = np.minimum(np.floor(np.arange(g["res_w"]) * (sw / g["res_w"])).astype(np.int64), sw - 1)
        d = descs[i]
        d.src_off, d.src_w, d.src_h = src_elems, sw, sh
        d.rows_off, d.cols_off, d.out_w, d.out_h, d.out_off = index_len, index_len + ys.size, xs.size, ys.size, g["out_off"]
        index.extend([ys, xs])
        index_len += ys.size + xs.size
        src_elems += a.size
    st = _Staging([ctypes.sizeof(descs), 4 * index_len, 4 * src_elems])
    ctypes.memmove(st.host_ptr(0), descs, ctypes.sizeof(descs))
    st.view(1, np.int32, index_len)[:] = np.concatenate(index)
    vals = st.view(2, np.float32, src_elems)
    for i, (_, a) in enumerate(chunk):
        vals[descs[i].src_off:descs[i].src_off + a.size] = a.reshape(-1)
    st.upload(device)
    p = L.DepthParams(frames=st.dev_ptr(0), frames_host=st.host_ptr(0), nframes=n, max_depth=float(np.float32(max_depth)),
                      src=st.dev_ptr(2), src_elems=src_elems, index=st.dev_ptr(1), index_host=st.host_ptr(1), index_len=index_len,
                      depth=depth.data_ptr(), mask=mask.data_ptr(), out_elems=depth.numel())
    L.call("ovg_depth_frames", p, torch.cuda.current_stream(device).cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------------
# Public API
# ---------------------------------------------------------------------------------------------------------------------------------

def _host_frame(f):
    a = f.numpy() if isinstance(f, torch.Tensor) and not f.is_cuda else f
    if not isinstance(a, np.ndarray):
        raise L.OvgError("resize_bicubic takes host frames (numpy arrays or CPU tensors), got %s" % type(f).__name__)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("frames must be (H, W, 3) uint8 arrays, got %s %s" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def resize_bicubic(frames, sizes, device=None):
    """Pillow's `Image.resize(size, Image.Resampling.BICUBIC)` of RGB frames on the device, bit for bit, all frames in one launch per
    pass. frames: (H, W, 3) uint8 host arrays (np.asarray of an RGB image); sizes: one (width, height) per frame, in PIL's order.
    -> list of (height, width, 3) uint8 device tensors (views of one allocation)."""
    if len(frames) != len(sizes) or not frames:
        raise ValueError("resize_bicubic needs one (width, height) per frame and at least one frame")
    dev = _device(device)
    frames = [_host_frame(f) for f in frames]
    geoms, total = [], 0
    for (w, h) in sizes:
        if w < 1 or h < 1:
            raise ValueError("height and width must be > 0")
        geoms.append(dict(res_w=w, res_h=h, crop_y=0, out_h=h, canvas_w=w, canvas_h=h, pad_top=0, pad_left=0, canvas_off=total))
        total += 3 * w * h
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    _resample(geoms, frames, out, L.RS_U8_HWC, dev)
    return [out[g["canvas_off"]:g["canvas_off"] + 3 * g["res_w"] * g["res_h"]].view(g["res_h"], g["res_w"], 3) for g in geoms]


def _check_workers(workers):
    if not isinstance(workers, int) or workers < 1:
        raise ValueError("workers must be a positive int")


def load_and_preprocess_images(image_path_list, mode="crop", device=None, workers=4):
    """omnivggt/utils/load_fn.py:12-146 on the device: sorted paths; mode "crop" (width 518, height a multiple of 14, centre-cropped to
    518) or "pad" (largest side 518, white borders to 518 x 518); frames of different shapes are padded white to the largest.
    -> (S, 3, H, W) f32 on the device, equal to the reference's tensor bit for bit."""
    if len(image_path_list) == 0:
        raise ValueError("At least 1 image is required")
    if mode not in ["crop", "pad"]:
        raise ValueError("Mode must be either 'crop' or 'pad'")
    _check_workers(workers)
    dev = _device(device)
    target_size = 518
    paths = sorted(image_path_list)
    geoms = []
    for path in paths:
        width, height = _image_size(path)
        if mode == "pad":
            new_w, new_h = pad_geometry(width, height, target_size)
            crop_y, out_h = 0, new_h
            shape = (target_size, target_size)
        else:
            new_w, new_h, crop_y, out_h = crop_geometry(width, height, target_size)
            shape = (out_h, new_w)
        if new_w < 1 or new_h < 1:
            raise ValueError("height and width must be > 0 (%s resizes to %d x %d)" % (path, new_w, new_h))
        geoms.append(dict(res_w=new_w, res_h=new_h, crop_y=crop_y, out_h=out_h, shape=shape))
    H, W = max(g["shape"][0] for g in geoms), max(g["shape"][1] for g in geoms)
    for s, g in enumerate(geoms):
        # the reference pads twice (to 518^2 in pad mode, then to the largest shape): offsets add up to (H - h) // 2 only when the
        # first pad already reached the final shape, so compose them as it does
        top = (g["shape"][0] - g["out_h"]) // 2 + (H - g["shape"][0]) // 2
        left = (g["shape"][1] - g["res_w"]) // 2 + (W - g["shape"][1]) // 2
        g.update(canvas_w=W, canvas_h=H, pad_top=top, pad_left=left, canvas_off=s * 3 * H * W)
    out = torch.empty(len(paths), 3, H, W, dtype=torch.float32, device=dev)
    _resample(geoms, _decode_ordered(paths, workers), out, L.RS_F32_CHW, dev)
    return out


def load_images_and_cameras(image_folder, camera_folder=None, depth_folder=None, target_size=518, max_depth=100, device=None, workers=4):
    """visual_util.py:679-845 on the device. Returns the reference's 7-tuple: images (S, 3, H, W), extrinsics (1, S, 3, 4)
    world-to-camera, intrinsics (1, S, 3, 3), depth (1, S, H, W, 1), mask (1, S, H, W) -- f32 tensors on the device, equal to the
    reference's bit for bit -- and the lists of view indices that have a depth map / a camera file.
    Depth maps are `<stem>.npy`; a `<stem>.png` depth map raises NotImplementedError (the reference reads it with cv2)."""
    _check_workers(workers)
    dev = _device(device)
    paths = sorted(glob.glob(os.path.join(image_folder, "*")))
    paths = [p for p in paths if p.lower().endswith(IMAGE_EXTENSIONS)]
    if not paths:
        raise RuntimeError("no .png / .jpg / .jpeg images in %s" % image_folder)
    geoms, depth_jobs, depth_indices, camera_indices, extrinsics, intrinsics = [], [], [], [], [], []
    for idx, path in enumerate(paths):
        stem = Path(path).stem
        width, height = _image_size(path)
        new_w, new_h, crop_y, out_h = crop_geometry(width, height, target_size)
        if new_h < 1:
            raise ValueError("height and width must be > 0 (%s resizes to %d x %d)" % (path, new_w, new_h))
        geoms.append(dict(res_w=new_w, res_h=new_h, crop_y=crop_y, out_h=out_h, canvas_w=new_w, canvas_h=out_h, pad_top=0, pad_left=0))
        if depth_folder is not None:
            png = os.path.join(depth_folder, stem + ".png")
            if os.path.exists(png):
                raise NotImplementedError("%s: .png depth maps are not supported (the reference reads them with cv2); use .npy" % png)
            npy = os.path.join(depth_folder, stem + ".npy")
            if os.path.exists(npy):
                d = np.load(npy).astype(np.float32)
                if d.ndim != 2 or d.size == 0:
                    raise ValueError("%s: expected a 2-D depth map, got shape %s" % (npy, d.shape))
                depth_indices.append(idx)
                depth_jobs.append((idx, d))
        ext = intr = None
        if camera_folder is not None:
            cam = os.path.join(camera_folder, stem + ".txt")
            if os.path.exists(cam):
                ext, intr = view_camera(cam, width, height, target_size)
        if ext is not None:
            camera_indices.append(idx)
        else:
            ext, intr = np.zeros((3, 4), dtype=np.float32), np.zeros((3, 3), dtype=np.float32)
        extrinsics.append(ext)
        intrinsics.append(intr)
    heights = sorted({g["out_h"] for g in geoms})
    if len(heights) > 1:
        raise RuntimeError("stack expects each tensor to be equal size, but the frames of %s have heights %s after resizing"
                           % (image_folder, heights))
    S, H, W = len(paths), heights[0], target_size
    for s, g in enumerate(geoms):
        g["canvas_off"] = s * 3 * H * W
    images = torch.empty(S, 3, H, W, dtype=torch.float32, device=dev)
    depth = torch.zeros(1, S, H, W, 1, dtype=torch.float32, device=dev)
    mask = torch.zeros(1, S, H, W, dtype=torch.float32, device=dev)
    _resample(geoms, _decode_ordered(paths, workers), images, L.RS_F32_CHW, dev)
    if depth_jobs:
        jobs = [(dict(geoms[i], out_off=i * H * W), d) for i, d in depth_jobs]
        with torch.cuda.device(dev):
            for chunk in _chunks(jobs, lambda item: item[1].nbytes):
                _depth_chunk(chunk, depth, mask, max_depth, dev)
    ext_t = torch.from_numpy(np.array(extrinsics))[None, ...].float().to(dev)
    intr_t = torch.from_numpy(np.array(intrinsics))[None, ...].float().to(dev)
    return images, ext_t, intr_t, depth, mask, depth_indices, camera_indices
