"""Host reference loader against the device loader, end to end from files in a temporary folder (load_images_and_cameras, images only).

Frames are generated from a seed (smooth gradients + noise, so JPEG / PNG sizes are realistic) and written as JPEG (quality 90) or PNG.
For each set it reports, in ms:
  host reference   oracle/loader_oracle.load_images_and_cameras (PIL decode + PIL bicubic + ToTensor + stack, one thread), one run
  device loader    preprocess.load_images_and_cameras (decode in a pool of `workers` threads, upload, kernels), ending in a sync;
                   median of 3 after one warm-up
  decode only      the same pool decoding the same files, nothing else (the host floor of the device loader); median of 3
  upload+kernels   the device part for already-decoded frames (pinned packing, copy, both passes), events; median of 3
  kernels          the ovg_resample_frames launches alone, events around the call; median of 3
and checks that the device result equals the host reference bit for bit.

    python tools/probes/preprocess_probe.py [--views 8 64] [--workers 4]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import loader_oracle as lo  # noqa: E402
from omnivggt_official_amd import lib as L, preprocess  # noqa: E402


def write_frames(folder, n, h, w, ext, seed):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        base = np.stack([(xx * (i + 1) // 7) % 256, (yy * 3 + i * 11) % 256, ((xx + yy) // 5) % 256], -1)
        a = np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(folder, "f%03d.%s" % (i, ext)), **({"quality": 90} if ext == "jpg" else {}))


def median_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def device_part(folder, workers):
    """(upload + kernels ms, kernels ms) for frames decoded beforehand, measured with events on the current stream."""
    paths = sorted(os.path.join(folder, f) for f in os.listdir(folder))
    frames = list(preprocess._decode_ordered(paths, workers))
    geoms = []
    for s, a in enumerate(frames):
        w, h, crop, out_h = preprocess.crop_geometry(a.shape[1], a.shape[0])
        geoms.append(dict(res_w=w, res_h=h, crop_y=crop, out_h=out_h, canvas_w=w, canvas_h=out_h, pad_top=0, pad_left=0))
    H = geoms[0]["out_h"]
    for s, g in enumerate(geoms):
        g["canvas_off"] = s * 3 * H * 518
    out = torch.empty(len(frames), 3, H, 518, device="cuda")
    dev = out.device
    kern = []
    real_call = L.call

    def call(name, p, stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        real_call(name, p, stream)
        b.record()
        kern.append((a, b))

    total = []
    L.call = call
    try:
        for _ in range(4):
            kern.clear()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            preprocess._resample(geoms, frames, out, L.RS_F32_CHW, dev)
            b.record()
            torch.cuda.synchronize()
            total.append((a.elapsed_time(b), sum(x.elapsed_time(y) for x, y in kern)))
    finally:
        L.call = real_call
    total = total[1:]
    return statistics.median(t for t, _ in total), statistics.median(k for _, k in total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--workers", type=int, default=4)
    args = ap.parse_args()
    L.require_gpu()
    sets = [(v, 1080, 1920, ext) for v in args.views for ext in ("jpg", "png")] + [(8, 3024, 4032, "jpg")]
    print("device loader vs host reference (load_images_and_cameras, images only), %d decode workers; ms" % args.workers)
    print("%-26s %9s %9s %9s %9s %9s %8s" % ("set", "host ref", "device", "decode", "up+kern", "kernels", "speedup"))
    with tempfile.TemporaryDirectory() as tmp:
        for views, h, w, ext in sets:
            folder = os.path.join(tmp, "%d_%dx%d_%s" % (views, w, h, ext))
            write_frames(folder, views, h, w, ext, seed=views + h)
            t = time.perf_counter()
            ref = lo.load_images_and_cameras(folder)[0]
            host_ms = 1e3 * (time.perf_counter() - t)
            got = preprocess.load_images_and_cameras(folder, workers=args.workers)[0]
            assert torch.equal(got.cpu(), ref), folder
            dev_ms = median_ms(lambda: preprocess.load_images_and_cameras(folder, workers=args.workers))
            paths = sorted(os.path.join(folder, f) for f in os.listdir(folder))
            dec_ms = median_ms(lambda: list(preprocess._decode_ordered(paths, args.workers)))
            up_ms, k_ms = device_part(folder, args.workers)
            name = "%2d x %dx%d %s" % (views, w, h, ext.upper())
            print("%-26s %9.1f %9.1f %9.1f %9.2f %9.3f %7.1fx" % (name, host_ms, dev_ms, dec_ms, up_ms, k_ms, host_ms / dev_ms))
            sys.stdout.flush()
    print("every device result equals the host reference bit for bit")


if __name__ == "__main__":
    main()
