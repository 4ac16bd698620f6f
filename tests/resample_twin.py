"""numpy restatement of Pillow's 8-bit BICUBIC resize (Image.resize(size, Image.Resampling.BICUBIC) on RGB), written from the published
rules of Pillow's Resample.c and independent of the product's table code (omnivggt_official_amd/preprocess.py). Like
tests/pointcloud_twin.py it is the yardstick the product is compared against on the host, and it is itself checked against PIL.

Rules (per axis (in -> out), separable, horizontal pass first, each pass writes uint8; a pass runs only if its axis changes size):
  filter (a = -0.5, support 2)  |x| < 1: ((a+2)|x| - (a+3))|x|^2 + 1;  |x| < 2: (((|x|-5)|x| + 8)|x| - 4) a;  else 0
  scale = in/out, fs = max(scale, 1), support = 2 fs, ksize = 2 ceil(support) + 1
  output i: center = (i + 0.5) scale, xmin = max(int(center - support + 0.5), 0) (C truncation),
            n = min(int(center + support + 0.5), in) - xmin, w[j] = filter((j + xmin - center + 0.5) * (1 / fs)), j < n
            normalised by their left-to-right sum (kept when the sum is 0)
  fixed point: k = int(w 2^22 + 0.5) for w >= 0, int(w 2^22 - 0.5) otherwise (truncation)
  pass: acc = 2^21 + sum src * k in int32, out = clamp(acc >> 22, 0, 255)
"""
import math

import numpy as np

PB = 22

# (source (h, w), output (width, height)) of the tests: identity, one axis only, upscale, x8 downscale, 1-pixel sources, odd sizes,
# portrait, landscape camera and phone frames
GEOMETRIES = [((392, 518), (518, 392)), ((392, 700), (518, 392)), ((400, 518), (518, 392)), ((288, 512), (518, 294)),
              ((23, 37), (518, 322)), ((2048, 4144), (518, 256)), ((50, 1), (518, 700)), ((1, 50), (7, 3)), ((333, 517), (519, 331)),
              ((640, 480), (518, 686)), ((480, 640), (518, 392)), ((1080, 1920), (518, 294)), ((3024, 4032), (518, 392))]


def _filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """-> (xmin int64 [out], n int64 [out], k int64 [out, ksize]) of the rules above (scalar Python, one output at a time)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    inv = 1.0 / fs
    xmin = np.zeros(out_size, np.int64)
    n = np.zeros(out_size, np.int64)
    k = np.zeros((out_size, ksize), np.int64)
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - lo
        w = [_filter((j + lo - center + 0.5) * inv) for j in range(cnt)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        for j, v in enumerate(w):
            k[i, j] = int(v * (1 << PB) + 0.5) if v >= 0 else int(v * (1 << PB) - 0.5)
        xmin[i], n[i] = lo, cnt
    return xmin, n, k


def _pass(src, in_size, out_size, axis):
    """One pass over `axis` (0: rows / vertical, 1: columns / horizontal) of an (H, W, 3) uint8 array."""
    xmin, n, k = coeffs(in_size, out_size)
    a = np.moveaxis(src.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i in range(out_size):
        acc = np.full(a.shape[1:], 1 << (PB - 1), np.int64)
        for j in range(n[i]):
            acc += a[xmin[i] + j] * k[i, j]
        assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)          # Pillow accumulates in int32
        out[i] = np.clip(acc >> PB, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(src, size):
    """Image.fromarray(src).resize(size, BICUBIC) for an (H, W, 3) uint8 array; size = (width, height)."""
    w, h = size
    out = np.ascontiguousarray(src)
    if w != src.shape[1]:
        out = _pass(out, src.shape[1], w, 1)
    if h != src.shape[0]:
        out = _pass(out, src.shape[0], h, 0)
    return out.copy()


def test_image(h, w, seed):
    """Seeded noise with full-scale 0 / 255 stripes in both directions, so the negative lobes of the filter clamp."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[:, ::7] = 0
    a[:, 3::7] = 255
    a[::5] = 255
    a[2::5] = 0
    return a
