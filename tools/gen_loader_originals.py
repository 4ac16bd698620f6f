"""Write tests/golden/real/loader_originals.npz: original files behind the real-input fixtures of tests/golden/real/.

    python tools/gen_loader_originals.py

Runs only where the reference tree exists (oracle/ref_shim.py, read-only). It stores, byte for byte, some of the first 4 sorted images
of the reference's example/office and example/infinigen scenes (VIEWS below) and their camera .txt files, under keys
"<scene>/<subfolder>/<file name>" (uint8 arrays of the file bytes), and "<scene>/views": the positions of the stored images among the 4
views of the fixtures. The loaders treat every view on its own, so a subset pins the same arithmetic as all 4 views, and the frames
are the bulk of the bytes: all 4 views of both scenes with their depth maps took 3.7 MB.

The infinigen depth .npy files are not stored. Their 288 x 512 maps are upsampled to 294 x 518 by the nearest-neighbour resize, which
reads every source row and column, so tests/test_gpu_preprocess.py rebuilds each filtered map from infinigen_294_aux_inputs.npz.
tests/test_gpu_preprocess.py writes the files back into a temporary folder and runs the device loaders on them, which must reproduce
office_*.png, infinigen_*.png and the *_inputs.npz fixtures of the stored views bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "real", "loader_originals.npz")
VIEWS = {"office": [3], "infinigen": [0, 1]}          # about 0.7 MB of PNG bytes


def main():
    ex = os.path.join(ref_shim.REFERENCE_ROOT, "example")
    if not os.path.isdir(ex):
        raise SystemExit("reference example scenes not found under %s" % ex)
    files = {}
    for scene, views in VIEWS.items():
        images = sorted(os.listdir(os.path.join(ex, scene, "images")))[:4]
        files["%s/views" % scene] = np.array(views, np.int64)
        for v in views:
            stem = os.path.splitext(images[v])[0]
            for sub, name in (("images", images[v]), ("cameras", stem + ".txt")):
                with open(os.path.join(ex, scene, sub, name), "rb") as fh:
                    files["%s/%s/%s" % (scene, sub, name)] = np.frombuffer(fh.read(), np.uint8)
    np.savez_compressed(OUT, **files)
    print("wrote %s: %d entries, %.2f MB" % (OUT, len(files), os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
