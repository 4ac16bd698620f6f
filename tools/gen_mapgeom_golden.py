"""tests/golden/mapgeom_reference.npz from the REAL reference pts3d_to_trimesh (reference tree only; no test runs this).

    python tools/gen_mapgeom_golden.py /path/to/reference/checkout [--out tests/golden/mapgeom_reference.npz]

Loads omnivggt/viz.py of the checkout (its imports of PIL, scipy, trimesh and the package's own utilities, none of which the
triangulation uses, are stubbed where they do not import), runs pts3d_to_trimesh(img, pts3d, valid) on two small seeded maps with
validity masks (5 x 7 and 12 x 9) and records the inputs with the reference's faces as sorted pixel triples, duplicates removed (the
reference emits every triangle twice, once backward). Before writing it asserts that tests/mapgeom_twin.py, with the tear test off
and keep = valid, emits exactly that set of pixel triples: that is why the diagonal of a quad is b-c. Data only, a few KB.
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
STUBBED = ("PIL", "PIL.Image", "scipy", "scipy.spatial", "scipy.spatial.transform", "trimesh", "omnivggt", "omnivggt.utils",
           "omnivggt.utils.geometry", "omnivggt.utils.device", "omnivggt.utils.image")


def scene(H, W, seed):
    """A bumpy surface in front of the camera, a colour image and a validity mask with holes, a dead row segment and a dead corner."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    z = (2.0 + 0.1 * x + 0.05 * y + rng.uniform(0.0, 0.2, (H, W))).astype(F)
    pts = np.stack([(x - W / 2) * z / 8, (y - H / 2) * z / 8, z], -1).astype(F)
    img = rng.uniform(0.0, 1.0, (H, W, 3)).astype(F)
    valid = rng.uniform(0.0, 1.0, (H, W)) > 0.2
    valid[H // 2, : W // 2] = False
    valid[0, 0] = valid[H - 1, W - 1] = False
    return img, pts, valid


def _stub_attribute(attr):
    if attr.startswith("__"):
        raise AttributeError(attr)
    return object                                                             # any name a `from ... import` of the module asks for


def load_viz(reference):
    for name in STUBBED:
        try:
            importlib.import_module(name)
        except Exception:                                                     # not installed here, or the package's own import chain fails
            stub = types.ModuleType(name)
            stub.__path__ = []
            stub.__getattr__ = _stub_attribute
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("reference_viz", os.path.join(reference, "omnivggt", "viz.py"))
    viz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(viz)
    return viz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mapgeom_reference.npz"))
    a = ap.parse_args()
    import mapgeom_twin as twin
    viz = load_viz(a.reference)
    out = {}
    for name, H, W, seed in (("small", 5, 7, 21), ("large", 12, 9, 22)):
        img, pts, valid = scene(H, W, seed)
        mesh = viz.pts3d_to_trimesh(img, pts, valid=valid)
        assert mesh["vertices"].shape == (H * W, 3) and (mesh["vertices"] == pts.reshape(-1, 3)).all()      # vertex = pixel, in pixel order
        want = twin.pixel_triples(mesh["faces"])
        assert len(want) * 2 == len(mesh["faces"]) and 0 < len(want) < 2 * (H - 1) * (W - 1), (name, len(want))
        z = twin.map_depth(depth=pts[None, ..., 2])
        pix, emitted = twin.quad_faces(z, pts[None], keep=valid[None], rel_tol=np.inf)
        mine = twin.pixel_triples(pix[emitted])
        assert mine.shape == want.shape and (mine == want).all(), (name, mine.shape, want.shape)
        out[name + "_img"], out[name + "_pts"], out[name + "_valid"] = img, pts, valid
        out[name + "_triples"] = want.astype(np.int16)
    np.savez_compressed(a.out, **out)
    print("%s: %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
