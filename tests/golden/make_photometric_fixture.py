"""Generates tests/golden/photometric.npz by IMPORTING the reference's own
classification_part/vgg_jpeg_keras/generators/helper.py and calling its `saturation`, `brightness`, `contrast` and
`lighting` on small seeded uint8 images with `np.random` seeded per case.  The outputs are data: inputs, the draws each
call made (recovered by replaying the seed), and the bytes it returned.

    python tests/golden/make_photometric_fixture.py <root of the reference checkout>     (or DJ_REFERENCE_ROOT)

helper.py imports cv2 and two scipy.ndimage modules at the top that none of the four functions uses; whichever of them is
not installed is stubbed in `sys.modules` for the import.

Per function: sizes 1x1, 1x5, 8x16 (exactly one 128-element leaf of numpy's pairwise sum), 3x43 (129 pixels: the first
split), 24x40 and 33x47; content noise, all-white, all-black, r=g=b ramps (where one ulp of the grey value flips a
truncation) and 0/255 patches; seeds searched so that alpha lies near the low end, near the high end and in between.
Chains of two to four of saturation / brightness / contrast pass uint8 from one call to the next, as the generators do.
`probe/*` holds 4096 pixels and what `dot` made of them here, so that a test can tell whether the BLAS it runs on
evaluates the grey value in the same way.  `lighting/*` cases also hold the shift the call added and whether LAPACK's
eigenvector signs happened to follow the port's sign rule (data/photometric.py:fix_signs)."""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "photometric.npz")
SIZES = [(1, 1), (1, 5), (8, 16), (3, 43), (24, 40), (33, 47)]
CONTENTS = ["noise", "white", "black", "ramp", "patches"]
FUNCTIONS = ["saturation", "brightness", "contrast", "lighting"]
CHAINS = [("saturation", "brightness"), ("contrast", "saturation"), ("brightness", "contrast", "saturation"),
          ("contrast", "contrast"), ("saturation", "contrast", "brightness", "saturation"),
          ("brightness", "brightness", "contrast")]


def load_helper(root):
    for name, attrs in (("cv2", ()), ("scipy.ndimage.interpolation", ("map_coordinates",)),
                        ("scipy.ndimage.filters", ("gaussian_filter",))):
        try:
            importlib.import_module(name)
        except Exception:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
            for a in attrs:
                setattr(sys.modules[name], a, None)
    path = os.path.join(root, "classification_part", "vgg_jpeg_keras", "generators", "helper.py")
    spec = importlib.util.spec_from_file_location("reference_helper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def content(rng, kind, h, w):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == "black":
        return np.zeros((h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        v = ((np.arange(h * w) * 255) // max(h * w - 1, 1)).astype(np.uint8).reshape(h, w)
        return np.ascontiguousarray(np.stack([v, v, v], axis=-1))
    img = (rng.integers(0, 2, (-(-h // 4), -(-w // 4), 3)) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.kron(img, np.ones((4, 4, 1), dtype=np.uint8))[:h, :w])


def seed_for(where, start):
    """First seed >= start whose first uniform draw lies near the low end, near the high end, or anywhere."""
    s = start
    while True:
        np.random.seed(s)
        u = np.random.random()
        if where == "mid" or (where == "low" and u < 0.02) or (where == "high" and u > 0.98):
            return s
        s += 1


def replay(names, seed):
    """The draws the calls `names` make after np.random.seed(seed): alpha (one float) or randn(3) * 0.5, padded to 3."""
    np.random.seed(seed)
    out = np.zeros((len(names), 3))
    for i, name in enumerate(names):
        if name == "lighting":
            out[i] = np.random.randn(3) * 0.5
        else:
            alpha = 2 * np.random.random() * 0.5
            out[i, 0] = alpha + 1 - 0.5
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DJ_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    helper = load_helper(root)
    rng = np.random.default_rng(2024)
    data, names = {}, []

    def add(name, src, fns, seed):
        np.random.seed(seed)
        out = src
        for fn in fns:
            out = getattr(helper, fn)(out)
        assert out.dtype == np.uint8 and out.shape == src.shape
        names.append(name)
        data[name + "/src"], data[name + "/out"] = src, out
        data[name + "/ops"] = np.array([FUNCTIONS.index(fn) + 1 for fn in fns], dtype=np.int32)
        data[name + "/draws"] = replay(fns, seed)
        data[name + "/seed"] = np.int64(seed)
        if fns == ("lighting",):
            cov = np.cov(src.reshape(-1, 3) / 255.0, rowvar=False)
            eigval, eigvec = np.linalg.eigh(cov)
            data[name + "/shift"] = eigvec.dot(eigval * data[name + "/draws"][0]) * 255
            big = np.abs(eigvec).argmax(axis=0)
            data[name + "/signs_follow_rule"] = np.bool_((eigvec[big, np.arange(3)] >= 0).all())

    start = 0
    for fn in FUNCTIONS:
        for h, w in SIZES:
            if fn == "lighting" and h * w == 1:
                continue                   # one observation: np.cov is undefined and eigh raises
            for kind in CONTENTS:
                if kind != "noise" and (h, w) not in ((8, 16), (3, 43), (33, 47)):
                    continue
                for where in (("low", "high", "mid") if kind == "noise" else ("low", "high")[(h + len(kind)) % 2:][:1]):
                    seed = seed_for(where, start)
                    start = seed + 1
                    add("%s/%dx%d_%s_%s" % (fn, h, w, kind, where), content(rng, kind, h, w), (fn,), seed)
    for i, chain in enumerate(CHAINS):
        h, w = ((24, 40), (33, 47), (3, 43))[i % 3]
        kind = ("noise", "ramp")[i % 2]
        seed = seed_for(("low", "high", "mid")[i % 3], start)
        start = seed + 1
        add("chain/%d_%dx%d_%s" % (i, h, w, kind), content(rng, kind, h, w), chain, seed)

    probe = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    probe[:256] = np.arange(256, dtype=np.uint8)[:, None]          # every r=g=b value
    data["probe/pixels"] = probe
    data["probe/grey"] = helper.grayscale(probe.reshape(64, 64, 3)).reshape(-1)
    data["names"] = np.array(names)
    data["numpy_version"] = np.array(np.__version__)
    blas = "unknown"
    try:
        cfg = np.show_config(mode="dicts")["Build Dependencies"]["blas"]
        blas = "%s %s" % (cfg.get("name"), cfg.get("version"))
    except Exception:
        pass
    data["blas"] = np.array(blas)
    np.savez_compressed(OUT, **data)
    print("%d cases, %d bytes -> %s (numpy %s, %s)" % (len(names), os.path.getsize(OUT), OUT, np.__version__, blas))


if __name__ == "__main__":
    main()
