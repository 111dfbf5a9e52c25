"""Generates tests/golden/ssd_augment.npz by IMPORTING the reference's own localisation_part/data_generator modules
(data_augmentation_chain_original_ssd.py, object_detection_2d_geometric_ops.py and what they import) and running their
`SSDExpand`, `SSDRandomCrop`, `RandomFlip` and `ResizeRandomInterp` on small seeded images with `np.random` seeded per
case.  The outputs are data: the inputs, the pixels that reached the resize, the interpolation code drawn and the boxes
that came out.

    python tests/golden/make_ssd_augment_fixture.py <root of the reference checkout>     (or DJ_REFERENCE_ROOT)

The modules import cv2, which is not installed here; it is stubbed in `sys.modules`: the five interpolation codes, and a
`resize` that RECORDS the image and the code it was handed and returns zeros of the requested size (the resize itself is
the one stage this package does not take from OpenCV).

Groups: `full/*` expand, crop, flip, resize to 24 x 20 (height x width); `nocrop/*` flip and resize, the sequence of
data_augmentation_chain_original_ssd_no_crop.py without its photometric stage; `resize/*` `Resize` alone, once per
interpolation code.  Images have sides 20..64, odd ones included, and 1..4 integer boxes (every fourth case as float64)."""
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssd_augment.npz")
OUT_H, OUT_W = 24, 20
N_FULL, N_NOCROP = 40, 10


def load_reference(root):
    calls = []
    try:
        import cv2  # noqa: F401
        raise SystemExit("cv2 is installed: this maker is written for the stub that records what the resize is handed")
    except ImportError:
        cv2 = types.ModuleType("cv2")
        for code, name in enumerate(("INTER_NEAREST", "INTER_LINEAR", "INTER_CUBIC", "INTER_AREA", "INTER_LANCZOS4")):
            setattr(cv2, name, code)

        def resize(image, dsize, interpolation=1):
            calls.append((np.array(image, dtype=np.uint8, copy=True), int(interpolation)))
            return np.zeros((dsize[1], dsize[0]) + image.shape[2:], dtype=image.dtype)
        cv2.resize = resize
        sys.modules["cv2"] = cv2
    if not hasattr(np, "bool"):
        np.bool = bool          # the reference predates its removal
    sys.path.insert(0, os.path.join(root, "localisation_part"))
    from data_generator import data_augmentation_chain_original_ssd as chain
    from data_generator import object_detection_2d_geometric_ops as geo
    return chain, geo, calls


def picture(rng, h, w):
    """Every pixel tells its position (two ramps) over 4 x 4 noise patches: a shifted, mirrored or mis-cropped copy differs."""
    yy, xx = np.mgrid[0:h, 0:w]
    noise = np.kron(rng.integers(0, 64, (-(-h // 4), -(-w // 4), 3)), np.ones((4, 4, 1), dtype=np.int64))[:h, :w]
    img = np.stack([3 * yy + noise[..., 0], 3 * xx + noise[..., 1], 2 * (xx + yy) + noise[..., 2]], axis=-1)
    return (img % 256).astype(np.uint8)


def boxes(rng, h, w, as_float):
    rows = []
    for _ in range(int(rng.integers(1, 5))):
        bw, bh = int(rng.integers(3, max(4, w // 2))), int(rng.integers(3, max(4, h // 2)))
        x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
        rows.append([int(rng.integers(1, 21)), x0, y0, x0 + bw, y0 + bh])
    return np.array(rows, dtype=np.float64 if as_float else np.int64)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DJ_REFERENCE_ROOT")
    if not root:
        sys.exit(__doc__)
    chain, geo, calls = load_reference(root)
    rng = np.random.default_rng(2025)
    data, names = {}, []

    def add(name, seed, sequence, h, w, as_float):
        image, labels = picture(rng, h, w), boxes(rng, h, w, as_float)
        del calls[:]
        np.random.seed(seed)
        out, out_labels = image, labels
        for transform in sequence:
            out, out_labels = transform(out, out_labels)
        assert len(calls) == 1 and out.shape == (OUT_H, OUT_W, 3)
        names.append(name)
        data[name + "/seed"] = np.int64(seed)
        data[name + "/image"], data[name + "/labels"] = image, labels
        data[name + "/pre_resize"], data[name + "/interpolation"] = calls[0][0], np.int64(calls[0][1])
        data[name + "/out_labels"] = out_labels

    def side(i):
        return int((20, 21, 33, 47, 64, 57, 40, 25)[i % 8] if i < 8 else rng.integers(20, 65))

    for i in range(N_FULL):
        sequence = [chain.SSDExpand(), chain.SSDRandomCrop(), geo.RandomFlip(dim='horizontal', prob=0.5),
                    geo.ResizeRandomInterp(height=OUT_H, width=OUT_W)]
        add("full/%02d" % i, 1000 + i, sequence, side(i), side(i + 3), i % 4 == 3)
    for i in range(N_NOCROP):
        sequence = [geo.RandomFlip(dim='horizontal', prob=0.5), geo.ResizeRandomInterp(height=OUT_H, width=OUT_W)]
        add("nocrop/%02d" % i, 2000 + i, sequence, side(i + 1), side(i + 5), i % 4 == 3)
    for code in range(5):
        add("resize/%d" % code, 3000 + code, [geo.Resize(height=OUT_H, width=OUT_W, interpolation_mode=code)],
            side(code + 2), side(code), code == 3)

    data["names"] = np.array(names)
    data["out_size"] = np.array([OUT_H, OUT_W])
    np.savez_compressed(OUT, **data)
    expanded = sum(data[n + "/pre_resize"].shape[0] > data[n + "/image"].shape[0] for n in names)
    print("%d cases (%d of them expanded), %d bytes -> %s" % (len(names), expanded, os.path.getsize(OUT), OUT))


if __name__ == "__main__":
    main()
