"""Fixtures for the RGB -> JPEG-DCT transform (data/jpeg_dct.py:rgb_to_dct_host, csrc/dj_rgb2dct.hip): for each case
the uint8 RGB array and the JPEG bytes PIL wrote for it (`Image.fromarray(x).save(f, format="jpeg", quality=q)`, the
reference's emission path), stored in tests/golden/rgb_dct.npz.  The expected coefficients are NOT stored: the tests
get them from the committed bytes through the in-tree coefficient reader (itself pinned to libjpeg by
jpeg_coefficients.npz), so a test machine needs neither PIL nor a live encode.  Needs PIL and numpy only:

    python tests/golden/make_rgb_dct_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


def smooth(h, w, seed):
    """Coarse random patches over a horizontal ramp (rows repeat in runs of six, so the array compresses)."""
    rng = np.random.default_rng(seed)
    patches = np.kron(rng.uniform(30, 225, (h // 6 + 1, w // 6 + 1, 3)), np.ones((6, 6, 1)))[:h, :w]
    ramp = (np.arange(w) * 60.0 / max(w - 1, 1) - 30.0)[None, :, None]
    return np.clip(patches + ramp, 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def saturated(h, w, seed):
    """0 / 255 only, in patches of a few pixels with single pixels flipped: the largest coefficients there are."""
    rng = np.random.default_rng(seed)
    coarse = np.kron(rng.integers(0, 2, (h // 5 + 1, w // 5 + 1, 3)), np.ones((5, 5, 1), dtype=np.int64))[:h, :w]
    flip = rng.random((h, w, 3)) < 0.03
    return (np.where(flip, 1 - coarse, coarse) * 255).astype(np.uint8)


# name: (image, quality).  Noise does not compress: one full-size noise image, the other noise cases small.
CASES = {
    "smooth_300x300_q75": (smooth(300, 300, 1), 75),          # the SSD trainer's emission
    "patches_300x300_q75": (smooth(300, 300, 13), 75),        # a second trainer-sized image: batches of two
    "noise_300x300_q30": (noise(300, 300, 2), 30),
    "saturated_300x300_q90": (saturated(300, 300, 3), 90),
    "smooth_224x224_q75": (smooth(224, 224, 4), 75),          # the classifier's
    "smooth_301x299_q75": (smooth(301, 299, 5), 75),          # odd height: the last row pairs with itself
    "smooth_296x300_q75": (smooth(296, 300, 6), 75),          # 8 of 16 rows in the last MCU
    "noise_37x53_q75": (noise(37, 53, 7), 75),
    "noise_17x16_q75": (noise(17, 16, 8), 75),
    "noise_8x8_q75": (noise(8, 8, 9), 75),
    "noise_1x1_q100": (noise(1, 1, 10), 100),
    "noise_300x20_q50": (noise(300, 20, 11), 50),             # 12 of 16 rows: the last AVERAGED chroma row is replicated
    "noise_15x33_q10": (noise(15, 33, 12), 10),
}


def main():
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    store = {}
    for name, (img, quality) in CASES.items():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="jpeg", quality=quality)
        data = buf.getvalue()
        planes = j2d.loads(data)          # a case the reader cannot take fails the script
        inf = j2d.info(data)
        assert inf.n_components == 3 and (inf.h_samp[0], inf.v_samp[0], inf.h_samp[1], inf.v_samp[1]) == (2, 2, 1, 1), name
        store[name + "/rgb"] = img
        store[name + "/jpeg"] = np.frombuffer(data, np.uint8)
        store[name + "/quality"] = np.int32(quality)
        print(name, img.shape, "q%d" % quality, len(data), "bytes", [p.shape for p in planes])
    path = os.path.join(OUT, "rgb_dct.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
