"""Fixture for resize + crop + flip of decoded images (data/image_prep.py:prep_host, csrc/dj_imgprep.hip): for each case a
small uint8 source image (numpy only, seeded), its parameters (target_length, scale, offset, flip, Pillow resampling
code), and what the INSTALLED Pillow makes of them -- `Image.fromarray(src).resize(size, resample).crop(box)` and, when the
flip is set, `.transpose(FLIP_LEFT_RIGHT)`, with `size` and `box` computed as the reference's classifier generators do
(classification_part/vgg_jpeg_keras/generators/generators.py:145-167) -- plus that Pillow's version string.

The cases cover up-scaling, down-scaling by 1.1 to more than 8, an unchanged dimension, 1x1 and 2x3 sources, offsets at both
ends of their range, both flip states and the two required filters, on noise, smooth and saturated content.

The file lets the GPU tests run where Pillow is absent.  Where the installed Pillow is of another version than the one
recorded here, the fixture is the contract: the kernel and the host twin are held to these bytes.

    python tests/golden/make_image_prep_fixture.py      # rewrites tests/golden/image_prep.npz"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "image_prep.npz")
BILINEAR, BICUBIC = 2, 3

# name: (height, width, content, target_length, scale, offset ("min" | "mid" | "max"), flip, resample)
CASES = {
    "down1p1_noise_bicubic": (100, 130, "noise", 91, True, "max", True, BICUBIC),
    "down1p1_noise_bilinear": (90, 110, "noise", 82, True, "min", False, BILINEAR),
    "down2_smooth_bicubic": (160, 200, "smooth", 80, True, "mid", False, BICUBIC),
    "down3p1_saturated_bilinear": (130, 170, "saturated", 42, True, "max", True, BILINEAR),
    "down9p4_noise_bicubic": (160, 200, "noise", 17, True, "min", True, BICUBIC),
    "down5_portrait_smooth_bilinear": (200, 90, "smooth", 18, True, "max", False, BILINEAR),
    "down5_portrait_saturated_bicubic": (200, 90, "saturated", 18, True, "min", True, BICUBIC),
    "up3p2_noise_bicubic": (20, 30, "noise", 64, True, "max", False, BICUBIC),
    "up2p9_portrait_noise_bilinear": (31, 17, "noise", 50, True, "max", True, BILINEAR),
    "unchanged_height_noise_bicubic": (64, 120, "noise", 64, False, "min", True, BICUBIC),
    "unchanged_both_smooth_bilinear": (48, 100, "smooth", 48, True, "max", False, BILINEAR),
    "squash_saturated_bicubic": (90, 160, "saturated", 56, False, "min", False, BICUBIC),
    "square_saturated_bilinear": (100, 100, "saturated", 37, True, "min", True, BILINEAR),
    "one_pixel_bicubic": (1, 1, "noise", 8, True, "min", False, BICUBIC),
    "two_by_three_bilinear": (2, 3, "noise", 7, True, "max", True, BILINEAR),
    "two_by_three_bicubic": (2, 3, "noise", 7, True, "min", False, BICUBIC),
}


def source(name, height, width, content):
    rng = np.random.default_rng(sum(name.encode()) * 7919 + height * 131 + width)
    if content == "noise":
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    if content == "smooth":
        coarse = rng.integers(0, 256, (-(-height // 8) + 2, -(-width // 8) + 2, 3)).astype(np.int64)
        fine = np.kron(coarse, np.ones((8, 8, 1), dtype=np.int64))
        for axis in (0, 1):                     # two box blurs of 8 along each axis
            for _ in range(2):
                c = np.cumsum(fine, axis=axis)
                lead = np.take(c, range(8, c.shape[axis]), axis=axis) - np.take(c, range(0, c.shape[axis] - 8), axis=axis)
                fine = lead // 8
        return fine[:height, :width].astype(np.uint8)
    if content == "saturated":                  # 0 / 255 patches: the bicubic overshoot meets clip8 on both sides
        coarse = rng.integers(0, 2, (-(-height // 5), -(-width // 5), 3)).astype(np.uint8) * 255
        img = np.kron(coarse, np.ones((5, 5, 1), dtype=np.uint8))[:height, :width]
        speckle = rng.random((height, width)) < 0.05
        img[speckle] = rng.integers(0, 256, (int(speckle.sum()), 3), dtype=np.uint8)
        return np.ascontiguousarray(img)
    raise ValueError(content)


def geometry(height, width, target, scale, where):
    """-> (resize size (w, h), crop box, offset), written out as the reference's generator computes them."""
    if not scale:
        return (target, target), (0, 0, target, target), 0
    ratio = target / min(width, height)
    rw, rh = int(round(width * ratio)), int(round(height * ratio))
    top = max(rw, rh) - target
    offset = {"min": 0, "mid": top // 2, "max": top}[where]
    box = (offset, 0, target + offset, target) if rw > rh else (0, offset, target, target + offset)
    return (rw, rh), box, offset


def make_cases():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array(sorted(CASES))}
    for name, (h, w, content, target, scale, where, flip, resample) in CASES.items():
        src = source(name, h, w, content)
        size, box, offset = geometry(h, w, target, scale, where)
        im = Image.fromarray(src).resize(size, resample).crop(box)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out[name + "/src"] = src
        out[name + "/params"] = np.array([target, int(scale), offset, int(flip), resample], dtype=np.int32)
        out[name + "/out"] = np.asarray(im)
    return out


if __name__ == "__main__":
    cases = make_cases()
    np.savez(PATH, **cases)
    print("wrote", PATH, os.path.getsize(PATH), "bytes, Pillow", cases["pillow_version"])
