"""Files and rectangles shared by tests/test_jpeg_pixels_cpu.py and tests/test_jpeg_pixels_gpu.py: JPEG files written
in-test with PIL over sampling layouts, qualities, content and sizes, plus the byte strings stored in
tests/golden/jpeg_coefficients.npz (optimised tables, restart markers, odd sizes)."""
import io
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_coefficients.npz")

LAYOUTS = ("420", "422", "444", "gray")
QUALITIES = (1, 10, 50, 75, 90, 100)
CONTENTS = ("noise", "smooth", "saturated")
# (width, height).  The first twelve, each pair in both orientations: a chroma component of 2 samples or fewer across takes
# libjpeg's replication rule, where the triangle filter would give other bytes (tests/test_jpeg_pixels_cpu.py pins at
# which of these sizes), next to sizes whose component is 3 or 5 across and takes the filter; 1x1 and one-MCU images
SMALL_SIZES = ((1, 1), (2, 2), (5, 1), (1, 5), (5, 2), (2, 5), (3, 4), (4, 3), (9, 2), (2, 9), (2, 3), (3, 2))
SIZES = SMALL_SIZES + ((8, 9), (16, 16), (17, 33), (37, 53), (50, 31), (300, 300))


def content(kind, height, width, seed=0):
    rng = np.random.RandomState(seed + 131 * height + width)
    if kind == "noise":
        return rng.randint(0, 256, (height, width, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "smooth":
        return np.stack([yy * 255 // max(height - 1, 1), xx * 255 // max(width - 1, 1),
                         (yy + xx) * 255 // max(height + width - 2, 1)], axis=-1).astype(np.uint8)
    # saturated: full-scale primaries in stripes and checks, which overshoot 0..255 after quantisation
    img = np.zeros((height, width, 3), dtype=np.uint8)
    img[::2, :, 0] = 255
    img[:, ::3, 2] = 255
    img[height // 2:, :, 1] = 255
    img[(yy + xx) % 5 == 0] = 255
    return img


def write_jpeg(pixels, layout, quality, **kwargs):
    from PIL import Image
    image = Image.fromarray(pixels)
    if layout == "gray":
        image = image.convert("L")
    else:
        kwargs["subsampling"] = {"444": 0, "422": 1, "420": 2}[layout]
    buf = io.BytesIO()
    image.save(buf, "JPEG", quality=quality, **kwargs)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as image:
        return np.array(image.convert("RGB"), dtype=np.uint8)


def jpeg_case(layout, quality, kind, size, **kwargs):
    width, height = size
    return write_jpeg(content(kind, height, width), layout, quality, **kwargs)


def golden_jpegs():
    """name -> bytes of the stored files the pixel reconstruction covers (every one but the progressive file)."""
    gold = np.load(GOLD)
    return {k.split("/")[0]: gold[k].tobytes() for k in sorted(gold.files) if k.endswith("/jpeg")}


def rectangles(height, width):
    """(ya, yb, xa, xb): the whole image, rectangles that start at odd coordinates, lie inside one MCU, are 1 x 1, and
    touch the bottom / right edge -- those that fit the image, without duplicates."""
    cand = [(0, height, 0, width), (1, height, 1, width), (1, min(4, height), 3, min(6, width)),
            (height // 2, height // 2 + 1, width // 2, width // 2 + 1), (height - 1, height, width - 1, width),
            (max(height - 9, 0), height, max(width - 11, 0), width), (3, min(14, height), 5, min(30, width)),
            (0, 1, 0, width), (0, height, width - 1, width), (17, min(40, height), 15, min(34, width))]
    out = []
    for r in cand:
        if 0 <= r[0] < r[1] <= height and 0 <= r[2] < r[3] <= width and r not in out:
            out.append(r)
    return out
