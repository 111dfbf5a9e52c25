"""The batch shared by tests/test_classifier_decode_cpu.py and tests/test_classifier_decode_gpu.py: JPEG files written with
PIL at the smallest sizes that still exercise the edges -- baseline gray, 4:4:4, 4:2:2, 4:2:0, one file with optimised
tables, all of which travel as `CoefficientImage`s, and one progressive file, which falls back to Pillow -- and the
directory trees the two classifier pipelines read them from (the RGB iterator's also holds a PNG of the target's size)."""
import io
import json
import os

import numpy as np

import jpeg_pixels_cases as C

# (name, layout, (width, height), quality, content, save arguments); 17 x 23 is no multiple of an MCU in any layout
FILES = (("gray", "gray", (1, 1), 90, "noise", {}),
         ("f444", "444", (7, 5), 75, "saturated", {}),
         ("f422", "422", (16, 16), 50, "noise", {}),
         ("f420", "420", (17, 23), 90, "smooth", {}),
         ("optimised", "420", (40, 33), 75, "noise", {"optimize": True}),
         ("progressive", "420", (17, 23), 90, "noise", {"progressive": True}))
BASELINE = [k for k, f in enumerate(FILES) if "progressive" not in f[5]]      # the items that must travel as coefficients
TARGET = 16                 # of the DCT generators' `BatchPlan`
RGB_TARGET = (12, 20)       # (height, width) of the RGB iterator
CLASSES = {"0": ["n_cat", "cat"], "1": ["n_dog", "dog"], "2": ["n_eel", "eel"]}


def files():
    """[(name, bytes)] in the order of FILES."""
    return [(name, C.jpeg_case(layout, quality, kind, size, **kw)) for name, layout, size, quality, kind, kw in FILES]


def items(jp):
    """-> (bytes, the items as a `device_decode` generator hands them over, Pillow's pixels) of the shared batch."""
    data = [d for _, d in files()]
    arrays = [C.pillow_pixels(d) for d in data]
    mixed = [jp.CoefficientImage(d) if jp.decodable(d) else a for d, a in zip(data, arrays)]
    return data, mixed, arrays


def coefficient_items(images):
    """The positions of a batch that hold `CoefficientImage`s."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    return [i for i, im in enumerate(images) if isinstance(im, CoefficientImage)]


def write_tree(root, png=False):
    """The shared files in three class directories under `root`/train, named so that sorted order is the order of FILES,
    and (`png`) a PNG of RGB_TARGET's size behind them -> (directory, index file)."""
    from PIL import Image
    train = os.path.join(root, "train")
    for k, (name, data) in enumerate(files()):
        directory = os.path.join(train, CLASSES[str(k % 3)][0])
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "img%d_%s.jpg" % (k, name)), "wb") as f:
            f.write(data)
    if png:
        pixels = C.content("noise", RGB_TARGET[0], RGB_TARGET[1], seed=9)
        buf = io.BytesIO()
        Image.fromarray(pixels).save(buf, "PNG")
        with open(os.path.join(train, CLASSES["0"][0], "img6_same_size.png"), "wb") as f:
            f.write(buf.getvalue())
    index_file = os.path.join(root, "index.json")
    with open(index_file, "w") as f:
        json.dump(CLASSES, f)
    return train, index_file
