"""What tests/test_coefficient_inputs_cpu.py and tests/test_coefficient_inputs_gpu.py share: files written in-test with PIL
(content and writers of tests/jpeg_pixels_cases.py), hand-made planes whose de-quantised product leaves int16, a four-line
restatement of the mirror, and the directory tree the generators read."""
import json
import os
import random

import numpy as np

import jpeg_pixels_cases as C

CLASSES = {"0": ["n_cat", "cat"], "1": ["n_dog", "dog"], "2": ["n_eel", "eel"]}
# (height, width) of the tree's files, in sorted path order: class n_cat holds files 0 and 3, n_dog 1 and 4, n_eel 2 and 5
TREE_SIZES = ((48, 64), (32, 32), (40, 56), (64, 48), (33, 47), (48, 48))
TREE_GRAY = 3


def jpeg(height, width, quality=75, kind="noise", layout="420", seed=0, **kw):
    return C.write_jpeg(C.content(kind, height, width, seed=seed), layout, quality, **kw)


def wrap_planes():
    """-> (planes [(2, 2, 64), (1, 1, 64), (1, 1, 64)] int16, tables (3, 64) int32): every extreme of int16 against table
    entries that take the product out of int16 -- 32767 * 255, -32768 * 2, -32768 * 1 (whose mirror negation wraps too),
    -1 * 255 -- on even and odd horizontal frequencies, the rest noise."""
    rng = np.random.RandomState(7)
    planes = [rng.randint(-2048, 2048, s).astype(np.int16) for s in ((2, 2, 64), (1, 1, 64), (1, 1, 64))]
    tables = rng.randint(1, 256, (3, 64)).astype(np.int32)
    for c, plane in enumerate(planes):
        flat = plane.reshape(-1, 64)
        flat[0, :8] = [32767, 32767, -32768, -32768, -32768, -32768, -1, 16384]
        tables[c, :8] = [255, 255, 2, 2, 1, 1, 255, 2]
        flat[-1, 56:] = [-32768, -32768, 32767, 32767, 12345, -12345, 129, -129]
        tables[c, 56:] = [1, 1, 3, 3, 255, 255, 254, 254]
    return planes, tables


def wrapped(plane, table):
    """The value rule restated: np.int16 wrap of the int32 product."""
    return (plane.astype(np.int64) * table.astype(np.int64)).astype(np.int32).astype(np.int16)


def mirror_restated(blocks):
    """(rows, cols, 64) -> jpegtran's horizontal flip, restated: column j takes column cols - 1 - j, odd v negated."""
    out = blocks[:, ::-1].reshape(blocks.shape[0], blocks.shape[1], 8, 8).copy()
    out[..., 1::2] = -out[..., 1::2]
    return out.reshape(blocks.shape)


def legal_origins(height, width, h, w):
    """Every (y0, x0) multiple of 16 at which an (h, w) window with h % 16 == w % 16 == 0 lies inside a 4:2:0 file."""
    return [(y0, x0) for y0 in range(0, height - h + 1, 16) for x0 in range(0, width - w + 1, 16)]


def write_tree(root, sizes=TREE_SIZES, gray=TREE_GRAY):
    """Six 4:2:0 files (one gray) of `sizes` in three class directories -> (directory, index file, paths in sorted order)."""
    train = os.path.join(root, "train")
    paths = []
    for k, (h, w) in enumerate(sizes):
        directory = os.path.join(train, CLASSES[str(k % 3)][0])
        os.makedirs(directory, exist_ok=True)
        paths.append(os.path.join(directory, "img%d.jpg" % k))
        with open(paths[-1], "wb") as f:
            f.write(jpeg(h, w, quality=90, kind="noise" if k % 2 else "smooth", layout="gray" if k == gray else "420", seed=k))
    index_file = os.path.join(root, "index.json")
    with open(index_file, "w") as f:
        json.dump(CLASSES, f)
    return train, index_file, sorted(paths)


def restated_draws(sizes, target, random_crop=True, flip=True):
    """What the generators draw for images of `sizes`, consuming `random` the same way -> [((y0, x0, T, T), mirror)]."""
    out = []
    for h, w in sizes:
        if random_crop:
            y0 = 16 * random.randint(0, h // 16 - target // 16)
            x0 = 16 * random.randint(0, w // 16 - target // 16)
        else:
            y0, x0 = 16 * ((h // 16 - target // 16) // 2), 16 * ((w // 16 - target // 16) // 2)
        out.append(((y0, x0, target, target), bool(flip and random.uniform(0, 1) > 0.5)))
    return out
