"""Generates tests/golden/staging_blobs.npz: the staging blobs of `BatchPlan` (data/image_prep.py) and `PatchPlan`
(data/patch_resize.py) for small ragged batches, byte for byte, as this package laid them out BEFORE the two plans were
put on one staging base.  tests/test_staging_cpu.py holds the refactored classes to these bytes, so run this maker only
at a commit whose layout is the one to pin:

    python tests/golden/make_staging_fixture.py

Per case `<name>/`: `desc` (the descriptor array as bytes), `pool`, `nbytes`, `scratch_bytes`, `src_bytes`, `offsets`
(pool, src and the optional part: `ops_offset` of a BatchPlan, `photo_offset` of a PatchPlan, -1 where there is none) and
`blob`: `fill()` into an `np.zeros` buffer, so the padding between the parts is zero.  The inputs are not stored:
`images()`, `BATCH_CASES` and `PATCH_CASES` below are imported by the test.

Cases: three images (30x40, 40x30, 24x24).  BatchPlan at target 24: scale with a nonzero offset and a flip, scale without
a flip, scale off; without and with photometric operation lists.  PatchPlan at 20x12 (height x width): a window inside the
image, mirrored, BICUBIC; one that starts at negative coordinates and runs past both far edges, NEAREST; one that misses
the image, LANCZOS; and a second batch whose first window has the size of the output (identity taps on both axes); each
without and with photometric records."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "staging_blobs.npz")
SHAPES = [(30, 40), (40, 30), (24, 24)]
TARGET = 24
OUT_H, OUT_W = 20, 12
F = np.float32

PARAMS = [(True, 3, True), (True, 0, False), (False, 0, False)]
OPS = [[(1, 0.7), (4, (0.1, -0.2, 0.3))], [], [(3, 1.3), (2, 0.6)]]
BATCH_CASES = {"batch/plain": None, "batch/ops": OPS}

WINDOWS = [(4, 6, 18, 22, True, 3, (1, 2, 3)), (-5, -7, 60, 50, False, 0, (200, 100, 50)), (40, 0, 9, 11, False, 1, (7, 8, 9))]
IDENTITY = [(2, 5, OUT_H, OUT_W, False, 2, (0, 0, 0))] + WINDOWS[1:]
RECORDS = [(1, F(5), None, None, None, (0, 1, 2)), (2, None, F(0.75), F(1.5), None, (2, 1, 0)), (1, None, None, None, F(9), (0, 1, 2))]
PATCH_CASES = {"patch/plain": (WINDOWS, None), "patch/photo": (WINDOWS, RECORDS),
               "patch_identity/plain": (IDENTITY, None), "patch_identity/photo": (IDENTITY, RECORDS)}


def images():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SHAPES]


def make_plan(name):
    from jpeg_detection_resnet_ssd_amd.data.image_prep import BatchPlan
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    if name in BATCH_CASES:
        return BatchPlan(SHAPES, PARAMS, TARGET, ops=BATCH_CASES[name])
    windows, records = PATCH_CASES[name]
    return PatchPlan(SHAPES, windows, OUT_H, OUT_W, records)


def record(plan):
    """Everything the fixture pins of one plan, as arrays."""
    blob = np.zeros(plan.nbytes, dtype=np.uint8)
    plan.fill(blob, images())
    extra = plan.ops_offset if hasattr(plan, "ops_offset") else plan.photo_offset
    return {"desc": plan.desc.view(np.uint8).copy(), "pool": plan.pool, "nbytes": np.int64(plan.nbytes),
            "scratch_bytes": np.int64(plan.scratch_bytes), "src_bytes": np.int64(plan.src_bytes),
            "offsets": np.array([plan.pool_offset, plan.src_offset, -1 if extra is None else extra], dtype=np.int64),
            "blob": blob}


def main():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    data = {}
    for name in list(BATCH_CASES) + list(PATCH_CASES):
        for key, value in record(make_plan(name)).items():
            data[name + "/" + key] = value
    np.savez_compressed(OUT, **data)
    print("%d cases, %d bytes -> %s" % (len(BATCH_CASES) + len(PATCH_CASES), os.path.getsize(OUT), OUT))


if __name__ == "__main__":
    main()
