"""CPU: the staging blobs of `BatchPlan` and `PatchPlan` are, byte for byte, what tests/golden/staging_blobs.npz recorded
before the two plans were put on data/device_staging.py: descriptors, pool, sizes, part offsets and the whole filled blob."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_staging_fixture", os.path.join(GOLDEN, "make_staging_fixture.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


MAKER = _maker()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "staging_blobs.npz"))


@pytest.mark.parametrize("name", list(MAKER.BATCH_CASES) + list(MAKER.PATCH_CASES))
def test_blob_bytes_equal_the_recorded_ones(golden, name):
    got = MAKER.record(MAKER.make_plan(name))
    assert sorted(k for k in golden.files if k.startswith(name + "/")) == sorted(name + "/" + k for k in got)
    for key, value in got.items():
        want = golden[name + "/" + key]
        assert want.dtype == np.asarray(value).dtype and np.array_equal(want, value), key
