"""GPU: dj_jpeg_entropy_decode_chunked (csrc/dj_jpeg_entropy_chunked.hip) writes, byte for byte, the planes and statuses of
the contract -- `entropy_decode_host(data, scan_segments(data, unmarked=True))` -- for files without restart intervals at
every chunk size, alone, in mixed batches and for the corrupted copies of one file in one launch; touches nothing outside
the planes and its scratch; takes at most as many synchronisation rounds as a segment has chunks; and carries batches of
ordinary files into a model's inputs.  No tolerance anywhere: every comparison is equality.  The corrupted inputs were
chosen on the CPU (tests/test_entropy_chunked_cpu.py), where the model shows what they do: they end in statuses."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import coefficient_inputs_cases as K
import entropy_cases as E
import entropy_chunked_cases as H
import jpeg_pixels_cases as C

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 256      # canary bytes in front of and behind the scratch


@pytest.fixture(scope="module")
def ci():
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs
    return coefficient_inputs


def _chunk_sizes(ci):
    return H.CHUNK_SIZES + (ci.DEFAULT_CHUNK_BYTES,)


def _dev(array, cuda):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(cuda)


def _launch(cuda, batch):
    """One call over `batch` (H.kernel_batch): the output buffer and the scratch's surroundings pre-filled with the canary
    byte, the scratch itself with 0xFF (garbage the kernels must not depend on), statuses and rounds with -1 -> (output
    bytes, statuses, rounds), downloaded."""
    from jpeg_detection_resnet_ssd_amd import kernels
    out = torch.full((batch["out_bytes"],), CANARY, dtype=torch.uint8, device=cuda)
    n = len(batch["segs"])
    status = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    rounds = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    guarded = torch.full((batch["scratch_bytes"] + 2 * GUARD,), CANARY, dtype=torch.uint8, device=cuda)
    scratch = guarded[GUARD:GUARD + batch["scratch_bytes"]]
    scratch.fill_(0xFF)
    assert out.data_ptr() % 64 == 0 and scratch.data_ptr() % 16 == 0
    try:
        kernels.jpeg_entropy_decode_chunked(_dev(batch["bytes"], cuda), _dev(batch["desc"], cuda), batch["desc"],
                                            _dev(batch["segs"], cuda), batch["segs"], _dev(batch["tables"], cuda), batch["tables"],
                                            out, status, batch["chunk_bytes"], scratch, rounds=rounds)
    finally:
        torch.cuda.synchronize()
    guarded = guarded.cpu().numpy()
    assert (guarded[:GUARD] == CANARY).all() and (guarded[-GUARD:] == CANARY).all(), "bytes around the scratch were written"
    return out.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()


def _kernel_equals(cuda, ci, datas, scans, want, chunk_bytes):
    """want: [(planes, status)] per file."""
    batch = H.kernel_batch(datas, scans, chunk_bytes)
    out, status, rounds = _launch(cuda, batch)
    files, spare = E.planes_of(batch, out)
    assert (out[spare] == CANARY).all(), "bytes outside the planes were written"
    assert spare[:48].all() and spare[-48:].all()
    chunks = ci.chunk_counts(batch["segs"], chunk_bytes)
    assert (rounds >= 0).all() and (rounds <= chunks).all(), (rounds.tolist(), chunks.tolist())
    first = 0
    for i, (planes, (want_planes, want_status)) in enumerate(zip(files, want)):
        n = len(want_status)
        assert np.array_equal(status[first:first + n], want_status), (i, status[first:first + n].tolist(), want_status.tolist())
        first += n
        for c, (got, w) in enumerate(zip(planes, want_planes)):
            bad = got != w
            assert not bad.any(), (i, c, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert first == len(status)
    return rounds


# ---- the kernels against the contract ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.cases()))
def test_kernel_equals_contract(cuda, ci, name):
    for chunk_bytes in _chunk_sizes(ci):
        _kernel_equals(cuda, ci, [H.cases()[name]], [H.scan(name)], [H.contract(name)], chunk_bytes)


def test_mixed_batch_of_gray_colour_and_marked_files(cuda, ci):
    names = ["48x64_q90", "gray_33x47", "marked_48x64_i5", "gray_8x8", "444_24x40", "leftover_16x16", "422_17x33", "noise_q100"]
    for chunk_bytes in _chunk_sizes(ci):
        _kernel_equals(cuda, ci, [H.cases()[n] for n in names], [H.scan(n) for n in names], [H.contract(n) for n in names],
                       chunk_bytes)


def test_corrupted_batch_in_one_launch(cuda, ci):
    scan = H.scan(H.CORRUPTED_CASE)
    datas = [H.corrupted(seed) for seed in H.CORRUPTED_SEEDS]
    want = [H.corrupted_contract(seed) for seed in H.CORRUPTED_SEEDS]
    seen = np.bincount(np.concatenate([s for _, s in want]), minlength=5)
    assert (seen >= 1).all(), seen.tolist()
    for chunk_bytes in _chunk_sizes(ci):
        _kernel_equals(cuda, ci, datas, [scan] * len(datas), want, chunk_bytes)


def test_a_short_scratch_launches_nothing(cuda, ci):
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd._lib import DjError
    name = "48x64_q90"
    batch = H.kernel_batch([H.cases()[name]], [H.scan(name)], 64)
    out = torch.full((batch["out_bytes"],), CANARY, dtype=torch.uint8, device=cuda)
    status = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    scratch = torch.full((batch["scratch_bytes"] - 16,), CANARY, dtype=torch.uint8, device=cuda)
    with pytest.raises(DjError, match="bytes of scratch"):
        kernels.jpeg_entropy_decode_chunked(_dev(batch["bytes"], cuda), _dev(batch["desc"], cuda), batch["desc"],
                                            _dev(batch["segs"], cuda), batch["segs"], _dev(batch["tables"], cuda), batch["tables"],
                                            out, status, 64, scratch)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((status == -1).all()) and bool((scratch == CANARY).all())


# ---- the path --------------------------------------------------------------------------------------------------------------------
def _nan(cuda, shapes):
    return [torch.full(tuple(s), float("nan"), device=cuda) for s in shapes]


def test_emit_into_equals_numpy_over_both_staging_slots(ci, cuda):
    """Three batches through one emitter, nothing synchronising in between: both pinned slots, blob and scratch grow, a
    marked file rides along in a chunked batch, and an all-marked batch keeps the one-lane-per-interval plan."""
    emit = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=64)
    v = H.cases()
    first = emit([v["48x64_q90"], v["marked_48x64_i5"]], [(0, 0, 32, 32), (16, 32, 32, 32)], [False, True])
    second = emit([v["48x64_q90"], v["gray_33x47"], v["noise_q100"], v["48x64_q10_opt"]],
                  [(16, 16, 16, 16), (16, 0, 16, 16), (0, 16, 16, 16), (16, 32, 16, 16)], [True, True, False, False])
    third = emit([v["marked_48x64_i5"], v["marked_48x64_i5"]], [(0, 32, 32, 32), (16, 0, 32, 32)], [True, False])
    assert [type(p.plan) for p in (first, second, third)] == [ci.ChunkedEntropyCoefficientPlan] * 2 + [ci.EntropyCoefficientPlan]
    assert emit.host_batches == 0
    results = []
    for pending in (first, second, third, first):
        buffers = _nan(cuda, pending.shapes)
        pending.emit_into(buffers)
        results.append(buffers)
    emit.check(cuda)
    for pending, got in zip((first, second, third, first), results):
        off = ci.DeviceCoefficientInputs()(pending.images, pending.windows, pending.flips)
        host = _nan(cuda, pending.shapes)
        off.emit_into(host)                                                        # the host path
        torch.cuda.synchronize()
        for g, h, w in zip(got, host, pending.numpy()):
            assert np.array_equal(g.cpu().numpy(), w) and np.array_equal(h.cpu().numpy(), w)
    assert not results[1][1][1].cpu().numpy().any() and results[1][1][0].cpu().numpy().any()      # the gray file's chroma


def test_300_x_300_file_at_the_default_chunk_size_equals_the_host_reader(ci, cuda):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs
    data = H.cases()["300x300_smooth_q90"]
    pending = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True)([data])
    assert type(pending.plan) is ci.ChunkedEntropyCoefficientPlan and pending.plan.chunk_bytes == ci.DEFAULT_CHUNK_BYTES
    outs = _nan(cuda, pending.shapes)
    pending.emit_into(outs)
    pending.emitter.check(cuda)
    want = emit_dct_inputs(None, jpeg_bytes=[data])
    assert [w.shape for w in want] == [(1, 38, 38, 64), (1, 19, 19, 128)]
    for got, w, s in zip(outs, want, pending.numpy()):
        assert np.array_equal(got.cpu().numpy(), w) and np.array_equal(w, s)


def _compiled(block=2):
    """The smallest DCT classifier, at a (16 block) x (16 block) window."""
    from jpeg_detection_resnet_ssd_amd.keras import backend as B
    from jpeg_detection_resnet_ssd_amd.keras import layers as L
    from jpeg_detection_resnet_ssd_amd.keras.models import Model
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    B.clear_session()
    B.set_random_seed(5)
    iy, icc = L.Input(shape=(2 * block, 2 * block, 64)), L.Input(shape=(block, block, 128))
    features = L.Concatenate(axis=-1)([iy, L.UpSampling2D()(icc)])
    h = L.Conv2D(8, (3, 3), padding="same", activation="relu", name="conv")(features)
    y = L.Dense(3, activation="softmax", name="probs")(L.GlobalAveragePooling2D(name="pool")(h))
    model = Model([iy, icc], y)
    model.compile(optimizer=SGD(lr=1e-4, momentum=0.9), loss="categorical_crossentropy")
    return model


def test_predict_fed_either_way_gives_equal_outputs(ci, cuda):
    model = _compiled()
    v = H.cases()
    files = [v["48x64_q90"], E.jpeg(40, 40, 75, layout="gray"), v["marked_48x64_i5"]]
    windows, flips = [(16, 32, 32, 32), (0, 0, 32, 32), (0, 16, 32, 32)], [True, False, True]
    on = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=64)(files, windows, flips)
    off = ci.DeviceCoefficientInputs()(files, windows, flips)
    assert type(on.plan) is ci.ChunkedEntropyCoefficientPlan and type(off.plan) is ci.CoefficientPlan
    got = model.predict(on, batch_size=3)
    on.emitter.check(cuda)
    want = model.predict(off, batch_size=3)
    assert got.shape == (3, 3) and np.isfinite(got).all() and np.array_equal(got, want)
    assert np.array_equal(model.predict(on, batch_size=2), want)                   # sliced along the batch
    on.emitter.check(cuda)
    assert on.emitter.host_batches == 0


def _plain_tree(root):
    """A tree of six ordinary 4:2:0 files (no restart intervals) of about 50 x 70 -> (directory, index file)."""
    from PIL import Image
    dst = os.path.join(root, "train")
    for k in range(6):
        directory = os.path.join(dst, K.CLASSES[str(k % 3)][0])
        os.makedirs(directory, exist_ok=True)
        pixels = Image.fromarray(C.content("noise" if k % 2 else "smooth", 50 + k, 70 - k, seed=k))
        pixels.save(os.path.join(directory, "img%d.jpg" % k), "JPEG", quality=90, subsampling=2)
    index_file = os.path.join(root, "index.json")
    with open(index_file, "w") as f:
        json.dump(K.CLASSES, f)
    return dst, index_file


def test_fit_and_evaluate_from_a_tree_of_ordinary_files(cuda, tmp_path):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients
    tree = _plain_tree(str(tmp_path))
    model = _compiled()

    def generator(**kw):
        return DCTGeneratorCoefficients(tree[0], tree[1], batch_size=3, shuffle=False, target_length=32, device=True,
                                        decode_threads=2, **kw)
    on, off = generator(device_entropy=True, unmarked=True, chunk_bytes=64), generator()
    marked_only = generator(device_entropy=True)
    random.seed(3)
    history = model.fit_generator(on, steps_per_epoch=2, epochs=1, verbose=0)
    assert math.isfinite(history.history["loss"][0]) and on.host_batches == 0
    random.seed(4)
    got = model.evaluate_generator(on)
    random.seed(4)
    want = model.evaluate_generator(off)
    assert math.isfinite(got) and got == want and on.host_batches == 0
    random.seed(4)
    assert model.evaluate_generator(marked_only) == want and marked_only.host_batches == 2      # what the switch saves


def test_a_corrupted_files_batch_raises_naming_the_file(ci, cuda):
    reader = E.reader()
    good = H.cases()[H.CORRUPTED_CASE]
    # a corrupted copy that the pre-pass still accepts (the change made no marker) and whose contract reports a failure
    seed = next(s for s in H.CORRUPTED_SEEDS
                if H.corrupted_contract(s)[1].any() and reader.scan_segments(H.corrupted(s), unmarked=True).entropy_decodable)
    emit = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=16)
    windows = [(0, 0, 32, 32)] * 2
    bad, fine = emit([good, H.corrupted(seed)], windows), emit([good, good], windows)
    bad.images[1].name = "somewhere/corrupted.jpg"
    assert type(bad.plan) is ci.ChunkedEntropyCoefficientPlan
    buffers = _nan(cuda, bad.shapes)
    text = "file 1 \\(somewhere/corrupted.jpg\\): segment 0"
    bad.emit_into(buffers)                                                          # asynchronous: nothing raises here
    with pytest.raises(ValueError, match=text):
        emit.check(cuda)
    emit.check(cuda)                                                                # reported once
    fine.emit_into(buffers)
    emit.check(cuda)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(buffers, fine.numpy()))
