"""GPU: csrc/dj_ssd_photometric.hip distorts the staged rectangles of a ragged batch in place into exactly the bytes the
numpy statement gives (data/ssd_photometric.py:ssd_photometric_host), touches nothing else of the staging blob, writes
nothing when an argument is rejected, and the stage runs in front of dj_patch_resize when a `PendingPatchInputs` or the VOC
generator carries records.  Equality throughout: the float32 arithmetic is the same operation for operation."""
import numpy as np
import pytest
import torch

from test_ssd_photometric_cpu import colour_grid, write_voc_tree

pytestmark = pytest.mark.gpu

F = np.float32
BG = (123, 117, 104)
SHAPES = [(64, 48), (1, 1), (37, 53), (5, 3), (512, 512)]
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _images(seed):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES[:4]]
    return images + [np.ascontiguousarray(colour_grid().reshape(512, 512, 3))]


def _whole(images, filt=2):
    return [(0, 0, im.shape[0], im.shape[1], False, filt, BG) for im in images]


def _record_batches():
    """Batches of five records: both sequences, every subset of the four operations, the ends of the ranges, the hue
    delta that lifts H = 0 to the byte 180, all six channel orders."""
    ends = {"brightness": (F(-32), F(32)), "contrast": (F(0.5), F(1.5)), "saturation": (F(0.5), F(1.5)), "hue": (F(-18), F(18))}
    inner = {"brightness": F(11.3), "contrast": F(1.2173), "saturation": F(0.8341), "hue": F(-7.77)}
    records = []
    for sequence in (1, 2):
        for mask in range(16):
            for pick in range(2):
                values = [ends[name][pick] if mask >> k & 1 else None
                          for k, name in enumerate(("brightness", "contrast", "saturation", "hue"))]
                records.append((sequence,) + tuple(values) + (ORDERS[(mask + pick) % 6],))
    for k, order in enumerate(ORDERS):
        records.append((1 + k % 2, inner["brightness"], inner["contrast"], inner["saturation"], inner["hue"], order))
        records.append((2 - k % 2, None, F(1.5) if k % 3 == 0 else None, None, F(-1e-9), order))
    while len(records) % 5:
        records.append(records[len(records) % 7])
    # shift by one per batch so that the 512 x 512 colour grid, the last image, meets different kinds of record
    return [records[i:i + 5][k % 5:] + records[i:i + 5][:k % 5] for k, i in enumerate(range(0, len(records), 5))]


def _stage(plan, images, cuda, guard=0, sentinel=0):
    host = np.full(plan.nbytes + guard, sentinel, dtype=np.uint8)
    plan.fill(host, images)
    return host, torch.from_numpy(host).to(cuda)


def _run(plan, host, blob):
    from jpeg_detection_resnet_ssd_amd import kernels
    src_h, desc_h, _ = plan.views(host)
    src_d, desc_d, _ = plan.views(blob)
    kernels.ssd_photometric(src_d, desc_d, desc_h, plan.photo_view(blob), plan.photo_view(host))
    torch.cuda.synchronize()
    return blob.cpu().numpy()


def _rect(plan, blob, i):
    d = plan.desc[i]
    o = plan.src_offset + int(d["src_offset"])
    h, w = int(d["src_h"]), int(d["src_w"])
    return blob[o:o + 3 * h * w].reshape(h, w, 3)


def test_ragged_batch_equals_the_host_statement(cuda):
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import ssd_photometric_host
    images = _images(51)
    batches = _record_batches()
    assert len(batches) >= 15
    seen_on_grid = set()
    for records in batches:
        plan = PatchPlan(SHAPES, _whole(images), 8, 8, records)
        host, blob = _stage(plan, images, cuda)
        got = _run(plan, host, blob)
        for i, (im, rec) in enumerate(zip(images, records)):
            want = ssd_photometric_host(im, rec)
            bad = (_rect(plan, got, i) != want).any(axis=-1)
            assert not bad.any(), (im.shape, rec, int(bad.sum()), im[bad][:4].tolist(), _rect(plan, got, i)[bad][:4].tolist(),
                                   want[bad][:4].tolist())
        seen_on_grid.add((records[4][0],) + tuple(v is not None for v in records[4][1:5]))
    assert {s[0] for s in seen_on_grid} == {1, 2} and all(any(s[k] for s in seen_on_grid) for k in range(1, 5))


def test_cropping_windows_leave_everything_but_the_rectangles_untouched(cuda):
    """Windows smaller than the images, one that misses its image (nothing staged) and one that covers it: descriptors,
    pool, the padding behind each rectangle, the records and a guard band behind the blob keep their bytes."""
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import ssd_photometric_host
    images = _images(52)[:4]
    geometries = [(10, 7, 31, 22, True, 3, BG), (5, 5, 2, 2, False, 0, BG), (-4, 20, 30, 50, False, 1, BG), (1, 1, 3, 1, True, 4, BG)]
    records = [(1, F(20), F(1.4), F(0.6), F(10), (2, 1, 0)), (2, F(-5), None, None, None, (0, 1, 2)),
               (2, None, F(0.7), F(1.5), F(-1e-9), (1, 2, 0)), (1, None, None, None, None, (0, 2, 1))]
    guard, sentinel = 4096, 0xA5
    plan = PatchPlan(SHAPES[:4], geometries, 8, 8, records)
    assert plan.rects == [(10, 41, 7, 29), (0, 0, 0, 0), (0, 26, 20, 53), (1, 4, 1, 2)]
    host, blob = _stage(plan, images, cuda, guard, sentinel)
    got = _run(plan, host, blob)
    want = host.copy()
    for i, (im, rec, (ya, yb, xa, xb)) in enumerate(zip(images, records, plan.rects)):
        if yb > ya:
            _rect(plan, want, i)[...] = ssd_photometric_host(im, rec)[ya:yb, xa:xb]
    assert (want != host).sum() > 1000
    assert np.array_equal(got, want)
    assert (got[plan.nbytes:] == sentinel).all() and np.array_equal(got[:plan.src_offset], host[:plan.src_offset])


@pytest.mark.parametrize("what, image, value", [
    ("sequence", 0, 0), ("sequence", 1, 3), ("brightness", 0, np.nan), ("contrast", 1, np.inf), ("saturation", 0, -np.inf),
    ("hue", 1, np.nan), ("order", 0, (0, 0, 1)), ("order", 1, (0, 1, 3)), ("flags", 0, 16), ("src_offset", 1, 1 << 40),
    ("src_h", 0, 500), ("src_stride", 1, 3),
])
def test_rejected_arguments_return_an_error_and_write_nothing(cuda, what, image, value):
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    images = _images(53)[:1] + _images(53)[2:3]
    records = [(1, F(20), F(1.4), F(0.6), F(10), (2, 1, 0)), (2, F(-5), F(0.7), F(1.5), F(-3), (0, 1, 2))]
    plan = PatchPlan([im.shape[:2] for im in images], _whole(images), 8, 8, records)
    host, blob = _stage(plan, images, cuda, 256, 0x5A)
    src_h, desc_h, _ = plan.views(host)
    src_d, desc_d, _ = plan.views(blob)
    desc_h, params_h = desc_h.copy(), plan.photo_view(host).copy()
    (desc_h if what.startswith("src_") else params_h)[what][image] = value
    with pytest.raises(_lib.DjError) as e:
        kernels.ssd_photometric(src_d, desc_d, desc_h, plan.photo_view(blob), params_h)
    assert "image %d" % image in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(blob.cpu().numpy(), host)


def test_emission_with_records_equals_its_host_twin_and_without_them_is_unchanged(cuda):
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    images = _images(54)[:4]
    geometries = [(10, 7, 31, 22, True, 3, BG), (-3, -2, 9, 8, False, 0, BG), (-40, -60, 120, 170, False, 1, BG),
                  (1, 1, 3, 1, True, 4, (7, 250, 0))]
    records = [(1, F(20), F(1.4), F(0.6), F(10), (0, 1, 2)), (2, F(-5), None, None, None, (0, 1, 2)),
               (2, None, F(0.7), F(1.5), F(-1e-9), (0, 1, 2)), (1, None, None, None, None, (0, 1, 2))]
    for deconv in (False, True):
        prep = DevicePatchResize(out_height=24, out_width=20, deconv=deconv)
        batches = [prep(images, geometries, photometric=records), prep(images, geometries),
                   prep(images, geometries, photometric=records)[1:3]]
        assert batches[0].plan.nbytes == batches[1].plan.nbytes + 4 * 40 and len(batches[2]) == 2
        outs = [[torch.full(s, float("nan"), device=cuda) for s in b.shapes] for b in batches]
        for b, o in zip(batches, outs):          # queued without a synchronise in between, through one emitter
            b.emit_into(o)
        torch.cuda.synchronize()
        for b, o in zip(batches, outs):
            for got, want in zip(o, b.numpy()):
                assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert not all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
        assert all(torch.equal(a[1:3], b) for a, b in zip(outs[0], outs[2]))


def test_generator_with_device_prep_equals_the_host_path(cuda, tmp_path):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    gen = write_voc_tree(tmp_path)
    prep = DevicePatchResize(48, 40)
    for make in (sa.SSDDataAugmentation, sa.SSDDataAugmentationNoCrop):
        for seed in (0, 1):
            chain = make(48, 40, photometric_distortions=sa.SSDPhotometricDistortions())
            np.random.seed(seed)
            host_x, host_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain],
                                               returns=["processed_images", "processed_labels"]))
            np.random.seed(seed)
            pending, dev_y = next(gen.generate(batch_size=3, shuffle=False, transformations=[chain],
                                               returns=["processed_images", "processed_labels"], device_prep=prep))
            assert pending.plan.photo is not None and len(pending) == 3
            assert all(np.array_equal(a, b) for a, b in zip(host_y, dev_y))
            bufs = [torch.full(s, float("nan"), device=cuda) for s in pending.shapes]
            pending.emit_into(bufs)
            torch.cuda.synchronize()
            for got, want in zip(bufs, host_x):
                assert torch.equal(got.cpu(), torch.from_numpy(want))
