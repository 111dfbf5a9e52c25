"""GPU: `DeviceImagePrep` and `DevicePatchResize` keep their buffers through one base (data/device_staging.py:
ResidentBuffers).  Two emitters on one device, their uploads and kernels interleaved on one stream, must neither share a
buffer nor disturb each other's batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32


def _images(rng, shapes):
    return [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]


def test_two_emitters_on_one_device_keep_apart(cuda):
    import torch
    from jpeg_detection_resnet_ssd_amd.data.image_prep import DeviceImagePrep, max_offset
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    rng = np.random.default_rng(91)
    prep = DeviceImagePrep(target_length=16, deconv=True)
    patch = DevicePatchResize(out_height=12, out_width=20, deconv=True)

    def image_batch(shapes, ops=None):
        params = [(i != 1, max_offset(h, w, 16, i != 1) // (1 + i % 2), i % 2 == 0) for i, (h, w) in enumerate(shapes)]
        return prep(_images(rng, shapes), params, ops)

    image_batches = [image_batch([(17, 23), (40, 56), (31, 18)], [[(1, 0.7), (4, (0.1, -0.2, 0.3))], [], [(3, 1.3), (2, 0.6)]]),
                     image_batch([(40, 56), (23, 17)])]
    patch_batches = [patch(_images(rng, [(17, 23), (40, 56)]),
                           [(3, 2, 12, 15, True, 3, (1, 2, 3)), (-6, -9, 60, 70, False, 0, (200, 100, 50))]),
                     patch(_images(rng, [(40, 56), (25, 30), (17, 23)]),
                           [(5, 8, 30, 40, False, 1, (9, 8, 7)), (50, 0, 6, 7, False, 2, (4, 5, 6)), (2, 1, 12, 20, True, 4, (0, 0, 0))],
                           photometric=[(1, F(5), None, None, None, (0, 1, 2)), (2, None, F(0.75), F(1.5), None, (2, 1, 0)),
                                        (1, None, None, None, F(9), (0, 1, 2))])]
    order = [image_batches[0], patch_batches[0], patch_batches[1], image_batches[1]]
    wants = [b.numpy() for b in order]
    outs = [[torch.full(s, float("nan"), device=cuda) for s in b.shapes] for b in order]

    def held(emitter):
        st = emitter._state[str(cuda)]
        return [st["blob"].data_ptr(), st["scratch"].data_ptr(), st["out"].data_ptr()] + [s[0].data_ptr() for s in st["slots"]]

    for round_ in range(2):
        for b, o in zip(order, outs):          # no synchronise in between: all on the current stream
            b.emit_into(o)
        torch.cuda.synchronize()
        for o, want in zip(outs, wants):
            for got, w in zip(o, want):
                assert torch.equal(got.cpu(), torch.from_numpy(w))
        now = held(prep) + held(patch)
        assert len(set(now)) == len(now)       # the two emitters hold distinct buffers
        if round_ == 0:
            before = now
            for o in outs:
                for t in o:
                    t.fill_(float("nan"))
    assert now == before
