"""GPU: dj_jpeg_pixels (csrc/dj_jpegpix.hip) writes, byte for byte, what data/jpeg_pixels.py:jpeg_pixels_host states --
for every file of the CPU case table (tests/jpeg_pixels_cases.py) and every rectangle, in ragged batches that mix
`CoefficientImage`s with decoded arrays -- and `DevicePatchResize` run on `CoefficientImage`s gives the batch and the model
inputs it gives on the Pillow-decoded arrays.  Equality everywhere, no tolerance."""
import numpy as np
import pytest
import torch

import jpeg_pixels_cases as C

pytestmark = pytest.mark.gpu
BG = (3, 100, 250)


def _geometry(rect):
    ya, yb, xa, xb = rect
    return (ya, xa, yb - ya, xb - xa, False, 0, BG)      # the window IS the rectangle: exactly it is staged


def _stage(plan, images, cuda, guard=256, sentinel=0xA5):
    host = np.full(plan.nbytes + guard, sentinel, dtype=np.uint8)
    plan.fill(host, images)
    return host, torch.from_numpy(host).to(cuda)


def _decode(plan, host, blob, cuda, guard=256, sentinel=0x5C):
    scratch = torch.full((plan.scratch_bytes + guard,), sentinel, dtype=torch.uint8, device=cuda)
    plan.launch_decode(host, blob, scratch[:plan.scratch_bytes])
    torch.cuda.synchronize()
    assert (scratch[plan.scratch_bytes:] == sentinel).all()
    return blob.cpu().numpy()


def _expected(plan, host, images):
    """The staged blob with the statement's rectangle of every `CoefficientImage` written where `_fill_pixels` writes an
    array's."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    want = host.copy()
    for d, (ya, yb, xa, xb), im in zip(plan.desc, plan.rects, images):
        if isinstance(im, CoefficientImage) and yb > ya:
            o = plan.src_offset + int(d["src_offset"])
            want[o:o + 3 * (yb - ya) * (xb - xa)].reshape(yb - ya, xb - xa, 3)[...] = im.pixels()[ya:yb, xa:xb]
    return want


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_every_case_and_rectangle_equals_the_statement(cuda, layout):
    """One ragged batch per sampling layout: every size x quality x content of the case table (the 300 x 300 size at two
    qualities), each size meeting every one of its rectangles; every seventh item travels as a decoded array instead,
    and one `CoefficientImage` has a window that misses it (nothing of it is staged, nothing is written for it).  The
    whole blob is compared: the rectangles hold the statement's bytes and nothing else changed."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan, _plan_items
    images, geometries, used = [], [], set()
    for size in C.SIZES:
        rects = C.rectangles(size[1], size[0])
        k = 0
        for quality in C.QUALITIES:
            if size == (300, 300) and quality not in (10, 90):
                continue
            for kind in C.CONTENTS:
                data = C.jpeg_case(layout, quality, kind, size, optimize=(quality == 50))
                image = CoefficientImage(data)
                rect = rects[k % len(rects)]
                used.add((size, rect))
                k += 1
                images.append(image.pixels() if len(images) % 7 == 3 else image)
                geometries.append(_geometry(rect))
        assert {r for s, r in used if s == size} == set(rects) or size == (300, 300) and k == 6
    for data in C.golden_jpegs().values():
        try:
            images.append(CoefficientImage(data))
        except ValueError:
            continue                                       # the progressive file
        geometries.append(_geometry((0,) + (images[-1].shape[0], 0, images[-1].shape[1])))
    images.append(CoefficientImage(C.jpeg_case(layout, 75, "noise", (37, 53))))
    geometries.append((200, 200, 9, 9, False, 0, BG))      # misses the image
    plan = PatchPlan(_plan_items(images), geometries, 4, 4)
    assert plan.rects[-1] == (0, 0, 0, 0) and len(images) - 1 not in plan.decode_items
    assert len(plan.decode_items) > 200
    host, blob = _stage(plan, images, cuda)
    got = _decode(plan, host, blob, cuda)
    want = _expected(plan, host, images)
    assert (want != host).sum() > 100000
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), plan.src_offset, plan.decode_offset)


def test_rectangles_of_the_large_image(cuda):
    """300 x 300 at 4:2:0 and 4:2:2: every rectangle of the table, several blocks of the colour pass and of the inverse
    DCT per image."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan, _plan_items
    images, geometries = [], []
    for layout in ("420", "422"):
        image = CoefficientImage(C.jpeg_case(layout, 90, "noise", (300, 300)))
        for rect in C.rectangles(300, 300) + [(101, 300, 3, 299), (255, 300, 0, 300)]:
            images.append(image)
            geometries.append(_geometry(rect))
    plan = PatchPlan(_plan_items(images), geometries, 4, 4)
    host, blob = _stage(plan, images, cuda)
    assert np.array_equal(_decode(plan, host, blob, cuda), _expected(plan, host, images))


def _end_to_end_batch():
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    files = [C.jpeg_case("420", 90, "noise", (53, 37)), C.jpeg_case("422", 75, "smooth", (31, 50)),
             C.jpeg_case("444", 50, "saturated", (16, 16)), C.jpeg_case("gray", 75, "noise", (33, 17)),
             C.jpeg_case("420", 90, "saturated", (5, 2)), C.jpeg_case("420", 75, "noise", (300, 300))]
    geometries = [(-3, -4, 50, 60, True, 2, BG), (5, 3, 20, 11, False, 3, (0, 0, 0)), (0, 0, 16, 16, False, 0, BG),
                  (100, 100, 5, 5, False, 1, BG), (0, 1, 2, 3, True, 4, BG), (31, 17, 250, 270, False, 1, BG)]
    coefficient = [CoefficientImage(f) for f in files]
    return coefficient, [C.pillow_pixels(f) for f in files], geometries


F = np.float32
RECORDS = [(1, F(20), F(1.4), F(0.6), F(10), (0, 1, 2)), (2, F(-5), None, None, None, (2, 1, 0)),
           (2, None, F(0.7), F(1.5), F(-1e-9), (0, 1, 2)), (1, None, None, None, None, (0, 1, 2)),
           (1, F(3), None, F(1.2), None, (1, 0, 2)), (2, F(-11), F(1.1), None, F(5), (0, 2, 1))]


@pytest.mark.parametrize("photometric", [False, True])
def test_patch_resize_on_coefficient_images_equals_pillow_decoded_arrays(cuda, photometric):
    """`DevicePatchResize.run`: the uint8 batch, and after dj_rgb_to_dct the model inputs, for `CoefficientImage`s, for a
    mixed batch and for the arrays Pillow decodes from the same files -- through one emitter, queued back to back."""
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    coefficient, arrays, geometries = _end_to_end_batch()
    records = RECORDS if photometric else None
    mixed = [coefficient[0], arrays[1]] + coefficient[2:]
    for deconv in (False, True):
        prep = DevicePatchResize(out_height=24, out_width=20, deconv=deconv)
        batches = [prep(images, geometries, photometric=records) for images in (arrays, coefficient, mixed, arrays)]
        assert batches[0].plan.decode is None and batches[1].plan.decode_items == [0, 1, 2, 4, 5]
        pixels = [prep.run(b.plan, b.images, cuda).clone() for b in batches]
        outs = [[torch.full(s, float("nan"), device=cuda) for s in b.shapes] for b in batches]
        for b, o in zip(batches, outs):
            b.emit_into(o)
        torch.cuda.synchronize()
        want = batches[0].pixels()
        for p in pixels:
            assert np.array_equal(p.cpu().numpy(), want)
        for o in outs:
            for got, ref, host in zip(o, outs[0], batches[0].numpy()):
                assert torch.equal(got, ref) and torch.equal(got.cpu(), torch.from_numpy(host))


def _bad_descriptor_cases():
    big = 1 << 40
    return [("coef_offset", (0, 1), big), ("coef_offset", (1, 2), 1), ("coef_offset", (0, 0), -2), ("sample_offset", (1, 0), big),
            ("sample_offset", (0, 1), 4), ("sample_offset", (1, 0), 0), ("dst_offset", (0,), big), ("dst_offset", (1,), -1),
            ("dst_stride", (0,), 3), ("table_offset", (1,), 1 << 20), ("table_offset", (0,), -64), ("n_components", (0,), 2),
            ("h_samp", (0,), 4), ("v_samp", (1,), 2), ("height", (0,), 70000), ("width", (1,), 0), ("yb", (0,), 38), ("xa", (1,), -1),
            ("xb", (1,), 0), ("blocks_w", (0, 0), 8), ("blocks_h", (1, 1), 1), ("by1", (0, 2), 4), ("bx0", (0, 1), 1),
            ("bx1", (1, 0), 9), ("by0", (1, 0), -1)]


@pytest.mark.parametrize("field, index, value", _bad_descriptor_cases())
def test_bad_descriptors_return_the_error_code_without_launching(cuda, field, index, value):
    """A descriptor that points outside a buffer, names a grid the frame does not have or block ranges that do not cover
    the rectangle: DJ_ERR_ARG naming the image, and neither the blob nor the scratch buffer is written."""
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import PatchPlan
    images = [CoefficientImage(C.jpeg_case("420", 75, "noise", (53, 37))), CoefficientImage(C.jpeg_case("422", 75, "noise", (50, 31)))]
    plan = PatchPlan(images, [_geometry((0, 37, 0, 53)), _geometry((2, 31, 30, 50))], 4, 4)
    host, blob = _stage(plan, images, cuda)
    scratch = torch.full((plan.scratch_bytes,), 0x5C, dtype=torch.uint8, device=cuda)
    desc_h, tables_h, _ = plan.decode_views(host)
    desc_d, tables_d, coef_d = plan.decode_views(blob)
    desc_h = desc_h.copy()
    desc_h[field][index] = value                     # index = (image,) or (image, component)
    src_d = blob[plan.src_offset:plan.src_offset + plan.src_bytes]
    with pytest.raises(_lib.DjError) as e:
        kernels.jpeg_pixels(coef_d, desc_d, desc_h, tables_d, tables_h, src_d, scratch)
    assert "rc=-1" in str(e.value) and "image %d" % index[0] in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(blob.cpu().numpy(), host) and (scratch == 0x5C).all()
