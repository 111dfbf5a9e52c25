"""GPU: csrc/dj_photometric.hip turns a uint8 batch into exactly the bytes the reference's saturation / brightness /
contrast return (tests/golden/photometric.npz) and the host twin states (data/photometric.py:photometric_host), whatever
the batch, the row stride or the stream; lighting adds exactly the shift it reports, and that shift is the twin's to
fp64 rounding; a classifier fed by the generators' device path with the four callables sees the twin's input tensors.
Nothing here reads the reference or compares against the installed `dot`."""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric.npz")
SAT, BRI, CON, LIG = 1, 2, 3, 4
SIZES = [(1, 1), (1, 5), (8, 16), (3, 43), (24, 40), (33, 47)]
# Largest |kernel shift - twin shift| / (255 * lambda_max * max|normal|) over the images of
# test_lighting_shift_equals_the_twins: 7.71e-16 measured on an MI355X (cyclic Jacobi in fp64 against LAPACK's eigh, relative
# eigenvalue gaps >= 3e-2 there); the bound is 16 times that, and may never exceed 1e-9.
SHIFT_BOUND = 16 * 7.71e-16
E2E_SEEDS = (6, 106)          # of `random` and `np.random`: the two images draw [lighting, saturation] and [saturation, contrast, brightness]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _content(rng, kind, h, w):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        v = ((np.arange(h * w) * 255) // max(h * w - 1, 1)).astype(np.uint8).reshape(h, w)
        return np.ascontiguousarray(np.stack([v, v, v], axis=-1))
    if kind == "constant":
        return np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)))
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        planes = [127.5 + (50 + 35 * c) * np.sin(xx / (3.0 + c) + yy / (5.0 + 2 * c) + c) for c in range(3)]
        return np.clip(np.stack(planes, axis=-1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
    img = (rng.integers(0, 2, (-(-h // 4), -(-w // 4), 3)) * 255).astype(np.uint8)      # 0 / 255 patches
    return np.ascontiguousarray(np.kron(img, np.ones((4, 4, 1), dtype=np.uint8))[:h, :w])


KINDS = ["noise", "ramp", "patches", "smooth", "constant"]


def _draw_ops(rng, n_ops, lighting=True):
    """A chain of n_ops operations in random order, lighting at most once (as the generators draw them), alpha over the
    callables' range [0.5, 1.5] with the ends over-represented."""
    codes = [int(c) for c in rng.permutation([SAT, BRI, CON, LIG] if lighting else [SAT, BRI, CON, SAT])[:n_ops]]
    ops = []
    for c in codes:
        if c == LIG:
            ops.append((c, tuple(float(v) for v in rng.standard_normal(3) * 0.5)))
        else:
            ops.append((c, (float(rng.choice([0.5 + rng.random(), 0.5 + 0.01 * rng.random(), 1.5 - 0.01 * rng.random()])),)))
    return ops


def _run(cuda, images, ops, shift_out=True):
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_device
    pixels = torch.from_numpy(np.stack(images)).to(cuda)
    out = photometric_device(pixels, ops, shift_out=shift_out)
    if shift_out:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def _host_with_reported_shift(image, ops, shift):
    """The twin's chain with the lighting step (at most one) adding `shift` instead of its own: what the kernel must have
    stored if every other step is the twin's and lighting is trunc(clip(pixels + reported shift))."""
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_host
    codes = [c for c, _ in ops]
    if LIG not in codes:
        return photometric_host(image[None], [ops])[0]
    k = codes.index(LIG)
    assert LIG not in codes[k + 1:]
    before = photometric_host(image[None], [ops[:k]])[0]
    lit = np.clip(before + shift, 0, 255).astype(np.uint8)
    return photometric_host(lit[None], [ops[k + 1:]])[0]


def _shift_scale(image, normals):
    from jpeg_detection_resnet_ssd_amd.data.photometric import moment_covariance
    lam = np.linalg.eigvalsh(moment_covariance(image))
    return 255.0 * lam.max() * np.abs(normals).max(), lam


# ---- against the reference's bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["saturation", "brightness", "contrast", "chain"])
def test_kernel_equals_the_fixture(cuda, golden, family):
    names = [str(n) for n in golden["names"] if str(n).startswith(family + "/")]
    assert len(names) >= 4
    failures = []
    for name in names:
        ops = [(int(c), (float(golden[name + "/draws"][i, 0]),)) for i, c in enumerate(golden[name + "/ops"])]
        got = _run(cuda, [golden[name + "/src"]], [ops], shift_out=False)[0]
        want = golden[name + "/out"]
        bad = got != want
        if bad.any():
            failures.append(name)
            print(name, "mismatching bytes:", int(bad.sum()), "of", want.size, "first:", np.argwhere(bad)[:4].tolist())
    assert not failures, failures


# ---- against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES + [(130, 63), (1, 129)])
def test_kernel_equals_the_host_twin_on_fresh_batches(cuda, shape):
    """B = 5, content of five kinds, chains of 0 to 4 operations in mixed orders.  (130, 63) holds 8190 pixels, one tree
    of numpy's sum just under its 8192-element buffer; test_mean_above_the_reduction_buffer goes past it."""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    images = [_content(rng, KINDS[i], h, w) for i in range(5)]
    ops = [_draw_ops(rng, n) for n in (3, 4, 0, 2, 1)]
    ops[1], ops[3] = _draw_ops(rng, 4), [(CON, (0.5,)), (CON, (1.5,))]
    got, shifts = _run(cuda, images, ops)
    for i in range(5):
        want = _host_with_reported_shift(images[i], ops[i], shifts[i])
        assert np.array_equal(got[i], want), (shape, i, ops[i], int((got[i] != want).sum()))
        if LIG not in [c for c, _ in ops[i]]:
            assert not shifts[i].any()


def test_mean_above_the_reduction_buffer(cuda):
    """96 x 96 = 9216 and 224 x 224 = 50176 grey values: numpy adds the sums of 8192-element chunks in order, the kernel's
    trees do the same.  Patches and grey noise keep the twin's exact arithmetic to a few hundred distinct pixels."""
    rng = np.random.default_rng(77)
    for h, w in ((96, 96), (224, 224)):
        base = _content(rng, "patches", h, w)
        base[::3, ::5] = rng.integers(0, 256, base[::3, ::5].shape[:2] + (1,), dtype=np.uint8)      # grey noise: 256 more pixels
        images = [base, np.ascontiguousarray(base[::-1])]
        ops = [[(CON, (0.5,))], [(SAT, (1.37,)), (CON, (1.49,)), (CON, (0.61,))]]
        got = _run(cuda, images, ops, shift_out=False)
        from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_host
        want = photometric_host(np.stack(images), ops)
        assert np.array_equal(got, want), (h, w, int((got != want).sum()))


def test_batch_of_64_equals_its_single_image_runs(cuda):
    rng = np.random.default_rng(64)
    images = [_content(rng, KINDS[i % 5], 33, 47) for i in range(64)]
    ops = [_draw_ops(rng, int(rng.integers(0, 5))) for _ in range(64)]
    whole, shifts = _run(cuda, images, ops)
    assert whole.shape == (64, 33, 47, 3) and whole.dtype == np.uint8
    for i in range(64):
        single, shift = _run(cuda, images[i:i + 1], ops[i:i + 1])
        assert np.array_equal(whole[i], single[0]) and np.array_equal(shifts[i], shift[0]), i


def test_strided_batch_leaves_everything_else_untouched(cuda):
    """Rows of 3 * W bytes inside rows of 3 * W + 40: the bytes between rows and a guard band behind the tensor keep their
    sentinel, and the operation lists stay as uploaded."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.photometric import pack_ops
    rng = np.random.default_rng(33)
    b, h, w, guard, sentinel = 4, 33, 47, 4096, 0xA5
    pitch = 3 * w + 40
    images = [_content(rng, KINDS[i], h, w) for i in range(b)]
    ops = [_draw_ops(rng, 4), _draw_ops(rng, 3), [(CON, (0.7,))], _draw_ops(rng, 4)]
    flat = torch.full((b * h * pitch + guard,), sentinel, dtype=torch.uint8, device=cuda)
    pixels = flat[:b * h * pitch].view(b, h, pitch)[:, :, :3 * w].unflatten(2, (w, 3))
    assert pixels.stride() == (h * pitch, pitch, 3, 1)
    pixels.copy_(torch.from_numpy(np.stack(images)))
    arr = pack_ops(ops)
    ops_dev = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(cuda)
    shifts = torch.zeros((b, 3), dtype=torch.float64, device=cuda)
    kernels.photometric(pixels, ops_dev, arr, shift_out=shifts)
    torch.cuda.synchronize()
    got, shifts = pixels.cpu().numpy(), shifts.cpu().numpy()
    for i in range(b):
        assert np.array_equal(got[i], _host_with_reported_shift(images[i], ops[i], shifts[i])), i
    rows = flat[:b * h * pitch].view(b * h, pitch)
    assert bool((rows[:, 3 * w:] == sentinel).all()) and bool((flat[-guard:] == sentinel).all())
    assert np.array_equal(ops_dev.cpu().numpy(), arr.view(np.uint8).reshape(-1))


def test_one_row_images_with_a_padded_pitch(cuda):
    """H = 1: the row pitch is the image pitch, and it need not be 3 * W."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.photometric import pack_ops, photometric_host
    rng = np.random.default_rng(38)
    b, w, pitch, sentinel = 3, 129, 3 * 129 + 13, 0x5A
    images = [_content(rng, k, 1, w) for k in ("noise", "ramp", "smooth")]
    ops = [[(CON, (0.55,)), (SAT, (1.4,))], [(SAT, (0.51,)), (CON, (1.49,))], [(BRI, (1.2,)), (CON, (0.7,))]]
    flat = torch.full((b * pitch,), sentinel, dtype=torch.uint8, device=cuda)
    pixels = flat.view(b, 1, pitch)[:, :, :3 * w].unflatten(2, (w, 3))
    assert pixels.stride(0) == pitch
    pixels.copy_(torch.from_numpy(np.stack(images)))
    arr = pack_ops(ops)
    kernels.photometric(pixels, torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(cuda), arr)
    torch.cuda.synchronize()
    assert np.array_equal(pixels.cpu().numpy(), photometric_host(np.stack(images), ops))
    assert bool((flat.view(b, pitch)[:, 3 * w:] == sentinel).all())


def test_launch_on_a_side_stream(cuda):
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_device
    rng = np.random.default_rng(35)
    images = [_content(rng, k, 24, 40) for k in ("noise", "smooth", "ramp")]
    ops = [_draw_ops(rng, 4), _draw_ops(rng, 2), _draw_ops(rng, 3)]
    want, want_shift = _run(cuda, images, ops)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):        # the uploads go to the same stream as the kernel
        pixels = torch.from_numpy(np.stack(images)).to(cuda)
        out, shift = photometric_device(pixels, ops, shift_out=True, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(shift.cpu().numpy(), want_shift)


def test_call_is_capturable_in_a_graph(cuda):
    """No synchronisation inside dj_photometric: the launch can be captured and replayed on new pixels and new lists (the
    lists are read from the device buffer when the kernel runs)."""
    from jpeg_detection_resnet_ssd_amd import kernels
    from jpeg_detection_resnet_ssd_amd.data.photometric import pack_ops
    rng = np.random.default_rng(36)
    images = [_content(rng, k, 33, 47) for k in ("noise", "patches", "smooth")]
    ops = [_draw_ops(rng, 4), _draw_ops(rng, 3), _draw_ops(rng, 4)]
    arr = pack_ops(ops)
    pixels = torch.from_numpy(np.stack(images)).to(cuda)
    ops_dev = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(cuda)
    shifts = torch.zeros((3, 3), dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.photometric(pixels, ops_dev, arr, shift_out=shifts, stream=torch.cuda.current_stream().cuda_stream)
    fresh = [_content(rng, k, 33, 47) for k in ("smooth", "noise", "ramp")]
    fresh_ops = [_draw_ops(rng, 2), _draw_ops(rng, 4), _draw_ops(rng, 1)]
    pixels.copy_(torch.from_numpy(np.stack(fresh)))
    ops_dev.copy_(torch.from_numpy(pack_ops(fresh_ops).view(np.uint8).reshape(-1).copy()))
    graph.replay()
    torch.cuda.synchronize()
    got, reported = pixels.cpu().numpy(), shifts.cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], _host_with_reported_shift(fresh[i], fresh_ops[i], reported[i])), i


def test_rejected_arguments_return_an_error_and_write_nothing(cuda):
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    from jpeg_detection_resnet_ssd_amd.data.photometric import pack_ops
    rng = np.random.default_rng(34)
    images = np.stack([_content(rng, "noise", 24, 40) for _ in range(2)])
    good = pack_ops([[(SAT, (0.8,)), (LIG, (0.1, 0.2, 0.3))], [(CON, (1.2,)), (BRI, (0.9,))]])
    ops_dev = torch.from_numpy(good.view(np.uint8).reshape(-1).copy()).to(cuda)
    for field, image, value in (("code", 1, 7), ("code", 0, 0), ("n_ops", 1, 5), ("param", 0, float("nan"))):
        bad = good.copy()
        if field == "n_ops":
            bad[field][image] = value
        else:
            bad[field][image, 1] = value
        pixels = torch.from_numpy(images).to(cuda)
        shifts = torch.full((2, 3), 7.0, dtype=torch.float64, device=cuda)
        with pytest.raises(_lib.DjError) as e:
            kernels.photometric(pixels, ops_dev, bad, shift_out=shifts)
        assert "image %d" % image in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(pixels.cpu().numpy(), images) and bool((shifts == 7.0).all())


# ---- lighting -----------------------------------------------------------------------------------------------------------
def test_lighting_adds_exactly_the_shift_it_reports(cuda):
    rng = np.random.default_rng(41)
    for h, w in SIZES[1:] + [(130, 63)]:
        images = [_content(rng, k, h, w) for k in ("noise", "smooth", "patches", "ramp")]
        ops = [[(LIG, tuple(float(v) for v in rng.standard_normal(3) * s))] for s in (0.5, 0.5, 2.0, 0.5)]
        got, shifts = _run(cuda, images, ops)
        for i in range(4):
            want = np.clip(images[i] + shifts[i], 0, 255).astype(np.uint8)
            assert np.array_equal(got[i], want), (h, w, i)
        assert np.abs(shifts[:3]).max() > 0.5 or h * w < 6          # the shift moves pixels: the check is not vacuous


def test_lighting_of_a_constant_image_is_the_identity(cuda):
    rng = np.random.default_rng(42)
    images = [_content(rng, "constant", 24, 40) for _ in range(3)] + [np.zeros((24, 40, 3), np.uint8),
                                                                      np.full((24, 40, 3), 255, np.uint8)]
    ops = [[(LIG, tuple(float(v) for v in rng.standard_normal(3) * 0.5))] for _ in range(5)]
    got, shifts = _run(cuda, images, ops)
    assert not shifts.any() and np.array_equal(got, np.stack(images))
    one, shift = _run(cuda, [_content(rng, "noise", 1, 1)], [[(LIG, (0.3, -0.2, 0.9))]])          # one pixel: no covariance
    assert not shift.any()


def test_lighting_shift_equals_the_twins(cuda):
    """The reported shift against the twin's (exact moments, LAPACK's eigh, the sign rule), relative to
    255 * lambda_max * max|normal|, on images whose relative eigenvalue gaps exceed 1e-3."""
    from jpeg_detection_resnet_ssd_amd.data.photometric import lighting_shift
    rng = np.random.default_rng(43)
    worst = 0.0
    for h, w in ((8, 16), (3, 43), (24, 40), (33, 47), (130, 63)):
        images = [_content(rng, "smooth", h, w) for _ in range(5)]
        ops = [[(LIG, tuple(float(v) for v in rng.standard_normal(3) * 0.5))] for _ in range(5)]
        _, shifts = _run(cuda, images, ops)
        for i in range(5):
            scale, lam = _shift_scale(images[i], np.array(ops[i][0][1]))
            gaps = np.diff(lam) / lam.max()
            assert gaps.min() > 1e-3, (h, w, i, gaps)
            dev = np.abs(shifts[i] - lighting_shift(images[i], ops[i][0][1])).max() / scale
            print("lighting shift deviation", (h, w), i, dev, "gaps", gaps.tolist())
            worst = max(worst, dev)
    print("largest lighting shift deviation:", worst, "bound:", SHIFT_BOUND)
    assert SHIFT_BOUND <= 1e-9
    assert worst <= SHIFT_BOUND


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_classifier_fed_by_the_device_path_with_the_four_callables_sees_the_twins_inputs(cuda, tmp_path):
    """Batch 2, ResNet50-DCT classifier, DCTGeneratorJPEG2DCT(device_prep=True, transformations=the four callables): the
    model's input buffers hold what rgb_to_dct_host makes of the host twin's pixels (prep_host, photometric_host), and the
    predictions are those of the host-made inputs."""
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.image_prep import prep_host
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import rgb_to_dct_host
    from jpeg_detection_resnet_ssd_amd.data.photometric import photometric_host
    from jpeg_detection_resnet_ssd_amd.keras import backend as K
    from jpeg_detection_resnet_ssd_amd.keras.losses import categorical_crossentropy
    from jpeg_detection_resnet_ssd_amd.keras.optimizers import SGD
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import (DCTGeneratorJPEG2DCT, brightness, contrast, lighting,
                                                                         saturation)
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.networks.resnet_dct import ResNet50Custom
    rng = np.random.default_rng(37)
    index = {"0": ["n_cat", "cat"], "1": ["n_dog", "dog"]}
    for i, (h, w) in enumerate([(120, 160), (150, 110)]):
        directory = tmp_path / "train" / index[str(i)][0]
        directory.mkdir(parents=True)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + (60 + 25 * c) * np.sin(xx / (9.0 + c) + c) * np.cos(yy / (7.0 + 2 * c)) for c in range(3)], axis=-1)
        Image.fromarray(np.clip(img + rng.normal(0, 4, img.shape), 0, 255).astype(np.uint8)).save(str(directory / "img.png"))
    (tmp_path / "index.json").write_text(json.dumps(index))
    gen = DCTGeneratorJPEG2DCT(str(tmp_path / "train"), str(tmp_path / "index.json"), batch_size=2, shuffle=False,
                               target_length=224, transformations=[lighting, contrast, brightness, saturation], device_prep=True)
    random.seed(E2E_SEEDS[0])
    np.random.seed(E2E_SEEDS[1])
    pending, _ = gen[0]
    codes = [[c for c, _ in lst] for lst in pending.ops]
    assert {c for lst in codes for c in lst} == {SAT, BRI, CON, LIG}, codes          # the seeds draw all four
    pixels = photometric_host(np.stack([prep_host(im, 224, *p) for im, p in zip(pending.images, pending.params)]), pending.ops)
    planes = [rgb_to_dct_host(p) for p in pixels]
    host_x = [np.stack([p[0] for p in planes]).astype(np.float32),
              np.stack([np.concatenate([p[1], p[2]], axis=-1) for p in planes]).astype(np.float32)]
    K.clear_session()
    K.set_random_seed(11)
    model = ResNet50Custom(weights=None, archi="late_concat_rfa_thinner")
    model.compile(loss=categorical_crossentropy, optimizer=SGD(lr=0.1, momentum=0.9, decay=1e-4, nesterov=True))
    got = model.predict_on_batch(pending)
    torch.cuda.synchronize()
    for buf, want in zip(model._plan(2, False, False).inputs, host_x):
        assert torch.equal(buf.detach().cpu(), torch.from_numpy(want))
    assert got.shape == (2, 1000) and np.isfinite(got).all()
    assert np.array_equal(model.predict_on_batch(host_x), got)
