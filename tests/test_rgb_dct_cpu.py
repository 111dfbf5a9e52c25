"""CPU: the RGB -> JPEG-DCT transform as a statement in numpy (data/jpeg_dct.py:rgb_to_dct_host, the twin of
csrc/dj_rgb2dct.hip) equals, coefficient for coefficient, what the in-tree reader gets out of the JPEG that PIL wrote of
the same pixels (tests/golden/rgb_dct.npz holds pixels and bytes; the reader is pinned to libjpeg by
test_jpeg_cpu.py); the C entry point is exported and refuses bad arguments before any launch."""
import ctypes
import io
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgb_dct.npz")
CASES = ["smooth_300x300_q75", "patches_300x300_q75", "noise_300x300_q30", "saturated_300x300_q90",
         "smooth_224x224_q75", "smooth_301x299_q75", "smooth_296x300_q75", "noise_37x53_q75", "noise_17x16_q75",
         "noise_8x8_q75", "noise_1x1_q100", "noise_300x20_q50", "noise_15x33_q10"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_exactly_the_listed_cases(golden):
    assert sorted({k.split("/")[0] for k in golden}) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("normalized", [True, False])
def test_host_twin_equals_the_reader_on_the_jpeg_pil_wrote(golden, case, normalized):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import blocks_for, rgb_to_dct_host
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    rgb, data, quality = golden[case + "/rgb"], golden[case + "/jpeg"].tobytes(), int(golden[case + "/quality"])
    want = j2d.loads(data, normalized=normalized)
    got = rgb_to_dct_host(rgb, quality, normalized=normalized)
    (yh, yw), (ch, cw) = blocks_for(*rgb.shape[:2])
    assert [p.shape for p in got] == [(yh, yw, 64), (ch, cw, 64), (ch, cw, 64)]
    for name, w, g in zip(("y", "cb", "cr"), want, got):
        assert g.dtype == np.int16 and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        print(case, name, "mismatching coefficients:", int((g != w).sum()), "of", w.size)
        assert np.array_equal(g, w), (case, name)


@pytest.mark.parametrize("case", CASES)
def test_quant_tables_equal_the_tables_in_the_file(golden, case):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    inf = j2d.info(golden[case + "/jpeg"].tobytes())
    luma, chroma = quant_tables(int(golden[case + "/quality"]))
    assert luma.shape == chroma.shape == (64,)
    assert np.array_equal(luma, np.array(list(inf.quant[0]))) and np.array_equal(chroma, np.array(list(inf.quant[1])))


def test_explicit_tables_replace_the_quality(golden):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import quant_tables, rgb_to_dct_host
    rgb = golden["noise_37x53_q75/rgb"]
    for a, b in zip(rgb_to_dct_host(rgb, quality=75), rgb_to_dct_host(rgb, quality=1, tables=quant_tables(75))):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        rgb_to_dct_host(rgb, tables=(np.zeros(64), np.ones(64)))
    with pytest.raises(ValueError):
        quant_tables(0)


def test_live_encodes_of_random_sizes_and_qualities():
    """20 further sizes / qualities / contents against a live PIL encode (only where PIL is installed)."""
    Image = pytest.importorskip("PIL.Image")
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import rgb_to_dct_host
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as j2d
    rng = np.random.default_rng(2024)
    for i in range(20):
        h, w = int(rng.integers(1, 330)), int(rng.integers(1, 330))
        quality = int(rng.choice([1, 10, 30, 50, 75, 90, 95, 100]))
        kind = i % 3
        if kind == 0:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif kind == 1:
            img = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        else:
            img = np.kron(rng.integers(0, 256, (h // 7 + 1, w // 7 + 1, 3)), np.ones((7, 7, 1), dtype=np.int64))[:h, :w]
            img = np.clip(img + rng.normal(0, 5, img.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="jpeg", quality=quality)
        want = j2d.loads(buf.getvalue())
        got = rgb_to_dct_host(img, quality)
        for name, a, b in zip(("y", "cb", "cr"), want, got):
            assert a.shape == b.shape and np.array_equal(a, b), (h, w, quality, kind, name, int((a != b).sum()))


# ---- the C entry point -----------------------------------------------------------------------------------------------------
def _call(lib, rgb=0x1000, batch=1, h=16, w=16, stride=48, luma=None, chroma=None, normalized=1, y=0x2000, ld_y=64,
          cb=0x3000, ld_cb=64, cr=0x4000, ld_cr=64):
    """The pointers are never dereferenced on the device: every call made through here must fail in the checks."""
    ok = (ctypes.c_ushort * 64)(*([16] * 64))
    luma = ok if luma is None else luma
    chroma = ok if chroma is None else chroma
    return lib.dj_rgb_to_dct(rgb, batch, h, w, stride, luma, chroma, normalized, y, ld_y, cb, ld_cb, cr, ld_cr, None)


def test_library_exports_the_entry_point():
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    assert "dj_rgb_to_dct" in _lib.SIGNATURES and hasattr(lib, "dj_rgb_to_dct")
    assert lib.dj_abi_version() == 5


@pytest.mark.parametrize("kwargs, names", [
    (dict(rgb=None), "rgb"), (dict(y=None), "out_y"), (dict(cb=None), "out_cb"), (dict(cr=None), "out_cr"),
    (dict(luma=0), "luma_table"), (dict(chroma=0), "chroma_table"),
    (dict(h=0), "height"), (dict(w=0), "width"), (dict(h=-3), "height"),
    (dict(ld_y=63), "ld_y"), (dict(ld_cb=32), "ld_cb"), (dict(ld_cr=0), "ld_cr"),
    (dict(stride=47), "stride_bytes"),
    (dict(luma="zero"), "luma_table[5]"), (dict(chroma="big"), "chroma_table[63]"),
])
def test_argument_errors_are_refused_on_the_host(kwargs, names):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    kw = dict(kwargs)
    for key in ("luma", "chroma"):
        if kw.get(key) == "zero":
            kw[key] = (ctypes.c_ushort * 64)(*[0 if i == 5 else 16 for i in range(64)])
        elif kw.get(key) == "big":
            kw[key] = (ctypes.c_ushort * 64)(*[256 if i == 63 else 16 for i in range(64)])
        elif kw.get(key) == 0:
            kw[key] = ctypes.c_void_p(None)
    rc = _call(lib, **kw)
    assert rc < 0
    msg = lib.dj_last_error().decode()
    assert names in msg, msg
    with pytest.raises(_lib.DjError):
        _lib.check(rc, "dj_rgb_to_dct")


# ---- the Python surface, without a device ---------------------------------------------------------------------------------
def test_pending_inputs_report_the_shapes_the_reader_returns(golden):
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import DeviceDCTEmitter, PendingDCTInputs
    batch = np.stack([golden["smooth_300x300_q75/rgb"], golden["noise_300x300_q30/rgb"]])
    pend = DeviceDCTEmitter()(batch)
    assert isinstance(pend, PendingDCTInputs) and len(pend) == 2 and pend.shape[0] == 2
    assert pend.shapes == [(2, 38, 38, 64), (2, 19, 19, 128)]
    assert DeviceDCTEmitter(deconv=True)(batch).shapes == [(2, 38, 38, 64), (2, 19, 19, 64), (2, 19, 19, 64)]
    assert DeviceDCTEmitter(deconv=True)(batch[:, :224, :224]).shapes == [(2, 28, 28, 64), (2, 14, 14, 64), (2, 14, 14, 64)]
    assert pend[1:].shape[0] == 1
    with pytest.raises(ValueError):
        DeviceDCTEmitter()(batch.astype(np.float32))
    # the host form of the same inputs is the reader's output
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import emit_dct_inputs
    ref = emit_dct_inputs(None, deconv=False, jpeg_bytes=[golden["smooth_300x300_q75/jpeg"].tobytes()])
    got = DeviceDCTEmitter(quality=75)(batch[:1]).numpy()
    assert all(np.array_equal(a, b) and b.dtype == np.float32 for a, b in zip(ref, got))


def test_wrong_image_size_raises_the_keras_shape_error(monkeypatch):
    """A 224x224 batch handed to the SSD300 model: the same ValueError text as for arrays, raised before anything is
    uploaded (plan lowered on the host: structure only)."""
    import torch
    monkeypatch.setenv("DJ_AUTOTUNE", "table")
    from jpeg_detection_resnet_ssd_amd import workloads
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import DeviceDCTEmitter
    model, _ = workloads.build_ssd("ssd_custom")
    model._ensure_params(device=torch.device("cpu"))
    plan = model._plan(2, False, False)
    small = np.zeros((2, 224, 224, 3), np.uint8)
    with pytest.raises(ValueError, match=r"expected shape \(2, 38, 38, 64\) but got array with shape \(2, 28, 28, 64\)"):
        model._upload(plan, DeviceDCTEmitter()(small), None)
    with pytest.raises(ValueError, match="expected 2 arrays but got 3"):
        model._upload(plan, DeviceDCTEmitter(deconv=True)(np.zeros((2, 300, 300, 3), np.uint8)), None)


def test_synthetic_generator_and_adapter_carry_pixels():
    from jpeg_detection_resnet_ssd_amd.data.generators import SyntheticDataGeneratorDCT, with_device_dct
    from jpeg_detection_resnet_ssd_amd.data.jpeg_dct import DeviceDCTEmitter, PendingDCTInputs
    em = DeviceDCTEmitter(deconv=True)
    gen = SyntheticDataGeneratorDCT(n_images=8, seed=3).generate(batch_size=2, deconv=True, dct_emitter=em)
    x, y = next(gen)
    assert isinstance(x, PendingDCTInputs) and x.shape == (2, 300, 300, 3) and len(y) == 2
    x2, _ = next(SyntheticDataGeneratorDCT(n_images=8, seed=3).generate(batch_size=2, deconv=True, dct_emitter=em))
    assert np.array_equal(x.pixels, x2.pixels)

    def user_generator():
        while True:
            yield np.zeros((2, 300, 300, 3), np.uint8), "labels", "extra"
    x, y, extra = next(with_device_dct(user_generator(), em))
    assert isinstance(x, PendingDCTInputs) and y == "labels" and extra == "extra"
